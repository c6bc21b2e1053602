// flux_sample_order.h -- the order in which the split kernel traces a pixel's samples (DevSetRows::order, render_body.inc
// render_split_kernel phase A).  One source for the device's table build (tables.hip), the kernel's slice bounds and the CPU tests
// (tests/test_sample_order.py, tests/sample_order_selftest.cpp).
//
// A wave's 64 phase-A samples were consecutive sample indices: 64 independent first-bounce directions, of which some lane practically
// always points at some sphere, so every pass paid phase B's sparse candidate trips.  The order in which a pixel's samples are traced is
// free -- each is still traced exactly once -- and for a Matte hit on a stored-normal record the first-bounce direction is
// hemi[set][0][i] in a fixed frame: a function of (set, i) alone.  So each set's sample indices are sorted by that direction once, at
// context creation, and a wave's 64 first-bounce rays leave into one small cone.  (The primary ray's two tables are read from copies in
// this order, DevSetRows::pix_o / disc_o: through the order their gathers touched 64 cache lines a wave and cost more than the trips saved.)
//
//   key    order_key(hemi.x, hemi.y): each component quantised from [-1, 1] to 7 bits (clamped: a NaN or an out-of-range value maps to
//          a defined cell), the two interleaved into a 14-bit Morton code.
//   sort   (key, i) pairs, stable: ties keep ascending i.  The values are a permutation of 0 .. N-1 WHATEVER the keys are -- the pairs
//          are permuted, never computed -- so the kernel's gather through the table cannot leave the set's rows.
//   deal   the sorted sequence is cut into groups of kOrderGroup = 64; group g goes to quarter g mod 4 of the row, quarter q being the
//          kernel's own slice [N q / 4, N (q + 1) / 4) of a four-wave block; each quarter fills front to back, and what a full quarter
//          cannot take spills into the next one with room.  Without the deal a block's waves would get contiguous quarters of the
//          hemisphere -- one the spheres, another the sky -- and the block would wait for the slowest.  For N a multiple of 256 every
//          64-aligned batch of every slice (K = 1, 2, 4 waves a pixel) is exactly one sorted group; other N stay correct and are merely
//          less coherent.
#pragma once
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FLUX_SO_HD __host__ __device__ inline
#else
#define FLUX_SO_HD inline
#endif

namespace flux {

constexpr uint32_t kOrderCellBits = 7;                 // bits per component
constexpr uint32_t kOrderKeyBits = 2 * kOrderCellBits; // the Morton code's
constexpr uint32_t kOrderGroup = 64;                   // a wave's batch
constexpr uint32_t kOrderQuarters = 4;                 // FLUX_MAX_WAVES_PER_PIXEL (flux_device.h; tables.hip holds the two equal)

// [-1, 1] -> 0 .. 127.  Negated compare first: a NaN, -inf and everything at or below -1 take cell 0; +inf and everything from
// 1 - 1/64 up take cell 127.  Between the two the product is in (0, 127): the conversion is defined.
FLUX_SO_HD uint32_t order_cell(double v) {
    const double s = (v + 1.0) * 64.0;
    if (!(s > 0.0)) return 0u;
    if (s >= 127.0) return 127u;
    return (uint32_t)s;
}

// bit k of a 7-bit value to bit 2 k
FLUX_SO_HD uint32_t order_spread(uint32_t v) {
    v &= 0x7fu;
    v = (v | (v << 4)) & 0x0f0fu;
    v = (v | (v << 2)) & 0x3333u;
    v = (v | (v << 1)) & 0x5555u;
    return v;
}

FLUX_SO_HD uint32_t order_key(double x, double y) { return order_spread(order_cell(x)) | (order_spread(order_cell(y)) << 1); }

// the slice of wave `sub` of K: the split kernel's own formula (and the refill kernel's)
FLUX_SO_HD uint32_t order_slice_lo(uint32_t N, uint32_t sub, uint32_t K) { return (uint32_t)((uint64_t)N * sub / K); }

// The deal as a walk over the groups in order: group(g, f) calls f(e0, count, pos) for each run of the group's elements
// e0 .. e0 + count - 1 (indices WITHIN the group) that lands at row positions pos .. pos + count - 1.  Every position of the row is
// handed out exactly once over the groups 0 .. groups() - 1 taken in ascending order: a quarter's fill only grows, never past its
// size, and the sizes sum to N.
struct OrderDeal {
    uint32_t N;
    uint32_t fill[kOrderQuarters];
    FLUX_SO_HD explicit OrderDeal(uint32_t n) : N(n), fill{0u, 0u, 0u, 0u} {}
    FLUX_SO_HD uint32_t groups() const { return (N + kOrderGroup - 1u) / kOrderGroup; }
    template <class F>
    FLUX_SO_HD void group(uint32_t g, F &&f) {
        const uint32_t first = g * kOrderGroup;
        uint32_t left = N - first < kOrderGroup ? N - first : kOrderGroup, e0 = 0u;
        uint32_t q = g % kOrderQuarters;
        while (left) {  // (ends: the room of all quarters together is what no group has taken yet, this group's elements among it)
            const uint32_t lo = order_slice_lo(N, q, kOrderQuarters), hi = order_slice_lo(N, q + 1u, kOrderQuarters);
            const uint32_t room = hi - lo - fill[q];
            const uint32_t take = room < left ? room : left;
            if (take) f(e0, take, lo + fill[q]);
            fill[q] += take;
            e0 += take;
            left -= take;
            q = (q + 1u) % kOrderQuarters;
        }
    }
};

// (host) The whole row from the keys: what the device builds (tables.hip), restated for the tests.  stable_sort_by_key(first, last,
// keys) is any stable sort of the indices by their key; std::stable_sort in the callers.
template <class Keys, class Index, class StableSort>
inline void order_row_host(const Keys &keys, uint32_t N, Index *row, StableSort &&stable_sort_by_key) {
    std::vector<Index> sorted(N);
    for (uint32_t i = 0; i < N; i++) sorted[i] = (Index)i;
    stable_sort_by_key(sorted.data(), sorted.data() + N, keys);
    OrderDeal deal(N);
    for (uint32_t g = 0; g < deal.groups(); g++)
        deal.group(g, [&](uint32_t e0, uint32_t count, uint32_t pos) {
            for (uint32_t k = 0; k < count; k++) row[pos + k] = sorted[g * kOrderGroup + e0 + k];
        });
}

}  // namespace flux
