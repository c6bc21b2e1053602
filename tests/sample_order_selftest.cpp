// The split kernel's per-set sample order (flux_amd/csrc/flux_sample_order.h) on the CPU: the header the table build and the kernel
// share, compiled for the host (tests/test_sample_order.py builds and runs it, once plain and once under AddressSanitizer and UBSan).
//   usage: sample_order_selftest                the checks below; one "ok <name>" per family and "all ok", exit 1 on the first failure
//          sample_order_selftest deal N         the row built from N EQUAL keys (the deal alone: sorted order = index order), one per line
//          sample_order_selftest slices N       the quarter bounds lo(0) .. lo(4)
//          sample_order_selftest keys           reads "x y" pairs (hex floats or decimals, "nan", "inf") from stdin, prints one key per line
//          sample_order_selftest row            reads one key per line from stdin, prints the row
//   1. keys: every special value lands in a cell 0 .. 127, monotone in between, the Morton code below 2^14 and invertible;
//   2. deal: for N = 1 .. 700 and a list of larger N the row of equal keys is a bijection of 0 .. N-1, the quarters equal the kernel's
//      slices, and for N a multiple of 256 every 64-aligned batch of every slice at K = 1, 2, 4 is one sorted group;
//   3. rows: for random, constant, reversed, two-valued and out-of-range key arrays the row is a permutation, and within one key the
//      sorted sequence keeps index order.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../flux_amd/csrc/flux_sample_order.h"

using namespace flux;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t next_u64() {  // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static std::vector<uint32_t> build_row(const std::vector<uint32_t> &keys) {
    const uint32_t N = (uint32_t)keys.size();
    std::vector<uint32_t> row(N, 0xffffffffu);
    order_row_host(keys, N, row.data(), [](uint32_t *b, uint32_t *e, const std::vector<uint32_t> &k) {
        std::stable_sort(b, e, [&](uint32_t x, uint32_t y) { return k[x] < k[y]; });
    });
    return row;
}

static void check_permutation(const std::vector<uint32_t> &row) {
    std::vector<unsigned char> seen(row.size(), 0);
    for (uint32_t v : row) {
        CHECK(v < row.size());
        CHECK(!seen[v]);
        seen[v] = 1;
    }
}

// the sorted sequence back out of the row: the inverse of the deal
static std::vector<uint32_t> undeal(const std::vector<uint32_t> &row) {
    const uint32_t N = (uint32_t)row.size();
    std::vector<uint32_t> sorted(N);
    OrderDeal deal(N);
    for (uint32_t g = 0; g < deal.groups(); g++)
        deal.group(g, [&](uint32_t e0, uint32_t count, uint32_t pos) {
            for (uint32_t k = 0; k < count; k++) sorted[g * kOrderGroup + e0 + k] = row[pos + k];
        });
    return sorted;
}

static void check_keys() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(order_cell(nan) == 0u && order_cell(-nan) == 0u);
    CHECK(order_cell(-inf) == 0u && order_cell(inf) == 127u);
    CHECK(order_cell(-1.0) == 0u && order_cell(1.0) == 127u);
    CHECK(order_cell(-1e300) == 0u && order_cell(1e300) == 127u && order_cell(-2.0) == 0u && order_cell(2.0) == 127u);
    CHECK(order_cell(std::nextafter(1.0, 2.0)) == 127u && order_cell(std::nextafter(-1.0, -2.0)) == 0u);
    CHECK(order_cell(0.0) == 64u && order_cell(-0.0) == 64u);
    CHECK(order_cell(std::numeric_limits<double>::denorm_min()) == 64u && order_cell(-std::numeric_limits<double>::denorm_min()) == 64u);
    uint32_t last = 0;
    for (int k = -40000; k <= 40000; k++) {  // monotone, in range
        const uint32_t c = order_cell(k / 32768.0);
        CHECK(c <= 127u && c >= last);
        last = c;
    }
    CHECK(last == 127u);
    for (uint32_t a = 0; a < 128; a++) {
        const uint32_t s = order_spread(a);
        CHECK((s & ~0x1555u) == 0u);
        uint32_t back = 0;
        for (int b = 0; b < 7; b++) back |= ((s >> (2 * b)) & 1u) << b;
        CHECK(back == a);
    }
    const double special[] = {nan, inf, -inf, 1.0, -1.0, 0.0, 0.5, -0.5, 1e300, -1e300, 0.999999, -0.999999};
    for (double x : special)
        for (double y : special) {
            const uint32_t k = order_key(x, y);
            CHECK(k < (1u << kOrderKeyBits));
            CHECK(k == (order_spread(order_cell(x)) | (order_spread(order_cell(y)) << 1)));
        }
    std::printf("ok keys\n");
}

static void check_deal_of(uint32_t N) {
    const std::vector<uint32_t> row = build_row(std::vector<uint32_t>(N, 5u));  // equal keys: sorted = index order
    check_permutation(row);
    CHECK(order_slice_lo(N, 0, kOrderQuarters) == 0u && order_slice_lo(N, kOrderQuarters, kOrderQuarters) == N);
    for (uint32_t K = 1; K <= kOrderQuarters; K *= 2)  // the kernel's slices at K = 1, 2, 4 are unions of quarters
        for (uint32_t sub = 0; sub <= K; sub++)
            CHECK(order_slice_lo(N, sub, K) == order_slice_lo(N, sub * (kOrderQuarters / K), kOrderQuarters));
    if (N % (kOrderGroup * kOrderQuarters) == 0)
        for (uint32_t K = 1; K <= kOrderQuarters; K *= 2)
            for (uint32_t sub = 0; sub < K; sub++)
                for (uint32_t b = order_slice_lo(N, sub, K); b < order_slice_lo(N, sub + 1, K); b += kOrderGroup) {
                    CHECK(row[b] % kOrderGroup == 0u);
                    for (uint32_t l = 0; l < kOrderGroup; l++) CHECK(row[b + l] == row[b] + l);
                }
    CHECK(undeal(row) == [&] {
        std::vector<uint32_t> id(N);
        for (uint32_t i = 0; i < N; i++) id[i] = i;
        return id;
    }());
}

static void check_deal(bool quick) {
    for (uint32_t N = 1; N <= (quick ? 300u : 700u); N++) check_deal_of(N);
    const uint32_t big[] = {1024, 4225, 8281, 16129, 16384, 16641, 65536};
    for (uint32_t N : big) check_deal_of(N);
    std::printf("ok deal\n");
}

static void check_rows(bool quick) {
    const uint32_t sizes[] = {1, 2, 63, 64, 65, 81, 255, 256, 257, 289, 4225, 16384};
    for (uint32_t N : sizes)
        for (int family = 0; family < 6; family++) {
            if (quick && N > 4225 && family > 1) continue;
            std::vector<uint32_t> keys(N);
            for (uint32_t i = 0; i < N; i++)
                keys[i] = family == 0   ? (uint32_t)(next_u64() & 0x3fffu)
                          : family == 1 ? 0u
                          : family == 2 ? N - i               // reversed, every key its own
                          : family == 3 ? (uint32_t)(i & 1u)  // two values, interleaved
                          : family == 4 ? (uint32_t)next_u64()  // beyond 14 bits: whatever the keys are
                                        : (uint32_t)(next_u64() % 3u) * 0x7fffffffu;
            const std::vector<uint32_t> row = build_row(keys);
            check_permutation(row);
            const std::vector<uint32_t> sorted = undeal(row);
            for (uint32_t r = 1; r < N; r++) {
                CHECK(keys[sorted[r - 1]] <= keys[sorted[r]]);
                if (keys[sorted[r - 1]] == keys[sorted[r]]) CHECK(sorted[r - 1] < sorted[r]);  // ties keep index order
            }
        }
    std::printf("ok rows\n");
}

static double parse(const std::string &s) { return std::strtod(s.c_str(), nullptr); }  // (takes "nan", "inf", "-inf" and hex floats)

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "deal" && argc > 2) {
        for (uint32_t v : build_row(std::vector<uint32_t>((size_t)std::atol(argv[2]), 0u))) std::printf("%u\n", v);
        return 0;
    }
    if (mode == "slices" && argc > 2) {
        for (uint32_t q = 0; q <= kOrderQuarters; q++) std::printf("%u\n", order_slice_lo((uint32_t)std::atol(argv[2]), q, kOrderQuarters));
        return 0;
    }
    if (mode == "keys") {
        char a[128], b[128];
        while (std::scanf("%127s %127s", a, b) == 2) std::printf("%u\n", order_key(parse(a), parse(b)));
        return 0;
    }
    if (mode == "row") {
        std::vector<uint32_t> keys;
        unsigned k;
        while (std::scanf("%u", &k) == 1) keys.push_back(k);
        for (uint32_t v : build_row(keys)) std::printf("%u\n", v);
        return 0;
    }
    const bool quick = mode == "quick";
    check_keys();
    check_deal(quick);
    check_rows(quick);
    std::printf("all ok\n");
    return 0;
}
