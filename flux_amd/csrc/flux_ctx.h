// flux_ctx.h -- the context behind include/flux_abi.h's opaque flux_ctx, shared by abi.hip (the single-device entry
// points) and multi.hip (the multi-GPU frame).  Internal: nothing here crosses the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <new>
#include <optional>
#include <string>
#include <system_error>
#include <utility>
#include <vector>

#include "../../include/flux_abi.h"
#include "flux_device.h"
#include "flux_tables.h"
#include "scene_build.h"

namespace flux {

// message of the calling thread's last failed call (flux_last_error); fail() sets it and returns `code`
extern thread_local std::string g_last_error;
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// Runs f() and returns its FLUX code.  What it throws becomes a code instead of unwinding through the C ABI: a failed host
// allocation or thread creation is FLUX_E_NOMEM.
template <class F> int no_throw(F &&f) {
    try {
        return f();
    } catch (const std::bad_alloc &) {
        return fail(FLUX_E_NOMEM, "host allocation failed");
    } catch (const std::system_error &e) {
        return fail(FLUX_E_NOMEM, "%s", e.what());
    }
}

// Where the wall time of a context's creation goes (flux_ctx_create_timing): lap(k) books the time since the previous lap under
// word k.  A context of flux_multi_create starts with the shared host build already booked under HOST.
struct CreateLaps {
    double ms[FLUX_CREATE_TIMING_WORDS] = {};
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    void lap(int k) {
        const auto now = std::chrono::steady_clock::now();
        ms[k] += std::chrono::duration<double, std::milli>(now - last).count();
        last = now;
    }
};

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// The entry points' two device checks (abi.hip): FLUX_E_DEVICE unless a HIP device is visible, then FLUX_E_INVALID for one out of range ...
int check_device(int device);
int require_device(int device);  // ... or FLUX_E_DEVICE for either

// What DevBuf<T>, Stream and Event share: each owns one handle, is move-only and empty by default, releases in its destructor or reset(), and
// converts to the handle.  A release runs on the CURRENT device: the structs that hold owners (flux_ctx, flux_multi) make theirs current.
template <class H, hipError_t (*Release)(H)> class Owner {
  protected:
    H h_ = nullptr;

  public:
    Owner() = default;
    Owner(Owner &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Owner &operator=(Owner &&o) noexcept {
        if (this != &o) {
            reset();
            h_ = std::exchange(o.h_, nullptr);
        }
        return *this;
    }
    ~Owner() { reset(); }
    void reset() {
        if (H h = std::exchange(h_, nullptr)) (void)Release(h);
    }
    operator H() const { return h_; }
};
template <class T> hipError_t free_device(T *p) { return hipFree(p); }
inline hipError_t drain_and_destroy(hipStream_t s) {  // (what the stream still runs may use what is released after it)
    (void)hipStreamSynchronize(s);
    return hipStreamDestroy(s);
}
template <class T> struct DevBuf : Owner<T *, free_device<T>> {  // a hipMalloc allocation of T
    hipError_t alloc_bytes(size_t bytes) {  // releases what it held; hipMalloc's result
        this->reset();
        return hipMalloc((void **)&this->h_, bytes);
    }
    hipError_t alloc(size_t count) { return alloc_bytes(count * sizeof(T)); }
};
// What grow-only device scratch holds, in its owner's units.  grow(want, alloc) runs alloc() -- which allocates everything sized by
// this capacity -- where `want` exceeds it.  The capacity is 0 while alloc() runs and stays 0 if it fails: a DevBuf releases what it
// held before it allocates.
struct Capacity {
    size_t n = 0;
    template <class F> hipError_t grow(size_t want, F &&alloc) {
        if (want <= n) return hipSuccess;
        n = 0;
        const hipError_t e = alloc();
        if (e == hipSuccess) n = want;
        return e;
    }
};
template <class T> struct Scratch : DevBuf<T> {  // one grow-only buffer
    Capacity held;
    hipError_t reserve(size_t count) {
        return held.grow(count, [&] { return this->alloc(count); });
    }
};
struct Stream : Owner<hipStream_t, drain_and_destroy> {
    hipError_t create() { return hipStreamCreateWithFlags(&h_, hipStreamNonBlocking); }
};
struct Event : Owner<hipEvent_t, hipEventDestroy> {
    hipError_t create() { return hipEventCreate(&h_); }
};

// The three phases of context creation (abi.hip): the job's checks, which need no device; the host scene build (scene_build.h),
// its failures reported through fail(); the device half, which makes the context on `device` for the sample sets first_set +
// k * set_stride and books its time from RUNTIME on.
int validate_job(const flux_scene_desc &scene, const flux_job_cfg &cfg, uint64_t first_set, uint64_t set_stride);
int build_host(const flux_scene_desc &scene, HostScene &host);
int upload(const HostScene &host, const flux_job_cfg &cfg, uint64_t seed, int device, uint64_t first_set, uint64_t set_stride,
           CreateLaps &laps, flux_ctx **out);

}  // namespace flux

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return flux::fail(e_ == hipErrorOutOfMemory ? FLUX_E_NOMEM : FLUX_E_DEVICE, "%s: %s", \
                              #expr, hipGetErrorString(e_));                                      \
    } while (0)

struct flux_ctx {
    // Engaged by the destructor.  As the FIRST member it outlives every owner below, so their releases run with `device` current.
    std::optional<flux::DeviceGuard> dying;
    ~flux_ctx() { dying.emplace(device); }
    int device = 0;
    flux::RenderParams rp{};  // camera + table pointers; work fields set per launch
    uint64_t seed = 0;
    uint32_t n = 0, N = 0, D = 0, S = 0, W = 0, H = 0;
    flux::SetRange sets{0, 1, 0};  // sets with tables in this context (all S unless created by flux_ctx_create_sets)
    flux::DevBuf<flux::DevShape> d_shapes;
    flux::DevBuf<flux::DevMaterial> d_mats;  // the materials, followed by their bounce weights
    flux::DevBuf<unsigned char> d_fscene;    // the FAST scene image, regions as HostScene::fs lays them out (scene_build.h)
    flux::DevBuf<double2> d_pix, d_disc;
    flux::DevBuf<double> d_hemi;
    flux::DevBuf<double> d_gloss;     // FAST glossy-lobe factors of pixel_sets
    flux::DevBuf<double2> d_glossx;   // the glossy lobe's angles per held sample and exponent slot (RenderParams::glossx), or empty
    flux::DevBuf<int32_t> d_gxoff;    // RenderParams::gx_off, with d_glossx
    flux::DevBuf<double> d_tput;      // RenderParams::tput, or empty
    flux::DevBuf<double> d_lobe;      // RenderParams::lobe_frame, or empty
    flux::DevBuf<double2> d_pix_o, d_disc_o;  // [slots held][N]: pix and disc in the order of d_order, what the split kernel's phase A reads
    flux::DevBuf<uint32_t> d_order;  // [slots held][N]: the split kernel's sample order (flux_sample_order.h)
    flux::DevBuf<flux::DevSetRows> d_setrows;  // per table slot: where the set's rows of the sample tables start
    flux::DevBuf<int32_t> d_rowperm, d_invperm;
    flux::DevBuf<unsigned long long> d_stats;
    bool stats_on = false;
    // extension: triangle meshes
    flux::DevBuf<flux::DevTri> d_tris;
    flux::DevBuf<flux::DevNode> d_nodes;
    flux::DevBuf<flux::DevNode4A> d_arena;  // the 4-wide tree of the FAST traversal kernel (RenderParams::nodes4), or empty
    flux::DevBuf<flux::DevNodeQ> d_nodesq;
    // extension: smooth meshes (flux_ctx_set_mesh_normals).  mesh_first: HostScene::mesh_first; mesh_smooth[m]: mesh m has corner
    // normals in d_tri_attrs (RenderParams::tri_attrs), which is held while any mesh has
    std::vector<uint64_t> mesh_first;
    std::vector<unsigned char> mesh_smooth;
    std::vector<unsigned char> mesh_colored;  // vertex colours (flux_ctx_set_mesh_colors): mesh m has corner colours in the same table
    flux::DevBuf<double> d_tri_attrs;
    flux::BvhInfo bvh{};
    int traversal = FLUX_TRAVERSE_BVH;
    int variant = FLUX_KERNEL_DEFAULT;
    int math = FLUX_MATH_FAST;
    // scratch framebuffer for the host-output path (flux_render_rows), the feature buffers' own (flux_render_aov_rows) and the sample
    // moments' own (flux_render_moments_rows), the chain feature buffers' own (flux_render_aov_chain_rows): no call resizes or
    // aliases another's
    flux::Scratch<double> d_out, d_aov, d_moments, d_aov_chain;
    // ... and the adaptive sampler's state and work list (flux_render_adaptive_rows*), all sized for d_adapt_pixels pixels: the running
    // sums [pixels][kAdaptiveSums], the pass counts, the hot flags, the list, and two counters (active pixels, pixels at max_passes);
    // d_adapt_out / d_adapt_map stage the host entry point's outputs, sized for d_adapt_out_pixels
    flux::DevBuf<double> d_adapt_sums, d_adapt_out;
    flux::DevBuf<uint32_t> d_adapt_passes, d_adapt_list, d_adapt_counts, d_adapt_map;
    flux::DevBuf<unsigned char> d_adapt_hot;
    flux::Capacity d_adapt_pixels, d_adapt_out_pixels;
    flux::Event ev0, ev1;
    bool timed = false;
    uint64_t device_bytes = 0;
    double U[3], V[3], Wv[3];
    // where flux_ctx_create's wall time went (flux_ctx_create_timing, CreateLaps), milliseconds
    double create_ms[FLUX_CREATE_TIMING_WORDS] = {};
};
