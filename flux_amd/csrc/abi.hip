// abi.hip -- implementation of include/flux_abi.h (the drop-in boundary).
//
// flux_ctx_create  = Scene::from_data (scene.rs:128-154) + Camera::new
//                    (trace.rs:26-42) as called from workers.rs:46-54
// flux_render_rows = Camera::render (trace.rs:53-97) as called from workers.rs:60
// There is no CPU fallback: without a usable HIP device every compute entry
// point fails with FLUX_E_DEVICE.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/flux_abi.h"
#include "flux_device.h"
#include "flux_tables.h"
#include "flux_math_coeffs.h"  // kExp2Poly -> RenderParams::exp2c

#include "flux_ctx.h"
#include "flux_mesh_attr.h"
#include "flux_switches.h"

namespace flux {

thread_local std::string g_last_error;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

}  // namespace flux

using flux::DeviceGuard;
using flux::fail;

extern "C" {

uint32_t flux_abi_version(void) { return FLUX_ABI_VERSION; }

const char *flux_last_error(void) { return flux::g_last_error.c_str(); }

int flux_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

#ifndef FLUX_BUILD_ID
#define FLUX_BUILD_ID "lib:unknown kernels:unknown"
#endif
const char *flux_build_id(void) { return FLUX_BUILD_ID; }

int flux_device_warmup(int device) {
    if (int rc = flux::check_device(device)) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(FLUX_E_DEVICE, "hipSetDevice(%d) failed", device);
    // the runtime initialises lazily, per subsystem: the device context, the copy engine's staging (first hipMemcpy), the
    // compute queue + this library's code object (first launch), the stream pool (scripts/micro/cold_start.hip times each)
    double xy[2 * 4];
    flux::DevBuf<double> d;
    flux::Stream s;
    HIP_TRY(d.alloc_bytes(sizeof(xy)));
    hipError_t e = hipMemcpy(d, xy, sizeof(xy), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = flux::generate_sampler_grid(FLUX_SAMPLER_REGULAR, 0, 2, d, nullptr, nullptr);
    if (e == hipSuccess) e = s.create();
    if (e != hipSuccess) return fail(FLUX_E_DEVICE, "flux_device_warmup: %s", hipGetErrorString(e));
    return FLUX_OK;
}

void flux_ctx_destroy(flux_ctx *ctx) { delete ctx; }

}  // extern "C"

namespace flux {

int check_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(FLUX_E_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(FLUX_E_INVALID, "device %d out of range [0,%d)", device, ndev);
    return FLUX_OK;
}
int require_device(int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) == hipSuccess && device >= 0 && device < count) return FLUX_OK;
    return fail(FLUX_E_DEVICE, "no HIP device %d (this library has no CPU fallback)", device);
}

// a material's kind and, for a Dielectric, its refraction index; `what` and `i` name its owner ("shape 3", "mesh 0")
static int validate_material(const flux_material &m, const char *what, uint64_t i) {
    if (m.kind < FLUX_MAT_MATTE || m.kind > FLUX_MAT_DIELECTRIC)
        return fail(FLUX_E_INVALID, "%s %llu: unknown material kind %d", what, (unsigned long long)i, m.kind);
    if (m.kind == FLUX_MAT_DIELECTRIC && !(std::isfinite(m.k) && m.k > 0.0))
        return fail(FLUX_E_INVALID, "%s %llu: dielectric refraction index must be finite and > 0, got %g", what, (unsigned long long)i, m.k);
    return FLUX_OK;
}

int validate_job(const flux_scene_desc &scene, const flux_job_cfg &cfg, uint64_t first_set, uint64_t set_stride) {
    if (set_stride < 1 || first_set >= set_stride)
        return fail(FLUX_E_INVALID, "sample-set share: need set_stride >= 1 and first_set < set_stride, got %llu / %llu",
                    (unsigned long long)first_set, (unsigned long long)set_stride);
    if (set_stride > 0xffffffffull)  // stored as 32-bit (SetRange); first_set < set_stride is then in range too
        return fail(FLUX_E_INVALID, "sample-set share: set_stride %llu exceeds 2^32 - 1", (unsigned long long)set_stride);
    if (cfg.sample_root < 1 || cfg.sample_root > 4096)
        return fail(FLUX_E_INVALID, "sample_root must be in [1,4096], got %llu", (unsigned long long)cfg.sample_root);
    if (cfg.max_trace_depth < 1 || cfg.max_trace_depth > 256)
        return fail(FLUX_E_INVALID, "max_trace_depth must be in [1,256], got %llu", (unsigned long long)cfg.max_trace_depth);
    // the render kernels address a pixel's Lambertian samples with a 32-bit byte offset from the set's base:
    // max_trace_depth * sample_root^2 * 32 B must stay below 4 GiB (the table of even ONE narrow image row would
    // otherwise be enormous: this only excludes e.g. sample_root 4096 with depth >= 8)
    if ((uint64_t)cfg.max_trace_depth * cfg.sample_root * cfg.sample_root * 32ull >= (1ull << 32))
        return fail(FLUX_E_INVALID, "max_trace_depth * sample_root^2 = %llu is too large (limit 2^27 = 134217728)",
                    (unsigned long long)(cfg.max_trace_depth * cfg.sample_root * cfg.sample_root));
    if (scene.image_width < 1 || scene.image_height < 1 || scene.image_width > 65535 || scene.image_height > (1u << 20))
        return fail(FLUX_E_INVALID, "image size %llux%llu out of range", (unsigned long long)scene.image_width,
                    (unsigned long long)scene.image_height);
    if (scene.num_shapes > 0 && !scene.shapes) return fail(FLUX_E_INVALID, "num_shapes > 0 but shapes is null");
    if (scene.num_shapes > 4096)
        return fail(FLUX_E_INVALID, "flat shape list limited to 4096 shapes, got %llu", (unsigned long long)scene.num_shapes);
    for (uint64_t i = 0; i < scene.num_shapes; i++) {
        const flux_shape &s = scene.shapes[i];
        if (s.kind != FLUX_SHAPE_SPHERE && s.kind != FLUX_SHAPE_PLANE && s.kind != FLUX_SHAPE_DISK && s.kind != FLUX_SHAPE_BOX)
            return fail(FLUX_E_INVALID, "shape %llu: unknown kind %d", (unsigned long long)i, s.kind);
        if (s.kind == FLUX_SHAPE_BOX)
            for (int a = 0; a < 3; a++)
                if (!(std::isfinite(s.p[a]) && std::isfinite(s.n[a]) && s.p[a] < s.n[a]))
                    return fail(FLUX_E_INVALID, "shape %llu: box corners must be finite with corner0 < corner1 on axis %c, got %g and %g",
                                (unsigned long long)i, "xyz"[a], s.p[a], s.n[a]);
        if (s.kind == FLUX_SHAPE_DISK && !(std::isfinite(s.radius) && s.radius >= 0.0))
            return fail(FLUX_E_INVALID, "shape %llu: disk radius must be finite and >= 0, got %g", (unsigned long long)i, s.radius);
        if (int rc = validate_material(s.material, "shape", i)) return rc;
    }
    if (scene.num_meshes > 0 && !scene.meshes) return fail(FLUX_E_INVALID, "num_meshes > 0 but meshes is null");
    uint64_t total_tris = 0;
    for (uint64_t m = 0; m < scene.num_meshes; m++) {
        const flux_mesh &me = scene.meshes[m];
        if (int rc = validate_material(me.material, "mesh", m)) return rc;
        if (me.num_triangles && (!me.vertices || !me.indices))
            return fail(FLUX_E_INVALID, "mesh %llu: null vertices/indices", (unsigned long long)m);
        for (uint64_t k = 0; k < 3 * me.num_triangles; k++)
            if (me.indices[k] >= me.num_vertices)
                return fail(FLUX_E_INVALID, "mesh %llu: vertex index %u out of range (%llu vertices)", (unsigned long long)m,
                            me.indices[k], (unsigned long long)me.num_vertices);
        total_tris += me.num_triangles;
    }
    if (total_tris >= (1ull << 27))  // leaf references pack (first << 3 | count) into 31 bits
        return fail(FLUX_E_INVALID, "too many triangles: %llu", (unsigned long long)total_tris);
    return FLUX_OK;
}

int build_host(const flux_scene_desc &scene, HostScene &host) {
    std::string error;
    const int rc = build_host_scene(scene, host, error);
    return rc == FLUX_OK ? rc : fail(rc, "%s", error.c_str());
}

int upload(const HostScene &h, const flux_job_cfg &cfg, uint64_t seed, int device, uint64_t first_set, uint64_t set_stride,
           CreateLaps &laps, flux_ctx **out) {
    *out = nullptr;
    // the creation switches (flux_switches.h), each named where it acts below
    const bool no_sample_tables = switch_off(kEnvSampleTables);
    const bool no_tput_table = switch_off(kEnvThroughputTable);
    const bool identity_order = switch_off(kEnvSampleOrder);
    const bool no_plane_axis = switch_off(kEnvPlaneAxis);
    DeviceGuard guard(device);
    if (!guard.ok) return fail(FLUX_E_DEVICE, "hipSetDevice(%d) failed", device);
    (void)hipFree(nullptr);  // the runtime's lazy per-device initialisation, booked under its own word (zero once the process has used the device)
    laps.lap(FLUX_CREATE_MS_RUNTIME);

    std::unique_ptr<flux_ctx> c(new flux_ctx());
    c->device = device;
    c->seed = seed;
    c->n = (uint32_t)cfg.sample_root;
    c->N = c->n * c->n;
    c->D = (uint32_t)cfg.max_trace_depth;
    c->W = (uint32_t)h.rp.img_w;
    c->H = (uint32_t)h.rp.img_h;
    c->S = h.rp.num_sets;
    // the sets this context holds tables for: all of them, or one rank's share of a set-sharded render
    c->sets.first = (uint32_t)first_set;
    c->sets.stride = (uint32_t)set_stride;
    c->sets.count = first_set < c->S ? (uint32_t)((c->S - first_set + set_stride - 1) / set_stride) : 0u;
    c->bvh = h.bvh;
    c->mesh_first = h.mesh_first;
    c->mesh_smooth.assign(h.mesh_first.empty() ? 0 : h.mesh_first.size() - 1, 0);
    c->mesh_colored.assign(c->mesh_smooth.size(), 0);
    for (int a = 0; a < 3; a++) {
        c->U[a] = h.U[a];
        c->V[a] = h.V[a];
        c->Wv[a] = h.W[a];
    }

    // ---- HBM allocations and uploads -------------------------------------------
    const size_t own = c->sets.count ? c->sets.count : 1;  // a share past the last set holds nothing (allocate one slot)
    const size_t pix_bytes = own * c->N * sizeof(double2);
    const size_t hemi_bytes = own * c->D * c->N * kHemiDoubles * sizeof(double);
    const size_t perm_bytes = (size_t)c->H * c->S * sizeof(int32_t);
    hipError_t e = hipSuccess;
    auto alloc = [&](auto &buf, size_t bytes) {
        if (e != hipSuccess) return;
        laps.lap(FLUX_CREATE_MS_UPLOAD);
        e = buf.alloc_bytes(bytes);
        if (e == hipSuccess) c->device_bytes += bytes;
        laps.lap(FLUX_CREATE_MS_ALLOC);
    };
    auto copy = [&](void *dst, const auto &v) {
        if (e == hipSuccess) e = hipMemcpy(dst, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice);
    };
    auto alloc_copy = [&](auto &buf, const auto &v) {
        alloc(buf, v.size() * sizeof(v[0]));
        copy(buf, v);
    };
    alloc_copy(c->d_shapes, h.shapes);
    // the materials, followed by their bounce weights (render_bvh4_kernel)
    alloc(c->d_mats, h.mats.size() * sizeof(DevMaterial) + h.wtab.size() * sizeof(double));
    copy(c->d_mats, h.mats);
    copy(c->d_mats + h.mats.size(), h.wtab);
    alloc_copy(c->d_fscene, h.fscene);
    alloc(c->d_pix, pix_bytes);
    alloc(c->d_disc, pix_bytes);
    alloc(c->d_hemi, hemi_bytes);
    alloc(c->d_gloss, pix_bytes * 2);
    // the glossy lobe's angle table (RenderParams::glossx) where the host scene assigned its exponents slots; FLUX_SAMPLE_TABLES=0
    // builds the context without it (tests and A/B runs: every glossy bounce then keeps the arithmetic in the loop)
    const int gx_stride = no_sample_tables ? 0 : h.rp.gx_stride;
    if (gx_stride) {
        alloc(c->d_glossx, own * c->N * (size_t)gx_stride);
        alloc_copy(c->d_gxoff, h.gx_off);
    }
    // the throughput product table (RenderParams::tput) where the job's renders would take parked hits from the hit queue and the
    // table stays within its cap (flux_plan.h); FLUX_THROUGHPUT_TABLE=0 builds the context without it (tests and A/B runs: the take then
    // multiplies the list up).  A switch of its own: what FLUX_SAMPLE_TABLES=0 removes from a context is the sample tables' bytes.
    // Whether every throughput product of the job is finite (RenderParams::tput_finite, the depth cut's condition: launch_plan.cpp
    // split_cut_depth) is judged on the host's table either way: the switch removes the device's copy, not what a frame is made of.
    int tput_bits = 0;
    bool tput_finite = false;
    {
        RenderParams job = h.rp;
        job.nsamp = c->N;
        job.max_depth = (int32_t)c->D;
        if (tput_table_bytes(job, &tput_bits)) {
            std::vector<double> tput;
            build_tput_table(h, tput_bits, (int)c->D, tput);
            tput_finite = tput_products_finite(h, tput_bits, (int)c->D, tput);
            if (!no_tput_table) alloc_copy(c->d_tput, tput);
        }
    }
    // the lobe-frame table (RenderParams::lobe_frame): 48 B per hit record, filled by the device below; FLUX_LOBE_FRAMES=0 builds the
    // context without it (scene_build.cpp lobe_frame_table: tests and A/B runs -- every bounce then builds its frame in the loop)
    std::vector<unsigned char> lobe_entries;
    const size_t lobe_bytes = lobe_frame_table(h, lobe_entries);
    if (lobe_bytes) alloc(c->d_lobe, lobe_bytes);
    alloc(c->d_order, own * c->N * sizeof(uint32_t));
    alloc(c->d_pix_o, pix_bytes);
    alloc(c->d_disc_o, pix_bytes);
    alloc(c->d_setrows, own * sizeof(DevSetRows));
    alloc(c->d_rowperm, perm_bytes);
    alloc(c->d_invperm, perm_bytes);
    alloc(c->d_stats, FLUX_NUM_STATS * sizeof(unsigned long long));
    if (!h.tris.empty()) {
        alloc_copy(c->d_tris, h.tris);
        alloc_copy(c->d_nodes, h.nodes);
        alloc_copy(c->d_nodesq, h.nodesq);
        if (!h.arena.empty()) alloc_copy(c->d_arena, h.arena);
    }
    if (e == hipSuccess) e = hipMemset(c->d_stats, 0, FLUX_NUM_STATS * sizeof(unsigned long long));
    laps.lap(FLUX_CREATE_MS_UPLOAD);
    if (e == hipSuccess) e = c->ev0.create();
    if (e == hipSuccess) e = c->ev1.create();
    laps.lap(FLUX_CREATE_MS_OTHER);
    // ---- MasterSampleSets::new on the device (sampling.rs:13-33) --------------
    double tab_ms[3] = {0, 0, 0};
    if (e == hipSuccess)
        e = generate_tables(seed, c->S, c->sets, c->D, c->n, c->H, c->d_pix, c->d_disc, c->d_hemi, c->d_rowperm, c->d_invperm, nullptr, tab_ms);
    if (e == hipSuccess) {
        e = generate_gloss_table(c->d_pix, (size_t)c->sets.count * c->N, c->d_gloss, nullptr);
        if (e == hipSuccess && gx_stride)
            e = generate_glossx_table(c->d_gloss, (size_t)c->sets.count * c->N, h.gx_inv_e1.data(), h.rp.n_gloss_exp, gx_stride / 16,
                                      c->d_glossx, nullptr);
        if (e == hipSuccess && c->d_lobe)
            e = generate_lobe_frame_table(reinterpret_cast<const DevHitRec *>(c->d_fscene + h.fs.rec), (int)lobe_entries.size(), c->d_lobe, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        // the split kernel's sample order, from the hemi rows just written; FLUX_SAMPLE_ORDER=0 fills it with the identity (tests and
        // A/B runs: the same kernel code then traces a pixel's samples in index order)
        if (e == hipSuccess)
            e = generate_sample_order(c->sets.count, c->D, c->n, c->d_hemi, c->d_order, identity_order, nullptr, tab_ms);
        // ... and the two primary-ray tables in that order, for phase A's consecutive reads (under the switch: plain copies)
        if (e == hipSuccess)
            e = generate_order_copies((size_t)c->sets.count * c->N, c->N, c->d_order, c->d_pix, c->d_disc, c->d_pix_o, c->d_disc_o, nullptr);
    }
    laps.lap(FLUX_CREATE_MS_TABLES);
    // the generator's scratch (the permutations of every grid: 262 MB at 16384 spp) is allocation, not table work
    laps.ms[FLUX_CREATE_MS_TABLES] -= tab_ms[0] + tab_ms[2];
    laps.ms[FLUX_CREATE_MS_ALLOC] += tab_ms[0];
    laps.ms[FLUX_CREATE_MS_FREE] += tab_ms[2];
    // where each held set's rows of the sample tables start: one 64-B record per slot, so that a kernel forms a table address with one
    // scalar load instead of a 64-bit multiply-add chain per table and pass (render_body.inc FLUX_SET_ROWS)
    if (e == hipSuccess) {
        std::vector<DevSetRows> rows(own, DevSetRows{});
        for (size_t m = 0; m < own; m++) {
            rows[m].pix = c->d_pix + m * c->N;
            rows[m].disc = c->d_disc + m * c->N;
            rows[m].hemi = c->d_hemi + m * c->D * c->N * kHemiDoubles;
            rows[m].gloss = c->d_gloss + m * c->N * 4;
            rows[m].order = c->d_order + m * c->N;
            rows[m].pix_o = c->d_pix_o + m * c->N;
            rows[m].disc_o = c->d_disc_o + m * c->N;
            rows[m].glossx = gx_stride ? c->d_glossx + m * c->N * (size_t)(gx_stride / 16) : nullptr;
        }
        copy(c->d_setrows, rows);
    }
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? FLUX_E_NOMEM : FLUX_E_DEVICE, "flux_ctx_create: %s", hipGetErrorString(e));

    // ---- RenderParams: the host scene's fields, pointed into this device's copies ----
    RenderParams &rp = c->rp;
    rp = h.rp;
    rp.pixel_denom = 1.0 / (double)((uint64_t)c->n * c->n);  // trace.rs:59
    rp.max_depth = (int32_t)c->D;
    rp.nsamp = c->N;
    rp.shapes = c->d_shapes;
    rp.mats = c->d_mats;
    rp.pix = c->d_pix;
    rp.disc = c->d_disc;
    rp.hemi = c->d_hemi;
    rp.gloss = c->d_gloss;
    rp.glossx = c->d_glossx;
    rp.gx_off = c->d_gxoff;
    rp.gx_stride = gx_stride;
    rp.tput = c->d_tput;
    rp.tput_bits = c->d_tput ? tput_bits : 0;
    rp.tput_finite = tput_finite ? 1 : 0;
    rp.lobe_frame = c->d_lobe;
    // the first plane's axis (RenderParams::plane_axis); FLUX_PLANE_AXIS=0 builds the context without it (tests and A/B runs: both scans
    // then form the first plane's dot products in full)
    if (no_plane_axis) rp.plane_axis = kPlaneAxisNone;
    rp.set_rows = c->d_setrows;
    rp.rowperm = c->d_rowperm;
    rp.invperm = c->d_invperm;
    for (int k = 0; k < 12; k++) rp.exp2c[k] = fastmath::kExp2Poly[k];
    rp.tris = c->d_tris;
    rp.nodes = c->d_nodes;
    rp.nodesq = c->d_nodesq;
    rp.nodes4 = reinterpret_cast<const DevNode4Q *>(static_cast<DevNode4A *>(c->d_arena));  // (the arena's kernel reads it as DevNode4A)
    const unsigned char *fs = c->d_fscene;
    rp.fsph = reinterpret_cast<const DevScanSphere *>(fs + h.fs.sph);
    rp.fpln = reinterpret_cast<const DevScanPlane *>(fs + h.fs.pln);
    rp.frec = reinterpret_cast<const DevHitRec *>(fs + h.fs.rec);
    rp.fsph32 = h.filter32 ? reinterpret_cast<const DevScanSphere32 *>(fs + h.fs.s32) : nullptr;
    rp.f32_half = rp.fsph32 && h.f32_half >= 0 ? rp.fsph32 + h.f32_half : nullptr;
    rp.f32_top = rp.fsph32 ? rp.fsph32 + h.f32_top : nullptr;
    rp.sshapes = reinterpret_cast<const DevShape *>(fs + h.fs.ss);
    rp.pxc = reinterpret_cast<const double *>(fs + h.fs.pxc);
    rp.fdsk = reinterpret_cast<const DevScanDisk *>(fs + h.fs.dsk);
    rp.fbox = reinterpret_cast<const DevScanBox *>(fs + h.fs.box);
    laps.lap(FLUX_CREATE_MS_UPLOAD);
    laps.ms[FLUX_CREATE_MS_TOTAL] = 0.0;
    for (int k = 1; k < FLUX_CREATE_TIMING_WORDS; k++) laps.ms[FLUX_CREATE_MS_TOTAL] += laps.ms[k];  // (the parts sum to the total by construction)
    for (int k = 0; k < FLUX_CREATE_TIMING_WORDS; k++) c->create_ms[k] = laps.ms[k];
    *out = c.release();
    return FLUX_OK;
}

// One per-triangle attribute of mesh m -- corner normals (V = double, flags = mesh_smooth) or corner colours (V = float, flags =
// mesh_colored) --, checked and converted by the caller; an empty `values` clears it.  The table where the context has none yet, the
// mesh's values staged in input order, and the device's own gather into leaf order, which leaves the other attribute alone.  Every
// allocation precedes the first change.  The table is freed when no mesh has either attribute any more.
template <class V>
int set_mesh_attribute(flux_ctx *ctx, size_t m, const std::vector<V> &values, std::vector<unsigned char> &flags,
                       hipError_t (*gather)(DevTri *, int, int, int, const V *, double *, hipStream_t)) {
    const bool set = !values.empty();
    const uint64_t own = ctx->mesh_first[m + 1] - ctx->mesh_first[m];
    if (!set && !flags[m]) return (int)FLUX_OK;  // (a mesh without triangles, or nothing to clear)
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(FLUX_E_DEVICE, "hipSetDevice(%d) failed", ctx->device);
    const size_t table_bytes = (size_t)ctx->rp.n_tris * kTriAttrDoubles * sizeof(double);
    DevBuf<double> fresh;
    DevBuf<V> stage;
    if (set && !ctx->d_tri_attrs) {
        HIP_TRY(fresh.alloc_bytes(table_bytes));
        HIP_TRY(hipMemset(fresh, 0, table_bytes));
    }
    if (set) {
        HIP_TRY(stage.alloc(values.size()));
        HIP_TRY(hipMemcpy(stage, values.data(), values.size() * sizeof(V), hipMemcpyHostToDevice));
    }
    double *table = fresh ? fresh : ctx->d_tri_attrs;
    HIP_TRY(gather(ctx->d_tris, ctx->rp.n_tris, ctx->rp.n_shapes + (int)ctx->mesh_first[m], (int)own, stage, table, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    if (fresh) {
        ctx->d_tri_attrs = std::move(fresh);
        ctx->device_bytes += table_bytes;
    }
    flags[m] = set ? 1 : 0;
    bool any = false;
    for (unsigned char f : ctx->mesh_smooth) any = any || f;
    for (unsigned char f : ctx->mesh_colored) any = any || f;
    if (!any && ctx->d_tri_attrs) {  // the last attribute of the last mesh went: the context is as it was created
        ctx->d_tri_attrs.reset();
        ctx->device_bytes -= table_bytes;
    }
    ctx->rp.tri_attrs = ctx->d_tri_attrs;
    return (int)FLUX_OK;
}

// flux_ctx_set_mesh_normals and flux_ctx_set_mesh_colors: the checks and the conversion (flux_mesh_attr.h) before any device call;
// then set_mesh_attribute
template <class V>
int convert_and_set_mesh_attribute(flux_ctx *ctx, uint64_t mesh, const double *corners, uint64_t num_triangles,
                                   bool (*convert)(const std::vector<uint64_t> &, uint64_t, const double *, uint64_t, std::vector<V> &, std::string &),
                                   std::vector<unsigned char> flux_ctx::*flags,
                                   hipError_t (*gather)(DevTri *, int, int, int, const V *, double *, hipStream_t)) {
    if (!ctx) return fail(FLUX_E_INVALID, "null context");
    return no_throw([&] {
        std::vector<V> values;
        std::string error;
        if (!convert(ctx->mesh_first, mesh, corners, num_triangles, values, error)) return fail(FLUX_E_INVALID, "%s", error.c_str());
        return set_mesh_attribute(ctx, (size_t)mesh, values, ctx->*flags, gather);
    });
}

}  // namespace flux

extern "C" {

int flux_ctx_create(const flux_scene_desc *scene, const flux_job_cfg *cfg, uint64_t seed, int device,
                    flux_ctx **out) {
    return flux_ctx_create_sets(scene, cfg, seed, device, 0, 1, out);
}

// validation (before the device check: a CPU-only machine still reports a bad job as such) -> device check -> host build -> upload
int flux_ctx_create_sets(const flux_scene_desc *scene, const flux_job_cfg *cfg, uint64_t seed, int device,
                         uint64_t first_set, uint64_t set_stride, flux_ctx **out) {
    if (!scene || !cfg || !out) return fail(FLUX_E_INVALID, "flux_ctx_create: null argument");
    *out = nullptr;
    flux::CreateLaps laps;
    if (int rc = flux::validate_job(*scene, *cfg, first_set, set_stride)) return rc;
    laps.lap(FLUX_CREATE_MS_HOST);
    if (int rc = flux::check_device(device)) return rc;
    laps.lap(FLUX_CREATE_MS_RUNTIME);
    return flux::no_throw([&] {
        flux::HostScene host;
        if (int rc = flux::build_host(*scene, host)) return rc;
        laps.lap(FLUX_CREATE_MS_HOST);
        return flux::upload(host, *cfg, seed, device, first_set, set_stride, laps, out);
    });
}

static bool holds_all_sets(const flux_ctx *c) { return c->sets.stride == 1 && c->sets.first == 0; }

// The arithmetic a render really runs with.  FLUX_MATH_FAST is defined for scenes whose surface normals are unit vectors (every
// sphere; a plane stored with a unit normal): there its closed-form bounce weights and its front-to-back throughput product
// are the reference's values to rounding.  A plane stored with a NON-unit normal (RenderParams::glossy_long) makes reflected
// directions non-unit, Phong lobes under- / overflow, and the reference's recursion L = (f (*) L) * s (materials.rs:31-33,
// 69-71) then meets its zeros and infinities in an order no reordered product reproduces (a 240 000-scene soak: three
// pixels' channels finite in FAST where the reference holds NaN).  Such a scene is rendered with the
// STRICT arithmetic, whatever flux_ctx_set_math says: the reference's own operation order, identical in every soak scene.
// ... unless STRICT cannot run the job at all: it keeps 32 B of recursion stack per level and lane in LDS (one wave per block
// holds 31 levels beside nothing else), FAST keeps none.  A FAST job deeper than that, on such a scene, stays with FAST and its
// long-form glossy weights (RenderParams::glossy_long; what every FAST render of such a scene was before round 4: the
// reference's NaN pixels in all but the rarest orderings of an overflow and a zero) instead of being refused.
// (a function of the JOB alone -- max_trace_depth and the mesh's BVH depth --, not of flux_ctx_set_traversal: the arithmetic a scene
// is rendered with must not flip with a test hook; a brute-force traversal leaves the BVH stack's bytes unused)
static bool strict_fits_lds(const flux_ctx *ctx) {
    // (the smallest block the planner can choose: one wave; launch_plan.cpp plan_render)
    return flux::lane_stacks_lds(FLUX_MATH_STRICT, ctx->D, ctx->rp.n_tris > 0, (size_t)ctx->bvh.max_depth, 64) + 512 <= 64 * 1024;
}
static int effective_math(const flux_ctx *ctx) {
    return (ctx->math == FLUX_MATH_FAST && ctx->rp.glossy_long && strict_fits_lds(ctx)) ? FLUX_MATH_STRICT : ctx->math;
}

// LDS one block of the kernel about to be launched needs: asked of the launch plan itself (launch_plan.cpp plan_render:
// STRICT keeps the (f,s) recursion stack, 4 doubles per level per lane; mesh scenes the BVH traversal stack, one int per
// level per lane -- 64 lanes in the FAST state-machine kernel, the block's in the others --; the split kernel its path
// queues), plus the few static words of the refill / split kernels.  64 KiB per block is the launch limit.
using flux::Pass;  // (an adaptive pass is checked as kPassMoments: the same LDS, and no work list to size it by yet)
static int check_lds_budget(const flux_ctx *ctx, const flux::RenderParams &p, const char *what, Pass pass = flux::kPassRender) {
    const size_t dyn = flux::plan_pass(pass, p, ctx->variant, effective_math(ctx)).lds;
    const size_t fixed = 512;
    if (dyn + fixed > 64 * 1024)
        return fail(FLUX_E_INVALID, "%s: %zu B of LDS per block (max_trace_depth %u%s, BVH depth %llu) exceed the 64 KiB limit; use %s", what,
                    dyn + fixed, ctx->D,
                    effective_math(ctx) == FLUX_MATH_STRICT ? " in the STRICT arithmetic: 32 B of recursion stack per level and lane" : "",
                    (unsigned long long)(p.bvh_stack > 0 ? ctx->bvh.max_depth : 0),
                    // (a FAST context only gets here in FAST: the routing to STRICT is dropped where STRICT does not fit)
                    ctx->math == FLUX_MATH_STRICT ? "FLUX_MATH_FAST or a smaller max_trace_depth" : "a smaller max_trace_depth");
    return FLUX_OK;
}
// flux_debug_shade: 64-thread blocks, STRICT recursion stack + per-lane BVH stack (launch_plan.cpp shade_rays_lds)
static int check_lds_budget_rays(const flux_ctx *ctx, const flux::RenderParams &p) {
    const size_t lds = flux::shade_rays_lds(p, effective_math(ctx));
    if (lds > 64 * 1024) return fail(FLUX_E_INVALID, "flux_debug_shade: %zu B of LDS per block exceed the 64 KiB limit", lds);
    return FLUX_OK;
}

int flux_ctx_set_kernel(flux_ctx *ctx, int variant) {
    if (!ctx) return fail(FLUX_E_INVALID, "null context");
    if (variant < FLUX_KERNEL_DEFAULT || variant > FLUX_KERNEL_SPLIT)
        return fail(FLUX_E_INVALID, "unknown kernel variant %d", variant);
    ctx->variant = variant;
    return FLUX_OK;
}

int flux_ctx_set_math(flux_ctx *ctx, int mode) {
    if (!ctx) return fail(FLUX_E_INVALID, "null context");
    if (mode != FLUX_MATH_FAST && mode != FLUX_MATH_STRICT) return fail(FLUX_E_INVALID, "unknown math mode %d", mode);
    ctx->math = mode;
    return FLUX_OK;
}

static flux::RenderParams apply_traversal(const flux_ctx *ctx, flux::RenderParams p) {  // flux_ctx_set_traversal, for renders and flux_debug_shade alike
    if (ctx->traversal == FLUX_TRAVERSE_BRUTE) p.bvh_stack = 0;
    if (ctx->traversal == FLUX_TRAVERSE_BVH_BINARY) p.nodes4 = nullptr;
    return p;
}

int flux_debug_shade(flux_ctx *ctx, uint64_t n, const double *rays, uint64_t depth, uint64_t set_index,
                     uint64_t sample_index, double *out_rgb, int32_t *out_hit, double *out_t) {
    if (!ctx || !rays || !out_rgb) return fail(FLUX_E_INVALID, "null argument");
    if (n == 0) return FLUX_OK;
    if (n > (1u << 24)) return fail(FLUX_E_INVALID, "too many rays");
    if (!holds_all_sets(ctx)) return fail(FLUX_E_INVALID, "this context holds a share of the sample sets only (flux_ctx_create_sets)");
    if (depth < 1 || set_index >= ctx->S || sample_index >= ctx->N)
        return fail(FLUX_E_INVALID, "depth >= 1, set_index < %u and sample_index < %u required", ctx->S, ctx->N);
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(FLUX_E_DEVICE, "hipSetDevice(%d) failed", ctx->device);
    flux::DevBuf<double> d_rays, d_rgb, d_t;
    flux::DevBuf<int> d_hit;
    hipError_t e = d_rays.alloc((size_t)n * 6);
    if (e == hipSuccess) e = d_rgb.alloc((size_t)n * 3);
    if (e == hipSuccess) e = d_t.alloc((size_t)n);
    if (e == hipSuccess) e = d_hit.alloc((size_t)n);
    if (e == hipSuccess) e = hipMemcpy(d_rays, rays, (size_t)n * 6 * sizeof(double), hipMemcpyHostToDevice);
    flux::RenderParams p = apply_traversal(ctx, ctx->rp);
    p.glossy_long = 1;  // caller-supplied directions need not be unit vectors
    p.unit_dirs = 0;
    p.self_skip = 0;
    p.env_short = 0;
    if (int rc = check_lds_budget_rays(ctx, p)) return rc;
    if (e == hipSuccess)
        e = flux::launch_shade_rays(p, effective_math(ctx), d_rays, (int)n, (int)depth, (uint32_t)set_index, (uint32_t)sample_index,
                                    d_rgb, d_hit, d_t, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out_rgb, d_rgb, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && out_hit) e = hipMemcpy(out_hit, d_hit, (size_t)n * sizeof(int), hipMemcpyDeviceToHost);
    if (e == hipSuccess && out_t) e = hipMemcpy(out_t, d_t, (size_t)n * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(FLUX_E_DEVICE, "debug shade: %s", hipGetErrorString(e));
    return FLUX_OK;
}

int flux_sampler_grid(int device, int kind, uint64_t sample_root, uint64_t seed, double *out_xy, double *out_hemi) {
    if (!out_xy) return fail(FLUX_E_INVALID, "null output");
    if (kind < FLUX_SAMPLER_REGULAR || kind > FLUX_SAMPLER_CORRELATED_MULTI_JITTERED)
        return fail(FLUX_E_INVALID, "unknown sampler kind %d", kind);
    if (sample_root < 1 || sample_root > 4096) return fail(FLUX_E_INVALID, "sample_root must be in [1, 4096]");
    if (int rc = flux::require_device(device)) return rc;
    DeviceGuard guard(device);
    const size_t N = (size_t)sample_root * sample_root;
    flux::DevBuf<double> dxy, dh;
    hipError_t e = dxy.alloc(N * 2);
    if (e == hipSuccess && out_hemi) e = dh.alloc(N * 3);
    if (e == hipSuccess) e = flux::generate_sampler_grid(kind, seed, (uint32_t)sample_root, dxy, dh, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out_xy, dxy, N * 2 * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && out_hemi) e = hipMemcpy(out_hemi, dh, N * 3 * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(FLUX_E_DEVICE, "sampler grid: %s", hipGetErrorString(e));
    return FLUX_OK;
}

int flux_debug_fastmath(int device, int fn, const double *a, const double *b, double *out, uint64_t n) {
    if (!a || !out) return fail(FLUX_E_INVALID, "null argument");
    if (fn < 0 || fn > 9) return fail(FLUX_E_INVALID, "unknown function %d", fn);
    if (int rc = flux::require_device(device)) return rc;
    DeviceGuard guard(device);
    if (n == 0) return FLUX_OK;
    flux::DevBuf<double> da, db, dout;
    const size_t bytes = (size_t)n * sizeof(double);
    hipError_t e = da.alloc((size_t)n);
    if (e == hipSuccess) e = dout.alloc((size_t)n);
    if (e == hipSuccess && b) e = db.alloc((size_t)n);
    if (e == hipSuccess) e = hipMemcpy(da, a, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && b) e = hipMemcpy(db, b, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = flux::launch_fastmath_probe(fn, da, db, dout, (size_t)n, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(FLUX_E_DEVICE, "fastmath probe: %s", hipGetErrorString(e));
    return FLUX_OK;
}

int flux_debug_plane_div(int device, const double *num, const double *den, double *out_unscaled, double *out_quotient, int32_t *out_admit,
                         uint64_t n) {
    if (!num || !den || !out_unscaled || !out_quotient || !out_admit) return fail(FLUX_E_INVALID, "null argument");
    if (int rc = flux::require_device(device)) return rc;
    DeviceGuard guard(device);
    if (n == 0) return FLUX_OK;
    flux::DevBuf<double> dn, dd, du, dq;
    flux::DevBuf<int32_t> da;
    const size_t bytes = (size_t)n * sizeof(double);
    hipError_t e = dn.alloc((size_t)n);
    if (e == hipSuccess) e = dd.alloc((size_t)n);
    if (e == hipSuccess) e = du.alloc((size_t)n);
    if (e == hipSuccess) e = dq.alloc((size_t)n);
    if (e == hipSuccess) e = da.alloc((size_t)n);
    if (e == hipSuccess) e = hipMemcpy(dn, num, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dd, den, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = flux::launch_plane_div_probe(dn, dd, du, dq, da, (size_t)n, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out_unscaled, du, bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_quotient, dq, bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_admit, da, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(FLUX_E_DEVICE, "plane division probe: %s", hipGetErrorString(e));
    return FLUX_OK;
}

// The work fields of a launch: ONE place per entry point, shared by the render call and flux_ctx_launch_plan.
static flux::RenderParams apply_context(const flux_ctx *ctx, flux::RenderParams p) {
    p.stats = ctx->stats_on ? ctx->d_stats : nullptr;
    return apply_traversal(ctx, p);
}
static flux::RenderParams rows_params(const flux_ctx *ctx, uint64_t first_row, uint64_t row_stride, uint64_t num_rows, double *out) {
    flux::RenderParams p = ctx->rp;
    p.out = out;
    p.first_row = (int32_t)first_row;
    p.row_stride = (int32_t)row_stride;
    p.num_rows = (int32_t)num_rows;
    return apply_context(ctx, p);
}
static flux::RenderParams sets_params(const flux_ctx *ctx, uint64_t first_set, uint64_t set_stride, uint64_t num_sets, double *out) {
    flux::RenderParams p = ctx->rp;
    p.out = out;
    p.first_row = 0;
    p.row_stride = 1;
    p.num_rows = (int32_t)ctx->H;
    p.set_first = (int32_t)first_set;
    p.set_stride = (int32_t)set_stride;
    p.set_count = (int32_t)num_sets;
    p.out_by_set = 1;
    p.slot_first = (int32_t)((first_set - ctx->sets.first) / ctx->sets.stride);
    p.slot_stride = (int32_t)(set_stride / ctx->sets.stride);
    return apply_context(ctx, p);
}

int flux_ctx_launch_plan(flux_ctx *ctx, uint64_t num_rows, uint64_t num_sets, int64_t out[FLUX_PLAN_WORDS]) {
    if (!ctx || !out) return fail(FLUX_E_INVALID, "null argument");
    if (num_rows > ctx->H) return fail(FLUX_E_INVALID, "%llu rows exceed image height %u", (unsigned long long)num_rows, ctx->H);
    flux::RenderParams p;
    if (num_sets == 0) {
        p = rows_params(ctx, 0, 1, num_rows, nullptr);
    } else {
        const uint64_t held = ctx->sets.count;
        if (num_sets > held) return fail(FLUX_E_INVALID, "%llu sets exceed the %llu this context holds", (unsigned long long)num_sets,
                                         (unsigned long long)held);
        p = sets_params(ctx, ctx->sets.first, ctx->sets.stride, num_sets, nullptr);
    }
    const flux::LaunchPlan L = flux::plan_render(p, ctx->variant, effective_math(ctx));
    out[0] = L.kernel;
    out[1] = L.block;
    out[2] = (int64_t)L.blocks;
    out[3] = (int64_t)L.lds;
    out[4] = L.waves_per_pixel;
    out[5] = effective_math(ctx);
    // why the arithmetic is not the requested one, or why it SHOULD not be: a FAST job on a scene with a non-unit plane normal
    out[6] = (ctx->math == FLUX_MATH_FAST && ctx->rp.glossy_long) ? (strict_fits_lds(ctx) ? FLUX_ROUTE_TO_STRICT : FLUX_ROUTE_KEPT_FAST)
                                                                 : FLUX_ROUTE_NONE;
    out[7] = (int64_t)flux::plan_flags(p, L);
    return FLUX_OK;
}

// the launch of the render calls, of the feature-buffer calls and of the moments calls (`pass`), between the context's two events
// (flux_ctx_last_kernel_ms); `what` names the caller in the LDS refusal
// (`launch(math)`: the pass's launch in that arithmetic -- launch_pass for the passes RenderParams describes whole, a launcher of its
// own for one that takes a further argument)
extern "C++" template <class Launch>
static int launch_timed_by(flux_ctx *ctx, const flux::RenderParams &p, const char *what, hipStream_t stream, Pass pass, Launch &&launch) {
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(FLUX_E_DEVICE, "hipSetDevice(%d) failed", ctx->device);
    if (int rc = check_lds_budget(ctx, p, what, pass)) return rc;
    HIP_TRY(hipEventRecord(ctx->ev0, stream));
    HIP_TRY(launch(effective_math(ctx)));
    HIP_TRY(hipEventRecord(ctx->ev1, stream));
    ctx->timed = true;
    return FLUX_OK;
}
static int launch_timed(flux_ctx *ctx, const flux::RenderParams &p, const char *what, hipStream_t stream, Pass pass = flux::kPassRender) {
    return launch_timed_by(ctx, p, what, stream, pass, [&](int math) { return flux::launch_pass(pass, p, ctx->variant, math, stream); });
}

// Every row uses every sample set (trace.rs:64-69): the refusal of a context that holds a share of them, in the caller's words
static int check_all_sets(const flux_ctx *ctx, const char *who_needs, const char *instead) {
    if (holds_all_sets(ctx)) return FLUX_OK;
    return fail(FLUX_E_INVALID, "%s all sample sets; this context holds the share %u + k*%u (flux_ctx_create_sets)%s", who_needs,
                ctx->sets.first, ctx->sets.stride, instead);
}
// The checks the device row calls share, in the order they fire: no rows are in order before the output pointer is looked at (the
// caller then returns), then the pointer, the stride, the share of the sets -- for the calls that name `who_needs`; the moments and
// adaptive calls have refused a share before they get here --, and the rows.
static int check_rows_call(const flux_ctx *ctx, uint64_t first_row, uint64_t row_stride, uint64_t num_rows, const void *out,
                           const char *who_needs = nullptr, const char *instead = nullptr) {
    if (num_rows == 0) return FLUX_OK;
    if (!out) return fail(FLUX_E_INVALID, "null output pointer");
    if (row_stride < 1) return fail(FLUX_E_INVALID, "row_stride must be >= 1");
    if (who_needs)
        if (int rc = check_all_sets(ctx, who_needs, instead)) return rc;
    if (first_row >= ctx->H || first_row + (num_rows - 1) * row_stride >= ctx->H)
        return fail(FLUX_E_INVALID, "rows %llu + k*%llu (k<%llu) exceed image height %u",
                    (unsigned long long)first_row, (unsigned long long)row_stride,
                    (unsigned long long)num_rows, ctx->H);
    return FLUX_OK;
}
// ... and what a per-pixel pass launches behind them: rows_params with the statistics off -- these kernels keep none
static int launch_pass_rows(flux_ctx *ctx, uint64_t first_row, uint64_t row_stride, uint64_t num_rows, void *d_out, const char *what,
                            void *hip_stream, Pass pass) {
    flux::RenderParams p = rows_params(ctx, first_row, row_stride, num_rows, (double *)d_out);
    p.stats = nullptr;
    return launch_timed(ctx, p, what, (hipStream_t)hip_stream, pass);
}

int flux_render_rows_device(flux_ctx *ctx, uint64_t first_row, uint64_t row_stride, uint64_t num_rows,
                            void *d_out_rgb, void *hip_stream) {
    if (!ctx) return fail(FLUX_E_INVALID, "null context");
    if (int rc = check_rows_call(ctx, first_row, row_stride, num_rows, d_out_rgb, "rendering rows needs", ": use flux_render_sets_device")) return rc;
    if (num_rows == 0) return FLUX_OK;
    return launch_timed(ctx, rows_params(ctx, first_row, row_stride, num_rows, (double *)d_out_rgb), "flux_render_rows", (hipStream_t)hip_stream);
}

int flux_render_sets_device(flux_ctx *ctx, uint64_t first_set, uint64_t set_stride, uint64_t num_sets, void *d_out_rgb,
                            void *hip_stream) {
    if (!ctx) return fail(FLUX_E_INVALID, "null context");
    if (num_sets == 0) return FLUX_OK;
    if (!d_out_rgb) return fail(FLUX_E_INVALID, "null output pointer");
    if (set_stride < 1) return fail(FLUX_E_INVALID, "set_stride must be >= 1");
    if (first_set >= ctx->S || first_set + (num_sets - 1) * set_stride >= ctx->S)
        return fail(FLUX_E_INVALID, "sets %llu + k*%llu (k<%llu) exceed the %u sample sets", (unsigned long long)first_set,
                    (unsigned long long)set_stride, (unsigned long long)num_sets, ctx->S);
    if (ctx->N < 64 || ctx->variant == FLUX_KERNEL_STATIC)
        return fail(FLUX_E_INVALID, "set-sharded rendering needs the refill kernel (sample_root^2 >= 64)");
    // every requested set must have its tables here: first_set + m*set_stride = sets.first + (slot_first + m*slot_stride)*sets.stride
    if (first_set < ctx->sets.first || (first_set - ctx->sets.first) % ctx->sets.stride != 0 ||
        (num_sets > 1 && set_stride % ctx->sets.stride != 0))
        return fail(FLUX_E_INVALID, "sets %llu + k*%llu are not all among this context's share %u + k*%u (flux_ctx_create_sets)",
                    (unsigned long long)first_set, (unsigned long long)set_stride, ctx->sets.first, ctx->sets.stride);
    return launch_timed(ctx, sets_params(ctx, first_set, set_stride, num_sets, (double *)d_out_rgb), "flux_render_sets_device", (hipStream_t)hip_stream);
}

// The host entry points' rows: [row_start, row_end] within the image (`unit`: the caller's word in front of "rows")
static int check_row_range(const flux_ctx *ctx, uint64_t row_start, uint64_t row_end, const char *unit) {
    if (row_end < row_start || row_end >= ctx->H)
        return fail(FLUX_E_INVALID, "%srows [%llu,%llu] outside image height %u", unit,
                    (unsigned long long)row_start, (unsigned long long)row_end, ctx->H);
    return FLUX_OK;
}
// ... and their path: the checks, the device made current, the call's own scratch grown to rows x W x channels doubles, the device
// entry point run on it, the result copied back.  (Each call has a scratch buffer of its own: none resizes or aliases another's.)
// (`device_entry`: a device entry point, or a callable with its arguments -- one that binds a further argument of its call)
extern "C++" template <class DeviceEntry>
static int rows_to_host(flux_ctx *ctx, uint64_t row_start, uint64_t row_end, const char *unit, flux::Scratch<double> flux_ctx::*scratch,
                        size_t channels, double *out, DeviceEntry &&device_entry) {
    if (!ctx) return fail(FLUX_E_INVALID, "null context");
    if (!out) return fail(FLUX_E_INVALID, "null output pointer");
    if (int rc = check_row_range(ctx, row_start, row_end, unit)) return rc;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(FLUX_E_DEVICE, "hipSetDevice(%d) failed", ctx->device);
    const uint64_t rows = row_end - row_start + 1;
    const size_t doubles = (size_t)rows * ctx->W * channels;
    flux::Scratch<double> &d_buf = ctx->*scratch;
    HIP_TRY(d_buf.reserve(doubles));
    if (int rc = device_entry(ctx, row_start, 1, rows, d_buf, nullptr)) return rc;
    HIP_TRY(hipMemcpy(out, d_buf, doubles * sizeof(double), hipMemcpyDeviceToHost));
    return FLUX_OK;
}

int flux_render_rows(flux_ctx *ctx, uint64_t row_start, uint64_t row_end, double *out_rgb) {
    return rows_to_host(ctx, row_start, row_end, "work unit ", &flux_ctx::d_out, 3, out_rgb, flux_render_rows_device);
}

// The feature buffers (aov_body.inc)
int flux_render_aov_rows_device(flux_ctx *ctx, uint64_t first_row, uint64_t row_stride, uint64_t num_rows, void *d_out,
                                void *hip_stream) {
    if (!ctx) return fail(FLUX_E_INVALID, "null context");
    if (int rc = check_rows_call(ctx, first_row, row_stride, num_rows, d_out, "feature buffers need", ", which no feature-buffer call serves")) return rc;
    if (num_rows == 0) return FLUX_OK;
    return launch_pass_rows(ctx, first_row, row_stride, num_rows, d_out, "flux_render_aov_rows", hip_stream, flux::kPassAov);
}

int flux_render_aov_rows(flux_ctx *ctx, uint64_t row_start, uint64_t row_end, double *out) {
    return rows_to_host(ctx, row_start, row_end, "", &flux_ctx::d_aov, FLUX_AOV_CHANNELS, out, flux_render_aov_rows_device);
}

// The per-pixel sample moments (moments_body.inc): a share of the sets is refused first, and one more thing -- a single sample has
// no variance.
int flux_render_moments_rows_device(flux_ctx *ctx, uint64_t first_row, uint64_t row_stride, uint64_t num_rows, void *d_out,
                                    void *hip_stream) {
    if (!ctx) return fail(FLUX_E_INVALID, "null context");
    if (int rc = check_all_sets(ctx, "sample moments need", ", which no moments call serves")) return rc;
    if (ctx->N < 2)
        return fail(FLUX_E_INVALID, "sample moments need sample_root >= 2: one sample per pixel has no variance; flux_denoise "
                    "estimates the variance from the frame itself");
    if (int rc = check_rows_call(ctx, first_row, row_stride, num_rows, d_out)) return rc;
    if (num_rows == 0) return FLUX_OK;
    return launch_pass_rows(ctx, first_row, row_stride, num_rows, d_out, "flux_render_moments_rows", hip_stream, flux::kPassMoments);
}

int flux_render_moments_rows(flux_ctx *ctx, uint64_t row_start, uint64_t row_end, double *out) {
    return rows_to_host(ctx, row_start, row_end, "", &flux_ctx::d_moments, FLUX_MOMENT_CHANNELS, out, flux_render_moments_rows_device);
}

// The feature buffers at the first non-specular hit (aov_chain_body.inc).  The checks that need no context come
// first, each with its own message: the context and a max_chain no job can reach here, the output pointer, the stride and the order
// of the host entry's rows in the entry points.
static int check_chain_call(const char *what, const flux_ctx *ctx, uint32_t max_chain) {
    if (!ctx) return fail(FLUX_E_INVALID, "%s: null context", what);
    if (max_chain > 256) return fail(FLUX_E_INVALID, "%s: max_chain %u exceeds 256, the largest max_trace_depth of any job", what, max_chain);
    return FLUX_OK;
}
// ... then the ones that read it: a share of the sets, and a chain deeper than the job traces -- the hemisphere table holds no u for
// such a segment, and the render never traces one
static int check_chain_ctx(const char *what, const flux_ctx *ctx, uint32_t max_chain) {
    if (int rc = check_all_sets(ctx, "chain feature buffers need", ", which no feature-buffer call serves")) return rc;
    if (max_chain > ctx->D)
        return fail(FLUX_E_INVALID, "%s: max_chain %u exceeds the job's max_trace_depth %u (0 means max_trace_depth)", what, max_chain, ctx->D);
    return FLUX_OK;
}

int flux_render_aov_chain_rows_device(flux_ctx *ctx, uint64_t first_row, uint64_t row_stride, uint64_t num_rows, uint32_t max_chain,
                                      void *d_out, void *hip_stream) {
    const char *what = "flux_render_aov_chain_rows_device";
    // (no rows are in order before the output pointer is looked at, as in the other row calls)
    if (int rc = check_chain_call(what, ctx, max_chain)) return rc;
    if (num_rows == 0) return FLUX_OK;
    if (!d_out) return fail(FLUX_E_INVALID, "%s: null output pointer", what);
    if (row_stride < 1) return fail(FLUX_E_INVALID, "%s: row_stride must be >= 1", what);
    if (int rc = check_chain_ctx(what, ctx, max_chain)) return rc;
    if (int rc = check_rows_call(ctx, first_row, row_stride, num_rows, d_out)) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    flux::RenderParams p = rows_params(ctx, first_row, row_stride, num_rows, (double *)d_out);
    p.stats = nullptr;
    const int limit = (int)(max_chain == 0 ? ctx->D : max_chain);
    return launch_timed_by(ctx, p, what, stream, flux::kPassAovChain,
                           [&](int math) { return flux::launch_aov_chain(p, limit, math, stream); });
}

// (a staging buffer of its own, d_aov_chain: no other call's scratch is resized or aliased)
int flux_render_aov_chain_rows(flux_ctx *ctx, uint64_t row_start, uint64_t row_end, uint32_t max_chain, double *out) {
    const char *what = "flux_render_aov_chain_rows";
    if (int rc = check_chain_call(what, ctx, max_chain)) return rc;
    if (!out) return fail(FLUX_E_INVALID, "%s: null output pointer", what);
    if (row_end < row_start)
        return fail(FLUX_E_INVALID, "%s: row_end %llu is below row_start %llu", what, (unsigned long long)row_end, (unsigned long long)row_start);
    return rows_to_host(ctx, row_start, row_end, "", &flux_ctx::d_aov_chain, FLUX_AOV_CHANNELS, out,
                        [max_chain](flux_ctx *c, uint64_t first_row, uint64_t row_stride, uint64_t num_rows, void *d_out, void *hip_stream) {
                            return flux_render_aov_chain_rows_device(c, first_row, row_stride, num_rows, max_chain, d_out, hip_stream);
                        });
}

// ---- adaptive sampling (adaptive_body.inc, adaptive.hip) -------------------------------------------------------
// The checks that need no context, each with a message of its own; nullptr for a null `params`.
static int check_adaptive_params(const char *what, const flux_adaptive_params *a) {
    if (!a) return fail(FLUX_E_INVALID, "%s: null params", what);
    if (!std::isfinite(a->threshold) || a->threshold < 0.0)
        return fail(FLUX_E_INVALID, "%s: threshold %g must be finite and >= 0", what, a->threshold);
    if (!std::isfinite(a->lum_floor) || !(a->lum_floor > 0.0))
        return fail(FLUX_E_INVALID, "%s: lum_floor %g must be finite and > 0", what, a->lum_floor);
    if (a->min_passes < 1) return fail(FLUX_E_INVALID, "%s: min_passes must be >= 1", what);
    if (a->max_passes < a->min_passes)
        return fail(FLUX_E_INVALID, "%s: max_passes %u is below min_passes %u", what, a->max_passes, a->min_passes);
    if (a->dilate > 2) return fail(FLUX_E_INVALID, "%s: dilate %u exceeds 2", what, a->dilate);
    if (a->reserved != 0) return fail(FLUX_E_INVALID, "%s: the reserved word must be 0", what);
    return FLUX_OK;
}
// ... and the ones that need the context but no device
static int check_adaptive_ctx(const char *what, const flux_ctx *ctx, const flux_adaptive_params *a) {
    if (!ctx) return fail(FLUX_E_INVALID, "%s: null context", what);
    if (int rc = check_all_sets(ctx, "adaptive sampling needs", ", which no adaptive call serves")) return rc;
    if (ctx->N < 2)
        return fail(FLUX_E_INVALID, "adaptive sampling needs sample_root >= 2: one sample per pass has no variance to decide by");
    if (a->max_passes > ctx->S)
        return fail(FLUX_E_INVALID, "%s: max_passes %u exceeds the %u sample sets: a pixel would read a set twice", what, a->max_passes,
                    ctx->S);
    return FLUX_OK;
}

// The rounds.  Rounds r < min_passes run over the identity list and need no selection; every later round
// first runs the selection and reads its 4-byte count back -- ONE hipStreamSynchronize per such round -- to size the pass and to
// stop at 0.  `info` costs one more synchronisation behind the finish kernel.  The context's two events span the call's launches.
int flux_render_adaptive_rows_device(flux_ctx *ctx, uint64_t first_row, uint64_t row_stride, uint64_t num_rows, void *params,
                                     void *d_out_moments, void *d_out_passes, uint64_t info[FLUX_ADAPTIVE_INFO_WORDS], void *hip_stream) {
    const char *what = "flux_render_adaptive_rows_device";
    const flux_adaptive_params *a = (const flux_adaptive_params *)params;
    if (int rc = check_adaptive_params(what, a)) return rc;
    if (int rc = check_adaptive_ctx(what, ctx, a)) return rc;
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    if (num_rows == 0) return FLUX_OK;
    if (!d_out_moments || !d_out_passes) return fail(FLUX_E_INVALID, "%s: null output pointer", what);
    if (int rc = check_rows_call(ctx, first_row, row_stride, num_rows, d_out_moments)) return rc;
    const uint64_t pixels = num_rows * ctx->W;
    if (pixels > 0x7fffffffull) return fail(FLUX_E_INVALID, "%s: %llu pixels exceed 2^31 - 1", what, (unsigned long long)pixels);
    hipStream_t stream = (hipStream_t)hip_stream;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(FLUX_E_DEVICE, "hipSetDevice(%d) failed", ctx->device);
    flux::RenderParams p = rows_params(ctx, first_row, row_stride, num_rows, nullptr);
    p.stats = nullptr;
    if (int rc = check_lds_budget(ctx, p, "flux_render_adaptive_rows", flux::kPassMoments)) return rc;
    HIP_TRY(ctx->d_adapt_pixels.grow((size_t)pixels, [&] {
        hipError_t e = ctx->d_adapt_sums.alloc((size_t)pixels * flux::kAdaptiveSums);
        if (e == hipSuccess) e = ctx->d_adapt_passes.alloc((size_t)pixels);
        if (e == hipSuccess) e = ctx->d_adapt_list.alloc((size_t)pixels);
        if (e == hipSuccess) e = ctx->d_adapt_hot.alloc((size_t)pixels);
        if (e == hipSuccess) e = ctx->d_adapt_counts.alloc(2);
        return e;
    }));
    const int math = effective_math(ctx);
    flux::AdaptiveWork work{};
    work.sums = ctx->d_adapt_sums;
    work.passes = ctx->d_adapt_passes;
    const flux::AdaptiveRule rule{a->threshold * a->threshold, a->lum_floor, ctx->N, a->dilate};
    uint32_t *d_active = ctx->d_adapt_counts, *d_reached = d_active + 1;

    HIP_TRY(hipEventRecord(ctx->ev0, stream));
    ctx->timed = false;
    uint64_t rounds = 0, traced = 0;
    for (uint32_t r = 0; r < a->max_passes; ++r) {
        if (r < a->min_passes) {
            work.list = nullptr;
            work.count = (uint32_t)pixels;
        } else {
            HIP_TRY(flux::launch_adaptive_select(rule, (uint32_t)num_rows, ctx->W, work.sums, work.passes, ctx->d_adapt_hot,
                                                 ctx->d_adapt_list, d_active, stream));
            uint32_t active = 0;
            HIP_TRY(hipMemcpyAsync(&active, d_active, sizeof(active), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (active == 0) break;
            if (active > pixels) return fail(FLUX_E_DEVICE, "%s: the selection counted %u of %llu pixels", what, active,
                                             (unsigned long long)pixels);
            work.list = ctx->d_adapt_list;
            work.count = active;
        }
        work.fresh = r == 0 ? 1u : 0u;  // (the first pass writes the state: nothing is cleared)
        HIP_TRY(flux::launch_adaptive(p, work, math, stream));
        rounds += 1;
        traced += work.count;
    }
    HIP_TRY(flux::launch_adaptive_finish(ctx->N, pixels, work.sums, work.passes, (double *)d_out_moments, (uint32_t *)d_out_passes, stream));
    if (info) HIP_TRY(flux::launch_adaptive_count(a->max_passes, pixels, work.passes, d_reached, stream));
    HIP_TRY(hipEventRecord(ctx->ev1, stream));
    ctx->timed = true;
    if (info) {
        uint32_t reached = 0;
        HIP_TRY(hipMemcpyAsync(&reached, d_reached, sizeof(reached), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        info[0] = rounds;
        info[1] = traced;
        info[2] = reached;
        info[3] = 0;
    }
    return FLUX_OK;
}

// (staging buffers of its own, d_adapt_out and d_adapt_map: no other call's scratch is resized or aliased)
int flux_render_adaptive_rows(flux_ctx *ctx, uint64_t row_start, uint64_t row_end, void *params, double *out_moments, void *out_passes,
                              uint64_t info[FLUX_ADAPTIVE_INFO_WORDS]) {
    const char *what = "flux_render_adaptive_rows";
    const flux_adaptive_params *a = (const flux_adaptive_params *)params;
    if (int rc = check_adaptive_params(what, a)) return rc;
    if (int rc = check_adaptive_ctx(what, ctx, a)) return rc;
    if (!out_moments || !out_passes) return fail(FLUX_E_INVALID, "%s: null output pointer", what);
    if (int rc = check_row_range(ctx, row_start, row_end, "")) return rc;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(FLUX_E_DEVICE, "hipSetDevice(%d) failed", ctx->device);
    const uint64_t rows = row_end - row_start + 1;
    const size_t pixels = (size_t)rows * ctx->W;
    HIP_TRY(ctx->d_adapt_out_pixels.grow(pixels, [&] {
        const hipError_t e = ctx->d_adapt_out.alloc(pixels * FLUX_MOMENT_CHANNELS);
        return e == hipSuccess ? ctx->d_adapt_map.alloc(pixels) : e;
    }));
    int rc = flux_render_adaptive_rows_device(ctx, row_start, 1, rows, params, ctx->d_adapt_out, ctx->d_adapt_map, info, nullptr);
    if (rc != FLUX_OK) return rc;
    HIP_TRY(hipMemcpy(out_moments, ctx->d_adapt_out, pixels * FLUX_MOMENT_CHANNELS * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_passes, ctx->d_adapt_map, pixels * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return FLUX_OK;
}

double flux_ctx_last_kernel_ms(flux_ctx *ctx) {
    if (!ctx || !ctx->timed) return -1.0;
    DeviceGuard guard(ctx->device);
    if (hipEventSynchronize(ctx->ev1) != hipSuccess) return -1.0;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) != hipSuccess) return -1.0;
    return (double)ms;
}

int flux_ctx_set_mesh_normals(flux_ctx *ctx, uint64_t mesh, const double *corner_normals, uint64_t num_triangles) {
    return flux::convert_and_set_mesh_attribute(ctx, mesh, corner_normals, num_triangles, flux::normalize_corner_normals, &flux_ctx::mesh_smooth, flux::gather_tri_normals);
}

int flux_ctx_set_mesh_colors(flux_ctx *ctx, uint64_t mesh, const double *corner_colors, uint64_t num_triangles) {
    return flux::convert_and_set_mesh_attribute(ctx, mesh, corner_colors, num_triangles, flux::round_corner_colors, &flux_ctx::mesh_colored, flux::gather_tri_colors);
}

int flux_ctx_enable_stats(flux_ctx *ctx, int on) {
    if (!ctx) return fail(FLUX_E_INVALID, "null context");
    ctx->stats_on = on != 0;
    return FLUX_OK;
}

int flux_ctx_set_traversal(flux_ctx *ctx, int mode) {
    if (!ctx) return fail(FLUX_E_INVALID, "null context");
    if (mode != FLUX_TRAVERSE_BVH && mode != FLUX_TRAVERSE_BRUTE && mode != FLUX_TRAVERSE_BVH_BINARY)
        return fail(FLUX_E_INVALID, "unknown traversal mode %d", mode);
    ctx->traversal = mode;
    return FLUX_OK;
}

int flux_ctx_bvh_info(flux_ctx *ctx, uint64_t *out, uint64_t out_words) {
    if (!ctx || !out) return fail(FLUX_E_INVALID, "null argument");
    uint64_t w[FLUX_BVH_INFO_WORDS] = {};
    w[0] = ctx->bvh.nodes;
    w[1] = ctx->bvh.tris;
    w[2] = ctx->bvh.max_depth;
    w[3] = ctx->bvh.max_leaf;
    w[4] = sizeof(flux::DevNode);
    w[5] = sizeof(flux::DevTri);
    w[6] = ctx->bvh.build_us;
    w[7] = ctx->bvh.wide_nodes;
    w[8] = ctx->bvh.leaf_records;
    w[9] = ctx->bvh.fused_leaves;
    w[10] = ctx->bvh.wide_stack;
    w[11] = sizeof(flux::DevNode4Q);
    w[12] = sizeof(flux::DevLeafRec);
    // [13]: asked of the launch planner (a full-frame render with the current variant, arithmetic and traversal)
    w[13] = flux::plan_render(rows_params(ctx, 0, 1, ctx->H, nullptr), ctx->variant, effective_math(ctx)).kernel == FLUX_PLAN_BVH4 ? 1 : 0;
    for (uint64_t k = 0; k < out_words && k < FLUX_BVH_INFO_WORDS; k++) out[k] = w[k];
    return FLUX_OK;
}

int flux_ctx_stats(flux_ctx *ctx, uint64_t out[FLUX_NUM_STATS], int reset) {
    if (!ctx || !out) return fail(FLUX_E_INVALID, "null argument");
    DeviceGuard guard(ctx->device);
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long tmp[FLUX_NUM_STATS];
    HIP_TRY(hipMemcpy(tmp, ctx->d_stats, sizeof(tmp), hipMemcpyDeviceToHost));
    for (int i = 0; i < FLUX_NUM_STATS; i++) out[i] = tmp[i];
    if (reset) HIP_TRY(hipMemset(ctx->d_stats, 0, sizeof(tmp)));
    return FLUX_OK;
}

int flux_ctx_copy_table(flux_ctx *ctx, int which, double *out, uint64_t out_doubles) {
    if (!ctx || !out) return fail(FLUX_E_INVALID, "null argument");
    DeviceGuard guard(ctx->device);
    const size_t SN = (size_t)ctx->sets.count * ctx->N;  // the sets held here, in slot order
    if (which == FLUX_TABLE_PIXEL || which == FLUX_TABLE_DISC) {
        if (out_doubles < SN * 2) return fail(FLUX_E_INVALID, "output too small: need %zu doubles", SN * 2);
        HIP_TRY(hipMemcpy(out, which == FLUX_TABLE_PIXEL ? ctx->d_pix : ctx->d_disc, SN * 2 * sizeof(double),
                          hipMemcpyDeviceToHost));
        return FLUX_OK;
    }
    if (which == FLUX_TABLE_HEMI) {
        const size_t total = SN * ctx->D * 3;
        if (out_doubles < total) return fail(FLUX_E_INVALID, "output too small: need %zu doubles", total);
        flux::DevBuf<double> tmp;
        HIP_TRY(tmp.alloc(total));
        hipError_t e = flux::hemi_to_aos((size_t)ctx->sets.count * ctx->D, ctx->N, ctx->d_hemi, tmp, nullptr);
        if (e == hipSuccess) e = hipMemcpy(out, tmp, total * sizeof(double), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(FLUX_E_DEVICE, "hemi copy: %s", hipGetErrorString(e));
        return FLUX_OK;
    }
    if (which == FLUX_TABLE_ORDER) {  // (sample indices, below 2^24: exact as doubles)
        if (out_doubles < SN) return fail(FLUX_E_INVALID, "output too small: need %zu doubles", SN);
        return flux::no_throw([&]() -> int {
            std::vector<uint32_t> tmp(SN);
            HIP_TRY(hipMemcpy(tmp.data(), ctx->d_order, SN * sizeof(uint32_t), hipMemcpyDeviceToHost));
            for (size_t k = 0; k < SN; k++) out[k] = (double)tmp[k];
            return FLUX_OK;
        });
    }
    return fail(FLUX_E_INVALID, "unknown table %d", which);
}

int flux_ctx_copy_row_perm(flux_ctx *ctx, uint64_t row, int32_t *out, uint64_t out_len) {
    if (!ctx || !out) return fail(FLUX_E_INVALID, "null argument");
    if (row >= ctx->H) return fail(FLUX_E_INVALID, "row %llu outside image height %u", (unsigned long long)row, ctx->H);
    if (out_len < ctx->S) return fail(FLUX_E_INVALID, "output too small: need %u entries", ctx->S);
    DeviceGuard guard(ctx->device);
    HIP_TRY(hipMemcpy(out, ctx->d_rowperm + (size_t)row * ctx->S, (size_t)ctx->S * sizeof(int32_t),
                      hipMemcpyDeviceToHost));
    return FLUX_OK;
}

int flux_ctx_camera_basis(flux_ctx *ctx, double uvw[9]) {
    if (!ctx || !uvw) return fail(FLUX_E_INVALID, "null argument");
    for (int i = 0; i < 3; i++) {
        uvw[i] = ctx->U[i];
        uvw[3 + i] = ctx->V[i];
        uvw[6 + i] = ctx->Wv[i];
    }
    return FLUX_OK;
}

uint64_t flux_ctx_device_bytes(flux_ctx *ctx) { return ctx ? ctx->device_bytes : 0; }

int flux_ctx_create_timing(flux_ctx *ctx, double out_ms[FLUX_CREATE_TIMING_WORDS]) {
    if (!ctx || !out_ms) return fail(FLUX_E_INVALID, "null argument");
    for (int k = 0; k < FLUX_CREATE_TIMING_WORDS; k++) out_ms[k] = ctx->create_ms[k];
    return FLUX_OK;
}

// ---- host-side pieces of the boundary ------------------------------------------

// Job::work_units: job.rs:65-88
int64_t flux_work_units(uint64_t image_height, uint64_t rows_per_work_unit, flux_work_unit *out, uint64_t cap) {
    if (rows_per_work_unit == 0)
        return fail(FLUX_E_INVALID, "Job row per work unit count invalid: 0");  // job.rs:67-70 panics
    if (image_height == 0) return fail(FLUX_E_INVALID, "image_height must be >= 1");
    int64_t count = 0;
    uint64_t i = 0;
    while (i < image_height - 1) {  // sic: job.rs:74
        uint64_t remaining = image_height - i;
        uint64_t rows = rows_per_work_unit < remaining ? rows_per_work_unit : remaining;
        if (out && (uint64_t)count < cap) {
            out[count].row_start = i;
            out[count].row_end = i + rows - 1;
        }
        count++;
        i += rows;
    }
    return count;
}

static unsigned quantize16(double c) {  // `(c * 65535.99) as u16`: image.rs:50-53 (saturating cast)
    double v = c * 65535.99;
    if (!(v > 0.0)) return 0;
    if (v >= 65535.0) return 65535;
    return (unsigned)v;
}

// Image::write: image.rs:43-61
int flux_write_ppm(const char *path, const double *rgb, uint64_t width, uint64_t height,
                   const uint8_t *rows_present) {
    if (!path || !rgb) return fail(FLUX_E_INVALID, "null argument");
    FILE *f = std::fopen(path, "w");
    if (!f) return fail(FLUX_E_IO, "cannot open %s for writing", path);
    std::vector<char> buf(1 << 20);
    std::setvbuf(f, buf.data(), _IOFBF, buf.size());
    std::fprintf(f, "P3\n%llu %llu\n65535\n", (unsigned long long)width, (unsigned long long)height);
    for (uint64_t r = 0; r < height; r++) {
        const bool present = rows_present ? rows_present[r] != 0 : true;
        for (uint64_t col = 0; col < width; col++) {
            if (present) {
                const double *p = rgb + (r * width + col) * 3;
                std::fprintf(f, "%u %u %u\n", quantize16(p[0]), quantize16(p[1]), quantize16(p[2]));
            } else {
                std::fputs("0 0 0\n", f);
            }
        }
    }
    int bad = std::ferror(f);
    if (std::fclose(f) != 0 || bad) return fail(FLUX_E_IO, "write to %s failed", path);
    return FLUX_OK;
}

}  // extern "C"
