// scene_build.cpp -- the host half of context creation (scene_build.h): Scene::from_data (scene.rs:128-154) and CameraBasis::new
// (scene.rs:28-35) in the records the kernels read, plus the extension's triangle records and BVH.
#include "scene_build.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "flux_switches.h"
#include "joining_thread.h"

namespace flux {

namespace {

void normalize3(const double in[3], double out[3]) {
    double len = std::sqrt(in[0] * in[0] + in[1] * in[1] + in[2] * in[2]);
    out[0] = in[0] / len;
    out[1] = in[1] / len;
    out[2] = in[2] / len;
}
void cross3(const double a[3], const double b[3], double o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// material_from_data (scene.rs:87-125) + the per-material constants of brdf.rs:30,45,76 / materials.rs:45
DevMaterial make_material(const flux_material &m) {
    DevMaterial dm{};
    dm.kind = m.kind;
    if (m.kind == FLUX_MAT_DIELECTRIC) {
        // the transmitted bounce's weight as given; the refraction index where a Glossy material keeps 1 / (exponent + 1)
        // (flux_device.h DevMaterial)
        dm.inv_e1 = m.k;
        dm.fr = m.color[0];
        dm.fg = m.color[1];
        dm.fb = m.color[2];
        return dm;
    }
    dm.exponent = m.exponent;
    dm.inv_e1 = 1.0 / (m.exponent + 1.0);
    // powf(negative, e): +|x|^e for an even integral e, -|x|^e for an odd one, NaN otherwise
    if (std::isfinite(m.exponent) && std::floor(m.exponent) == m.exponent)
        dm.exp_parity = (std::fabs(m.exponent) >= 9007199254740992.0 || std::fmod(m.exponent, 2.0) == 0.0) ? 1 : 2;
    double f[3];
    for (int ch = 0; ch < 3; ch++) {
        f[ch] = m.color[ch] * m.k;
        if (m.kind == FLUX_MAT_MATTE) f[ch] = f[ch] * kInvPi;  // brdf.rs:30
    }
    dm.fr = f[0];
    dm.fg = f[1];
    dm.fb = f[2];
    return dm;
}

// Sphere::new (shapes.rs:154-169); a plane or disk keeps its normal as given in c0; a box its corners where a sphere keeps its AABB's
DevShape make_shape(const flux_shape &s) {
    DevShape d{};
    d.kind = s.kind;
    d.px = s.p[0];
    d.py = s.p[1];
    d.pz = s.p[2];
    if (s.kind == FLUX_SHAPE_SPHERE) {
        d.radius = s.radius;
        d.rr = s.radius * s.radius;
        d.inv = s.invert ? -1.0 : 1.0;
        d.inv_rad = d.inv / s.radius;
        d.c0x = s.p[0] - s.radius;
        d.c0y = s.p[1] - s.radius;
        d.c0z = s.p[2] - s.radius;
        d.c1x = s.p[0] + s.radius;
        d.c1y = s.p[1] + s.radius;
        d.c1z = s.p[2] + s.radius;
    } else if (s.kind == FLUX_SHAPE_BOX) {
        d.px = d.py = d.pz = 0.0;
        d.c0x = s.p[0];
        d.c0y = s.p[1];
        d.c0z = s.p[2];
        d.c1x = s.n[0];
        d.c1y = s.n[1];
        d.c1z = s.n[2];
        d.inv = s.invert ? -1.0 : 1.0;
    } else {
        d.c0x = s.n[0];
        d.c0y = s.n[1];
        d.c0z = s.n[2];
        if (s.kind == FLUX_SHAPE_DISK) {
            d.radius = s.radius;
            d.rr = s.radius * s.radius;
        }
    }
    return d;
}

// the FAST hit record of shape i (flux_device.h DevHitRec)
DevHitRec make_hit_record(const DevShape &d, const DevMaterial &m, size_t i) {
    DevHitRec r{};
    // the FAST bounce weight: the product is the one the kernels formed per bounce, `fr * scale`
    const double wsc = m.kind == kMatMatte ? 1.0 / kInvPi : 1.0;
    r.fr = m.kind == kMatMatte ? m.fr * wsc : m.fr;
    r.fg = m.kind == kMatMatte ? m.fg * wsc : m.fg;
    r.fb = m.kind == kMatMatte ? m.fb * wsc : m.fb;
    r.inv_e1 = m.inv_e1;
    r.ax = m.kind == kMatMatte ? 0.0034 : 0.00424;  // brdf.rs:22 / brdf.rs:58
    r.az = m.kind == kMatMatte ? 0.0071 : 0.00764;
    r.shape_kind = d.kind;
    r.mat_kind = m.kind;
    r.orig_id = (int32_t)i;
    // spheres: |(hit - centre) / radius| = 1 to rounding; planes and disks use the stored normal as is (shapes.rs:135-152)
    r.unit_normal = d.kind == kShapeSphere || std::fabs((d.c0x * d.c0x + d.c0y * d.c0y + d.c0z * d.c0z) - 1.0) <= 4.0 * 2.220446049250313e-16;
    if (d.kind == kShapeSphere) {
        r.cx = d.px; r.cy = d.py; r.cz = d.pz; r.inv_rad = d.inv_rad;
    } else {
        r.cx = d.c0x; r.cy = d.c0y; r.cz = d.c0z;
    }
    return r;
}

template <class T> void put(std::vector<unsigned char> &image, size_t offset, const std::vector<T> &v) {
    if (!v.empty()) std::memcpy(image.data() + offset, v.data(), v.size() * sizeof(T));
}

// The FAST path's layout of the shapes (scan records + hit records in scan order: spheres, planes, disks; the f32 filter; STRICT's
// spheres in scan order; the primary ray's constants) in one image, and the RenderParams flags that follow from the shapes
void build_fast_scene(const flux_scene_desc &scene, HostScene &h) {
    RenderParams &rp = h.rp;
    const size_t ns = (size_t)scene.num_shapes;
    const uint32_t W = (uint32_t)scene.image_width, H = (uint32_t)scene.image_height;
    std::vector<DevScanSphere> fsph;
    std::vector<DevScanPlane> fpln;
    std::vector<DevScanDisk> fdsk;
    std::vector<DevScanBox> fbox;
    std::vector<DevHitRec> frec_s, frec_p, frec_d, frec_b;
    // STRICT's sphere records in SCAN order (its scan takes its candidates from the same f32 filter, whose bit k is scan sphere
    // k): the DevShape as it is, with the YAML index -- the tie rule's key -- in pad0
    std::vector<DevShape> sshapes;
    for (size_t i = 0; i < ns; i++) {
        const DevShape &d = h.shapes[i];
        const DevHitRec r = make_hit_record(d, h.mats[i], i);
        if (d.kind == kShapeSphere) {
            fsph.push_back(DevScanSphere{d.px, d.py, d.pz, d.rr});
            frec_s.push_back(r);
            sshapes.push_back(d);
            sshapes.back().pad0 = (int32_t)i;
        } else if (d.kind == kShapeDisk) {
            DevScanDisk dk{};
            dk.px = d.px; dk.py = d.py; dk.pz = d.pz; dk.nx = d.c0x; dk.ny = d.c0y; dk.nz = d.c0z; dk.id = (int32_t)i; dk.rr = d.rr;
            fdsk.push_back(dk);
            frec_d.push_back(r);
        } else if (d.kind == kShapeBox) {
            DevScanBox bx{};
            bx.c0x = d.c0x; bx.c0y = d.c0y; bx.c0z = d.c0z; bx.c1x = d.c1x; bx.c1y = d.c1y; bx.c1z = d.c1z; bx.id = (int32_t)i; bx.inv = d.inv;
            fbox.push_back(bx);
            // six plane records, one per face: 2 axis + (1: the outward normal is +e_axis), the normal negated for `invert`
            for (int face = 0; face < 6; face++) {
                DevHitRec f = r;
                f.shape_kind = kShapePlane;
                f.unit_normal = 1;
                f.cx = f.cy = f.cz = 0.0;
                (face / 2 == 0 ? f.cx : face / 2 == 1 ? f.cy : f.cz) = ((face & 1) ? 1.0 : -1.0) * d.inv;
                frec_b.push_back(f);
            }
        } else {
            DevScanPlane pl{};
            pl.px = d.px; pl.py = d.py; pl.pz = d.pz; pl.nx = d.c0x; pl.ny = d.c0y; pl.nz = d.c0z; pl.id = (int32_t)i;
            fpln.push_back(pl);
            frec_p.push_back(r);
        }
    }
    // f32 records of the conservative candidate filter (flux_device.h DevScanSphere32): valid while every magnitude stays far
    // inside f32's range (squares are formed), else the f64 filter is used
    h.filter32 = true;
    for (const DevScanSphere &sp : fsph) {
        const double pp = sp.px * sp.px + sp.py * sp.py + sp.pz * sp.pz;
        if (!(pp < 1e30) || !(sp.rr < 1e30)) h.filter32 = false;
    }
    // `invert` spheres (environments: nearly every ray is inside and hits them) are tested for all lanes together with scalar
    // operands instead of through every lane's candidate list (render_body.inc scan_shapes_fast): up to two, given a filter
    // record that never passes (c = 3e38: "entirely behind the origin" or dq < 0)
    if (h.filter32)
        for (size_t k = 0; k < fsph.size() && rp.n_uni < FLUX_UNI_SPHERES; k++)
            if (frec_s[k].inv_rad < 0.0) rp.uni_idx[rp.n_uni++] = (int)k;
    std::vector<DevScanSphere32> fsph32((fsph.size() + 1) / 2, DevScanSphere32{});
    for (size_t k = 0; k < fsph.size(); k++) {
        const DevScanSphere &sp = fsph[k];
        const double pp = sp.px * sp.px + sp.py * sp.py + sp.pz * sp.pz;
        const double ppr = (pp - sp.rr) - 8e-6 * (pp + sp.rr) - 1e-30;
        float f = (float)ppr;
        if ((double)f > ppr) f = std::nextafterf(f, -INFINITY);  // rounded down: the bias is never reduced
        DevScanSphere32 &d = fsph32[k / 2];
        d.px[k & 1] = -(float)sp.px;  // the NEGATED centre (flux_device.h DevScanSphere32)
        d.py[k & 1] = -(float)sp.py;
        d.pz[k & 1] = -(float)sp.pz;
        d.ppr[k & 1] = f;
        if ((rp.n_uni > 0 && rp.uni_idx[0] == (int)k) || (rp.n_uni > 1 && rp.uni_idx[1] == (int)k)) {
            d.px[k & 1] = d.py[k & 1] = d.pz[k & 1] = 0.0f;
            d.ppr[k & 1] = 3.0e38f;
        }
    }

    h.fs = fscene_layout(fsph.size(), fpln.size(), fdsk.size(), fbox.size(), ns, W, H);
    h.fscene.assign(h.fs.bytes, 0);
    put(h.fscene, h.fs.sph, fsph);
    put(h.fscene, h.fs.pln, fpln);
    put(h.fscene, h.fs.rec, frec_s);
    put(h.fscene, h.fs.rec + frec_s.size() * sizeof(DevHitRec), frec_p);
    put(h.fscene, h.fs.rec + (frec_s.size() + frec_p.size()) * sizeof(DevHitRec), frec_d);
    put(h.fscene, h.fs.s32, fsph32);
    put(h.fscene, h.fs.ss, sshapes);
    put(h.fscene, h.fs.rec + (frec_s.size() + frec_p.size() + frec_d.size()) * sizeof(DevHitRec), frec_b);
    put(h.fscene, h.fs.dsk, fdsk);
    put(h.fscene, h.fs.box, fbox);
    // The split kernel's per-pixel constants of the primary ray (trace.rs:56-57, 93-94) as two tables a wave reads with scalar loads
    // in its ray-generation step: x - half_w for every column, (H - row) - half_h for every row -- the same two IEEE operations the
    // kernels perform, done once here
    double *pxc = reinterpret_cast<double *>(h.fscene.data() + h.fs.pxc);
    const double half_w = (double)W * 0.5, half_h = (double)H * 0.5;
    for (uint32_t x = 0; x < W; x++) pxc[x] = (double)(int32_t)x - half_w;
    for (uint32_t y = 0; y < H; y++) pxc[W + y] = (double)((int32_t)H - (int32_t)y) - half_h;

    rp.n_sph = (int32_t)fsph.size();
    rp.n_pln = (int32_t)fpln.size();
    // the first scan plane's axis, from the normal and the point as stored (flux_plane_axis.h); the camera's side: build_host_scene
    rp.plane_axis = fpln.empty() ? kPlaneAxisNone : plane_axis_of(fpln[0].nx, fpln[0].ny, fpln[0].nz, fpln[0].px, fpln[0].py, fpln[0].pz);
    if (rp.plane_axis != kPlaneAxisNone) {
        // ... and the axis component of its point, which the reduced arms' division needs of ordinary size (plane_div_point_ok)
        const double pa = rp.plane_axis == kPlaneAxisX ? fpln[0].px : rp.plane_axis == kPlaneAxisY ? fpln[0].py : fpln[0].pz;
        if (!plane_div_point_ok(pa)) rp.plane_axis = kPlaneAxisNone;
    }
    rp.n_dsk = (int32_t)fdsk.size();
    rp.n_box = (int32_t)fbox.size();
    // The glossy lobe's angle table (RenderParams::glossx): a slot for every distinct 1 / (exponent + 1) among the glossy records --
    // compared as bit patterns, collected in YAML order -- while at most kGlossExpSlots of them occur; each glossy record's byte offset
    // into a sample's entries (16 B a slot), in scan order as the records.  A scene with more exponents gets no table.
    std::vector<const DevHitRec *> frec_all;
    for (const auto *v : {&frec_s, &frec_p, &frec_d, &frec_b})
        for (const DevHitRec &hr : *v) frec_all.push_back(&hr);
    auto same_bits = [](double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; };
    auto slot_of = [&](double v) {
        size_t k = 0;
        while (k < h.gx_inv_e1.size() && !same_bits(h.gx_inv_e1[k], v)) k++;
        return k;
    };
    {
        std::vector<const DevHitRec *> yaml(frec_all);
        std::sort(yaml.begin(), yaml.end(), [](const DevHitRec *a, const DevHitRec *b) { return a->orig_id < b->orig_id; });
        for (const DevHitRec *hr : yaml)
            if (hr->mat_kind == kMatGlossy && h.gx_inv_e1.size() <= (size_t)kGlossExpSlots && slot_of(hr->inv_e1) == h.gx_inv_e1.size())
                h.gx_inv_e1.push_back(hr->inv_e1);
    }
    rp.n_gloss_exp = (int32_t)h.gx_inv_e1.size();
    h.gx_off.assign(frec_all.size() + 1, 0);  // (+1 as the records themselves, FsceneLayout::rec: never empty, so the upload has bytes to copy)
    for (const DevHitRec &hr : frec_p)
        if (!hr.unit_normal) rp.glossy_long = 1;
    for (const DevHitRec &hr : frec_d)  // a disk's normal is a plane's: the same rule
        if (!hr.unit_normal) rp.glossy_long = 1;
    rp.unit_dirs = rp.glossy_long ? 0 : 1;
    rp.self_skip = rp.glossy_long ? 0 : 1;
    // (a glossy_long scene takes the long-form weights, outside the kernels the table serves)
    if (rp.n_gloss_exp >= 1 && rp.n_gloss_exp <= kGlossExpSlots && !rp.glossy_long) {
        rp.gx_stride = 16 * rp.n_gloss_exp;
        for (size_t k = 0; k < frec_all.size(); k++)
            if (frec_all[k]->mat_kind == kMatGlossy) h.gx_off[k] = 16 * (int32_t)slot_of(frec_all[k]->inv_e1);
    }
    for (const DevScanSphere &sp : fsph)
        if (!(std::fabs(sp.px) < 1e3 && std::fabs(sp.py) < 1e3 && std::fabs(sp.pz) < 1e3 && sp.rr < 1e6)) rp.self_skip = 0;
    // the environment shortcut (flux_device.h env_short): exactly one `invert` sphere, Emissive, of ordinary size
    const int inverted = (int)std::count_if(frec_s.begin(), frec_s.end(), [](const DevHitRec &hr) { return hr.inv_rad < 0.0; });
    if (rp.n_uni == 1 && inverted == 1 && frec_s[rp.uni_idx[0]].mat_kind == kMatEmissive) {
        const double rad = std::sqrt(fsph[rp.uni_idx[0]].rr);
        if (rad > 1e-3 && rad < 1e6) {
            rp.env_short = 1;
            rp.env_radius = rad * (1.0 + 1e-12);  // never below the true radius: it bounds the exit distance from above
        }
    }
    rp.t_min = kTMin;
    rp.env_deep = -(4.0 * kTMin) * rp.env_radius;  // (the kernels' own expression, evaluated once)
    rp.env_eps = 1e-9;
    if (rp.n_uni == 1) {
        const DevScanSphere &es = fsph[rp.uni_idx[0]];
        rp.env_px = es.px; rp.env_py = es.py; rp.env_pz = es.pz; rp.env_rr = es.rr;
        rp.env32 = env_sphere32(es.px, es.py, es.pz, es.rr, rp.env_deep);  // ... and in f32, for the verdict in front of the shortcut
    }
    // the filter's group walk for at most 32 spheres (render_body.inc sphere_filter32: the same arithmetic, done once), as pair
    // indices into fsph32 that the upload turns into pointers
    rp.f32_valid = fsph.size() >= 32 ? 0xffffffffu : (1u << fsph.size()) - 1u;
    if (h.filter32 && fsph.size() <= 32) {
        int pairs = ((int)fsph.size() + 1) >> 1;
        const int rem = pairs & 3;
        if (rem == 1 || rem == 2) {
            h.f32_half = pairs - rem;
            pairs -= rem;
        } else if (rem == 3) {
            pairs += 1;  // its fourth pair is padding (zeros)
        }
        rp.f32_groups = pairs / 4;
        h.f32_top = pairs;
    }
}

}  // namespace

size_t lobe_frame_table(const HostScene &h, std::vector<unsigned char> &has_entry) {
    has_entry.clear();
    const size_t n_rec = (size_t)hit_records(h.rp);
    if (switch_off(kEnvLobeFrames) || n_rec == 0) return 0;
    const DevHitRec *rec = reinterpret_cast<const DevHitRec *>(h.fscene.data() + h.fs.rec);
    has_entry.resize(n_rec);
    for (size_t k = 0; k < n_rec; k++) has_entry[k] = rec[k].shape_kind != kShapeSphere;
    return n_rec * kLobeFrameBytes;
}

void build_tput_table(const HostScene &h, int bits, int max_depth, std::vector<double> &out) {
    const DevHitRec *rec = reinterpret_cast<const DevHitRec *>(h.fscene.data() + h.fs.rec);
    const uint32_t n_rec = (uint32_t)hit_records(h.rp);
    out.assign(((size_t)2 << (bits * (max_depth - 1))) * 3, 0.0);
    // lists of one entry: the first bounce's weight as it stands ...
    for (uint32_t e = 0; e < n_rec; e++) {
        double *t = &out[(size_t)tput_index((uint32_t)bits, e) * 3];
        t[0] = rec[e].fr; t[1] = rec[e].fg; t[2] = rec[e].fb;
    }
    // ... and a list of n entries: the product of its first n - 1, times its last one's weight (one IEEE multiplication per channel
    // and bounce, front to back, as the kernel's loop).  Only lists of records the scene has are visited: n_rec^n of the 2^(n bits).
    std::vector<uint32_t> heads(n_rec), lists;
    for (uint32_t e = 0; e < n_rec; e++) heads[e] = e;
    for (int n = 2; n < max_depth; n++) {
        const uint32_t head_bits = (uint32_t)(bits * (n - 1));
        lists.clear();
        lists.reserve(heads.size() * n_rec);
        for (uint32_t e = 0; e < n_rec; e++)
            for (const uint32_t head : heads) {
                const uint32_t ml = head | (e << head_bits);
                const double *a = &out[(size_t)tput_index(head_bits, head) * 3];
                double *t = &out[(size_t)tput_index(head_bits + (uint32_t)bits, ml) * 3];
                t[0] = a[0] * rec[e].fr; t[1] = a[1] * rec[e].fg; t[2] = a[2] * rec[e].fb;
                lists.push_back(ml);
            }
        heads.swap(lists);
    }
}

bool tput_products_finite(const HostScene &h, int bits, int max_depth, const std::vector<double> &table) {
    const size_t entries = (size_t)2 << (bits * (max_depth - 1));
    if (max_depth < 2 || table.size() != entries * 3) return false;
    for (const double v : table)
        if (!std::isfinite(v)) return false;
    const DevHitRec *rec = reinterpret_cast<const DevHitRec *>(h.fscene.data() + h.fs.rec);
    const uint32_t n_rec = (uint32_t)hit_records(h.rp);
    double top[3] = {0.0, 0.0, 0.0}, weight[3] = {0.0, 0.0, 0.0};
    for (size_t at = entries / 2; at < entries; at++)  // the lists of max_depth - 1 entries (tput_index: the table's upper half)
        for (int ch = 0; ch < 3; ch++) top[ch] = std::max(top[ch], std::fabs(table[at * 3 + ch]));
    for (uint32_t e = 0; e < n_rec; e++) {
        const double f[3] = {rec[e].fr, rec[e].fg, rec[e].fb};
        for (int ch = 0; ch < 3; ch++) weight[ch] = std::max(weight[ch], std::fabs(f[ch]));
    }
    return std::isfinite(top[0] * weight[0]) && std::isfinite(top[1] * weight[1]) && std::isfinite(top[2] * weight[2]);
}

namespace {
// The extension's meshes: one triangle record per triangle (hit order: after all shapes), the binary BVH, its quantised nodes and the
// 4-wide arena
int build_meshes(const flux_scene_desc &scene, HostScene &h, std::string &error) {
    const size_t ns = (size_t)scene.num_shapes;
    std::vector<size_t> first((size_t)scene.num_meshes + 1, 0);
    for (size_t m = 0; m < (size_t)scene.num_meshes; m++) first[m + 1] = first[m] + (size_t)scene.meshes[m].num_triangles;
    // the traversal addresses node and triangle records by 32-bit byte offsets from their bases (render_body.inc)
    if ((uint64_t)first.back() * sizeof(DevTri) >= (1ull << 32)) {
        char buf[160];
        std::snprintf(buf, sizeof(buf), "%zu triangles exceed the %llu a context can hold", first.back(),
                      (unsigned long long)((1ull << 32) / sizeof(DevTri)));
        error = buf;
        return FLUX_E_INVALID;
    }
    h.mesh_first.assign(first.begin(), first.end());
    h.tris.assign(first.back(), DevTri{});
    // edges and the geometric normal (a square root and three divisions each).  A million of them take tens of milliseconds on
    // one core, so large meshes are dealt to threads by index range (FLUX_BUILD_THREADS, as for the BVH)
    auto make = [&](size_t lo, size_t hi) {
        size_t m = 0;
        for (size_t g = lo; g < hi; g++) {
            while (g >= first[m + 1]) m++;
            const flux_mesh &me = scene.meshes[m];
            const size_t k = g - first[m];
            const double *a = me.vertices + 3 * (size_t)me.indices[3 * k];
            const double *b = me.vertices + 3 * (size_t)me.indices[3 * k + 1];
            const double *d = me.vertices + 3 * (size_t)me.indices[3 * k + 2];
            DevTri &t = h.tris[g];
            t.v0x = a[0]; t.v0y = a[1]; t.v0z = a[2];
            t.e1x = b[0] - a[0]; t.e1y = b[1] - a[1]; t.e1z = b[2] - a[2];
            t.e2x = d[0] - a[0]; t.e2y = d[1] - a[1]; t.e2z = d[2] - a[2];
            const double e1[3] = {t.e1x, t.e1y, t.e1z}, e2[3] = {t.e2x, t.e2y, t.e2z};
            double nn[3], nu[3] = {0.0, 0.0, 0.0};
            cross3(e1, e2, nn);
            if (nn[0] == 0.0 && nn[1] == 0.0 && nn[2] == 0.0) {
                // a triangle whose e1 x e2 is exactly zero (repeated or exactly collinear vertices) has no surface:
                // clearing the edges makes Moeller-Trumbore's det exactly 0, so it is never hit (and never NaN)
                t.e1x = t.e1y = t.e1z = t.e2x = t.e2y = t.e2z = 0.0;
            } else {
                normalize3(nn, nu);
            }
            t.nx = nu[0]; t.ny = nu[1]; t.nz = nu[2];
            t.id = (int32_t)(ns + g);
            t.mat = (int32_t)(ns + m);
        }
    };
    const unsigned threads = build_threads();
    const size_t n = h.tris.size();
    if (threads > 1 && n >= 65536) {
        std::vector<JoiningThread> pool;
        for (unsigned t = 0; t < threads; t++) {
            const size_t lo = n * t / threads, hi = n * (t + 1) / threads;
            pool.emplace_back([&make, lo, hi] { make(lo, hi); });
        }
    } else {
        make(0, n);
    }

    build_bvh(h.tris, h.nodes, h.bvh);
    if (!quantize_bvh(h.nodes, h.nodesq, h.bvh)) {
        error = "BVH quantisation lost containment (mesh coordinates beyond the 16-bit grid's reach)";
        return FLUX_E_INVALID;
    }
    // nodes and leaf records in ONE arena of 64-B units, a node's children contiguous (flux_bvh.h DevNode4A); an arena beyond the
    // 26-bit unit index comes back empty and the mesh is walked by the binary tree's kernel
    build_wide_arena(h.nodes, h.nodesq, h.tris, h.arena, h.bvh);
    if (h.bvh.max_depth > (uint64_t)kBvhMaxDepth) {
        char buf[160];
        std::snprintf(buf, sizeof(buf), "BVH depth %llu exceeds %d (degenerate mesh)", (unsigned long long)h.bvh.max_depth, kBvhMaxDepth);
        error = buf;
        return FLUX_E_INVALID;
    }
    RenderParams &rp = h.rp;
    rp.n_tris = (int32_t)h.tris.size();
    rp.bvh_stack = (int32_t)h.bvh.max_depth;
    rp.bvh4_stack = (int32_t)h.bvh.wide_stack;
    rp.bvh_mag = h.bvh.mag;
    for (int a = 0; a < 3; a++) {
        rp.bvh_qmin[a] = h.bvh.qmin[a];
        rp.bvh_qstep[a] = h.bvh.qstep[a];
    }
    return FLUX_OK;
}

// CameraBasis::new (scene.rs:28-35) and the camera's part of RenderParams (trace.rs:44-60)
void build_camera(const flux_scene_desc &scene, HostScene &h) {
    const double em[3] = {scene.eye[0] - scene.look_at[0], scene.eye[1] - scene.look_at[1], scene.eye[2] - scene.look_at[2]};
    double upxw[3];
    normalize3(em, h.W);
    cross3(scene.up, h.W, upxw);
    normalize3(upxw, h.U);
    cross3(h.W, h.U, h.V);
    RenderParams &rp = h.rp;
    rp.ex = scene.eye[0];
    rp.ey = scene.eye[1];
    rp.ez = scene.eye[2];
    rp.Ux = h.U[0]; rp.Uy = h.U[1]; rp.Uz = h.U[2];
    rp.Vx = h.V[0]; rp.Vy = h.V[1]; rp.Vz = h.V[2];
    rp.Wx = h.W[0]; rp.Wy = h.W[1]; rp.Wz = h.W[2];
    rp.aps = scene.pixel_size / scene.zoom_factor;                 // trace.rs:60
    rp.half_w = (double)scene.image_width * 0.5;                   // trace.rs:57
    rp.half_h = (double)scene.image_height * 0.5;                  // trace.rs:56
    rp.factor = scene.focal_distance / scene.view_plane_distance;  // trace.rs:45
    rp.focal = scene.focal_distance;
    rp.lens_radius = scene.lens_radius;
    rp.fwx = rp.focal * rp.Wx;  // trace.rs:96-98's focal_distance * w, one product per frame instead of per wave
    rp.fwy = rp.focal * rp.Wy;
    rp.fwz = rp.focal * rp.Wz;
    rp.bgr = scene.background[0];
    rp.bgg = scene.background[1];
    rp.bgb = scene.background[2];
}

}  // namespace

FsceneLayout fscene_layout(size_t n_sph, size_t n_pln, size_t n_dsk, size_t n_box, size_t n_shapes, uint32_t W, uint32_t H) {
    auto align128 = [](size_t x) { return (x + 127) & ~(size_t)127; };
    FsceneLayout f;
    f.sph = 0;
    f.pln = f.sph + (n_sph + 1) * sizeof(DevScanSphere);
    f.rec = f.pln + (n_pln + 1) * sizeof(DevScanPlane);
    f.s32 = f.rec + (n_shapes + 5 * n_box + 1) * sizeof(DevHitRec);  // (a box has six records)
    f.ss = align128(f.s32 + ((n_sph + 1) / 2 + 4) * sizeof(DevScanSphere32));
    f.pxc = align128(f.ss + (n_sph + 1) * sizeof(DevShape));
    f.dsk = align128(f.pxc + ((size_t)W + H) * sizeof(double));
    f.box = f.dsk + (n_dsk + 1) * sizeof(DevScanDisk);  // (no spare record: a scene without boxes keeps the bytes it had)
    f.bytes = f.box + n_box * sizeof(DevScanBox);
    return f;
}

int build_host_scene(const flux_scene_desc &scene, HostScene &h, std::string &error) {
    h = HostScene();
    const size_t ns = (size_t)scene.num_shapes, nm = (size_t)scene.num_meshes;
    h.shapes.assign(ns ? ns : 1, DevShape{});
    h.mats.assign(ns + nm + 1, DevMaterial{});
    for (size_t i = 0; i < ns; i++) {
        h.shapes[i] = make_shape(scene.shapes[i]);
        h.mats[i] = make_material(scene.shapes[i].material);
    }
    for (size_t m = 0; m < nm; m++) h.mats[ns + m] = make_material(scene.meshes[m].material);
    // behind the materials: their bounce weights {f * (n.wi)/pdf in FAST's closed form: f / INV_PI for Matte, f otherwise; pad} of
    // 32 B each (render_bvh4_kernel keeps a path's material indices and multiplies the weights when the path ends)
    h.wtab.assign(h.mats.size() * 4, 0.0);
    for (size_t k = 0; k < h.mats.size(); k++) {
        const double sc = h.mats[k].kind == kMatMatte ? 1.0 / kInvPi : 1.0;
        h.wtab[4 * k] = h.mats[k].fr * sc;
        h.wtab[4 * k + 1] = h.mats[k].fg * sc;
        h.wtab[4 * k + 2] = h.mats[k].fb * sc;
    }
    RenderParams &rp = h.rp;
    rp.img_w = (int32_t)scene.image_width;
    rp.img_h = (int32_t)scene.image_height;
    rp.num_sets = (uint32_t)scene.image_width;  // workers.rs:50: num_sets = image_width
    rp.n_shapes = (int32_t)ns;
    rp.n_mats = (int32_t)h.mats.size();
    rp.mat_bits = 1;
    while ((size_t)1 << rp.mat_bits < h.mats.size()) rp.mat_bits++;
    for (const DevMaterial &m : h.mats)
        if (m.kind == kMatDielectric) rp.has_diel = 1;
    // a launch narrows these; by default it covers every set
    rp.set_stride = 1;
    rp.set_count = (int32_t)rp.num_sets;
    rp.slot_stride = 1;

    build_fast_scene(scene, h);
    build_camera(scene, h);
    {   // the reduced first-plane test's word on primary rays rests on these (flux_plane_axis.h plane_axis_camera_ok)
        const double cam[] = {rp.ex, rp.ey, rp.ez, rp.Ux, rp.Uy, rp.Uz, rp.Vx, rp.Vy, rp.Vz, rp.Wx, rp.Wy, rp.Wz, rp.aps,
                              rp.half_w, rp.half_h, rp.factor, rp.focal, rp.lens_radius, rp.fwx, rp.fwy, rp.fwz};
        if (!plane_axis_camera_ok(cam, (int)(sizeof(cam) / sizeof(cam[0])))) rp.plane_axis = kPlaneAxisNone;
    }
    return build_meshes(scene, h, error);
}

}  // namespace flux
