// scene_build.h -- the host half of context creation: everything a context's scene buffers and RenderParams hold that depends on
// the scene alone, built once on the host (abi.hip uploads it to one device, multi.hip to each of its devices).  Plain C++: no HIP
// call and no device, so a CPU-only test can build and inspect it (tests/scene_build_selftest.cpp).
#pragma once
#include <cstddef>
#include <string>
#include <vector>

#include "../../include/flux_abi.h"
#include "flux_device.h"
#include "flux_plan.h"

namespace flux {

// Where each region of the FAST scene image starts, in bytes from its base.  fscene_layout() computes it once; the host build
// fills the image by it and the upload points RenderParams::fsph .. fbox into the device copy by it.
struct FsceneLayout {
    size_t sph = 0;    // DevScanSphere[n_sph + 1] (+1: the scan reads one record ahead)
    size_t pln = 0;    // DevScanPlane[n_pln + 1]
    size_t rec = 0;    // DevHitRec[n_shapes + 5 n_box + 1]: spheres, planes, disks, six per box
    size_t s32 = 0;    // DevScanSphere32[(n_sph + 1) / 2 + 4] (+4 pairs: the filter loads whole groups of 8 spheres)
    size_t ss = 0;     // DevShape[n_sph + 1], 128-B aligned: STRICT's spheres in scan order
    size_t pxc = 0;    // double[W + H], 128-B aligned: the primary ray's per-column and per-row constants
    size_t dsk = 0;    // DevScanDisk[n_dsk + 1], 128-B aligned
    size_t box = 0;    // DevScanBox[n_box], behind the disks
    size_t bytes = 0;  // the whole image
};
FsceneLayout fscene_layout(size_t n_sph, size_t n_pln, size_t n_dsk, size_t n_box, size_t n_shapes, uint32_t W, uint32_t H);

struct HostScene {
    std::vector<DevShape> shapes;   // one record at least
    std::vector<DevMaterial> mats;  // the shapes', then the meshes', then one unused record
    std::vector<double> wtab;       // behind the materials on the device: per material {its FAST bounce weight; 0}
    FsceneLayout fs;
    std::vector<unsigned char> fscene;
    // meshes (all empty without triangles)
    std::vector<DevTri> tris;
    std::vector<DevNode> nodes;
    std::vector<DevNodeQ> nodesq;
    std::vector<DevNode4A> arena;  // empty when the arena exceeds its 26-bit unit index: the binary tree's kernel walks the mesh
    BvhInfo bvh;
    std::vector<uint64_t> mesh_first;  // [meshes + 1]: mesh m holds the triangles mesh_first[m] .. mesh_first[m + 1] - 1 of the input order
    double U[3] = {}, V[3] = {}, W[3] = {};  // CameraBasis::new (scene.rs:28-35)
    // every field of RenderParams the scene decides.  The pointers stay null here; the upload sets them, f32_half and f32_top from
    // the pair indices below.
    RenderParams rp{};
    bool filter32 = false;  // fsph32 is usable (else RenderParams::fsph32 and f32_top are null)
    int f32_half = -1;      // RenderParams::f32_half = fsph32 + f32_half, null when -1
    int f32_top = 0;        // RenderParams::f32_top = fsph32 + f32_top
    // The glossy lobe's angle table (RenderParams::glossx).  gx_inv_e1: the distinct 1 / (exponent + 1) bit patterns of the
    // GlossyReflective hit records, in YAML order, at most kGlossExpSlots + 1 of them (rp.n_gloss_exp = its size; one more than the
    // cap means "too many": no table).  gx_off: per hit record, in scan order as the records, 16 * its value's index there -- all
    // zeros, and rp.gx_stride 0, for a scene that gets no table.
    std::vector<double> gx_inv_e1;
    std::vector<int32_t> gx_off;
};

// `scene` as validate_job (abi.hip) passed it.  Returns FLUX_OK, or FLUX_E_INVALID with the message in `error` (too many triangles
// for a context, or a mesh the BVH cannot hold).  Host allocation failures and thread creation throw.
int build_host_scene(const flux_scene_desc &scene, HostScene &out, std::string &error);

// The throughput product table (flux_plan.h tput_index, RenderParams::tput) of the scene's hit records for lists of `bits` bits per
// entry and 1 .. max_depth - 1 entries: 2 << bits * (max_depth - 1) entries of (r, g, b).  Entry (n, ml) is
// ((R[e0].f * R[e1].f) * ...) * R[e(n-1)].f per channel -- plain IEEE products in the order of the split kernel's loop, so bit for
// bit its result; entries whose list names a record the scene does not have stay zero.
void build_tput_table(const HostScene &h, int bits, int max_depth, std::vector<double> &out);
// Whether every throughput a path of this job can hold is finite (RenderParams::tput_finite): every entry of `table` -- the scene's,
// as build_tput_table made it for `bits` and `max_depth` -- and the product of every longest list's entry with one more record's
// weight, the throughput of the bounce at the depth limit.  The last is bounded, not enumerated: per channel, the largest magnitude
// among the longest lists' entries times the largest weight's; a product of smaller magnitudes rounds to no larger a value.
bool tput_products_finite(const HostScene &h, int bits, int max_depth, const std::vector<double> &table);

// The lobe-frame table (RenderParams::lobe_frame) of the scene: which hit records get an entry -- has_entry[k] = 1 for every record
// whose shape stores its normal (a plane, a disk, a box face), 0 for a sphere, in scan order as the records -- and the table's size in
// bytes, kLobeFrameBytes a record, entries or not.  0 and an empty list: no table (a scene without hit records, or FLUX_LOBE_FRAMES=0
// in the environment: tests and A/B runs).  The entries themselves are the device's work (render.hip generate_lobe_frame_table).
size_t lobe_frame_table(const HostScene &h, std::vector<unsigned char> &has_entry);

}  // namespace flux
