// The glossy lobe's angle table (RenderParams::glossx) seen from inside the library (tests/test_gpu_sample_tables.py builds and runs
// it against the internal headers; nothing here crosses the C ABI).
//   usage: sample_tables_selftest cpu | gpu
// cpu: the host scene build's slot assignment -- distinct 1 / (exponent + 1) bit patterns in YAML order, duplicates sharing a slot,
//      the cap of kGlossExpSlots, no table for a scene with a non-unit plane normal --, and the size of DevHitRec.  No HIP call.
// gpu: which contexts hold the table (one, three and five exponents, exponent 0, FLUX_SAMPLE_TABLES=0), what its entries are, and
//      that a set-share context's rows are the full context's rows of the same sets, bit for bit.
// Prints one "ok <name>" per passed check and "all ok" at the end; exits 1 on the first failure.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../flux_amd/csrc/flux_ctx.h"

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                  \
        }                                                              \
    } while (0)

namespace {

flux_material matte() {
    flux_material m{};
    m.kind = FLUX_MAT_MATTE;
    m.color[0] = 0.7; m.color[1] = 0.6; m.color[2] = 0.5;
    m.k = 0.8;
    return m;
}
flux_material glossy(double exponent) {
    flux_material m{};
    m.kind = FLUX_MAT_GLOSSY;
    m.color[0] = 0.9; m.color[1] = 0.8; m.color[2] = 0.9;
    m.k = 0.7;
    m.exponent = exponent;
    return m;
}
flux_material emissive() {
    flux_material m{};
    m.kind = FLUX_MAT_EMISSIVE;
    m.color[0] = m.color[1] = m.color[2] = 1.0;
    m.k = 1.5;
    return m;
}
flux_shape sphere(double x, double y, double z, double r, const flux_material &m, bool invert = false) {
    flux_shape s{};
    s.kind = FLUX_SHAPE_SPHERE;
    s.invert = invert ? 1 : 0;
    s.p[0] = x; s.p[1] = y; s.p[2] = z;
    s.radius = r;
    s.material = m;
    return s;
}
flux_shape plane(double y, double ny, const flux_material &m) {
    flux_shape s{};
    s.kind = FLUX_SHAPE_PLANE;
    s.p[1] = y;
    s.n[1] = ny;
    s.material = m;
    return s;
}

struct Scene {
    std::vector<flux_shape> shapes;
    flux_scene_desc desc{};
    const flux_scene_desc &get(uint64_t w = 9, uint64_t h = 4) {
        desc.scene_name = "sample_tables";
        desc.image_width = w;
        desc.image_height = h;
        desc.pixel_size = 1.0;
        desc.eye[1] = 2.0; desc.eye[2] = -10.0;
        desc.look_at[1] = 1.0;
        desc.up[1] = 1.0;
        desc.zoom_factor = 1.0;
        desc.view_plane_distance = 10.0;
        desc.focal_distance = 10.0;
        desc.lens_radius = 0.1;
        desc.num_shapes = shapes.size();
        desc.shapes = shapes.data();
        return desc;
    }
};

// an environment, then one glossy sphere or plane per exponent in the order given (a negative entry: a Matte sphere in between)
Scene scene_of(const std::vector<double> &exponents, bool glossy_plane_first = false, double plane_ny = 1.0) {
    Scene s;
    s.shapes.push_back(sphere(0, 0, 0, 100.0, emissive(), true));
    if (glossy_plane_first) s.shapes.push_back(plane(-0.5, plane_ny, glossy(exponents.back())));
    for (size_t k = 0; k < exponents.size(); k++)
        s.shapes.push_back(sphere(-3.0 + 1.5 * (double)k, 0.5, 2.0, 0.6, exponents[k] < 0.0 ? matte() : glossy(exponents[k])));
    if (!glossy_plane_first) s.shapes.push_back(plane(-0.5, plane_ny, matte()));
    return s;
}

int build(Scene &s, flux::HostScene &h) {
    std::string err;
    return flux::build_host_scene(s.get(), h, err);
}

// gx_off of the hit record of YAML shape `id` (the records are in scan order: spheres, planes, disks)
int32_t off_of_shape(const flux::HostScene &h, int id) {
    const flux::DevHitRec *rec = reinterpret_cast<const flux::DevHitRec *>(h.fscene.data() + h.fs.rec);
    for (int k = 0; k < h.rp.n_sph + h.rp.n_pln + h.rp.n_dsk; k++)
        if (rec[k].orig_id == id) return h.gx_off[(size_t)k];
    return -1;
}

int cpu() {
    static_assert(sizeof(flux::DevHitRec) == 96, "the hit queue's slot count and the 16 KiB rule depend on it");
    CHECK(sizeof(flux::DevHitRec) == 96 && sizeof(flux::DevSetRows) == 64 && flux::kGlossExpSlots == 4);
    std::printf("ok record sizes\n");
    flux::HostScene h;
    {   // no glossy record at all: nothing to tabulate
        Scene s = scene_of({-1.0, -1.0});
        CHECK(build(s, h) == FLUX_OK);
        CHECK(h.rp.n_gloss_exp == 0 && h.rp.gx_stride == 0 && h.gx_inv_e1.empty());
        std::printf("ok no glossy record\n");
    }
    {   // one exponent, used twice
        Scene s = scene_of({100.0, -1.0, 100.0});
        CHECK(build(s, h) == FLUX_OK);
        CHECK(h.rp.n_gloss_exp == 1 && h.rp.gx_stride == 16 && h.gx_inv_e1.size() == 1 && h.gx_inv_e1[0] == 1.0 / 101.0);
        CHECK(off_of_shape(h, 1) == 0 && off_of_shape(h, 2) == 0 && off_of_shape(h, 3) == 0);
        std::printf("ok one exponent\n");
    }
    {   // YAML order decides the slots, not scan order: the glossy PLANE is shape 1 (scanned after every sphere) and takes slot 0;
        // duplicates share a slot
        Scene s = scene_of({10.0, 1e4, -1.0, 10.0, 100.0}, true);
        CHECK(build(s, h) == FLUX_OK);
        CHECK(h.rp.n_gloss_exp == 3 && h.rp.gx_stride == 48);
        CHECK(h.gx_inv_e1[0] == 1.0 / 101.0 && h.gx_inv_e1[1] == 1.0 / 11.0 && h.gx_inv_e1[2] == 1.0 / 10001.0);
        CHECK(off_of_shape(h, 1) == 0);                                  // the plane: exponent 100
        CHECK(off_of_shape(h, 2) == 16 && off_of_shape(h, 5) == 16);     // exponent 10, twice
        CHECK(off_of_shape(h, 3) == 32 && off_of_shape(h, 6) == 0);      // 1e4; the last sphere shares the plane's slot
        CHECK(off_of_shape(h, 0) == 0 && off_of_shape(h, 4) == 0);       // Emissive, Matte: never read
        CHECK(h.gx_off.size() == s.shapes.size() + 1);
        std::printf("ok yaml order and duplicates\n");
    }
    {   // two exponents: two entries a sample; exponent 0 is a value like any other (inv_e1 = 1)
        Scene s = scene_of({0.0, 3.0});
        CHECK(build(s, h) == FLUX_OK);
        CHECK(h.rp.n_gloss_exp == 2 && h.rp.gx_stride == 32 && h.gx_inv_e1[0] == 1.0 && h.gx_inv_e1[1] == 0.25);
        std::printf("ok two exponents\n");
    }
    {   // the cap: four are held, five are not -- and no record is given an offset then
        Scene s4 = scene_of({1.0, 2.0, 3.0, 4.0, 2.0});
        CHECK(build(s4, h) == FLUX_OK);
        CHECK(h.rp.n_gloss_exp == 4 && h.rp.gx_stride == 64 && off_of_shape(h, 4) == 48 && off_of_shape(h, 5) == 16);
        Scene s5 = scene_of({1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0});
        CHECK(build(s5, h) == FLUX_OK);
        CHECK(h.rp.n_gloss_exp == flux::kGlossExpSlots + 1 && h.rp.gx_stride == 0);
        for (int32_t o : h.gx_off) CHECK(o == 0);
        std::printf("ok cap\n");
    }
    {   // a plane stored with a non-unit normal: long-form glossy weights, no table
        Scene s = scene_of({10.0, 100.0}, false, 2.5);
        CHECK(build(s, h) == FLUX_OK);
        CHECK(h.rp.glossy_long == 1 && h.rp.n_gloss_exp == 2 && h.rp.gx_stride == 0);
        std::printf("ok non-unit plane normal\n");
    }
    std::printf("all ok\n");
    return 0;
}

struct Ctx {
    flux_ctx *c = nullptr;
    ~Ctx() { flux_ctx_destroy(c); }
};

int create(Scene &s, uint64_t root, uint64_t first, uint64_t stride, Ctx &out) {
    flux_job_cfg cfg{root, 5, 50};
    return flux_ctx_create_sets(&s.get(), &cfg, 7, 0, first, stride, &out.c);
}

// the context's glossx entries and, beside them, its gloss and pixel tables (slot order)
int fetch(const flux_ctx *c, std::vector<double> &gx, std::vector<double> &gloss, std::vector<double> &pix) {
    const size_t SN = (size_t)c->sets.count * c->N;
    gx.assign(SN * (size_t)(c->rp.gx_stride / 8), 0.0);
    gloss.assign(SN * 4, 0.0);
    pix.assign(SN * 2, 0.0);
    CHECK(hipMemcpy(gx.data(), c->d_glossx, gx.size() * 8, hipMemcpyDeviceToHost) == hipSuccess);
    CHECK(hipMemcpy(gloss.data(), c->d_gloss, gloss.size() * 8, hipMemcpyDeviceToHost) == hipSuccess);
    CHECK(hipMemcpy(pix.data(), c->d_pix, pix.size() * 8, hipMemcpyDeviceToHost) == hipSuccess);
    return 0;
}

int gpu() {
    unsetenv("FLUX_SAMPLE_TABLES");
    const uint64_t root = 4;  // 16 samples a set
    Scene three = scene_of({0.0, 100.0, -1.0, 10.0});
    Ctx full;
    CHECK(create(three, root, 0, 1, full) == FLUX_OK);
    const flux_ctx *c = full.c;
    CHECK(c->rp.gx_stride == 48 && c->d_glossx != nullptr && c->rp.glossx == c->d_glossx && c->rp.gx_off == c->d_gxoff && c->sets.count == 9);
    std::vector<double> gx, gloss, pix;
    if (fetch(c, gx, gloss, pix)) return 1;
    for (size_t t = 0; t < (size_t)c->sets.count * c->N; t++) {
        const double y = pix[2 * t + 1];
        const double inv_e1[3] = {1.0, 1.0 / 101.0, 1.0 / 11.0};
        for (int k = 0; k < 3; k++) {
            const double co = gx[(t * 3 + k) * 2], si = gx[(t * 3 + k) * 2 + 1];
            // (cos theta, sin theta) of to_unit_hemi to rounding; exponent 0: cos theta = 1 - y
            CHECK(std::fabs(co - std::pow(1.0 - y, inv_e1[k])) < 1e-14 && std::fabs(si - std::sqrt(std::fma(-co, co, 1.0))) <= 1e-15 * si);
            CHECK(co > 0.0 && co <= 1.0 && si >= 0.0 && si <= 1.0);
        }
    }
    std::printf("ok table values\n");
    {   // the rows records point at each held set's entries
        std::vector<flux::DevSetRows> rows(c->sets.count);
        CHECK(hipMemcpy(rows.data(), c->d_setrows, rows.size() * sizeof(flux::DevSetRows), hipMemcpyDeviceToHost) == hipSuccess);
        for (size_t m = 0; m < rows.size(); m++)
            CHECK(rows[m].glossx == c->d_glossx + m * c->N * 3 && rows[m].gloss == c->d_gloss + m * c->N * 4);
        std::printf("ok set rows\n");
    }
    {   // a set-share context (1, 3): sets 1, 4, 7 -- its rows are the full context's rows of those sets
        Ctx share;
        CHECK(create(three, root, 1, 3, share) == FLUX_OK);
        CHECK(share.c->sets.count == 3 && share.c->rp.gx_stride == 48);
        std::vector<double> sgx, sgloss, spix;
        if (fetch(share.c, sgx, sgloss, spix)) return 1;
        const size_t row = (size_t)c->N * 6;  // doubles of one set's entries
        CHECK(sgx.size() == 3 * row);
        for (size_t m = 0; m < 3; m++) CHECK(std::memcmp(&sgx[m * row], &gx[(1 + 3 * m) * row], row * 8) == 0);
        std::vector<flux::DevSetRows> rows(3);
        CHECK(hipMemcpy(rows.data(), share.c->d_setrows, rows.size() * sizeof(flux::DevSetRows), hipMemcpyDeviceToHost) == hipSuccess);
        for (size_t m = 0; m < 3; m++) CHECK(rows[m].glossx == share.c->d_glossx + m * c->N * 3);
        CHECK(flux_ctx_device_bytes(share.c) < flux_ctx_device_bytes(full.c));
        std::printf("ok set share\n");
    }
    {   // one exponent: 16 B a sample
        Scene one = scene_of({100.0, 100.0});
        Ctx x;
        CHECK(create(one, root, 0, 1, x) == FLUX_OK);
        CHECK(x.c->rp.gx_stride == 16 && x.c->d_glossx != nullptr);
        std::printf("ok one exponent\n");
    }
    {   // five exponents, past the cap: no table, nothing allocated for it
        Scene five = scene_of({1.0, 2.0, 3.0, 4.0, 5.0});
        Ctx x;
        CHECK(create(five, root, 0, 1, x) == FLUX_OK);
        CHECK(x.c->rp.gx_stride == 0 && x.c->d_glossx == nullptr && x.c->d_gxoff == nullptr && x.c->rp.glossx == nullptr);
        std::vector<flux::DevSetRows> rows(x.c->sets.count);
        CHECK(hipMemcpy(rows.data(), x.c->d_setrows, rows.size() * sizeof(flux::DevSetRows), hipMemcpyDeviceToHost) == hipSuccess);
        for (const flux::DevSetRows &r : rows) CHECK(r.glossx == nullptr);
        std::printf("ok past the cap\n");
    }
    {   // FLUX_SAMPLE_TABLES=0, read at context creation: the same scene without the table, and less device memory by its size
        setenv("FLUX_SAMPLE_TABLES", "0", 1);
        Ctx x;
        CHECK(create(three, root, 0, 1, x) == FLUX_OK);
        unsetenv("FLUX_SAMPLE_TABLES");
        CHECK(x.c->rp.gx_stride == 0 && x.c->d_glossx == nullptr && x.c->rp.n_gloss_exp == 3);
        CHECK(flux_ctx_device_bytes(full.c) - flux_ctx_device_bytes(x.c) == 9 * 16 * 48 + three.shapes.size() * 4 + 4);
        std::printf("ok switch\n");
    }
    std::printf("all ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "cpu") return cpu();
    if (mode == "gpu") return gpu();
    std::fprintf(stderr, "usage: %s cpu | gpu\n", argv[0]);
    return 2;
}
