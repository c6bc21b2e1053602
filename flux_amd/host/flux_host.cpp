// flux_host.cpp -- see flux_host.hpp.
#include "flux_host.hpp"

#include <random>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "scene_schema.hpp"
#include "yaml_lite.hpp"

namespace flux_host {
namespace {

using yaml_lite::Node;

[[noreturn]] void bad(const std::string &m) { throw FluxError(FLUX_E_INVALID, m); }

// serde_yaml::from_reader over the lists of scene_schema.hpp: `n` is the node being read, `path` its dotted path for messages
struct YamlReader {
    const Node &n;
    std::string path;

    // the paths below the top level do not start at `scene.` (output_settings.image_width, shapes[3].Sphere.radius)
    std::string below() const { return path.rfind("scene.", 0) == 0 ? path.substr(6) : path; }

    template <class M> void operator()(const char *key, M &member) {
        const Node *f = n.find(key);
        if (!f) bad(below() + ": missing field `" + key + "`");
        YamlReader{*f, below() + "." + key}.value(member);
    }
    // a field the schema marks optional (scene_schema.hpp optional_field): absent, the member keeps its default
    template <class M> void optional(const char *key, M &member) {
        if (const Node *f = n.find(key)) YamlReader{*f, below() + "." + key}.value(member);
    }
    void value(double &v) {
        if (n.kind != Node::Scalar) bad(path + ": expected a number");
        char *end = nullptr;
        v = std::strtod(n.scalar.c_str(), &end);
        if (end == n.scalar.c_str() || *end != '\0') bad(path + ": expected a number, got `" + n.scalar + "`");
    }
    void value(size_t &v) {
        double d;
        value(d);
        if (d < 0 || d != (double)(size_t)d) bad(path + ": expected an unsigned integer");
        v = (size_t)d;
    }
    void value(bool &v) {
        if (n.kind != Node::Scalar || (n.scalar != "true" && n.scalar != "false")) bad(path + ": expected a boolean");
        v = n.scalar == "true";
    }
    void value(std::string &s) {
        if (n.kind != Node::Scalar) bad(path + ": expected a string");
        s = n.scalar;
    }
    void value(Vec3 &v) {
        if (n.kind != Node::Seq || n.seq.size() != 3) bad(path + ": expected a sequence of 3 numbers");
        YamlReader{n.seq[0], path}.value(v.x);
        YamlReader{n.seq[1], path}.value(v.y);
        YamlReader{n.seq[2], path}.value(v.z);
    }
    void value(Color &c) {  // color.rs:8-16: a sequence here, a map on the wire
        Vec3 v;
        value(v);
        c = Color{v.x, v.y, v.z};
    }
    template <class T> void value(std::vector<T> &items) {
        if (n.kind != Node::Seq && n.kind != Node::Null) bad(path + ": expected a sequence");
        items.resize(n.seq.size());
        for (size_t i = 0; i < n.seq.size(); i++) YamlReader{n.seq[i], below() + "[" + std::to_string(i) + "]"}.value(items[i]);
    }
    void value(MaterialData &m) { enumeration(m); }
    void value(ShapeData &s) { enumeration(s); }
    // the variant called as the map's one key, if the enum has one, becomes current and reads the key's value
    struct Variant {
        const YamlReader &r;
        bool found = false;
        template <class Select> void variant(const char *name, bool, Select select) {
            if (r.n.map[0].first != name) return;
            found = true;
            YamlReader{r.n.map[0].second, r.path + "." + name}.value(select());
        }
    };
    template <class E> void enumeration(E &e) {  // externally tagged: a one-key map
        if (n.kind != Node::Map || n.map.size() != 1) bad(path + ": expected an externally tagged enum (one-key map)");
        Variant chosen{*this};
        variants(chosen, e);
        if (!chosen.found) bad(path + ": unknown variant `" + n.map[0].first + "`, expected one of " + variant_names(e));
    }
    template <class S> void value(S &s) {
        if (n.kind != Node::Map) bad(below() + ": expected a map");
        fields(*this, s);
        check(s);
    }

    // what only the loader refuses, once the struct is read (the ABI checks the same values again, flux_abi.h)
    template <class S> void check(const S &) {}
    void check(DiskData &k) {
        if (!(std::isfinite(k.radius) && k.radius >= 0.0)) bad(below() + "." + field_name(k, k.radius) + ": expected a finite number >= 0");
    }
    void check(BoxData &k) {
        const double c0[3] = {k.corner0.x, k.corner0.y, k.corner0.z}, c1[3] = {k.corner1.x, k.corner1.y, k.corner1.z};
        for (int a = 0; a < 3; a++) {
            const std::string axis(1, "xyz"[a]);
            if (!std::isfinite(c0[a])) bad(below() + "." + field_name(k, k.corner0) + ": expected finite numbers (axis " + axis + ")");
            if (!(std::isfinite(c1[a]) && c0[a] < c1[a]))
                bad(below() + "." + field_name(k, k.corner1) + ": expected finite numbers above corner0 (axis " + axis + ")");
        }
    }
    void check(DielectricData &m) {
        if (!(std::isfinite(m.refraction_index) && m.refraction_index > 0.0))
            bad(below() + "." + field_name(m, m.refraction_index) + ": expected a finite number > 0");
    }
};

SceneData scene_from_node(const Node &d) {
    SceneData sd;
    YamlReader{d, "scene"}.value(sd);
    return sd;
}

double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

void set3(double *d, const Vec3 &v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; }
void set3(double *d, const Color &c) { d[0] = c.r; d[1] = c.g; d[2] = c.b; }

flux_material to_abi(const MaterialData &m) {
    flux_material o{};
    if (auto p = std::get_if<MatteData>(&m)) {
        o.kind = FLUX_MAT_MATTE;
        set3(o.color, p->diffuse_color);
        set3(o.ambient, p->ambient_color);
        o.k = p->diffuse_coefficient;
    } else if (auto p = std::get_if<EmissiveData>(&m)) {
        o.kind = FLUX_MAT_EMISSIVE;
        set3(o.color, p->color);
        o.k = p->power;
    } else if (auto p = std::get_if<ReflectiveData>(&m)) {
        o.kind = FLUX_MAT_REFLECTIVE;
        set3(o.color, p->reflect_color);
        o.k = p->reflect_amount;
    } else if (auto p = std::get_if<GlossyReflectiveData>(&m)) {
        o.kind = FLUX_MAT_GLOSSY;
        set3(o.color, p->reflect_color);
        o.k = p->reflect_amount;
        o.exponent = p->reflect_exponent;
    } else if (auto p = std::get_if<DielectricData>(&m)) {
        o.kind = FLUX_MAT_DIELECTRIC;
        set3(o.color, p->transmit_color);
        o.k = p->refraction_index;
    }
    return o;
}

flux_job_cfg to_abi(const JobConfiguration &c) { return flux_job_cfg{c.sample_root, c.max_trace_depth, c.rows_per_work_unit}; }

// the C ABI's handles, destroyed on every path out of their scope
struct CtxDestroy { void operator()(flux_ctx *c) const { flux_ctx_destroy(c); } };
struct MultiDestroy { void operator()(flux_multi *m) const { flux_multi_destroy(m); } };
using CtxPtr = std::unique_ptr<flux_ctx, CtxDestroy>;
using MultiPtr = std::unique_ptr<flux_multi, MultiDestroy>;

// Scene::from_data + Camera::new (workers.rs:46-54); empty with the library's message in flux_last_error(), its code in *rc
CtxPtr create_ctx(const SceneData &scene_data, const JobConfiguration &config, uint64_t seed, int device, int *rc = nullptr) {
    AbiScene abi(scene_data);
    const flux_job_cfg cfg = to_abi(config);
    flux_ctx *ctx = nullptr;
    const int code = flux_ctx_create(&abi.desc, &cfg, seed, device, &ctx);
    if (rc) *rc = code;
    return CtxPtr(code == FLUX_OK ? ctx : nullptr);
}

// [nrows][W][3] doubles -> the rows of a WorkUnitResult
std::vector<std::vector<Color>> to_rows(const double *p, size_t nrows, size_t w) {
    std::vector<std::vector<Color>> rows(nrows, std::vector<Color>(w));
    for (auto &row : rows)
        for (Color &c : row) {
            c = Color{p[0], p[1], p[2]};
            p += 3;
        }
    return rows;
}

}  // namespace

SceneData scene_from_yaml_text(const std::string &text) {
    try {
        return scene_from_node(yaml_lite::parse(text));
    } catch (const yaml_lite::Error &e) {
        throw FluxError(FLUX_E_INVALID, e.what());
    }
}

SceneData scene_from_yaml_file(const std::string &path) {
    try {
        return scene_from_node(yaml_lite::parse_file(path));
    } catch (const yaml_lite::Error &e) {
        throw FluxError(FLUX_E_INVALID, path + ": " + e.what());
    }
}

AbiScene::AbiScene(const SceneData &sd) : name(sd.scene_name) {
    shapes.resize(sd.shapes.size());
    for (size_t i = 0; i < sd.shapes.size(); i++) {
        flux_shape &fs = shapes[i];
        fs = flux_shape{};
        if (auto s = std::get_if<SphereData>(&sd.shapes[i])) {
            fs.kind = FLUX_SHAPE_SPHERE;
            set3(fs.p, s->center);
            fs.radius = s->radius;
            fs.invert = s->invert ? 1 : 0;
            fs.material = to_abi(s->material);
        } else if (auto p = std::get_if<PlaneData>(&sd.shapes[i])) {
            fs.kind = FLUX_SHAPE_PLANE;
            set3(fs.p, p->point);
            set3(fs.n, p->normal);
            fs.material = to_abi(p->material);
        } else if (auto k = std::get_if<DiskData>(&sd.shapes[i])) {
            fs.kind = FLUX_SHAPE_DISK;
            set3(fs.p, k->center);
            set3(fs.n, k->normal);
            fs.radius = k->radius;
            fs.material = to_abi(k->material);
        } else if (auto b = std::get_if<BoxData>(&sd.shapes[i])) {
            fs.kind = FLUX_SHAPE_BOX;
            set3(fs.p, b->corner0);
            set3(fs.n, b->corner1);
            fs.invert = b->invert ? 1 : 0;
            fs.material = to_abi(b->material);
        }
    }
    desc.scene_name = name.c_str();
    desc.image_width = sd.output_settings.image_width;
    desc.image_height = sd.output_settings.image_height;
    desc.pixel_size = sd.output_settings.pixel_size;
    set3(desc.background, sd.background);
    const CameraSettings &c = sd.camera_settings;
    set3(desc.eye, c.eye);
    set3(desc.look_at, c.look_at);
    set3(desc.up, c.up);
    desc.zoom_factor = sd.camera_data.zoom_factor;
    desc.view_plane_distance = sd.camera_data.view_plane_distance;
    desc.focal_distance = sd.camera_data.focal_distance;
    desc.lens_radius = sd.camera_data.lens_radius;
    desc.num_shapes = shapes.size();
    desc.shapes = shapes.empty() ? nullptr : shapes.data();
    desc.num_meshes = 0;
    desc.meshes = nullptr;
}

std::vector<double> render_feature_buffers(const SceneData &scene_data, const JobConfiguration &config, uint64_t seed, int device) {
    int rc = FLUX_OK;
    const CtxPtr ctx = create_ctx(scene_data, config, seed, device, &rc);
    if (!ctx) throw FluxError(rc, flux_last_error());
    const size_t w = scene_data.output_settings.image_width, h = scene_data.output_settings.image_height;
    std::vector<double> aov(w * h * FLUX_AOV_CHANNELS);
    rc = flux_render_aov_rows(ctx.get(), 0, h - 1, aov.data());
    if (rc != FLUX_OK) throw FluxError(rc, flux_last_error());  // (the message is copied before the context goes)
    return aov;
}

void render_aov_chain(const SceneData &scene_data, const JobConfiguration &config, uint64_t seed, int device, uint32_t max_chain,
                      std::vector<double> &out) {
    const size_t w = scene_data.output_settings.image_width, h = scene_data.output_settings.image_height;
    if (out.size() != w * h * FLUX_AOV_CHANNELS)
        throw FluxError(FLUX_E_INVALID, "render_aov_chain: the buffer holds " + std::to_string(out.size()) + " doubles, the frame needs " +
                                            std::to_string(w * h * FLUX_AOV_CHANNELS));
    if (max_chain > config.max_trace_depth)
        throw FluxError(FLUX_E_INVALID, "render_aov_chain: max_chain " + std::to_string(max_chain) + " exceeds max_trace_depth " +
                                            std::to_string(config.max_trace_depth));
    if (w == 0 || h == 0) throw FluxError(FLUX_E_INVALID, "render_aov_chain: an empty frame");
    int rc = FLUX_OK;
    const CtxPtr ctx = create_ctx(scene_data, config, seed, device, &rc);
    if (!ctx) throw FluxError(rc, flux_last_error());
    rc = flux_render_aov_chain_rows(ctx.get(), 0, h - 1, max_chain, out.data());
    if (rc != FLUX_OK) throw FluxError(rc, flux_last_error());  // (the message is copied before the context goes)
}

std::vector<double> render_moments(const SceneData &scene_data, const JobConfiguration &config, uint64_t seed, int device) {
    int rc = FLUX_OK;
    const CtxPtr ctx = create_ctx(scene_data, config, seed, device, &rc);
    if (!ctx) throw FluxError(rc, flux_last_error());
    const size_t w = scene_data.output_settings.image_width, h = scene_data.output_settings.image_height;
    std::vector<double> moments(w * h * FLUX_MOMENT_CHANNELS);
    rc = flux_render_moments_rows(ctx.get(), 0, h - 1, moments.data());
    if (rc != FLUX_OK) throw FluxError(rc, flux_last_error());  // (the message is copied before the context goes)
    return moments;
}

std::vector<double> aov_image(const double *aov, size_t width, size_t height, AovKind kind) {
    const size_t npix = width * height;
    std::vector<double> rgb(npix * 3);
    double t_max = 0.0;
    for (size_t k = 0; k < npix; k++) {
        const double t = aov[k * FLUX_AOV_CHANNELS + FLUX_AOV_DEPTH];
        if (std::isfinite(t) && t > t_max) t_max = t;
    }
    if (!(t_max > 0.0)) t_max = 1.0;
    for (size_t k = 0; k < npix; k++) {
        const double *p = aov + k * FLUX_AOV_CHANNELS;
        double *o = rgb.data() + k * 3;
        switch (kind) {
            case AovKind::Albedo:
                for (int c = 0; c < 3; c++) o[c] = p[FLUX_AOV_ALBEDO + c] < 1.0 ? p[FLUX_AOV_ALBEDO + c] : 1.0;
                break;
            case AovKind::Normal: {
                const double *n = p + FLUX_AOV_NORMAL;
                const double len = std::sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
                for (int c = 0; c < 3; c++) o[c] = len > 0.0 ? 0.5 + 0.5 * (n[c] / len) : 0.5;
                break;
            }
            case AovKind::Depth: {
                const double t = p[FLUX_AOV_DEPTH];
                o[0] = o[1] = o[2] = std::isfinite(t) ? p[FLUX_AOV_COVERAGE] * (1.0 - t / t_max) : 0.0;
                break;
            }
            case AovKind::Coverage:
                o[0] = o[1] = o[2] = p[FLUX_AOV_COVERAGE];
                break;
        }
    }
    return rgb;
}

std::vector<double> denoise_frame(const std::vector<double> &rgb, const std::vector<double> &aov, size_t width, size_t height, int device) {
    if (rgb.size() != width * height * 3 || aov.size() != width * height * FLUX_AOV_CHANNELS)
        throw FluxError(FLUX_E_INVALID, "denoise_frame: the buffers do not hold width * height pixels");
    std::vector<double> out(rgb.size());
    const int rc = flux_denoise(device, width, height, rgb.data(), aov.data(), nullptr, out.data());
    if (rc != FLUX_OK) throw FluxError(rc, flux_last_error());
    return out;
}

std::vector<double> denoise_moments_frame(const std::vector<double> &moments, const std::vector<double> &aov, size_t width, size_t height,
                                          int device) {
    if (moments.size() != width * height * FLUX_MOMENT_CHANNELS || aov.size() != width * height * FLUX_AOV_CHANNELS)
        throw FluxError(FLUX_E_INVALID, "denoise_moments_frame: the buffers do not hold width * height pixels");
    std::vector<double> out(width * height * 3);
    const int rc = flux_denoise_moments(device, width, height, moments.data(), aov.data(), nullptr, out.data());
    if (rc != FLUX_OK) throw FluxError(rc, flux_last_error());
    return out;
}

flux_adaptive_params adaptive_defaults() {
    flux_adaptive_params p{};
    p.threshold = FLUX_ADAPTIVE_THRESHOLD;
    p.lum_floor = FLUX_ADAPTIVE_LUM_FLOOR;
    p.min_passes = FLUX_ADAPTIVE_MIN_PASSES;
    p.max_passes = FLUX_ADAPTIVE_MAX_PASSES;
    p.dilate = FLUX_ADAPTIVE_DILATE;
    return p;
}

AdaptiveFrame render_adaptive(const SceneData &scene_data, const JobConfiguration &config, uint64_t seed, int device,
                              const flux_adaptive_params &params) {
    const size_t w = scene_data.output_settings.image_width, h = scene_data.output_settings.image_height;
    if (params.max_passes > w)
        throw FluxError(FLUX_E_INVALID, "render_adaptive: max_passes " + std::to_string(params.max_passes) + " exceeds the " +
                                            std::to_string(w) + " sample sets of an image this wide");
    int rc = FLUX_OK;
    const CtxPtr ctx = create_ctx(scene_data, config, seed, device, &rc);
    if (!ctx) throw FluxError(rc, flux_last_error());
    AdaptiveFrame f;
    f.moments.resize(w * h * FLUX_MOMENT_CHANNELS);
    f.passes.resize(w * h);
    flux_adaptive_params p = params;
    uint64_t info[FLUX_ADAPTIVE_INFO_WORDS] = {};
    rc = flux_render_adaptive_rows(ctx.get(), 0, h - 1, &p, f.moments.data(), f.passes.data(), info);
    if (rc != FLUX_OK) throw FluxError(rc, flux_last_error());  // (the message is copied before the context goes)
    f.rounds = info[0];
    f.pixel_passes = info[1];
    f.pixels_at_max_passes = info[2];
    return f;
}

std::vector<double> moments_frame(const std::vector<double> &moments, size_t width, size_t height) {
    if (moments.size() != width * height * FLUX_MOMENT_CHANNELS)
        throw FluxError(FLUX_E_INVALID, "moments_frame: the buffer does not hold width * height pixels");
    std::vector<double> rgb(width * height * 3);
    for (size_t k = 0; k < width * height; k++)
        for (int c = 0; c < 3; c++) rgb[k * 3 + c] = moments[k * FLUX_MOMENT_CHANNELS + FLUX_MOMENT_RGB + c];
    return rgb;
}

std::vector<double> passes_image(const std::vector<uint32_t> &passes, size_t width, size_t height, uint32_t max_passes) {
    if (passes.size() != width * height) throw FluxError(FLUX_E_INVALID, "passes_image: the map does not hold width * height pixels");
    if (max_passes == 0) throw FluxError(FLUX_E_INVALID, "passes_image: max_passes must be >= 1");
    std::vector<double> rgb(width * height * 3);
    for (size_t k = 0; k < width * height; k++) {
        const double g = passes[k] < max_passes ? (double)passes[k] / (double)max_passes : 1.0;
        rgb[k * 3] = rgb[k * 3 + 1] = rgb[k * 3 + 2] = g;
    }
    return rgb;
}

std::vector<WorkUnit> Job::work_units() const {
    const uint64_t h = scene_data.output_settings.image_height;
    int64_t n = flux_work_units(h, config.rows_per_work_unit, nullptr, 0);
    // the reference panics here: "Job row per work unit count invalid" (job.rs:67-70)
    if (n < 0) throw FluxError((int)n, flux_last_error());
    std::vector<flux_work_unit> raw((size_t)n);
    if (n > 0) flux_work_units(h, config.rows_per_work_unit, raw.data(), (uint64_t)n);
    std::vector<WorkUnit> us;
    for (const auto &u : raw) us.push_back(WorkUnit{(size_t)u.row_start, (size_t)u.row_end, id});
    return us;
}

// ---- the local workers' job loop: workers.rs:43-75 ----------------------------------------------
namespace {
std::atomic<int> worker_failures{0};
}
int GpuWorker::failures() { return worker_failures.load(); }
void GpuWorker::note_failure() { worker_failures.fetch_add(1); }

void serve_job(WorkerRequest req, const std::string &who, const std::string &range_who,
               const std::function<std::unique_ptr<RowSource>(const Job &)> &open) {
    // a C++ worker thread records a failure so that the front-end exits non-zero instead of reporting a frame with missing rows
    auto give_up = [&](const char *why) {
        std::fprintf(stderr, "%s: %s\n", who.c_str(), why);
        GpuWorker::note_failure();
    };
    try {
        const std::unique_ptr<RowSource> source = open(*req.job);
        if (!source) return give_up(flux_last_error());
        const size_t w = req.job->scene_data.output_settings.image_width;
        const size_t h = req.job->scene_data.output_settings.image_height;
        // while let Ok(unit) = recv_unit.recv()   (workers.rs:56)
        while (auto unit = req.recv_unit->recv()) {
            // A unit may come straight off a socket (flux_node): validate before sizing anything.  Rows past the image would make
            // the reference's ImageBuilder index out of bounds (manager.rs:322-324) -- here the unit is refused.
            RenderEvent ev;
            ev.kind = RenderEvent::RowsReady;
            ev.result.work_unit = *unit;
            if (unit->row_start <= unit->row_end) {
                if (unit->row_end >= h) {
                    std::fprintf(stderr, "%s: work unit rows [%zu,%zu] outside image height %zu\n", range_who.c_str(),
                                 (size_t)unit->row_start, (size_t)unit->row_end, h);
                    GpuWorker::note_failure();
                    return;
                }
                const double *p = source->rows(unit->row_start, unit->row_end);  // camera.render(&scene, unit)   (workers.rs:60)
                if (!p) return give_up(flux_last_error());
                ev.result.rows = to_rows(p, unit->row_end - unit->row_start + 1, w);
            }
            req.send_result->send(std::move(ev));
        }
    } catch (const std::exception &e) {
        give_up(e.what());
    }
}

// ---- GpuWorker: workers.rs:26-103 ---------------------------------------------------------------
namespace {
struct CtxRows : RowSource {  // one flux_render_rows per unit
    CtxPtr ctx;
    size_t w;
    std::vector<double> buf;
    CtxRows(CtxPtr c, size_t width) : ctx(std::move(c)), w(width) {}
    const double *rows(size_t row_start, size_t row_end) override {
        buf.resize((row_end - row_start + 1) * w * 3);
        return flux_render_rows(ctx.get(), row_start, row_end, buf.data()) == FLUX_OK ? buf.data() : nullptr;
    }
};
}  // namespace

GpuWorker::GpuWorker(int device, uint64_t seed) : device_(device), seed_(seed), service_([this] { run(); }) {}

void GpuWorker::run() {
    // the worker's one-time set-up, before any job (LocalWorker::new builds its rayon pool here, workers.rs:27-38): the HIP runtime's
    // lazy initialisation on this device, so that a job's timer (manager.rs:145) sees the context's work and not the process's
    (void)flux_device_warmup(device_);
    const std::string who = "GpuWorker(device " + std::to_string(device_) + ")";
    // 'main: while let Ok(Some((job, recv_unit, send_result, wg))) = r.recv()   (workers.rs:43)
    while (auto req = service_.next())
        serve_job(std::move(*req), who, who, [this](const Job &job) -> std::unique_ptr<RowSource> {
            CtxPtr ctx = create_ctx(job.scene_data, job.config, seed_, device_);
            if (!ctx) return nullptr;
            return std::make_unique<CtxRows>(std::move(ctx), job.scene_data.output_settings.image_width);
        });
}

// ---- MultiGpuWorker: the node's GPUs as one worker (flux_multi_*) ----------------------------------
namespace {
struct FrameRows : RowSource {  // the whole frame at the first unit, slices of it afterwards
    MultiPtr multi;
    size_t w, h;
    std::mutex &mu;  // the worker's, over `timing`
    std::vector<double> &timing;
    std::vector<double> frame;
    FrameRows(MultiPtr m, size_t width, size_t height, std::mutex &timing_mu, std::vector<double> &timing_words)
        : multi(std::move(m)), w(width), h(height), mu(timing_mu), timing(timing_words) {}
    const double *rows(size_t row_start, size_t) override {
        if (frame.empty()) {  // camera.render for the whole image, on all devices (workers.rs:60)
            frame.resize(w * h * 3);
            if (flux_multi_render_frame(multi.get(), frame.data()) != FLUX_OK) return nullptr;
            double t[FLUX_MULTI_TIMING_WORDS];
            if (flux_multi_timing(multi.get(), t) == FLUX_OK) {
                std::lock_guard<std::mutex> g(mu);
                timing.assign(t, t + FLUX_MULTI_TIMING_WORDS);
            }
        }
        return frame.data() + row_start * w * 3;
    }
};
}  // namespace

MultiGpuWorker::MultiGpuWorker(std::vector<int> devices, uint64_t seed, int shard)
    : devices_(std::move(devices)), seed_(seed), shard_(shard), service_([this] { run(); }) {}

std::vector<double> MultiGpuWorker::last_timing() const {
    std::lock_guard<std::mutex> g(mu_);
    return timing_;
}

void MultiGpuWorker::run() {
    {   // one-time set-up per device, concurrently (see GpuWorker::run)
        std::vector<JoiningThread> th;
        for (int d : devices_) th.emplace_back([d] { (void)flux_device_warmup(d); });
    }
    const std::string who = "MultiGpuWorker(" + std::to_string(devices_.size()) + " devices)";
    while (auto req = service_.next())
        serve_job(std::move(*req), who, "MultiGpuWorker", [this](const Job &job) -> std::unique_ptr<RowSource> {
            // Scene::from_data + Camera::new on every device (workers.rs:46-54), concurrently, + the communicators
            AbiScene abi(job.scene_data);
            const flux_job_cfg cfg = to_abi(job.config);
            flux_multi *m = nullptr;
            if (flux_multi_create(&abi.desc, &cfg, seed_, devices_.data(), devices_.size(), shard_, &m) != FLUX_OK) return nullptr;
            return std::make_unique<FrameRows>(MultiPtr(m), job.scene_data.output_settings.image_width,
                                               job.scene_data.output_settings.image_height, mu_, timing_);
        });
}

// ---- ImageBuilder: manager.rs:278-363 -----------------------------------------------------------
ImageBuilder::ImageBuilder() : service_([this] { run(); }) {}

void ImageBuilder::run() {
    const auto first = service_.next();
    if (!first || first->kind != RenderEvent::ImageInfo) return;  // manager.rs:291-297
    const std::string scene_name = first->scene_name;
    const size_t width = first->width, height = first->height;
    const auto second = service_.next();
    if (!second || second->kind != RenderEvent::RenderingStarted) return;  // manager.rs:301-307
    const double start_time = second->time_s;
    std::vector<double> img(width * height * 3, 0.0);
    std::vector<uint8_t> present(height, 0);
    while (const auto m = service_.next()) {
        const RenderEvent &ev = *m;
        if (ev.kind == RenderEvent::RowsReady) {  // manager.rs:316-324
            for (size_t i = 0; i < ev.result.rows.size(); i++) {
                const size_t r = i + ev.result.work_unit.row_start;
                if (r >= height) continue;
                present[r] = 1;
                const auto &row = ev.result.rows[i];
                for (size_t c = 0; c < row.size() && c < width; c++) {
                    double *p = &img[(r * width + c) * 3];
                    p[0] = row[c].r; p[1] = row[c].g; p[2] = row[c].b;
                }
            }
        } else if (ev.kind == RenderEvent::RenderingFinished) {  // manager.rs:326-335
            total_time_s = ev.time_s - start_time;
            std::printf("rendering finished, total time %.6fs\n", total_time_s);
            written_path = output_dir + "/" + scene_name + ".ppm";
            if (flux_write_ppm(written_path.c_str(), img.data(), width, height, present.data()) != FLUX_OK)
                std::fprintf(stderr, "ImageBuilder: %s\n", flux_last_error());
            image = img;
        } else {
            return;  // unexpected message (manager.rs:336-339)
        }
    }
}

// ---- JobIDAllocator / RenderManager: job.rs:14-34, manager.rs:72-219 ------------------------------
JobIDAllocator::JobIDAllocator() {
    std::random_device rd;  // rand::thread_rng().gen() (job.rs:21-24)
    allocator_id_ = ((size_t)rd() << 32) ^ (size_t)rd();
}

RenderManager::RenderManager(std::vector<WorkerHandle> workers) : workers_(std::move(workers)), service_([this] { run(); }) {
    // (the thread started above takes nothing but its mailbox until a job is scheduled, and is joined as this unwinds)
    if (workers_.empty()) throw FluxError(FLUX_E_INVALID, "RenderManager::new: must provide at least one worker handle");
}

JobHandle RenderManager::schedule_job(const SceneData &scene_data, const JobConfiguration &config,
                                      std::shared_ptr<Channel<std::optional<RenderEvent>>> result_sender) {
    ScheduledJob sj;  // manager.rs:198-213
    sj.job.id = ids_.next_id();
    sj.job.scene_data = scene_data;
    sj.job.config = config;
    sj.notify_done = std::make_shared<Channel<int>>();
    sj.notify_cancel = std::make_shared<Channel<int>>();
    sj.result_sender = std::move(result_sender);
    JobHandle h;
    h.job_id = sj.job.id;
    h.waiter_ = sj.notify_done;
    h.canceller_ = sj.notify_cancel;
    service_.mailbox()->send(std::move(sj));
    return h;
}

void RenderManager::run() {
    // while let Ok(Some((job, notify_done, notify_cancel, result_sender))) = r.recv()   (manager.rs:83)
    while (auto msg = service_.next()) {
        const ScheduledJob &sj = *msg;
        const Job &job = sj.job;
        RenderEvent info;
        info.kind = RenderEvent::ImageInfo;  // manager.rs:86-98
        info.scene_name = job.scene_data.scene_name;
        info.width = job.scene_data.output_settings.image_width;
        info.height = job.scene_data.output_settings.image_height;
        if (!sj.result_sender->send(info)) continue;

        auto ws = std::make_shared<Channel<WorkUnit>>(1);  // bounded(1), manager.rs:100
        auto wg = std::make_shared<WaitGroup>();
        std::vector<WorkUnit> units;
        try {
            units = job.work_units();  // the reference panics on rows_per_work_unit == 0 (job.rs:67-70)
        } catch (const FluxError &e) {
            std::fprintf(stderr, "RenderManager: %s\n", e.what());
            sj.notify_done->send(0);
            continue;
        }
        auto wu_queue = std::make_shared<CancellableWorkUnits>(std::move(units));
        auto cancel_ch = sj.notify_cancel;
        bool started_ok = false;
        {
            // On every path out of this block, first `release` lets both threads end, then they are joined.  A producer still blocked
            // in send() must fail once every worker has dropped its Receiver (crossbeam: send on a channel with no receivers errors,
            // manager.rs:131-136); the reference leaves the listener blocked until the JobHandle drops.
            JoiningThread cancel_listener, producer;
            ScopeExit release{[&] {
                wu_queue->cancel();
                ws->close();
                cancel_ch->close();
            }};
            // cancel listener (manager.rs:105-116): ends when a cancel arrives or the job's handle side closes
            cancel_listener = JoiningThread([cancel_ch, wu_queue] {
                if (cancel_ch->recv()) wu_queue->cancel();
            });
            // work-unit producer (manager.rs:118-141): blocks in send() until a worker takes the unit
            producer = JoiningThread([ws, wu_queue] {
                while (auto u = wu_queue->next())
                    if (!ws->send(*u)) break;
                ws->close();  // dropping the Sender: workers' recv() then fails and they finish the job
            });

            RenderEvent started;
            started.kind = RenderEvent::RenderingStarted;  // manager.rs:145-154
            started.job_id = job.id;
            started.time_s = now_s();
            started_ok = sj.result_sender->send(started);
            if (started_ok) {
                auto shared_job = std::make_shared<Job>(job);
                for (const WorkerHandle &w : workers_) w.send(shared_job, ws, sj.result_sender, wg);  // manager.rs:156-162
                wg->wait();                                                                           // manager.rs:166
            }
        }
        if (!started_ok) continue;
        RenderEvent fin;
        fin.kind = RenderEvent::RenderingFinished;  // manager.rs:170-177
        fin.time_s = now_s();
        if (!sj.result_sender->send(fin)) continue;
        sj.notify_done->send(0);  // manager.rs:179-185
    }
}

}  // namespace flux_host
