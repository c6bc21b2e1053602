// flux_cli.cpp -- flag-compatible `flux` front-end driving GpuWorkers.
//
// Mirrors flux/src/main.rs: config_from_args (:126-205; same flags, same defaults: root 1, depth 5,
// 50 rows per work unit), load YAML -> SceneData (:27-29), start workers (:37-70), schedule one job and
// wait (:92-94), ImageBuilder writes "<scene_name>.ppm" into the cwd and prints the total time
// (manager.rs:326-335).  -n/--node ADDRESS[:PORT] adds NetworkWorkers (flux_node processes, flux_net.hpp) and
// -L leaves the local GPUs out, as in main.rs:37-66.  Additions: --seed (the reference seeds from OS
// entropy), --gpus, --outdir, --split, --aov, --aov-chain, --denoise, --denoise-variance, --denoise-guides, --adaptive, --adaptive-max-passes.  Not carried over: -g (SDL preview), rejected.
//
// --split sets|rows|units: how the local GPUs share a frame.  `units` is the reference's scheme -- one worker per device pulling
// WorkUnits from the shared channel (manager.rs:100) --, `sets` / `rows` hand the node's GPUs to ONE MultiGpuWorker (flux_multi_*:
// per-device contexts with 1/G of the tables, one launch per device, one RCCL all-gather).  Default: sets (rows below 64 spp) when
// two or more local GPUs are the whole pool, units otherwise (a pool with network nodes needs the shared channel's balancing).
// --aov: after the frame is written, the first-hit feature buffers of the same job (include/flux_abi.h flux_render_aov_rows: the
// job's --seed and -r) are rendered on local device 0 and written beside it as <scene_name>.albedo.ppm, .normal.ppm, .depth.ppm
// and .coverage.ppm (flux_host.hpp aov_image).  They never travel through the worker / node protocol, so a run without a local
// GPU (-L, --gpus 0, none visible) refuses the flag before any job starts.
// --denoise: the finished frame and the feature buffers of the same job go through the a-trous filter (flux_abi.h flux_denoise) on
// local device 0 and the result is written beside the frame as <scene_name>.denoised.ppm; refused like --aov without a local GPU.
// With --aov as well the feature buffers are rendered once and all five files are written.
// --aov-chain K: the feature buffers at the first non-specular hit (flux_render_aov_chain_rows, chains of at most K segments, 0 = the
// tracing depth) as <scene_name>.chain_albedo.ppm, .chain_normal.ppm, .chain_depth.ppm and .chain_coverage.ppm, mapped as --aov maps
// them.  --denoise-guides first|chain says which buffers steer --denoise (default first).  A K beyond the tracing depth, another word
// for the guides, --denoise-guides without --denoise, and either flag without a local GPU end the run with status 2 before any job.
// --denoise-variance measured|spatial (with --denoise; default spatial): `measured` renders the job's per-pixel sample moments on local
// device 0 (flux_render_moments_rows: the frame again, with the variance of its samples) and writes <scene_name>.denoised.ppm from
// them through flux_denoise_moments, which takes the noise from the samples instead of guessing it from the frame.  Without
// --denoise, or with another word, the flag is refused with status 2 before any job starts.
// --adaptive <threshold> [--adaptive-max-passes M, default 8]: after the frame is written, the job is rendered once more on local
// device 0 with adaptive sampling (flux_abi.h flux_render_adaptive_rows: passes of sample_root^2 samples, further ones only where the
// relative standard error exceeds the threshold; the other parameters at their defaults) and written as <scene_name>.adaptive.ppm,
// with the passes per pixel as <scene_name>.passes.ppm (grey, c / M); the rounds and the mean samples per pixel are printed.  Refused
// like --aov without a local GPU.  A threshold that is no finite number >= 0, M = 0, or --adaptive-max-passes without --adaptive,
// exits with status 2 before any job starts.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "flux_host.hpp"
#include "flux_net.hpp"

using namespace flux_host;

namespace {

const size_t DEFAULT_SAMPLE_ROOT = 1;  // flux/src/main.rs:20
const size_t DEFAULT_DEPTH = 5;        // flux/src/main.rs:21

struct Config {  // flux/src/main.rs:115-124
    std::vector<std::string> network_workers;
    bool use_local_worker = true;
    size_t sample_root = DEFAULT_SAMPLE_ROOT;
    size_t max_depth = DEFAULT_DEPTH;
    size_t rows_per_work_unit = 50;
    std::string input_filename;
    bool show_live_preview = false;
    size_t num_threads = 0;
    // additions
    uint64_t seed = 1;
    int gpus = -1;
    std::string outdir = ".";
    std::string split = "auto";
    bool aov = false;
    bool denoise = false;
    std::string denoise_variance;  // "" (not given), "spatial" or "measured"
    std::string denoise_guides;    // "" (not given), "first" or "chain"
    bool aov_chain = false;
    size_t aov_chain_limit = 0;    // --aov-chain K: 0 = the tracing depth
    bool adaptive = false;
    double adaptive_threshold = 0.0;
    size_t adaptive_max_passes = 0;  // 0: not given
};

void usage() {
    std::fprintf(stderr,
                 "flux (MI355X render path)\n\nUSAGE:\n    flux [FLAGS] [OPTIONS] <scene_file>\n\nFLAGS:\n"
                 "    -L               Do not use the local host (its GPUs) for rendering\n"
                 "    -g               Show a live graphical preview window during rendering (not supported)\n"
                 "        --aov        Also write <scene_name>.albedo.ppm, .normal.ppm, .depth.ppm and .coverage.ppm: the first-hit\n"
                 "                     feature buffers of the frame, rendered on local GPU 0\n"
                 "        --denoise    Also write <scene_name>.denoised.ppm: the frame after a feature-guided a-trous filter on local\n"
                 "                     GPU 0 (for noisy previews of 1-16 samples per pixel; a clean frame may lose detail)\n\nOPTIONS:\n"
                 "        --denoise-variance <measured|spatial>  with --denoise: where the filter takes a pixel's noise from [default spatial:\n"
                 "                     the frame's neighbourhood; measured: the variance of the pixel's samples, from one more render pass]\n"
                 "        --denoise-guides <first|chain>  with --denoise: the feature buffers that steer the filter [default first: what a pixel\n"
                 "                     sees first; chain: what it sees through mirrors and glass, the first non-specular hit]\n"
                 "        --aov-chain <K>  Also write <scene_name>.chain_albedo.ppm, .chain_normal.ppm, .chain_depth.ppm and .chain_coverage.ppm:\n"
                 "                     the feature buffers at the first non-specular hit, Reflective and Dielectric bounces followed for at\n"
                 "                     most K segments (0: the tracing depth; at most the tracing depth), rendered on local GPU 0\n"
                 "        --adaptive <THRESHOLD>   Also write <scene_name>.adaptive.ppm and <scene_name>.passes.ppm: the job with adaptive sampling on\n"
                 "                     local GPU 0 -- further passes of ROOT^2 samples only where the relative standard error exceeds THRESHOLD\n"
                 "        --adaptive-max-passes <M>  with --adaptive: most passes a pixel takes [default 8; at most the image width]\n"
                 "    -d, --depth <DEPTH>          Tracing depth [default 5]\n"
                 "    -n, --node <ADDRESS[:PORT]>  Render using the flux_node process at this address (repeatable)\n"
                 "    -R, --rows <COUNT>           Image rows per work unit [default 50]\n"
                 "    -r, --root <ROOT>            Sample root [default 1]\n"
                 "    -t, --threads <N>            CPU rendering threads (accepted, unused)\n"
                 "        --seed <SEED>            RNG seed [default 1]\n"
                 "        --gpus <N>               number of GPUs to use [default: all]\n"
                 "        --outdir <DIR>           where <scene_name>.ppm is written [default .]\n"
                 "        --split <sets|rows|units> how the local GPUs share a frame [default: sets for >= 2 GPUs without nodes, else units]\n");
}

size_t parse_usize(const char *flag, const char *v) {
    char *end = nullptr;
    unsigned long long x = std::strtoull(v, &end, 10);
    if (end == v || *end != '\0' || v[0] == '-') {
        // usize::from_str(..).unwrap() panics in the reference
        std::fprintf(stderr, "error: invalid value '%s' for '%s'\n", v, flag);
        std::exit(2);
    }
    return (size_t)x;
}

Config config_from_args(int argc, char **argv) {
    Config c;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto need = [&](const char *flag) -> const char * {
            if (i + 1 >= argc) {
                std::fprintf(stderr, "error: The argument '%s' requires a value\n", flag);
                std::exit(2);
            }
            return argv[++i];
        };
        if (a == "-h" || a == "--help") {
            usage();
            std::exit(0);
        } else if (a == "-d" || a == "--depth") {
            c.max_depth = parse_usize("--depth", need("--depth"));
        } else if (a == "-R" || a == "--rows") {
            c.rows_per_work_unit = parse_usize("--rows", need("--rows"));
        } else if (a == "-r" || a == "--root") {
            c.sample_root = parse_usize("--root", need("--root"));
        } else if (a == "-t" || a == "--threads") {
            c.num_threads = parse_usize("--threads", need("--threads"));
        } else if (a == "-n" || a == "--node") {
            c.network_workers.push_back(need("--node"));
        } else if (a == "-L") {
            c.use_local_worker = false;
        } else if (a == "-g") {
            c.show_live_preview = true;
        } else if (a == "--seed") {
            c.seed = (uint64_t)parse_usize("--seed", need("--seed"));
        } else if (a == "--gpus") {
            c.gpus = (int)parse_usize("--gpus", need("--gpus"));
        } else if (a == "--aov") {
            c.aov = true;
        } else if (a == "--denoise") {
            c.denoise = true;
        } else if (a == "--denoise-variance") {
            c.denoise_variance = need("--denoise-variance");
            if (c.denoise_variance != "measured" && c.denoise_variance != "spatial") {
                std::fprintf(stderr, "error: invalid value '%s' for '--denoise-variance' (measured, spatial)\n", c.denoise_variance.c_str());
                std::exit(2);
            }
        } else if (a == "--denoise-guides") {
            c.denoise_guides = need("--denoise-guides");
            if (c.denoise_guides != "first" && c.denoise_guides != "chain") {
                std::fprintf(stderr, "error: invalid value '%s' for '--denoise-guides' (first, chain)\n", c.denoise_guides.c_str());
                std::exit(2);
            }
        } else if (a == "--aov-chain") {
            c.aov_chain_limit = parse_usize("--aov-chain", need("--aov-chain"));
            c.aov_chain = true;
        } else if (a == "--adaptive") {
            const char *v = need("--adaptive");
            char *end = nullptr;
            c.adaptive_threshold = std::strtod(v, &end);
            if (end == v || *end != '\0' || !std::isfinite(c.adaptive_threshold) || c.adaptive_threshold < 0.0) {
                std::fprintf(stderr, "error: invalid value '%s' for '--adaptive' (a finite threshold >= 0)\n", v);
                std::exit(2);
            }
            c.adaptive = true;
        } else if (a == "--adaptive-max-passes") {
            c.adaptive_max_passes = parse_usize("--adaptive-max-passes", need("--adaptive-max-passes"));
            if (c.adaptive_max_passes < 1 || c.adaptive_max_passes > 0xffffffffull) {
                std::fprintf(stderr, "error: invalid value for '--adaptive-max-passes' (at least 1)\n");
                std::exit(2);
            }
        } else if (a == "--outdir") {
            c.outdir = need("--outdir");
        } else if (a == "--split") {
            c.split = need("--split");
            if (c.split != "sets" && c.split != "rows" && c.split != "units" && c.split != "auto") {
                std::fprintf(stderr, "error: invalid value '%s' for '--split' (sets, rows, units)\n", c.split.c_str());
                std::exit(2);
            }
        } else if (!a.empty() && a[0] == '-') {
            std::fprintf(stderr, "error: Found argument '%s' which wasn't expected\n", a.c_str());
            std::exit(2);
        } else if (c.input_filename.empty()) {
            c.input_filename = a;
        } else {
            std::fprintf(stderr, "error: Found argument '%s' which wasn't expected\n", a.c_str());
            std::exit(2);
        }
    }
    if (!c.denoise_variance.empty() && !c.denoise) {
        std::fprintf(stderr, "error: --denoise-variance says how --denoise measures the noise and needs that flag\n");
        std::exit(2);
    }
    if (!c.denoise_guides.empty() && !c.denoise) {
        std::fprintf(stderr, "error: --denoise-guides says which feature buffers steer --denoise and needs that flag\n");
        std::exit(2);
    }
    if (c.aov_chain && c.aov_chain_limit > c.max_depth) {  // (after the loop: --depth may follow the flag)
        std::fprintf(stderr, "error: invalid value '%zu' for '--aov-chain' (at most the tracing depth %zu; 0 means the tracing depth)\n",
                     c.aov_chain_limit, c.max_depth);
        std::exit(2);
    }
    if (c.adaptive_max_passes != 0 && !c.adaptive) {
        std::fprintf(stderr, "error: --adaptive-max-passes bounds the passes of --adaptive and needs that flag\n");
        std::exit(2);
    }
    if (c.input_filename.empty()) {
        std::fprintf(stderr, "error: The following required arguments were not provided:\n    <scene_file>\n");
        usage();
        std::exit(2);
    }
    return c;
}

}  // namespace

int main(int argc, char **argv) {
    Config config = config_from_args(argc, argv);
    if (config.show_live_preview) {
        std::fprintf(stderr, "error: -g: the SDL live preview is not part of the MI355X render path\n");
        return 2;
    }
    SceneData s;
    try {
        s = scene_from_yaml_file(config.input_filename);
    } catch (const FluxError &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    if (config.aov && (!config.use_local_worker || config.gpus == 0 || flux_device_count() < 1)) {
        std::fprintf(stderr, "error: --aov renders the feature buffers on a local GPU, and this run has none (-L, --gpus 0 or no HIP device visible)\n");
        return 2;
    }
    if (config.aov_chain && (!config.use_local_worker || config.gpus == 0 || flux_device_count() < 1)) {
        std::fprintf(stderr, "error: --aov-chain renders the feature buffers on a local GPU, and this run has none (-L, --gpus 0 or no HIP device visible)\n");
        return 2;
    }
    if (config.denoise && (!config.use_local_worker || config.gpus == 0 || flux_device_count() < 1)) {
        std::fprintf(stderr, "error: --denoise filters the frame on a local GPU, and this run has none (-L, --gpus 0 or no HIP device visible)\n");
        return 2;
    }
    if (config.adaptive && (!config.use_local_worker || config.gpus == 0 || flux_device_count() < 1)) {
        std::fprintf(stderr, "error: --adaptive renders the adaptive frame on a local GPU, and this run has none (-L, --gpus 0 or no HIP device visible)\n");
        return 2;
    }
    // main.rs:37-66: the local worker(s) unless -L, then one NetworkWorker per -n
    int ndev = config.use_local_worker ? flux_device_count() : 0;
    if (config.use_local_worker && ndev < 1) {
        std::fprintf(stderr, "error: no HIP device visible (this renderer has no CPU fallback)\n");
        return 1;
    }
    if (config.gpus > 0 && config.gpus < ndev) ndev = config.gpus;

    std::vector<std::unique_ptr<Worker>> workers;
    std::vector<WorkerHandle> handles;
    std::string split = config.split;
    if (split == "auto") split = (ndev >= 2 && config.network_workers.empty()) ? "sets" : "units";
    if (split != "units" && !config.network_workers.empty()) {
        std::fprintf(stderr, "error: --split %s renders whole frames on the local GPUs and cannot share a job with -n nodes; use --split units\n",
                     split.c_str());
        return 2;
    }
    MultiGpuWorker *multi = nullptr;
    if (split != "units" && ndev >= 1) {
        std::vector<int> devs;
        for (int d = 0; d < ndev; d++) devs.push_back(d);
        // (sets need 64 spp: below that the library's AUTO picks rows)
        const int shard = split == "rows" ? FLUX_SHARD_ROWS : (config.sample_root * config.sample_root >= 64 ? FLUX_SHARD_SETS : FLUX_SHARD_AUTO);
        multi = new MultiGpuWorker(devs, config.seed, shard);
        workers.emplace_back(multi);
        handles.push_back(workers.back()->handle());
    } else {
        for (int d = 0; d < ndev; d++) {
            workers.emplace_back(new GpuWorker(d, config.seed));
            handles.push_back(workers.back()->handle());
        }
    }
    for (const std::string &endpoint : config.network_workers) {
        std::printf("Connecting to worker %s\n", endpoint.c_str());
        try {
            workers.emplace_back(new NetworkWorker(endpoint));
        } catch (const FluxError &e) {
            std::fprintf(stderr, "Error connecting to %s: %s\n", endpoint.c_str(), e.what());  // main.rs:60-63
            return 1;
        }
        handles.push_back(workers.back()->handle());
    }
    if (handles.empty()) {
        std::fprintf(stderr, "No workers specified, exiting\n");  // main.rs:68-71
        return 1;
    }
    std::printf("Rendering %s with %d GPU worker(s) and %zu network node(s), sample root %zu, depth %zu, %zu rows per work unit\n",
                s.scene_name.c_str(), ndev, config.network_workers.size(), config.sample_root, config.max_depth, config.rows_per_work_unit);
    if (multi) std::printf("The %d local GPU(s) render whole frames as one worker (--split %s: one launch per device, one RCCL all-gather)\n", ndev, split.c_str());

    // flux/src/main.rs:70-111: manager, image builder, schedule one job, wait, shut everything down
    const JobConfiguration job_config{config.sample_root, config.max_depth, config.rows_per_work_unit};
    ImageBuilder image_builder;
    image_builder.output_dir = config.outdir;
    int rc = 0;
    if (config.rows_per_work_unit == 0) {  // the reference panics in Job::work_units (job.rs:67-70)
        std::fprintf(stderr, "error: Job row per work unit count invalid\n");
        rc = 1;
    } else {
        RenderManager manager(handles);
        JobHandle job = manager.schedule_job(s, job_config, image_builder.sender());
        job.wait();
        manager.stop();
    }
    image_builder.stop();
    if (multi) {
        const std::vector<double> t = multi->last_timing();
        if (t.size() >= 8)
            std::printf("multi-GPU frame: create %.1f ms (slowest context %.1f, communicators %.1f), frame %.1f ms (kernel %.1f, all-gather %.2f, "
                        "reassembly %.2f, copy %.2f)\n", t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7]);
    }
    for (auto &w : workers) w->stop();
    flux_multi_release_comms();
    if (GpuWorker::failures() > 0) {
        std::fprintf(stderr, "error: %d job(s) / work unit(s) were abandoned by a GPU worker; the image is incomplete\n",
                     GpuWorker::failures());
        rc = 1;
    }
    if (rc == 0 && !image_builder.written_path.empty()) {
        const double samples = (double)s.output_settings.image_width * s.output_settings.image_height *
                               config.sample_root * config.sample_root;
        std::printf("wrote %s (%.1f Msamples/s incl. context creation)\n", image_builder.written_path.c_str(),
                    image_builder.total_time_s > 0 ? samples / image_builder.total_time_s / 1e6 : 0.0);
    }
    if (rc == 0 && (config.aov || config.aov_chain || config.denoise) && !image_builder.written_path.empty()) {
        const char *flag = config.aov ? "--aov" : config.aov_chain ? "--aov-chain" : "--denoise";
        try {
            const size_t w = s.output_settings.image_width, h = s.output_settings.image_height;
            const bool chain_guides = config.denoise && config.denoise_guides == "chain";
            // (each buffer is rendered only where a flag asks for it: the first-hit one, the chain one of --aov-chain's K, and the
            // full-depth chain one that steers the filter -- the same buffer where K says the tracing depth)
            std::vector<double> aov, chain, guides;
            if (config.aov || (config.denoise && !chain_guides)) aov = render_feature_buffers(s, job_config, config.seed, 0);
            if (config.aov_chain) {
                flag = "--aov-chain";
                chain.resize(w * h * FLUX_AOV_CHANNELS);
                render_aov_chain(s, job_config, config.seed, 0, (uint32_t)config.aov_chain_limit, chain);
            }
            if (chain_guides) {
                flag = "--denoise";
                if (config.aov_chain && (config.aov_chain_limit == 0 || config.aov_chain_limit == job_config.max_trace_depth)) {
                    guides = chain;
                } else {
                    guides.resize(w * h * FLUX_AOV_CHANNELS);
                    render_aov_chain(s, job_config, config.seed, 0, 0, guides);
                }
            }
            const std::vector<double> &steer = chain_guides ? guides : aov;
            const auto write = [&](const char *name, const std::vector<double> &img) {
                const std::string path = config.outdir + "/" + s.scene_name + "." + name + ".ppm";
                if (flux_write_ppm(path.c_str(), img.data(), w, h, nullptr) != FLUX_OK) throw FluxError(FLUX_E_IO, flux_last_error());
                std::printf("wrote %s\n", path.c_str());
            };
            if (config.aov) {
                const struct { AovKind kind; const char *name; } outs[] = {
                    {AovKind::Albedo, "albedo"}, {AovKind::Normal, "normal"}, {AovKind::Depth, "depth"}, {AovKind::Coverage, "coverage"}};
                for (const auto &o : outs) write(o.name, aov_image(aov.data(), w, h, o.kind));
            }
            if (config.aov_chain) {
                const struct { AovKind kind; const char *name; } outs[] = {{AovKind::Albedo, "chain_albedo"}, {AovKind::Normal, "chain_normal"},
                                                                       {AovKind::Depth, "chain_depth"}, {AovKind::Coverage, "chain_coverage"}};
                for (const auto &o : outs) write(o.name, aov_image(chain.data(), w, h, o.kind));
            }
            if (config.denoise) {
                flag = "--denoise";
                if (config.denoise_variance == "measured")
                    write("denoised", denoise_moments_frame(render_moments(s, job_config, config.seed, 0), steer, w, h, 0));
                else
                    write("denoised", denoise_frame(image_builder.image, steer, w, h, 0));
            }
        } catch (const FluxError &e) {
            std::fprintf(stderr, "error: %s: %s\n", flag, e.what());
            rc = 1;
        }
    }
    if (rc == 0 && config.adaptive && !image_builder.written_path.empty()) {
        try {
            flux_adaptive_params par = adaptive_defaults();
            par.threshold = config.adaptive_threshold;
            if (config.adaptive_max_passes != 0) par.max_passes = (uint32_t)config.adaptive_max_passes;
            const AdaptiveFrame f = render_adaptive(s, job_config, config.seed, 0, par);
            const size_t w = s.output_settings.image_width, h = s.output_settings.image_height;
            const auto write = [&](const char *name, const std::vector<double> &img) {
                const std::string path = config.outdir + "/" + s.scene_name + "." + name + ".ppm";
                if (flux_write_ppm(path.c_str(), img.data(), w, h, nullptr) != FLUX_OK) throw FluxError(FLUX_E_IO, flux_last_error());
                std::printf("wrote %s\n", path.c_str());
            };
            write("adaptive", moments_frame(f.moments, w, h));
            write("passes", passes_image(f.passes, w, h, par.max_passes));
            const double spp = (double)f.pixel_passes * (double)(config.sample_root * config.sample_root) / (double)(w * h);
            std::printf("adaptive: %llu round(s), %.2f samples per pixel on average, %llu pixel(s) at the %u-pass limit\n",
                        (unsigned long long)f.rounds, spp, (unsigned long long)f.pixels_at_max_passes, par.max_passes);
        } catch (const FluxError &e) {
            std::fprintf(stderr, "error: --adaptive: %s\n", e.what());
            rc = 1;
        }
    }
    return rc;
}
