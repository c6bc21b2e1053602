// flux_host.hpp -- C++ host side above the C ABI, mirroring the reference's plain-data types and
// its worker interface (same names, same argument meaning), so a GPU sits where a LocalWorker does:
//
//   SceneData & friends        fluxcore/src/scene.rs:12-74, shapes.rs:15-81, color.rs:8-16
//   JobConfiguration, WorkUnit, Job::work_units      fluxcore/src/job.rs:40-88
//   RenderEvent, WorkUnitResult, WorkerInfo, trait Worker, WorkerHandle
//                                                    fluxcore/src/manager.rs:16-52,221-236
//   LocalWorker job loop -> serve_job (GpuWorker, MultiGpuWorker)   fluxcore/src/workers.rs:26-103
//   ImageBuilder, Image::write                       fluxcore/src/manager.rs:278-363, image.rs:43-61
//
// The reference is Rust; this image has no Rust toolchain, so the mirror is C++ (joining threads and a
// small channel instead of crossbeam).  All rendering goes through include/flux_abi.h.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <string>
#include <variant>
#include <vector>

#include "../../include/flux_abi.h"
#include "../csrc/joining_thread.h"

namespace flux_host {

using flux::JoiningThread;

// runs `f` on every path out of the scope, unwinding included
template <class F> struct ScopeExit {
    F f;
    ~ScopeExit() { f(); }
};
template <class F> ScopeExit(F) -> ScopeExit<F>;

struct FluxError : std::runtime_error {
    int code;
    FluxError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

// ---- scene description (the reference's plain data; field and variant names: scene_schema.hpp) ----
struct Color { double r = 0, g = 0, b = 0; };
struct Vec3 { double x = 0, y = 0, z = 0; };

struct MatteData { Color diffuse_color, ambient_color; double diffuse_coefficient = 0; };
struct EmissiveData { Color color; double power = 0; };
struct ReflectiveData { double reflect_amount = 0; Color reflect_color; };
struct GlossyReflectiveData { double reflect_amount = 0; Color reflect_color; double reflect_exponent = 0; };
// extension (include/flux_abi.h FLUX_MAT_DIELECTRIC): Fresnel-sampled glass; a reference node cannot decode it
struct DielectricData { double refraction_index = 1; Color transmit_color; };
using MaterialData = std::variant<MatteData, EmissiveData, ReflectiveData, GlossyReflectiveData, DielectricData>;

struct SphereData { Vec3 center; double radius = 0; MaterialData material; bool invert = false; };
struct PlaneData { Vec3 point, normal; MaterialData material; };
// extension (include/flux_abi.h FLUX_SHAPE_DISK): a closed disk; a reference node cannot decode it
struct DiskData { Vec3 center, normal; double radius = 0; MaterialData material; };
// extension (include/flux_abi.h FLUX_SHAPE_BOX): an axis-aligned box, corner0 < corner1 on every axis; `invert` is optional in YAML
struct BoxData { Vec3 corner0, corner1; MaterialData material; bool invert = false; };
using ShapeData = std::variant<SphereData, PlaneData, DiskData, BoxData>;

struct CameraSettings { Vec3 eye, look_at, up; };
struct CameraData { double zoom_factor = 1, view_plane_distance = 0, focal_distance = 0, lens_radius = 0; };
struct OutputSettings { size_t image_width = 0, image_height = 0; double pixel_size = 0; };

struct SceneData {
    std::string scene_name;
    OutputSettings output_settings;
    Color background;
    std::vector<ShapeData> shapes;
    CameraSettings camera_settings;
    CameraData camera_data;
};

// serde_yaml::from_reader (flux/src/main.rs:27-29); throws FluxError(FLUX_E_INVALID) with a
// serde-style message on missing fields / unknown variants.
SceneData scene_from_yaml_file(const std::string &path);
SceneData scene_from_yaml_text(const std::string &text);

// ---- jobs ---------------------------------------------------------------------------------------
struct JobID { size_t allocator_id = 0, id = 0; };
struct JobConfiguration { size_t sample_root = 1, max_trace_depth = 5, rows_per_work_unit = 50; };
struct WorkUnit { size_t row_start = 0, row_end = 0; JobID job_id; };

struct Job {
    JobID id;
    SceneData scene_data;
    JobConfiguration config;
    std::vector<WorkUnit> work_units() const;  // job.rs:65-88 (via flux_work_units)
};

struct WorkUnitResult {
    WorkUnit work_unit;
    std::vector<std::vector<Color>> rows;
};

struct RenderEvent {  // manager.rs:16-22
    enum Kind { RenderingStarted, ImageInfo, RowsReady, RenderingFinished } kind = RowsReady;
    JobID job_id;
    double time_s = 0;  // start_time / end_time (seconds on a steady clock)
    std::string scene_name;
    size_t width = 0, height = 0;
    WorkUnitResult result;
};

struct WorkerInfo { size_t num_threads = 0; };  // manager.rs:221-230

// unbounded MPMC channel with close(), enough of crossbeam::channel for the job loop
template <typename T>
class Channel {
public:
    // capacity 0 = unbounded; otherwise crossbeam's bounded(cap): send blocks while the queue is full
    explicit Channel(size_t capacity = 0) : cap_(capacity) {}
    // returns false if the channel was closed before the value could be queued (crossbeam: send() -> Err)
    bool send(T v) {
        {
            std::unique_lock<std::mutex> l(mu_);
            if (cap_) space_.wait(l, [&] { return q_.size() < cap_ || closed_; });
            if (closed_) return false;
            q_.push_back(std::move(v));
        }
        cv_.notify_one();
        return true;
    }
    // returns nullopt once closed and drained (crossbeam: recv() -> Err)
    std::optional<T> recv() {
        std::unique_lock<std::mutex> l(mu_);
        cv_.wait(l, [&] { return !q_.empty() || closed_; });
        if (q_.empty()) return std::nullopt;
        T v = std::move(q_.front());
        q_.pop_front();
        l.unlock();
        space_.notify_one();
        return v;
    }
    void close() {
        { std::lock_guard<std::mutex> g(mu_); closed_ = true; }
        cv_.notify_all();
        space_.notify_all();
    }
private:
    size_t cap_ = 0;
    std::mutex mu_;
    std::condition_variable cv_, space_;
    std::deque<T> q_;
    bool closed_ = false;
};

// crossbeam::sync::WaitGroup: a clone is a move-only Ticket, taking one counts up and dropping it counts down; wait() for all
struct WaitGroup {
    class Ticket {
    public:
        Ticket() = default;
        explicit Ticket(std::shared_ptr<WaitGroup> wg) : wg_(std::move(wg)) { wg_->add(); }
        Ticket(Ticket &&) noexcept = default;  // (a moved-from shared_ptr is empty: the source releases nothing)
        Ticket &operator=(Ticket &&o) noexcept {
            if (this != &o) {
                if (wg_) wg_->done();
                wg_ = std::move(o.wg_);
            }
            return *this;
        }
        ~Ticket() { if (wg_) wg_->done(); }
    private:
        std::shared_ptr<WaitGroup> wg_;
    };
    void add() { std::lock_guard<std::mutex> g(mu); n++; }
    void done() { { std::lock_guard<std::mutex> g(mu); n--; } cv.notify_all(); }
    void wait() { std::unique_lock<std::mutex> l(mu); cv.wait(l, [&] { return n == 0; }); }
    std::mutex mu; std::condition_variable cv; int n = 0;
};

// WorkerRequest = Option<(Box<Job>, Receiver<WorkUnit>, Sender<Option<RenderEvent>>, WaitGroup)> (manager.rs:36).  A worker finishes
// a job by letting the request go out of scope: that drops the ticket, on every path (drop(wg), workers.rs:74).
struct WorkerRequest {
    std::shared_ptr<Job> job;
    std::shared_ptr<Channel<WorkUnit>> recv_unit;
    std::shared_ptr<Channel<std::optional<RenderEvent>>> send_result;
    WaitGroup::Ticket ticket;
};

// A mailbox of optional<Msg>, the thread that serves it and the stop-once logic (workers.rs:95-98: send(None), join).  `body` is the
// thread's function and takes its messages with next().  The thread starts in the constructor and is joined by stop() or by the
// destructor, so whatever holds a Service holds it as its LAST data member: every member the body reads is then built before the
// thread starts and destroyed after it is gone, and no owner needs a destructor of its own for that (a base class could not do
// it: its destructor runs after the derived members').
template <class Msg> class Service {
public:
    using Mailbox = Channel<std::optional<Msg>>;
    template <class F> explicit Service(F body) : mailbox_(std::make_shared<Mailbox>()), thread_(std::move(body)) {}
    Service(const Service &) = delete;
    Service &operator=(const Service &) = delete;
    ~Service() { stop(); }
    const std::shared_ptr<Mailbox> &mailbox() const { return mailbox_; }
    // the next message; nothing once stop() was called or the mailbox is closed
    std::optional<Msg> next() {
        auto m = mailbox_->recv();
        if (!m) return std::nullopt;
        return std::move(*m);
    }
    // idempotent, and fine after the body has returned by itself
    void stop() {
        if (stopped_) return;
        stopped_ = true;
        mailbox_->send(std::nullopt);
        thread_.join();
    }
private:
    std::shared_ptr<Mailbox> mailbox_;
    JoiningThread thread_;
    bool stopped_ = false;
};

class WorkerHandle {  // manager.rs:38-52
public:
    explicit WorkerHandle(std::shared_ptr<Channel<std::optional<WorkerRequest>>> s) : sender_(std::move(s)) {}
    // takes the worker's ticket of `wg` (wg.clone(), manager.rs:156-162); a request nobody serves releases it when it is destroyed
    void send(std::shared_ptr<Job> j, std::shared_ptr<Channel<WorkUnit>> r, std::shared_ptr<Channel<std::optional<RenderEvent>>> s,
              const std::shared_ptr<WaitGroup> &wg) const {
        sender_->send(WorkerRequest{std::move(j), std::move(r), std::move(s), WaitGroup::Ticket(wg)});
    }
private:
    std::shared_ptr<Channel<std::optional<WorkerRequest>>> sender_;
};

class Worker {  // trait Worker, manager.rs:232-236
public:
    virtual ~Worker() = default;
    virtual WorkerHandle handle() const = 0;
    virtual void stop() = 0;
    virtual WorkerInfo info() const = 0;
};

// Where a local worker's rows come from, for one job: the image rows [row_start, row_end] as [nrows][W][3] doubles, valid until the
// next call, or nullptr with the library's message left in flux_last_error().
class RowSource {
public:
    virtual ~RowSource() = default;
    virtual const double *rows(size_t row_start, size_t row_end) = 0;
};

// One job of a local worker (the body of LocalWorker's 'main loop, workers.rs:43-75): `open` makes the job's source (nullptr: as
// above), then every unit pulled from the request's channel is answered with a RowsReady.  An inverted range gets one without rows
// (what `row_start..=row_end` renders, trace.rs:62).  A unit past the image, a null from `open` or the source, and a std::exception
// anywhere in the job are reported on stderr after `who` (`range_who` for the unit), counted in GpuWorker::failures() and end the
// job: the reference panics there (workers.rs:78).  The request's ticket is released on return, on every path.
void serve_job(WorkerRequest req, const std::string &who, const std::string &range_who,
               const std::function<std::unique_ptr<RowSource>(const Job &)> &open);

// The GPU sibling of LocalWorker (workers.rs:26-103): one thread; per job it builds the context
// (Scene::from_data + Camera::new) once, then renders the work units it pulls from the shared channel
// and emits RenderEvent::RowsReady.
class GpuWorker : public Worker {
public:
    GpuWorker(int device, uint64_t seed);
    WorkerHandle handle() const override { return WorkerHandle(service_.mailbox()); }
    void stop() override { service_.stop(); }
    WorkerInfo info() const override { return WorkerInfo{1}; }
    // jobs / work units any local worker of this process had to give up (see serve_job); the front-ends exit non-zero when this is > 0
    static int failures();
    static void note_failure();
private:
    void run();
    int device_;
    uint64_t seed_;
    Service<WorkerRequest> service_;  // last: see Service
};

// The GPUs of this node as ONE worker behind the same trait: per job it creates a flux_multi (include/flux_abi.h: one context per
// device holding its share of the sample tables, created concurrently) and, when the first work unit arrives, renders the WHOLE frame
// with one launch per device and one RCCL all-gather; every unit it pulls from the shared channel (workers.rs:56) is then answered
// from that frame.  Against one GpuWorker per device -- each building ALL tables and pulling fifty-row units (12 units over 8 GPUs: two
// rounds, 75 % at best), each unit copied back through the host -- the frame costs one balanced launch and one device-side gather.
// It renders every row itself, so it is for a pool WITHOUT other workers (flux_cli.cpp selects it only then): rows a NetworkWorker
// renders as well would be work done twice.
class MultiGpuWorker : public Worker {
public:
    MultiGpuWorker(std::vector<int> devices, uint64_t seed, int shard = FLUX_SHARD_AUTO);
    WorkerHandle handle() const override { return WorkerHandle(service_.mailbox()); }
    void stop() override { service_.stop(); }
    WorkerInfo info() const override { return WorkerInfo{devices_.size()}; }
    // ms of the most recent job: flux_multi_timing's words (create, slowest context, communicators, frame, kernel, gather, reassembly, copy)
    std::vector<double> last_timing() const;
private:
    void run();
    std::vector<int> devices_;
    uint64_t seed_;
    int shard_;
    mutable std::mutex mu_;
    std::vector<double> timing_;
    Service<WorkerRequest> service_;  // last: see Service
};

// ImageBuilder (manager.rs:278-363): assembles RowsReady rows, prints the total time and writes
// "<scene_name>.ppm" on RenderingFinished; rows never received are written as zeros (image.rs:55-59).
class ImageBuilder {
public:
    ImageBuilder();
    std::shared_ptr<Channel<std::optional<RenderEvent>>> sender() const { return service_.mailbox(); }
    void stop() { service_.stop(); }
    std::string output_dir = ".";
    double total_time_s = 0;
    std::string written_path;
    std::vector<double> image;  // the frame as written, [H][W][3]: filled with written_path (read it after stop())
private:
    void run();
    Service<RenderEvent> service_;  // last: see Service
};

// JobIDAllocator (job.rs:14-34): allocator_id is random per allocator, ids count from 0.
class JobIDAllocator {
public:
    JobIDAllocator();
    JobID next_id() { return JobID{allocator_id_, next_++}; }
private:
    size_t allocator_id_ = 0, next_ = 0;
};

// CancellableIterator (manager.rs:365-393) over a job's work units: after cancel() next() yields nothing.
class CancellableWorkUnits {
public:
    explicit CancellableWorkUnits(std::vector<WorkUnit> items) : items_(std::move(items)) {}
    void cancel() { std::lock_guard<std::mutex> g(mu_); cancelled_ = true; }
    std::optional<WorkUnit> next() {
        std::lock_guard<std::mutex> g(mu_);
        if (cancelled_ || pos_ >= items_.size()) return std::nullopt;
        return items_[pos_++];
    }
private:
    std::mutex mu_;
    std::vector<WorkUnit> items_;
    size_t pos_ = 0;
    bool cancelled_ = false;
};

// JobHandle (manager.rs:54-70): wait() blocks until the manager has sent RenderingFinished for the job;
// cancel() stops the hand-out of further work units (units already pulled by a worker complete).
class JobHandle {
public:
    JobID job_id;
    void wait() const { waiter_->recv(); }
    void cancel() const { canceller_->send(0); }
private:
    friend class RenderManager;
    std::shared_ptr<Channel<int>> waiter_, canceller_;
};

// RenderManager (manager.rs:30-219): a thread that takes scheduled jobs one at a time; per job it sends
// ImageInfo, starts a producer thread that feeds the job's work units into ONE bounded(1) channel shared by
// all workers (dynamic load balancing: a worker pulls its next unit when it is free) and a cancel-listener
// thread, sends RenderingStarted (its timestamp precedes the fan-out, manager.rs:145), hands the job to
// every worker, waits for the WaitGroup, sends RenderingFinished and wakes JobHandle::wait().
class RenderManager {
public:
    explicit RenderManager(std::vector<WorkerHandle> workers);  // throws on an empty vector (manager.rs:74-76)
    JobHandle schedule_job(const SceneData &scene_data, const JobConfiguration &config,
                           std::shared_ptr<Channel<std::optional<RenderEvent>>> result_sender);
    void stop() { service_.stop(); }
private:
    struct ScheduledJob {
        Job job;
        std::shared_ptr<Channel<int>> notify_done, notify_cancel;
        std::shared_ptr<Channel<std::optional<RenderEvent>>> result_sender;
    };
    void run();
    std::vector<WorkerHandle> workers_;
    JobIDAllocator ids_;
    Service<ScheduledJob> service_;  // last: see Service
};

// SceneData -> flux_scene_desc (+ the shape storage it points to)
struct AbiScene {
    std::vector<flux_shape> shapes;
    std::string name;
    flux_scene_desc desc{};
    explicit AbiScene(const SceneData &sd);
};

// ---- first-hit feature buffers (include/flux_abi.h flux_render_aov_rows) --------------------------
// The frame's albedo, normal, depth and coverage, [H][W][FLUX_AOV_CHANNELS]: a context on `device` for the job, one
// flux_render_aov_rows over the frame, the context dropped.  Throws FluxError with the library's message.
std::vector<double> render_feature_buffers(const SceneData &scene_data, const JobConfiguration &config, uint64_t seed, int device);

// The same buffers at the first non-specular hit (include/flux_abi.h flux_render_aov_chain_rows), chains of at most `max_chain`
// segments (0: max_trace_depth), into `out`, which must hold width * height * FLUX_AOV_CHANNELS doubles: a buffer of another size and
// a max_chain beyond the job's max_trace_depth are refused before any context exists.  Throws FluxError with the library's message.
void render_aov_chain(const SceneData &scene_data, const JobConfiguration &config, uint64_t seed, int device, uint32_t max_chain,
                      std::vector<double> &out);

// One channel group of such a frame as an image for flux_write_ppm: [H][W] RGB in [0, 1].
//   Albedo    min(1, x) per channel
//   Normal    0.5 + 0.5 n / |n| (the zero vector: 0.5)
//   Depth     grey coverage * (1 - t / t_max), t_max the largest finite depth of the frame (1 if there is none above 0); a
//             non-finite depth: 0
//   Coverage  grey
enum class AovKind { Albedo, Normal, Depth, Coverage };
std::vector<double> aov_image(const double *aov, size_t width, size_t height, AovKind kind);

// ---- the a-trous denoiser (include/flux_abi.h flux_denoise) ---------------------------------------
// A frame `rgb` [H][W][3] and its feature buffers `aov` [H][W][FLUX_AOV_CHANNELS] filtered on `device` with the default
// parameters: the filtered frame.  Throws FluxError with the library's message.
std::vector<double> denoise_frame(const std::vector<double> &rgb, const std::vector<double> &aov, size_t width, size_t height, int device);

// ---- per-pixel sample moments and the measured-variance filter (include/flux_abi.h flux_render_moments_rows, flux_denoise_moments) ----
// The frame with its measured variance, [H][W][FLUX_MOMENT_CHANNELS]: a context on `device` for the job, one
// flux_render_moments_rows over the frame, the context dropped.  Throws FluxError with the library's message (sample_root 1 is
// refused: one sample has no variance).
std::vector<double> render_moments(const SceneData &scene_data, const JobConfiguration &config, uint64_t seed, int device);
// `moments` [H][W][FLUX_MOMENT_CHANNELS] and `aov` [H][W][FLUX_AOV_CHANNELS] filtered on `device` with the default parameters: the
// filtered frame [H][W][3].  Buffers of another size are refused before the library is called.
std::vector<double> denoise_moments_frame(const std::vector<double> &moments, const std::vector<double> &aov, size_t width, size_t height,
                                          int device);

// ---- adaptive sampling (include/flux_abi.h flux_render_adaptive_rows) -----------------------------------------------------------
// What a call returns: the moments layout with each pixel's own sample count, the passes per pixel, and the call's `info` words.
struct AdaptiveFrame {
    std::vector<double> moments;   // [H][W][FLUX_MOMENT_CHANNELS]
    std::vector<uint32_t> passes;  // [H][W]
    uint64_t rounds = 0, pixel_passes = 0, pixels_at_max_passes = 0;
};
// The defaults of include/flux_abi.h (FLUX_ADAPTIVE_*).
flux_adaptive_params adaptive_defaults();
// A context on `device` for the job, one flux_render_adaptive_rows over the frame, the context dropped.  A max_passes beyond the
// image width is refused before any context exists; everything else throws FluxError with the library's message.
AdaptiveFrame render_adaptive(const SceneData &scene_data, const JobConfiguration &config, uint64_t seed, int device,
                              const flux_adaptive_params &params);
// Channels 0..2 of a moments buffer as a frame [H][W][3], and a pass map as a grey frame c / max_passes.  Buffers that do not hold
// width * height pixels, and max_passes 0, are refused.
std::vector<double> moments_frame(const std::vector<double> &moments, size_t width, size_t height);
std::vector<double> passes_image(const std::vector<uint32_t> &passes, size_t width, size_t height, uint32_t max_passes);

}  // namespace flux_host
