// flux_host::render_aov_chain without a GPU: a buffer of the wrong size and a max_chain beyond the job's depth are refused before any
// context exists, each with its own message, and a call in order reaches the library, whose answer is then about the device alone
// (FLUX_E_DEVICE here, the buffers on a GPU machine).
#include <cstdio>
#include <string>
#include <vector>

#include "../flux_amd/host/flux_host.hpp"

using namespace flux_host;

static SceneData tiny_scene(size_t w, size_t h) {
    SceneData s;
    s.scene_name = "tiny";
    s.output_settings.image_width = w;
    s.output_settings.image_height = h;
    s.output_settings.pixel_size = 1.0;
    s.camera_settings = CameraSettings{{0.0, 1.0, -6.0}, {0.0, 0.0, 0.0}, {0.0, 1.0, 0.0}};
    s.camera_data = CameraData{1.0, 8.0, 6.0, 0.1};
    s.shapes.push_back(SphereData{{0.0, 0.0, 0.0}, 1.0, ReflectiveData{0.9, {0.9, 0.9, 0.9}}, false});
    s.shapes.push_back(PlaneData{{0.0, -1.0, 0.0}, {0.0, 1.0, 0.0}, MatteData{{0.5, 0.5, 0.5}, {0.0, 0.0, 0.0}, 0.8}});
    return s;
}

static int refused(const SceneData &s, const JobConfiguration &cfg, uint32_t max_chain, std::vector<double> &out, std::string *msg = nullptr) {
    try {
        render_aov_chain(s, cfg, 1, 0, max_chain, out);
    } catch (const FluxError &e) {
        if (msg) *msg = e.what();
        return e.code;
    }
    return FLUX_OK;
}

int main() {
    const size_t w = 5, h = 3;
    const SceneData s = tiny_scene(w, h);
    const JobConfiguration cfg{2, 4, 50};
    int bad = 0;
    std::string msg;
    std::vector<double> small_buf(w * h * FLUX_AOV_CHANNELS - 1), frame(w * h * 3), empty, right(w * h * FLUX_AOV_CHANNELS, -1.0);
    bad += refused(s, cfg, 0, small_buf, &msg) != FLUX_E_INVALID || msg.find("the frame needs 120") == std::string::npos;
    bad += refused(s, cfg, 0, frame, &msg) != FLUX_E_INVALID || msg.find("holds 45 doubles") == std::string::npos;  // a frame is no feature buffer
    bad += refused(s, cfg, 0, empty) != FLUX_E_INVALID;
    bad += refused(s, cfg, 5, right, &msg) != FLUX_E_INVALID || msg.find("max_chain 5 exceeds max_trace_depth 4") == std::string::npos;
    std::vector<double> none;
    bad += refused(tiny_scene(0, 0), cfg, 0, none, &msg) != FLUX_E_INVALID || msg.find("empty frame") == std::string::npos;
    for (double v : right) bad += v != -1.0;  // a refused call writes nothing
    const int rc = refused(s, cfg, 4, right);
    std::printf("valid call: %d\n", rc);
    bad += !(rc == FLUX_OK || rc == FLUX_E_DEVICE);
    std::printf(bad ? "FAILED %d\n" : "all ok\n", bad);
    return bad ? 1 : 0;
}
