// flux_host's adaptive-sampling helpers without a GPU: buffers of the wrong size are refused before anything else happens, a
// max_passes beyond the image width is refused before a context is asked for, and a valid call reaches the library, whose answer is
// then about the device alone (FLUX_E_DEVICE here, a frame on a GPU machine).
#include <cstdio>
#include <vector>

#include "../flux_amd/host/flux_host.hpp"

using namespace flux_host;

template <class F> static int code_of(F &&f) {
    try {
        f();
    } catch (const FluxError &e) {
        return e.code;
    }
    return FLUX_OK;
}

int main() {
    const size_t w = 5, h = 3;
    int bad = 0;
    const std::vector<double> moments(w * h * FLUX_MOMENT_CHANNELS, 0.25);
    std::vector<uint32_t> passes(w * h, 2);
    passes[4] = 8;
    passes[7] = 11;  // beyond max_passes: clamped to white, never beyond the image's range
    bad += code_of([&] { moments_frame(std::vector<double>(w * h * 3), w, h); }) != FLUX_E_INVALID;  // a frame is not a moments buffer
    bad += code_of([&] { moments_frame(moments, w + 1, h); }) != FLUX_E_INVALID;
    bad += code_of([&] { passes_image(std::vector<uint32_t>(w * h - 1), w, h, 8); }) != FLUX_E_INVALID;
    bad += code_of([&] { passes_image(passes, h, w + 1, 8); }) != FLUX_E_INVALID;
    bad += code_of([&] { passes_image(passes, w, h, 0); }) != FLUX_E_INVALID;
    const std::vector<double> rgb = moments_frame(moments, w, h), grey = passes_image(passes, w, h, 8);
    bad += rgb.size() != w * h * 3 || rgb[7] != 0.25;
    bad += grey.size() != w * h * 3 || grey[0] != 0.25 || grey[4 * 3 + 2] != 1.0 || grey[7 * 3 + 1] != 1.0;

    const flux_adaptive_params d = adaptive_defaults();
    bad += !(d.threshold == FLUX_ADAPTIVE_THRESHOLD && d.lum_floor == FLUX_ADAPTIVE_LUM_FLOOR && d.min_passes == FLUX_ADAPTIVE_MIN_PASSES &&
             d.max_passes == FLUX_ADAPTIVE_MAX_PASSES && d.dilate == FLUX_ADAPTIVE_DILATE && d.reserved == 0);

    SceneData sd;
    sd.scene_name = "selftest";
    sd.output_settings.image_width = 4;
    sd.output_settings.image_height = 3;
    sd.output_settings.pixel_size = 1.0;
    const JobConfiguration job{2, 5, 50};
    flux_adaptive_params p = d;
    p.max_passes = 5;  // > the 4 sample sets of a 4-pixel-wide image: no context is created for this
    bad += code_of([&] { render_adaptive(sd, job, 7, 0, p); }) != FLUX_E_INVALID;
    p.max_passes = 4;
    const int rc = code_of([&] { render_adaptive(sd, job, 7, 0, p); });
    std::printf("valid call: %d\n", rc);
    bad += !(rc == FLUX_OK || rc == FLUX_E_DEVICE || rc == FLUX_E_INVALID);
    std::printf(bad ? "FAILED %d\n" : "all ok\n", bad);
    return bad ? 1 : 0;
}
