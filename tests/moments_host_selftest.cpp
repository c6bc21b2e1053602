// flux_host::denoise_moments_frame without a GPU: buffers of the wrong size are refused before the library is called, and buffers of
// the right size reach flux_denoise_moments, whose answer is then about the device alone (FLUX_E_DEVICE here, a frame on a GPU machine).
#include <cstdio>
#include <vector>

#include "../flux_amd/host/flux_host.hpp"

using namespace flux_host;

static int refused(const std::vector<double> &moments, const std::vector<double> &aov, size_t w, size_t h) {
    try {
        denoise_moments_frame(moments, aov, w, h, 0);
    } catch (const FluxError &e) {
        return e.code;
    }
    return FLUX_OK;
}

int main() {
    const size_t w = 5, h = 3;
    const std::vector<double> moments(w * h * FLUX_MOMENT_CHANNELS, 0.25), aov(w * h * FLUX_AOV_CHANNELS, 0.5);
    int bad = 0;
    bad += refused(std::vector<double>(w * h * FLUX_MOMENT_CHANNELS - 1), aov, w, h) != FLUX_E_INVALID;
    bad += refused(std::vector<double>(w * h * 3), aov, w, h) != FLUX_E_INVALID;  // a frame is not a moments buffer
    bad += refused(moments, std::vector<double>(w * h * 3), w, h) != FLUX_E_INVALID;
    bad += refused(moments, aov, h, w + 1) != FLUX_E_INVALID;
    bad += refused({}, {}, 0, 0) != FLUX_E_INVALID;  // the library's own check: width and height 0
    const int rc = refused(moments, aov, w, h);
    std::printf("valid buffers: %d\n", rc);
    bad += !(rc == FLUX_OK || rc == FLUX_E_DEVICE);
    std::printf(bad ? "FAILED %d\n" : "all ok\n", bad);
    return bad ? 1 : 0;
}
