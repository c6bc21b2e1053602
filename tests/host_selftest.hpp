// What the host selftests of the extensions (tests/{disk,dielectric,box}_host_selftest.cpp) share: the CHECK macro of a main() that
// exits 1 on the first failure, the loader-error probe, the "shape <i> <fields>" dump that the Python tests compare with their own
// loader, and the opening of the CBOR round trip through the node protocol's SetJob message.
#pragma once
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "../flux_amd/host/flux_host.hpp"
#include "../flux_amd/host/flux_net.hpp"

using namespace flux_host;

#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);      \
            return 1;                                                       \
        }                                                                   \
    } while (0)

// scene_from_yaml_text(text) fails with FLUX_E_INVALID and a message that holds `needle`
inline bool throws(const std::string &text, const std::string &needle) {
    try {
        scene_from_yaml_text(text);
    } catch (const FluxError &e) {
        if (std::string(e.what()).find(needle) != std::string::npos && e.code == FLUX_E_INVALID) return true;
        std::printf("message: %s\n", e.what());
    }
    return false;
}

inline bool same_vec(const Vec3 &a, const Vec3 &b) { return a.x == b.x && a.y == b.y && a.z == b.z; }

// `text` with the first `what` replaced by `with`; "" where there is none
inline std::string replaced(std::string text, const std::string &what, const std::string &with) {
    const size_t at = text.find(what);
    if (at == std::string::npos) return "";
    return text.replace(at, what.size(), with);
}

inline std::string read_file(const std::string &path) {
    std::ifstream f(path);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

// one line per flux_shape; %.17g round-trips every double, so the Python side compares the fields for equality
inline void print_flux_shapes(const AbiScene &abi) {
    for (size_t i = 0; i < abi.shapes.size(); i++) {
        const flux_shape &s = abi.shapes[i];
        std::printf("shape %zu %d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", i,
                    s.kind, s.invert, s.p[0], s.p[1], s.p[2], s.n[0], s.n[1], s.n[2], s.radius, s.material.kind, s.material.color[0],
                    s.material.color[1], s.material.color[2], s.material.ambient[0], s.material.ambient[1], s.material.ambient[2],
                    s.material.k, s.material.exponent);
    }
}

// CBOR: SetJob with the scene `sd` encoded to `raw`, decoded to `back` with the same shape variants, and re-encoded to the same
// bytes.  0, or 1 after a FAILED line -- as main() returns.
inline int set_job_round_trip(const SceneData &sd, std::string &raw, NetworkWorkerRequest &back) {
    NetworkWorkerRequest req;
    req.kind = NetworkWorkerRequest::SetJob;
    req.job.scene_data = sd;
    req.job.config = JobConfiguration{3, 5, 50};
    cbor::Encoder e;
    encode_request(e, req);
    raw = e.out;
    cbor::StringReader r(raw);
    cbor::Decoder d(r);
    CHECK(decode_request(d, back));
    CHECK(back.kind == NetworkWorkerRequest::SetJob);
    CHECK(back.job.scene_data.shapes.size() == sd.shapes.size());
    for (size_t i = 0; i < sd.shapes.size(); i++) CHECK(back.job.scene_data.shapes[i].index() == sd.shapes[i].index());
    cbor::Encoder e2;
    encode_request(e2, back);
    CHECK(e2.out == raw);
    return 0;
}
