// Disk shapes (extension, include/flux_abi.h FLUX_SHAPE_DISK) in the C++ host layer, CPU only (tests/test_disk_scene.py builds
// and runs it): the YAML loader and its radius checks, the conversion to flux_shape, and a CBOR round trip of a disk scene through
// the node protocol's SetJob message.
//   usage: disk_host_selftest <scenes dir>
// Prints "shape <i> <fields>" for every flux_shape of scenes/disk_light.yml (compared with the Python loader by the test), one
// "ok <name>" per passed check and "all ok" at the end; exits 1 on the first failure.
#include <cmath>
#include <cstdio>
#include <cstring>
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

static bool throws(const std::string &text, const std::string &needle) {
    try {
        scene_from_yaml_text(text);
    } catch (const FluxError &e) {
        if (std::string(e.what()).find(needle) != std::string::npos && e.code == FLUX_E_INVALID) return true;
        std::printf("message: %s\n", e.what());
    }
    return false;
}

static bool same_vec(const Vec3 &a, const Vec3 &b) { return a.x == b.x && a.y == b.y && a.z == b.z; }

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <scenes dir>\n", argv[0]);
        return 2;
    }
    const std::string path = std::string(argv[1]) + "/disk_light.yml";
    const SceneData sd = scene_from_yaml_file(path);
    CHECK(sd.shapes.size() == 13);
    const DiskData *disk = std::get_if<DiskData>(&sd.shapes[1]);
    CHECK(disk != nullptr);
    CHECK(disk->radius == 5.0 && disk->center.x == -9.0 && disk->normal.y == -1.0);
    {
        const AbiScene abi(sd);
        CHECK(abi.desc.num_shapes == 13 && abi.shapes[1].kind == FLUX_SHAPE_DISK && FLUX_SHAPE_DISK == 2);
        for (size_t i = 0; i < abi.shapes.size(); i++) {
            const flux_shape &s = abi.shapes[i];
            std::printf("shape %zu %d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", i,
                        s.kind, s.invert, s.p[0], s.p[1], s.p[2], s.n[0], s.n[1], s.n[2], s.radius, s.material.kind, s.material.color[0],
                        s.material.color[1], s.material.color[2], s.material.ambient[0], s.material.ambient[1], s.material.ambient[2],
                        s.material.k, s.material.exponent);
        }
        std::printf("ok abi scene\n");
    }
    {   // the loader's radius checks: the field's path in every message
        std::ifstream f(path);
        std::stringstream ss;
        ss << f.rdbuf();
        const std::string good = ss.str();
        CHECK(good.find("      radius: 5.0\n      material:\n        Emissive:\n          color: [1, 0.9686, 0.8588]\n          power: 10.0") !=
              std::string::npos);
        const size_t at = good.find("      radius: 5.0\n      material:\n        Emissive:\n          color: [1, 0.9686, 0.8588]\n          power: 10.0");
        auto with = [&](const std::string &line) {
            std::string t = good;
            t.replace(at, std::strlen("      radius: 5.0\n"), line);
            return t;
        };
        CHECK(throws(with(""), "shapes[1].Disk: missing field `radius`"));
        CHECK(throws(with("      radius: [5]\n"), "shapes[1].Disk.radius"));
        CHECK(throws(with("      radius: big\n"), "shapes[1].Disk.radius"));
        CHECK(throws(with("      radius: -1.0\n"), "shapes[1].Disk.radius"));
        CHECK(throws(with("      radius: nan\n"), "shapes[1].Disk.radius"));
        CHECK(throws(with("      radius: inf\n"), "shapes[1].Disk.radius"));
        const SceneData zero = scene_from_yaml_text(with("      radius: 0\n"));
        CHECK(std::get<DiskData>(zero.shapes[1]).radius == 0.0);
        std::string unknown = good;
        unknown.replace(unknown.find("- Disk:"), 7, "- Quad:");
        CHECK(throws(unknown, "unknown variant `Quad`, expected one of `Sphere`, `Plane`, `Disk`"));
        std::printf("ok yaml radius\n");
    }
    {   // CBOR: SetJob with the disk scene, decoded back field for field and re-encoded to the same bytes
        NetworkWorkerRequest req;
        req.kind = NetworkWorkerRequest::SetJob;
        req.job.scene_data = sd;
        req.job.config = JobConfiguration{3, 5, 50};
        cbor::Encoder e;
        encode_request(e, req);
        const std::string raw = e.out;
        CHECK(raw.find("Disk") != std::string::npos);
        cbor::StringReader r(raw);
        cbor::Decoder d(r);
        NetworkWorkerRequest back;
        CHECK(decode_request(d, back));
        CHECK(back.kind == NetworkWorkerRequest::SetJob);
        CHECK(back.job.scene_data.shapes.size() == sd.shapes.size());
        for (size_t i = 0; i < sd.shapes.size(); i++) CHECK(back.job.scene_data.shapes[i].index() == sd.shapes[i].index());
        const DiskData *b = std::get_if<DiskData>(&back.job.scene_data.shapes[1]);
        CHECK(b != nullptr);
        CHECK(same_vec(b->center, disk->center) && same_vec(b->normal, disk->normal) && b->radius == disk->radius);
        const EmissiveData *em = std::get_if<EmissiveData>(&b->material);
        CHECK(em != nullptr && em->power == 10.0 && em->color.g == 0.9686);
        cbor::Encoder e2;
        encode_request(e2, back);
        CHECK(e2.out == raw);
        // a disk of radius 0 and an odd radius survive too (shortest exact float encodings)
        req.job.scene_data.shapes[1] = DiskData{Vec3{0.1, -2.5, 1e300}, Vec3{0, 0, 0}, 0.0, EmissiveData{Color{1, 2, 3}, 0.5}};
        req.job.scene_data.shapes.push_back(DiskData{Vec3{1, 2, 3}, Vec3{0.3, -0.7, 1.1}, 1.0 / 3.0, MatteData{}});
        cbor::Encoder e3;
        encode_request(e3, req);
        cbor::StringReader r3(e3.out);
        cbor::Decoder d3(r3);
        NetworkWorkerRequest back3;
        CHECK(decode_request(d3, back3));
        const DiskData *z = std::get_if<DiskData>(&back3.job.scene_data.shapes[1]);
        const DiskData *t = std::get_if<DiskData>(&back3.job.scene_data.shapes.back());
        CHECK(z && z->radius == 0.0 && z->center.z == 1e300 && z->center.x == 0.1);
        CHECK(t && t->radius == 1.0 / 3.0 && t->normal.z == 1.1 && std::holds_alternative<MatteData>(t->material));
        std::printf("ok cbor round trip\n");
    }
    std::printf("all ok\n");
    return 0;
}
