// Disk shapes (extension, include/flux_abi.h FLUX_SHAPE_DISK) in the C++ host layer, CPU only (tests/test_disk_scene.py builds
// and runs it): the YAML loader and its radius checks, the conversion to flux_shape, and a CBOR round trip of a disk scene through
// the node protocol's SetJob message.
//   usage: disk_host_selftest <scenes dir>
// Prints "shape <i> <fields>" for every flux_shape of scenes/disk_light.yml (compared with the Python loader by the test), one
// "ok <name>" per passed check and "all ok" at the end; exits 1 on the first failure.
#include <cmath>
#include <cstring>
#include <string>

#include "host_selftest.hpp"

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
        print_flux_shapes(abi);
        std::printf("ok abi scene\n");
    }
    {   // the loader's radius checks: the field's path in every message
        const std::string good = read_file(path);
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
        std::string raw;
        NetworkWorkerRequest back;
        if (set_job_round_trip(sd, raw, back)) return 1;
        CHECK(raw.find("Disk") != std::string::npos);
        const DiskData *b = std::get_if<DiskData>(&back.job.scene_data.shapes[1]);
        CHECK(b != nullptr);
        CHECK(same_vec(b->center, disk->center) && same_vec(b->normal, disk->normal) && b->radius == disk->radius);
        const EmissiveData *em = std::get_if<EmissiveData>(&b->material);
        CHECK(em != nullptr && em->power == 10.0 && em->color.g == 0.9686);
        NetworkWorkerRequest req = back;  // the same scene: it re-encoded to the same bytes
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
