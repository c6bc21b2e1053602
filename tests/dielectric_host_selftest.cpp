// Dielectric materials (extension, include/flux_abi.h FLUX_MAT_DIELECTRIC) in the C++ host layer, CPU only
// (tests/test_dielectric_scene.py builds and runs it): the YAML loader and its refraction-index checks, the conversion to
// flux_material, and a CBOR round trip of a glass scene through the node protocol's SetJob message.
//   usage: dielectric_host_selftest <scenes dir>
// Prints "shape <i> <fields>" for every flux_shape of scenes/glass.yml (compared with the Python loader by the test), one
// "ok <name>" per passed check and "all ok" at the end; exits 1 on the first failure.
#include <cmath>
#include <cstring>
#include <string>

#include "host_selftest.hpp"

static const MaterialData &material_of(const ShapeData &s) {
    if (auto *p = std::get_if<SphereData>(&s)) return p->material;
    if (auto *p = std::get_if<PlaneData>(&s)) return p->material;
    return std::get<DiskData>(s).material;
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <scenes dir>\n", argv[0]);
        return 2;
    }
    const std::string path = std::string(argv[1]) + "/glass.yml";
    const SceneData sd = scene_from_yaml_file(path);
    CHECK(sd.shapes.size() == 13);
    const DielectricData *g3 = std::get_if<DielectricData>(&material_of(sd.shapes[3]));
    const DielectricData *g5 = std::get_if<DielectricData>(&material_of(sd.shapes[5]));
    const DielectricData *g7 = std::get_if<DielectricData>(&material_of(sd.shapes[7]));
    CHECK(g3 && g5 && g7);
    CHECK(g3->refraction_index == 1.5 && g7->refraction_index == 1.5 && g5->refraction_index == 1.33);
    CHECK(g3->transmit_color.r == 1.0 && g5->transmit_color.r == 0.8 && g5->transmit_color.g == 0.95);
    {
        const AbiScene abi(sd);
        CHECK(abi.desc.num_shapes == 13 && abi.shapes[3].material.kind == FLUX_MAT_DIELECTRIC && FLUX_MAT_DIELECTRIC == 4);
        CHECK(abi.shapes[5].material.k == 1.33 && abi.shapes[5].material.color[1] == 0.95);
        print_flux_shapes(abi);
        std::printf("ok abi scene\n");
    }
    {   // the loader's refraction-index checks: the field's path in every message
        const std::string good = read_file(path);
        const std::string line = "    refraction_index: 1.5\n";
        const size_t at = good.find(line);
        CHECK(at != std::string::npos);
        auto with = [&](const std::string &repl) {
            std::string t = good;
            t.replace(at, line.size(), repl);
            return t;
        };
        // the anchor is used by shapes[3] first: the error names the first shape that reads it
        CHECK(throws(with(""), "shapes[3].Sphere.material.Dielectric: missing field `refraction_index`"));
        CHECK(throws(with("    refraction_index: [1.5]\n"), "shapes[3].Sphere.material.Dielectric.refraction_index"));
        CHECK(throws(with("    refraction_index: glass\n"), "shapes[3].Sphere.material.Dielectric.refraction_index"));
        CHECK(throws(with("    refraction_index: 0\n"), "shapes[3].Sphere.material.Dielectric.refraction_index"));
        CHECK(throws(with("    refraction_index: -1.5\n"), "shapes[3].Sphere.material.Dielectric.refraction_index"));
        CHECK(throws(with("    refraction_index: nan\n"), "shapes[3].Sphere.material.Dielectric.refraction_index"));
        CHECK(throws(with("    refraction_index: inf\n"), "shapes[3].Sphere.material.Dielectric.refraction_index"));
        const SceneData one = scene_from_yaml_text(with("    refraction_index: 1\n"));
        CHECK(std::get<DielectricData>(material_of(one.shapes[3])).refraction_index == 1.0);
        std::string unknown = good;
        unknown.replace(unknown.find("  Dielectric:"), 13, "  Glass:");
        CHECK(throws(unknown, "unknown variant `Glass`, expected one of `Matte`, `Emissive`, `Reflective`, `GlossyReflective`, `Dielectric`"));
        std::string no_tc = good;
        no_tc.replace(no_tc.find("    transmit_color: [1, 1, 1]\n"), std::strlen("    transmit_color: [1, 1, 1]\n"), "");
        CHECK(throws(no_tc, "shapes[3].Sphere.material.Dielectric: missing field `transmit_color`"));
        std::printf("ok yaml refraction index\n");
    }
    {   // CBOR: SetJob with the glass scene, decoded back field for field and re-encoded to the same bytes
        std::string raw;
        NetworkWorkerRequest back;
        if (set_job_round_trip(sd, raw, back)) return 1;
        CHECK(raw.find("Dielectric") != std::string::npos);
        for (size_t i = 0; i < sd.shapes.size(); i++)
            CHECK(material_of(back.job.scene_data.shapes[i]).index() == material_of(sd.shapes[i]).index());
        const DielectricData *b = std::get_if<DielectricData>(&material_of(back.job.scene_data.shapes[5]));
        CHECK(b && b->refraction_index == 1.33 && b->transmit_color.r == 0.8 && b->transmit_color.g == 0.95 && b->transmit_color.b == 1.0);
        NetworkWorkerRequest req = back;  // the same scene: it re-encoded to the same bytes
        // odd values on a plane and a disk survive too (shortest exact float encodings)
        req.job.scene_data.shapes.push_back(PlaneData{Vec3{0, -3, 0}, Vec3{0, 1, 0}, DielectricData{1.0 / 3.0, Color{0.1, 1e-300, 2.5}}});
        req.job.scene_data.shapes.push_back(DiskData{Vec3{1, 2, 3}, Vec3{0, 0, -1}, 0.5, DielectricData{2.4175, Color{1, 1, 1}}});
        cbor::Encoder e3;
        encode_request(e3, req);
        cbor::StringReader r3(e3.out);
        cbor::Decoder d3(r3);
        NetworkWorkerRequest back3;
        CHECK(decode_request(d3, back3));
        const size_t n3 = back3.job.scene_data.shapes.size();
        CHECK(n3 == sd.shapes.size() + 2);
        const DielectricData *p = std::get_if<DielectricData>(&material_of(back3.job.scene_data.shapes[n3 - 2]));
        const DielectricData *k = std::get_if<DielectricData>(&material_of(back3.job.scene_data.shapes[n3 - 1]));
        CHECK(p && p->refraction_index == 1.0 / 3.0 && p->transmit_color.g == 1e-300 && p->transmit_color.b == 2.5);
        CHECK(k && k->refraction_index == 2.4175 && std::holds_alternative<DiskData>(back3.job.scene_data.shapes[n3 - 1]));
        std::printf("ok cbor round trip\n");
    }
    std::printf("all ok\n");
    return 0;
}
