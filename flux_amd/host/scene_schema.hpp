// scene_schema.hpp -- the serde schema of the reference's scene and node-protocol types, stated once: what the
// reference gets from #[derive(Serialize, Deserialize)] on
//   SceneData & friends          fluxcore/src/scene.rs:12-74, shapes.rs:15-81, color.rs:8-16
//   Job, JobConfiguration, WorkUnit                  fluxcore/src/job.rs:40-63
//   RenderEvent, WorkUnitResult, WorkerInfo          fluxcore/src/manager.rs:16-28,221-224
//
//   fields(v, s)    calls v("name", s.member) for every field of struct s, in wire order;
//   variants(v, e)  calls v.variant("Name", active, select) for every variant of tagged enum e, in wire order: `active`
//                   says whether e holds that variant now, select() makes it the one e holds and returns its payload.
//
// Three visitors walk these lists: the YAML reader (flux_host.cpp), the CBOR writer and the CBOR reader (flux_net.cpp).
// A visitor brings its own encodings of the leaves (numbers, strings, Vec3, Color, JobID, SystemTime, sequences); a new
// field, shape or material is one line here and nothing there.
#pragma once
#include <string>

#include "flux_host.hpp"

namespace flux_host {

// ---- structs ---------------------------------------------------------------------------------------
template <class V> void fields(V &v, Vec3 &p) {  // written as a 3-sequence; the CBOR reader also takes this map
    v("x", p.x);
    v("y", p.y);
    v("z", p.z);
}
template <class V> void fields(V &v, Color &c) {  // color.rs:12-16; a 3-sequence in YAML
    v("r", c.r);
    v("g", c.g);
    v("b", c.b);
}

template <class V> void fields(V &v, MatteData &m) {
    v("diffuse_color", m.diffuse_color);
    v("ambient_color", m.ambient_color);
    v("diffuse_coefficient", m.diffuse_coefficient);
}
template <class V> void fields(V &v, EmissiveData &m) {
    v("color", m.color);
    v("power", m.power);
}
template <class V> void fields(V &v, ReflectiveData &m) {
    v("reflect_amount", m.reflect_amount);
    v("reflect_color", m.reflect_color);
}
template <class V> void fields(V &v, GlossyReflectiveData &m) {
    v("reflect_amount", m.reflect_amount);
    v("reflect_color", m.reflect_color);
    v("reflect_exponent", m.reflect_exponent);
}
template <class V> void fields(V &v, DielectricData &m) {
    v("refraction_index", m.refraction_index);
    v("transmit_color", m.transmit_color);
}

template <class V> void fields(V &v, SphereData &s) {
    v("center", s.center);
    v("radius", s.radius);
    v("material", s.material);
    v("invert", s.invert);
}
template <class V> void fields(V &v, PlaneData &s) {
    v("point", s.point);
    v("normal", s.normal);
    v("material", s.material);
}
template <class V> void fields(V &v, DiskData &s) {
    v("center", s.center);
    v("normal", s.normal);
    v("radius", s.radius);
    v("material", s.material);
}

// a field a reader may not find: a visitor that has optional(name, member) gets that call, every other one the plain v(name, member)
template <class V, class M> auto optional_field(V &v, const char *name, M &member, int) -> decltype(v.optional(name, member)) {
    return v.optional(name, member);
}
template <class V, class M> void optional_field(V &v, const char *name, M &member, long) { v(name, member); }

template <class V> void fields(V &v, BoxData &s) {
    v("corner0", s.corner0);
    v("corner1", s.corner1);
    v("material", s.material);
    optional_field(v, "invert", s.invert, 0);  // may be absent in YAML (it keeps its default, false); always on the wire
}

template <class V> void fields(V &v, OutputSettings &o) {
    v("image_width", o.image_width);
    v("image_height", o.image_height);
    v("pixel_size", o.pixel_size);
}
template <class V> void fields(V &v, CameraSettings &c) {
    v("eye", c.eye);
    v("look_at", c.look_at);
    v("up", c.up);
}
template <class V> void fields(V &v, CameraData &c) {
    v("zoom_factor", c.zoom_factor);
    v("view_plane_distance", c.view_plane_distance);
    v("focal_distance", c.focal_distance);
    v("lens_radius", c.lens_radius);
}
template <class V> void fields(V &v, SceneData &s) {  // scene.rs:40-66
    v("scene_name", s.scene_name);
    v("output_settings", s.output_settings);
    v("background", s.background);
    v("shapes", s.shapes);
    v("camera_settings", s.camera_settings);
    v("camera_data", s.camera_data);
}

template <class V> void fields(V &v, JobConfiguration &c) {
    v("sample_root", c.sample_root);
    v("max_trace_depth", c.max_trace_depth);
    v("rows_per_work_unit", c.rows_per_work_unit);
}
template <class V> void fields(V &v, Job &j) {  // job.rs:59-63
    v("id", j.id);
    v("scene_data", j.scene_data);
    v("config", j.config);
}
template <class V> void fields(V &v, WorkUnit &u) {  // job.rs:40-44
    v("row_start", u.row_start);
    v("row_end", u.row_end);
    v("job_id", u.job_id);
}
template <class V> void fields(V &v, WorkerInfo &w) { v("num_threads", w.num_threads); }  // manager.rs:221-224

// serde's SystemTime; RenderEvent keeps the time as seconds in a double, the CBOR visitors convert (flux_net.cpp)
struct SystemTime { double &seconds; };
struct SystemTimeParts { size_t secs_since_epoch = 0, nanos_since_epoch = 0; };
template <class V> void fields(V &v, SystemTimeParts &t) {
    v("secs_since_epoch", t.secs_since_epoch);
    v("nanos_since_epoch", t.nanos_since_epoch);
}

// the struct variants of RenderEvent (manager.rs:16-22), as views of the flat RenderEvent; RowsReady's is WorkUnitResult
struct RenderingStartedEvent { JobID &job_id; SystemTime start_time; };
struct ImageInfoEvent { std::string &scene_name; size_t &width, &height; };
struct RenderingFinishedEvent { SystemTime end_time; };
template <class V> void fields(V &v, RenderingStartedEvent &p) {
    v("job_id", p.job_id);
    v("start_time", p.start_time);
}
template <class V> void fields(V &v, ImageInfoEvent &p) {
    v("scene_name", p.scene_name);
    v("width", p.width);
    v("height", p.height);
}
template <class V> void fields(V &v, WorkUnitResult &r) {  // manager.rs:24-28
    v("work_unit", r.work_unit);
    v("rows", r.rows);
}
template <class V> void fields(V &v, RenderingFinishedEvent &p) { v("end_time", p.end_time); }

// ---- tagged enums ----------------------------------------------------------------------------------
template <class A, class V, class Variant> void alternative(V &v, const char *name, Variant &e) {
    v.variant(name, std::holds_alternative<A>(e), [&]() -> A & { return std::holds_alternative<A>(e) ? std::get<A>(e) : e.template emplace<A>(); });
}
template <class V> void variants(V &v, MaterialData &m) {  // shapes.rs:42-47
    alternative<MatteData>(v, "Matte", m);
    alternative<EmissiveData>(v, "Emissive", m);
    alternative<ReflectiveData>(v, "Reflective", m);
    alternative<GlossyReflectiveData>(v, "GlossyReflective", m);
    alternative<DielectricData>(v, "Dielectric", m);  // extension: a reference node rejects the unknown variant
}
template <class V> void variants(V &v, ShapeData &s) {  // scene.rs:71-74
    alternative<SphereData>(v, "Sphere", s);
    alternative<PlaneData>(v, "Plane", s);
    alternative<DiskData>(v, "Disk", s);  // extension: a reference node rejects the unknown variant
    alternative<BoxData>(v, "Box", s);    // extension, likewise
}
template <class V> void variants(V &v, RenderEvent &ev) {  // manager.rs:16-22
    RenderingStartedEvent started{ev.job_id, {ev.time_s}};
    ImageInfoEvent info{ev.scene_name, ev.width, ev.height};
    RenderingFinishedEvent finished{{ev.time_s}};
    auto variant = [&](const char *name, RenderEvent::Kind kind, auto &payload) {
        v.variant(name, ev.kind == kind, [&]() -> decltype(payload) { ev.kind = kind; return payload; });
    };
    variant("RenderingStarted", RenderEvent::RenderingStarted, started);
    variant("ImageInfo", RenderEvent::ImageInfo, info);
    variant("RowsReady", RenderEvent::RowsReady, ev.result);
    variant("RenderingFinished", RenderEvent::RenderingFinished, finished);
}

// ---- what the lists answer without a format ------------------------------------------------------------
template <class S> size_t field_count(S &s) {
    size_t n = 0;
    auto count = [&](const char *, auto &) { n++; };
    fields(count, s);
    return n;
}

// the name of the field that is `member` of s (for messages about one field)
template <class S, class M> std::string field_name(S &s, const M &member) {
    std::string found;
    auto match = [&](const char *name, auto &m) {
        if ((const void *)&m == (const void *)&member) found = name;
    };
    fields(match, s);
    return found;
}

// "`A`, `B`, `C`": the variants of e, as the unknown-variant message lists them
struct VariantNames {
    std::string list;
    template <class Select> void variant(const char *name, bool, Select) { list += (list.empty() ? "`" : ", `") + std::string(name) + "`"; }
    template <class Select> void unit_variant(const char *name, bool active, Select select) { variant(name, active, select); }
};
template <class E> std::string variant_names(E &e) {
    VariantNames names;
    variants(names, e);
    return names.list;
}

}  // namespace flux_host
