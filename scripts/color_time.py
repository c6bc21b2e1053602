"""What vertex colours cost: the 1000 x 500 height field of configuration 5 at 4096 spp and
scenes/vertex_colors.yml at 800 x 600, each rendered by ONE context plain, with colours only, with normals only, with both, and
plain again after clearing -- flux_ctx_last_kernel_ms, median of five after a warm-up --, with the setters' wall time and the
table's bytes.  Two ratios: "both" against "normals only" (what sharing the 128-B line buys: the colours of a triangle that is
smooth already) and "colours only" against plain.  Reported, not bounded.  Development aid: the figures of section 5k.
usage: color_time.py [--hf NXxNZ] [--hf-root 64] [--demo-root 16] [--runs 5]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flux_amd  # noqa: E402
from flux_amd.procedural import ELEVATION_HIGH, ELEVATION_LOW, elevation_colors, heightfield_scene, vertex_normals  # noqa: E402
from flux_amd.scene import MeshData  # noqa: E402


def kernel_ms(r, runs):
    r.render_frame()
    out = []
    for _ in range(runs):
        r.render_frame()
        out.append(r.last_kernel_ms())
    return statistics.median(out), min(out), max(out)


def measure(name, sd, normals, colors, root, runs):
    """`sd`'s meshes carry no attribute; `normals` and `colors` hold one entry per mesh (MeshData.normals / .colors, or None)"""
    meshes = [s for s in sd.shapes if isinstance(s, MeshData)]
    with flux_amd.Renderer(sd, flux_amd.JobConfiguration(root, 5, 50), seed=1) as r:
        plan, bytes0 = r.launch_plan(flags=True), r.device_bytes()

        def put(setter, values):
            t0 = time.perf_counter()
            for k, v in enumerate(values):
                setter(k, v)
            return (time.perf_counter() - t0) * 1e3
        none = [None] * len(meshes)
        plain = kernel_ms(r, runs)
        set_colors_ms = put(r.set_mesh_colors, colors)
        table = r.device_bytes() - bytes0
        colors_only = kernel_ms(r, runs)
        put(r.set_mesh_colors, none)
        assert r.device_bytes() == bytes0
        set_normals_ms = put(r.set_mesh_normals, normals)
        normals_only = kernel_ms(r, runs)
        set_colors_second_ms = put(r.set_mesh_colors, colors)
        assert r.device_bytes() == bytes0 + table and r.launch_plan(flags=True) == plan
        both = kernel_ms(r, runs)
        put(r.set_mesh_colors, none)
        put(r.set_mesh_normals, none)
        assert r.device_bytes() == bytes0
        again = kernel_ms(r, runs)
    out = {"scene": name, "spp": root * root, "triangles": int(sum(len(m.triangles) for m in meshes)), "kernel": plan["kernel"],
           "plain_ms": plain, "colors_only_ms": colors_only, "normals_only_ms": normals_only, "both_ms": both, "plain_again_ms": again,
           "both_over_normals_only": both[0] / normals_only[0], "colors_only_over_plain": colors_only[0] / plain[0],
           "set_mesh_colors_wall_ms": set_colors_ms, "set_mesh_colors_on_a_table_wall_ms": set_colors_second_ms,
           "set_mesh_normals_wall_ms": set_normals_ms, "table_bytes": table, "context_bytes_plain": bytes0}
    print(json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    opt = lambda name, default: type(default)(args[args.index(name) + 1]) if name in args else default  # noqa: E731
    runs = opt("--runs", 5)
    nx, nz = [int(x) for x in opt("--hf", "1000x500").split("x")]
    sd = heightfield_scene(nx, nz)
    hf = sd.shapes[-1]
    measure(f"height field {nx}x{nz}", sd, [vertex_normals(hf.vertices, hf.triangles)],
            [elevation_colors(hf.vertices, ELEVATION_LOW, ELEVATION_HIGH)], opt("--hf-root", 64), runs)
    sd = flux_amd.load_scene(os.path.join(ROOT, "scenes", "vertex_colors.yml"))
    meshes = [s for s in sd.shapes if isinstance(s, MeshData)]
    colors = [m.colors for m in meshes]
    normals = [m.normals if m.normals is not None else vertex_normals(m.vertices, m.triangles) for m in meshes]
    for m in meshes:
        m.normals = m.colors = None
    measure("vertex_colors.yml", sd, normals, colors, opt("--demo-root", 16), runs)


if __name__ == "__main__":
    main()
