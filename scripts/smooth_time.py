"""What smooth shading costs: the 1000 x 500 height field of configuration 5 at 4096 spp and the four UV
spheres of scenes/smooth_sphere.yml at 256 spp, each rendered flat and with vertex normals on every mesh by the same context --
flux_ctx_last_kernel_ms, median of five after a warm-up --, with the setter's wall time and the table's bytes.  Reported, not bounded.
Development aid: the figures of section 5j.
usage: smooth_time.py [--hf NXxNZ] [--hf-root 64] [--sphere-root 16] [--runs 5]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flux_amd  # noqa: E402
from flux_amd.procedural import heightfield_scene, vertex_normals  # noqa: E402
from flux_amd.scene import MeshData  # noqa: E402


def kernel_ms(r, runs):
    r.render_frame()
    out = []
    for _ in range(runs):
        r.render_frame()
        out.append(r.last_kernel_ms())
    return statistics.median(out), min(out), max(out)


def measure(name, sd, root, runs):
    """`sd`'s meshes carry no normals; the context renders flat, gets area-weighted vertex normals on every mesh, renders smooth"""
    meshes = [s for s in sd.shapes if isinstance(s, MeshData)]
    normals = [vertex_normals(m.vertices, m.triangles) for m in meshes]
    with flux_amd.Renderer(sd, flux_amd.JobConfiguration(root, 5, 50), seed=1) as r:
        plan, bytes0 = r.launch_plan(flags=True), r.device_bytes()
        flat = kernel_ms(r, runs)
        t0 = time.perf_counter()
        for k, n in enumerate(normals):
            r.set_mesh_normals(k, n)
        set_ms = (time.perf_counter() - t0) * 1e3
        assert r.launch_plan(flags=True) == plan
        smooth = kernel_ms(r, runs)
        table = r.device_bytes() - bytes0
        for k in range(len(meshes)):
            r.set_mesh_normals(k, None)
        again = kernel_ms(r, runs)
    out = {"scene": name, "spp": root * root, "triangles": int(sum(len(m.triangles) for m in meshes)), "kernel": plan["kernel"],
           "flat_ms": flat, "smooth_ms": smooth, "flat_again_ms": again, "smooth_over_flat": smooth[0] / flat[0],
           "set_mesh_normals_wall_ms": set_ms, "table_bytes": table, "context_bytes_flat": bytes0}
    print(json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    opt = lambda name, default: type(default)(args[args.index(name) + 1]) if name in args else default  # noqa: E731
    runs = opt("--runs", 5)
    nx, nz = [int(x) for x in opt("--hf", "1000x500").split("x")]
    measure(f"height field {nx}x{nz}", heightfield_scene(nx, nz), opt("--hf-root", 64), runs)
    sd = flux_amd.load_scene(os.path.join(ROOT, "scenes", "smooth_sphere.yml"))
    for s in sd.shapes:
        if isinstance(s, MeshData):
            s.normals = None
    measure("smooth_sphere.yml", sd, opt("--sphere-root", 16), runs)


if __name__ == "__main__":
    main()
