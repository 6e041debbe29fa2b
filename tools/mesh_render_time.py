"""What a picture of a triangle mesh costs: `ops.render_mesh` (csrc/mesh_render.hip) beside the sphere pass and the whole
of `ops.render_surface` (csrc/surface.hip) on the same frame and camera, per launch kind.  GPU box.

  scene    the simulator's default scene (`simulate.random_scene(1)`, 61 445 particles) under `Camera.fit`, 768 x 768
  mesh     its `mesh.surface_mesh`, about 558 000 faces of one to a few pixels: the small-triangle path
  box      12 triangles around the scene's centre that fill about half the picture: the large-triangle path
  solids   `SequenceRenderer.push` per frame (PNG files included) without and with `solids`

Times are HIP events around one entry, ms per call of ONE frame; the kinds alternate inside one window, median of the
repeats after a warm-up of every kind.  Entry (a) is fill + raster + tiles + resolve (the labels say fill + raster + resolve), entry (b) the deferred shading; the split of
(a) into its three launches comes from the profiler's kernel records (one profiled call each), when it gives any.
Yardsticks, not code under test: tpg_render_spheres_f32 and `ops.render_surface` on the same frame and camera, and the
numpy statement of the rule (tests/mesh_render_rule.py) on the same mesh, one run on the host.

--small N=LIBRARY ... repeats the raster entry in a child process per library (another build of csrc/ with
-DTPG_MESH_SMALL=N; `_lib` takes it from TPGAN_HIP_LIBRARY) and adds the table of class edges.

    python tools/mesh_render_time.py [--repeats 10 --warm 12] [--small 8=build/small8.so --small 32=build/small32.so]
                                     [--out profiles/mesh_render.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import tpgan_amd  # noqa: F401
from tpgan_amd import mesh, ops, render
from tpgan_amd import simulate as S
from tpgan_amd.ops import _ptr

EXTENT = 768


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall_ms(fn, dev):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) * 1e3


def scene_frame(dev, warm):
    state = S.pack([S.random_scene(1)], dev)
    for _ in range(warm):
        x, v, lengths, lo, hi = state
        for _ in range(S.SUBSTEPS):
            x, v = ops.pbf_substep(x, v, lengths, lo, hi, 1.0 / (S.FPS * S.SUBSTEPS))
        state = (x, v, lengths, lo, hi)
    n = int(state[2][0]) if state[2] is not None else state[0].shape[1]
    return state[0][0, :n].contiguous()


def half_picture_box(cam, points):
    """12 triangles: a cube about the points' centre whose picture is about 0.7 x 0.7 of the frame."""
    lo, hi = render.bounding_box(points)
    centre = (lo + hi) / 2.0
    row = cam.row().astype(np.float64)
    zv = float((centre - row[0:3]) @ row[9:12])
    h = 0.35 * EXTENT * (zv / row[12] if row[17] != 0 else 1.0 / row[12])
    corners = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)]) + centre
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return corners.astype(np.float32), np.asarray(faces, np.int32)


class Entries:
    """The two mesh entries and the sphere pass on buffers of their own, one frame."""

    def __init__(self, be, row, dev):
        W = H = EXTENT
        self.be, self.dev = be, dev
        self.cams = np.ascontiguousarray(row.reshape(1, -1))
        self.keys = torch.empty((1, H, W), dtype=torch.int64, device=dev)
        self.list = torch.empty((1 + ops.MESH_LIST,), dtype=torch.int32, device=dev)
        self.depth = torch.empty((1, H, W), dtype=torch.float32, device=dev)
        self.winner = torch.empty((1, H, W), dtype=torch.int32, device=dev)
        self.image = torch.empty((1, H, W, 3), dtype=torch.uint8, device=dev)
        self.bg = torch.full((3,), 255, dtype=torch.uint8, device=dev)
        self.lut = torch.from_numpy(render.default_lut()).to(dev)
        self.shade, self.far = ops.surface_shade(), float(row[16] - row[15])

    def raster(self, v, f):
        self.be._call("tpg_render_mesh_f32", "render_mesh", 0, v, _ptr(v), None, _ptr(f), None, 1, v.shape[1], f.shape[1], 1,
                      self.cams.ctypes.data, 1, EXTENT, EXTENT, _ptr(self.keys), _ptr(self.list), _ptr(self.depth),
                      _ptr(self.winner))

    def shade_(self, v, f, n):
        self.be._call("tpg_mesh_shade_f32", "mesh_shade", 0, v, _ptr(self.depth), _ptr(self.winner), _ptr(v), None, _ptr(f),
                      None, _ptr(n), None, 1, v.shape[1], f.shape[1], 1, self.cams.ctypes.data, 1, EXTENT, EXTENT, 0.0,
                      self.far, _ptr(self.lut), None, _ptr(self.bg), self.shade.ctypes.data, _ptr(self.image))

    def spheres(self, pts, radius):
        self.be._call("tpg_render_spheres_f32", "render_spheres", 0, pts, _ptr(pts), None, 1, pts.shape[1],
                      self.cams.ctypes.data, 1, EXTENT, EXTENT, radius, _ptr(self.keys), _ptr(self.depth), _ptr(self.winner))


def medians(runs, repeats):
    for fn in runs.values():                                         # warm-up: code objects, workspaces
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(repeats):
        for k, fn in runs.items():
            times[k].append(event_ms(fn))
    return {k: statistics.median(v) for k, v in times.items()}


def kernel_split(fn):
    """name -> microseconds of every device kernel of one call of fn, from the profiler; {} if it gives none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.events():
            us = getattr(e, "device_time", None) or getattr(e, "cuda_time", 0)
            if us and "CUDA" in str(getattr(e, "device_type", "")):
                out[e.name] = out.get(e.name, 0.0) + float(us)
        return out
    except Exception as err:                                         # a timing tool: the split is extra
        return {"profiler unavailable: " + type(err).__name__: 0.0}


def workloads(dev, warm):
    pts = scene_frame(dev, warm)
    c = render.Camera.fit(pts, width=EXTENT, height=EXTENT)
    # the fitted view with the depth range opened up: there is no clipping, and the box reaches beyond the fluid's own
    cam = render.Camera(c.eye, c.r, c.d, c.f, c.mode, c.scale, c.cx, c.cy, 0.25 * c.near, 2.0 * c.far, c.width, c.height)
    m = mesh.surface_mesh(pts)
    box = half_picture_box(cam, pts)
    return pts, cam, m, box


def raster_only(dev, warm, repeats):
    """One JSON line: the raster entry's median on the scene's mesh and on the box (what a --small child prints)."""
    pts, cam, m, box = workloads(dev, warm)
    e = Entries(ops.backend_for(pts), cam.row(), dev)
    v, f = m.vertices[None].contiguous(), m.faces[None].contiguous()
    bv, bf = torch.from_numpy(box[0]).to(dev)[None], torch.from_numpy(box[1]).to(dev)[None]
    t = medians({"mesh": lambda: e.raster(v, f), "box": lambda: e.raster(bv, bf)}, repeats)
    print(json.dumps(dict(library=os.environ.get("TPGAN_HIP_LIBRARY", "in tree"), **t)), flush=True)


def report(dev, a, emit):
    import mesh_render_rule as MR
    pts, cam, m, box = workloads(dev, a.warm)
    row = cam.row()
    be = ops.backend_for(pts)
    e = Entries(be, row, dev)
    v, f, n = m.vertices[None].contiguous(), m.faces[None].contiguous(), m.normals[None].contiguous()
    bv, bf = torch.from_numpy(box[0]).to(dev)[None], torch.from_numpy(box[1]).to(dev)[None]
    p1, radius, lut = pts[None].contiguous(), 0.025, e.lut
    runs = {
        "mesh (a) fill + raster + resolve": lambda: e.raster(v, f),
        "mesh (b) shade, vertex normals": lambda: (e.raster(v, f), e.shade_(v, f, n)),
        "mesh ops.render_mesh": lambda: ops.render_mesh(v, f, row, EXTENT, EXTENT, lut, normals=n),
        "box (a) fill + raster + resolve": lambda: e.raster(bv, bf),
        "box ops.render_mesh": lambda: ops.render_mesh(bv, bf, row, EXTENT, EXTENT, lut, base=(150, 150, 150)),
        "yardstick: sphere pass": lambda: e.spheres(p1, radius),
        "yardstick: ops.render_surface": lambda: ops.render_surface(p1, row, EXTENT, EXTENT, lut, radius),
    }
    t = medians(runs, a.repeats)
    t["mesh (b) shade, vertex normals"] -= t["mesh (a) fill + raster + resolve"]
    depth = ops.render_mesh(v, f, row, EXTENT, EXTENT, lut)[1]
    bdepth = ops.render_mesh(bv, bf, row, EXTENT, EXTENT, lut)[1]
    emit(f"scene: {pts.shape[0]} particles, {EXTENT} x {EXTENT}, {cam.mode} camera; mesh: {v.shape[1]} vertices, "
         f"{f.shape[1]} faces, surface on {float(torch.isfinite(depth).float().mean()):.3f} of the picture; box: 12 triangles "
         f"on {float(torch.isfinite(bdepth).float().mean()):.3f} of the picture; TPG_MESH_SMALL = {ops.MESH_SMALL}")
    emit(f"{'':36} {'ms per frame':>13}")
    for k, ms in t.items():
        emit(f"{k:36} {ms:13.4f}")
    with tempfile.TemporaryDirectory() as tmp:
        frames = [pts.cpu().numpy()] * 4
        solid = (box[0], box[1])
        emit(f"SequenceRenderer.push, 4 frames per call, wall ms per frame with the PNG files (median of {max(3, a.repeats // 2)}):")
        for style in ("points", "surface"):
            for label, kw in (("", {}), (" + solids (the box)", dict(solids=solid))):
                seq = render.SequenceRenderer(tmp, width=EXTENT, height=EXTENT, camera=cam, device=dev, style=style, **kw)
                seq.push(frames, 0)
                ms = statistics.median(wall_ms(lambda: seq.push(frames, 0), dev) / 4 for _ in range(max(3, a.repeats // 2)))
                emit(f"  --style {style + label:32} {ms:9.3f}")
    t0 = time.perf_counter()
    want = MR.raster_rule(m.vertices.cpu().numpy()[None], m.faces.cpu().numpy()[None], row, EXTENT, EXTENT)
    host = time.perf_counter() - t0
    e.raster(v, f)
    same = (np.array_equal(e.winner.cpu().numpy(), want[1])
            and np.array_equal(e.depth.cpu().numpy().view(np.uint32), want[0].view(np.uint32)))
    emit(f"yardstick: numpy statement of the rule on the host, the same {f.shape[1]} faces: {host:.1f} s (one run), "
         f"{'equal to' if same else 'DIFFERENT from'} the device's depth and winner bit for bit")
    for label, fn in (("mesh", lambda: e.raster(v, f)), ("box", lambda: e.raster(bv, bf)), ("spheres", lambda: e.spheres(p1, radius))):
        for name, us in kernel_split(fn).items():
            emit(f"  kernels of one {label} call: {name[:60]:60} {us / 1e3:9.4f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warm", type=int, default=12, help="simulated frames before the scene's frame is taken")
    ap.add_argument("--small", action="append", default=[], metavar="N=LIBRARY",
                    help="another build of the library with -DTPG_MESH_SMALL=N: its raster times are added")
    ap.add_argument("--raster_only", action="store_true", help="print the raster entry's medians as one JSON line")
    ap.add_argument("--commit", default=None, help="the commit the times are taken on (default: git's HEAD)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    torch.backends.cudnn.enabled = False
    dev = torch.device("cuda", 0)
    if a.raster_only:
        return raster_only(dev, a.warm, a.repeats)
    commit = a.commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                        text=True).stdout.strip()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
        if a.out:                                                    # kept as it grows: a long run leaves what it had
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as out:
                out.write("\n".join(lines) + "\n")
    emit(f"# {torch.cuda.get_device_name(0)}; commit {commit or 'unknown'}; HIP events, {a.repeats} alternating repeats "
         f"after warm-up, median")
    report(dev, a, emit)
    if a.small:
        emit("class edge TPG_MESH_SMALL (pixels in a clipped box that one lane still draws), raster entry, ms per frame:")
        emit(f"  {'SMALL':>6} {'mesh':>10} {'box':>10}")
        for spec in [f"{ops.MESH_SMALL}="] + a.small:
            n, _, lib = spec.partition("=")
            env = dict(os.environ, **({"TPGAN_HIP_LIBRARY": os.path.abspath(lib)} if lib else {}))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--raster_only", "--repeats", str(a.repeats),
                                  "--warm", str(a.warm)], env=env, capture_output=True, text=True, timeout=600)
            rec = json.loads(out.stdout.strip().splitlines()[-1]) if out.returncode == 0 else None
            emit(f"  {n:>6} {rec['mesh']:10.4f} {rec['box']:10.4f}" if rec else f"  {n:>6} failed: exit {out.returncode}")
            if rec is None:                                          # nothing more is started on the device after a failure
                break


if __name__ == "__main__":
    main()
