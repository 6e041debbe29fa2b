"""What the translucent fluid costs: tpg_render_thickness_f32 beside tpg_render_spheres_f32 on the same frame and camera,
one blur pass, the absorption launch, and `render.render_surface` without and with `translucent`.  GPU box.

  scene    the simulator's default scene (`simulate.random_scene(1)`, 61 445 particles) under `Camera.fit`, 768 x 768,
           particle radius 0.025; the solids of the last two lines: a box of 12 triangles around the scene's centre

Times are HIP events around one entry, ms per call of ONE frame; the kinds alternate inside one window, median of the
repeats after a warm-up of every kind.  The thickness pass adds once per sphere per covered pixel, so the file also says
how many such pairs the frame has (`covered_pairs`: the pixel centres inside every kept disc, counted in float64 from the
projection) and the pairs per microsecond of both disc passes.

    python tools/translucent_time.py [--repeats 10 --warm 12] [--out profiles/translucent.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import tpgan_amd  # noqa: F401
from tpgan_amd import ops, render
from tpgan_amd.ops import _ptr
from mesh_render_time import EXTENT, event_ms, half_picture_box, scene_frame

RADIUS, HALF = 0.025, 2


def covered_pairs(pts, row, radius):
    """(sphere x pixel pairs with s < 1 in one frame, the median disc radius in pixels): per kept point the pixel centres
    inside its disc and the picture, counted in float64 from the projection, 4096 points at a time."""
    c = torch.from_numpy(row.astype(np.float64)).to(pts.device)
    q = pts.double() - c[0:3]
    xv, yv, zv = q @ c[3:6], q @ c[6:9], q @ c[9:12]
    pin = float(row[17]) != 0.0
    u = (xv / zv if pin else xv) * c[12] + c[13]
    v = (yv / zv if pin else yv) * c[12] + c[14]
    rp = torch.clamp((radius / zv if pin else torch.full_like(zv, radius)) * c[12], max=float(ops.SURFACE_MAX_RADIUS))
    keep = (zv - c[15] >= 0) & (zv <= c[16]) & (rp > 0)
    u, v, rp = u[keep], v[keep], rp[keep]
    reach = int(torch.ceil(rp.max()).item()) + 1
    off = torch.arange(-reach, reach + 1, device=pts.device, dtype=torch.float64)
    total = 0
    for k0 in range(0, u.shape[0], 4096):
        uu, vv, rr = (a[k0:k0 + 4096].view(-1, 1, 1) for a in (u, v, rp))
        x, y = torch.floor(uu) + off.view(1, 1, -1), torch.floor(vv) + off.view(1, -1, 1)
        inside = (x >= 0) & (x < EXTENT) & (y >= 0) & (y < EXTENT)
        s = ((x + 0.5 - uu) / rr) ** 2 + ((y + 0.5 - vv) / rr) ** 2
        total += int(((s < 1.0) & inside).sum())
    return total, float(rp.median())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warm", type=int, default=12, help="simulated frames before the scene's frame is taken")
    ap.add_argument("--commit", default=None, help="the commit the times are taken on (default: git's HEAD)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    torch.backends.cudnn.enabled = False
    dev = torch.device("cuda", 0)
    commit = a.commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                        text=True).stdout.strip()
    pts = scene_frame(dev, a.warm)
    cam = render.Camera.fit(pts, width=EXTENT, height=EXTENT)
    row, W, H = cam.row(), EXTENT, EXTENT
    cams = np.ascontiguousarray(row.reshape(1, -1))
    be = ops.backend_for(pts)
    p1, N = pts[None].contiguous(), pts.shape[0]
    box = half_picture_box(cam, pts)
    keys = torch.empty((1, H, W), dtype=torch.int64, device=dev)
    depth, thick, blurred, out_depth = (torch.empty((1, H, W), dtype=torch.float32, device=dev) for _ in range(4))
    winner = torch.empty((1, H, W), dtype=torch.int32, device=dev)
    image = torch.empty((1, H, W, 3), dtype=torch.uint8, device=dev)
    fluid, fdepth, _ = ops.render_surface(p1, row, W, H, render.default_lut(), RADIUS)
    solid = render._solid_layer(dev, box, render.SOLIDS_COLOR, cams, cam, 1, (255, 255, 255), ops.RENDER_KEY_BYTES)
    th_max = render.THICKNESS_DIAMETERS * 2.0 * RADIUS
    table = ops.absorb_table(np.asarray(render.ABSORPTION) / (2.0 * RADIUS), th_max)

    def spheres():
        be._call("tpg_render_spheres_f32", "render_spheres", 0, p1, _ptr(p1), None, 1, N, cams.ctypes.data, 1, W, H, RADIUS,
                 _ptr(keys), _ptr(depth), _ptr(winner))

    def thickness(limit):
        be._call("tpg_render_thickness_f32", "render_thickness", 0, p1, _ptr(p1), None, 1, N, cams.ctypes.data, 1, W, H,
                 RADIUS, _ptr(limit), _ptr(keys), _ptr(thick))

    def blur():
        be._call("tpg_surface_smooth_f32", "surface_smooth", 0, p1, _ptr(thick), 1, W, H, HALF, ops.SMOOTH_ALL, _ptr(blurred))

    def absorb():
        be._call("tpg_surface_absorb_u8", "surface_absorb", 0, p1, _ptr(fluid), _ptr(fdepth), _ptr(blurred), _ptr(solid[0]),
                 _ptr(solid[1]), 1, W, H, th_max, table.ctypes.data, _ptr(image), _ptr(out_depth))
    runs = {
        "tpg_render_spheres_f32": spheres,
        "tpg_render_thickness_f32, no limit": lambda: thickness(None),
        "tpg_render_thickness_f32, limit": lambda: thickness(solid[1]),
        "tpg_surface_smooth_f32 x1 (blur)": blur,
        "tpg_surface_absorb_u8": absorb,
        "render_surface": lambda: render.render_surface(p1, cam, RADIUS),
        "render_surface, translucent": lambda: render.render_surface(p1, cam, RADIUS, translucent=True),
        "render_surface, solids": lambda: render.render_surface(p1, cam, RADIUS, solids=box),
        "render_surface, solids, translucent": lambda: render.render_surface(p1, cam, RADIUS, solids=box, translucent=True),
    }
    for fn in runs.values():                                         # warm-up: code objects, workspaces
        for _ in range(3):
            fn()
    torch.cuda.synchronize(dev)
    times = {k: [] for k in runs}
    for _ in range(a.repeats):
        for k, fn in runs.items():
            times[k].append(event_ms(fn))
    t = {k: statistics.median(v) for k, v in times.items()}
    pairs, rp = covered_pairs(pts, row, RADIUS)
    thickness(None)
    lines = [f"# {torch.cuda.get_device_name(0)}; commit {commit or 'unknown'}; HIP events, {a.repeats} alternating repeats "
             f"after warm-up, median",
             f"scene: {N} particles, {W} x {H}, {cam.mode} camera, particle radius {RADIUS} (discs of median radius {rp:.2f} "
             f"pixels); fluid on {float((thick > 0).float().mean()):.3f} of the picture, thickness at most "
             f"{float(thick.max()) / (2.0 * RADIUS):.1f} diameters; covered sphere x pixel pairs: {pairs}",
             f"{'':40} {'ms per frame':>13}"]
    lines += [f"{k:40} {ms:13.4f}" for k, ms in t.items()]
    lines += [f"thickness / spheres: {t['tpg_render_thickness_f32, no limit'] / t['tpg_render_spheres_f32']:.2f} x; pairs per "
              f"microsecond: spheres {pairs / t['tpg_render_spheres_f32'] / 1e3:.0f}, thickness "
              f"{pairs / t['tpg_render_thickness_f32, no limit'] / 1e3:.0f} (fill and resolve included)"]
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
