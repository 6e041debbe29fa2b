"""What a picture of the fluid's surface costs: `ops.render_surface` (csrc/surface.hip) beside `ops.render_points`
(csrc/render.hip), stage by stage, and a rollout chunk with `--render` in both styles.  GPU box.

80 000 synthetic fluid points (the `synthetic.fluid_clip` ball) under `Camera.fit`, 768 x 768, depth colour, spheres whose
discs have about 4 pixels radius, 3 smoothing passes of half-width 2.  Times are HIP events, ms per FRAME of a call of 1
frame and of a call of 8; the shapes alternate inside one window, median of the repeats after a warm-up of every shape.
Stages: (a) tpg_render_spheres_f32, (b) ONE pass of tpg_surface_smooth_f32, (c) tpg_surface_shade_f32.

    python tools/surface_time.py [--repeats 30] [--out profiles/surface.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import tpgan_amd  # noqa: F401
from tpgan_amd import ops, render, rollout
from tpgan_amd.ops import _ptr
from tpgan_amd.srnet import SRNet
from tpgan_amd.synthetic import fluid_clip, force_all_keep

POINTS, EXTENT, BATCH, DISC = 80000, 768, 8, 4.0
HALF, ITERS = 2, 3


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


def stages(be, pts, row, radius, lut):
    """-> {name: callable} of the three entries on buffers of their own (the smoothing reads what (a) wrote)."""
    F, N, _ = pts.shape
    dev, W, H = pts.device, EXTENT, EXTENT
    keys = torch.empty((F, H, W), dtype=torch.int64, device=dev)
    raw, out = (torch.empty((F, H, W), dtype=torch.float32, device=dev) for _ in range(2))
    winner = torch.empty((F, H, W), dtype=torch.int32, device=dev)
    image = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    bg = torch.full((3,), 255, dtype=torch.uint8, device=dev)
    shade, cams = ops.surface_shade(), np.ascontiguousarray(row.reshape(1, -1))
    far = float(row[16] - row[15])

    def a():
        be._call("tpg_render_spheres_f32", "render_spheres", 0, pts, _ptr(pts), None, F, N, cams.ctypes.data, 1, W, H, radius,
                 _ptr(keys), _ptr(raw), _ptr(winner))

    def b():
        be._call("tpg_surface_smooth_f32", "surface_smooth", 0, pts, _ptr(raw), F, W, H, HALF, 2.0 * radius, _ptr(out))

    def c():
        be._call("tpg_surface_shade_f32", "surface_shade", 0, pts, _ptr(out), _ptr(winner), None, F, N, cams.ctypes.data, 1,
                 W, H, 0.0, far, _ptr(lut), _ptr(bg), shade.ctypes.data, _ptr(image))
    return {"(a) spheres": a, "(b) smooth x1": b, "(c) shade": c}


def kernel_lines(dev, repeats):
    lut = torch.from_numpy(render.default_lut()).to(dev)
    pts = torch.cat(fluid_clip(1, POINTS, 8, BATCH, seed=80, device=dev)[1]).contiguous()         # (BATCH, POINTS, 3)
    cam = render.Camera.fit(pts, width=EXTENT, height=EXTENT)
    row = cam.row()
    zv = float(((pts[0] - torch.from_numpy(row[0:3]).to(dev)) @ torch.from_numpy(row[9:12]).to(dev)).median())
    radius = float(np.float32(DISC * zv / row[12]))                  # pinhole: rp = (rad / zv) * scale
    be = ops.backend_for(pts)
    runs = {}
    for F in (1, BATCH):
        x = pts[:F].contiguous()
        runs[("render_points, size 3", F)] = lambda x=x: ops.render_points(x, row, EXTENT, EXTENT, lut, size=3)
        runs[("render_surface", F)] = lambda x=x: ops.render_surface(x, row, EXTENT, EXTENT, lut, radius, half_width=HALF,
                                                                     iters=ITERS)
        for name, fn in stages(be, x, row, radius, lut).items():
            runs[(name, F)] = fn
    for fn in runs.values():                                         # warm-up: code objects, workspaces
        for _ in range(3):
            fn()
    torch.cuda.synchronize(dev)
    times = {k: [] for k in runs}
    for _ in range(repeats):
        for k, fn in runs.items():
            times[k].append(event_ms(fn) / k[1])
    depth = ops.render_surface(pts[:1].contiguous(), row, EXTENT, EXTENT, lut, radius)[1]
    lines = [f"{POINTS} points, {EXTENT} x {EXTENT}, particle radius {radius:.5f} (discs of about {DISC:g} pixels), "
             f"{ITERS} passes of half-width {HALF}; surface on {float(torch.isfinite(depth).float().mean()):.3f} of the picture",
             f"{'':24} {'ms/frame F=1':>13} {'ms/frame F=' + str(BATCH):>14}"]
    for name in dict.fromkeys(k[0] for k in runs):
        lines.append(f"{name:24} {statistics.median(times[(name, 1)]):13.4f} {statistics.median(times[(name, BATCH)]):14.4f}")
    return lines


def rollout_lines(dev, repeats):
    """One chunk of 16 frames of 2048 points -> 16384 through SequenceUpsampler, outputs copied to the host as the CLI does,
    with SequenceRenderer.push in either style (768 x 768, PNG files included)."""
    frames, n = 16, 2048
    low = torch.cat(fluid_clip(1, n * 8, 8, frames, seed=32, device=dev)[0]).contiguous()
    torch.manual_seed(0)
    net = force_all_keep(SRNet(3, 128)).to(dev).eval()

    def run(pictures):
        outs = rollout.SequenceUpsampler(net, frames).push(low, low)
        if pictures is not None:
            pictures.push([o[0] for o in outs], 0)
        for o in outs:
            o[0].cpu().numpy()
    lines = [f"rollout, one chunk of {frames} frames of {n} -> {8 * n} points, wall ms per frame (median of {repeats}):"]
    with tempfile.TemporaryDirectory() as tmp:
        for label, seq in (("without --render", None),
                           ("--render --style points", render.SequenceRenderer(tmp, device=dev)),
                           ("--render --style surface", render.SequenceRenderer(tmp, device=dev, style="surface"))):
            run(seq)                                                 # warm-up, and the camera's fit
            lines.append(f"  {label:26} {statistics.median(wall_ms(lambda: run(seq), dev) / frames for _ in range(repeats)):8.3f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--commit", default=None, help="the commit the times are taken on (default: git's HEAD)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    torch.backends.cudnn.enabled = False
    dev = torch.device("cuda", 0)
    commit = a.commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                        text=True).stdout.strip()
    lines = [f"# {torch.cuda.get_device_name(0)}; commit {commit or 'unknown'}; HIP events, "
             f"{a.repeats} alternating repeats after warm-up, median"]
    lines += kernel_lines(dev, a.repeats)
    lines += [""] + rollout_lines(dev, max(3, a.repeats // 6))
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
