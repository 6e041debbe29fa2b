"""What a picture costs: `ops.render_points` (csrc/render.hip) beside the numpy statement of its rule on the host
(tests/render_rule.py), a rollout with and without `--render`, and one training test pass beside one cfg2 step.  GPU box.

Kernel table: for every cloud size, picture size and splat size, ms per FRAME of a call of 1 frame and of a call of 16
frames (HIP events; the shapes alternate inside one window, median of the repeats after a warm-up of every shape), and
the wall time of the host statement on one frame (once: it is a Python loop).  The clouds are synthetic fluid blobs
under `Camera.fit`, coloured by depth.

    python tools/render_time.py [--repeats 30] [--skip_host] [--out profiles/render.txt]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import tpgan_amd  # noqa: F401
from tpgan_amd import configs, ops, render, rollout, train
from tpgan_amd.srnet import SRNet
from tpgan_amd.synthetic import fluid_clip, force_all_keep

SIZES = (4096, 73728, 65536)
EXTENTS = (512, 768)
SPLATS = (1, 3, 5)
BATCH = 16


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


def kernel_table(dev, repeats, skip_host):
    import render_rule
    lut = torch.from_numpy(render.default_lut()).to(dev)
    lines = [f"{'points':>7} {'picture':>9} {'size':>4} {'ms/frame F=1':>13} {'ms/frame F=16':>14} {'host ms/frame':>14} "
             f"{'covered':>8}"]
    runs, info = {}, {}
    for n in SIZES:
        cloud = fluid_clip(1, n, 8, BATCH, seed=n, device=dev)[1]             # BATCH frames of one drifting blob
        pts = torch.cat(cloud).contiguous()                                   # (BATCH, n, 3)
        for e in EXTENTS:
            cam = render.Camera.fit(pts, width=e, height=e)
            row = cam.row()
            for s in SPLATS:
                for F in (1, BATCH):
                    x = pts[:F].contiguous()
                    runs[(n, e, s, F)] = lambda x=x, row=row, e=e, s=s: ops.render_points(x, row, e, e, lut, size=s)
                info[(n, e, s)] = (pts[:1].cpu().numpy(), row)
    for fn in runs.values():                                                  # warm-up: code object, key buffer
        for _ in range(3):
            fn()
    torch.cuda.synchronize(dev)
    times = {k: [] for k in runs}
    for _ in range(repeats):
        for k, fn in runs.items():
            times[k].append(event_ms(fn) / k[3])
    for (n, e, s), (host_pts, row) in info.items():
        covered = float((runs[(n, e, s, 1)]()[1] >= 0).float().mean())
        host = ""
        if not skip_host:
            t = time.perf_counter()
            render_rule.render_rule(host_pts, row, e, e, s, render.default_lut(), (255, 255, 255))
            host = f"{(time.perf_counter() - t) * 1e3:14.0f}"
        lines.append(f"{n:7d} {e:4d}x{e:<4d} {s:4d} {statistics.median(times[(n, e, s, 1)]):13.4f} "
                     f"{statistics.median(times[(n, e, s, BATCH)]):14.4f} {host:>14} {covered:8.3f}")
    return lines


def rollout_lines(dev, repeats):
    """32 frames of 2048 points -> 16384 through SequenceUpsampler in chunks of 16, outputs copied to the host as the
    CLI does; with --render additionally SequenceRenderer.push per chunk (768 x 768, size 3, PNG files included)."""
    frames, n = 32, 2048
    low = torch.cat(fluid_clip(1, n * 8, 8, frames, seed=32, device=dev)[0]).contiguous()
    torch.manual_seed(0)
    net = force_all_keep(SRNet(3, 128)).to(dev).eval()

    def run(pictures):
        up = rollout.SequenceUpsampler(net, 16)
        for i in range(0, frames, 16):
            outs = up.push(low[i:i + 16], low[i:i + 16])
            if pictures is not None:
                pictures.push([o[0] for o in outs], i)
            for o in outs:
                o[0].cpu().numpy()
    with tempfile.TemporaryDirectory() as tmp:
        seq = render.SequenceRenderer(tmp, device=dev)
        run(seq)                                                              # warm-up, and the camera's fit
        plain = [wall_ms(lambda: run(None), dev) / frames for _ in range(repeats)]
        drawn = [wall_ms(lambda: run(seq), dev) / frames for _ in range(repeats)]
        batch = [o[0] for o in rollout.SequenceUpsampler(net, 16).push(low[:16], low[:16])]
        padded, lengths = render.pad_frames(batch, dev)
        call = [event_ms(lambda: render.render(padded, seq.camera, lengths=lengths)) / 16 for _ in range(repeats)]
    return [f"rollout, 32 frames of {n} -> {8 * n} points, chunks of 16, wall ms per frame (median of {repeats}):",
            f"  without --render {statistics.median(plain):8.3f}",
            f"  with --render    {statistics.median(drawn):8.3f}   (768x768, size 3; the render call itself "
            f"{statistics.median(call):.4f} ms per frame by HIP events, the rest is the PNG encoding and the files)"]


def training_lines(dev, repeats):
    """One cfg2 eager step (bf16, as the trainer runs it) beside one test pass of 4 held-out clips of the reference's
    test patch (9216 points from 1152), pictures of 512 x 512 written to a scratch directory."""
    models = configs.build_models("cfg2", dev)
    clip = configs.make_clip("cfg2", device=dev)
    step = [wall_ms(lambda: configs.eager_step("cfg2", models, clip, amp_dtype=torch.bfloat16), dev)
            for _ in range(repeats + 3)][3:]
    low, high = fluid_clip(4, 9216, 8, 1, seed=9, device=dev)
    clips = [{"gt": high[0][j].contiguous(), "input": low[0][j].contiguous(), "feature": low[0][j:j + 1].contiguous()}
             for j in range(4)]
    with tempfile.TemporaryDirectory() as tmp:
        held = train.HeldOutPass(clips, lambda net, c: net(c["feature"], c["input"][None], hard_masking=True)[2], tmp,
                                 512, 512, torch.bfloat16)
        held(models[0], 0)
        test = [wall_ms(lambda: held(models[0], 1), dev) for _ in range(repeats)]
    for net in models[:3]:
        net.train()
    return [f"training, wall ms (median of {repeats}):",
            f"  one cfg2 eager step (batch 8, bf16)            {statistics.median(step):8.2f}",
            f"  one test pass, --samples 4 (4 x 3 PNG 512x512) {statistics.median(test):8.2f}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--skip_host", action="store_true", help="leave the host statement's column empty")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    torch.backends.cudnn.enabled = False
    dev = torch.device("cuda", 0)
    lines = [f"# {torch.cuda.get_device_name(0)}; ops.render_points, depth colour, Camera.fit; HIP events, {a.repeats} "
             "alternating repeats after warm-up, median; host = tests/render_rule.py on one frame, once"]
    lines += kernel_table(dev, a.repeats, a.skip_host)
    lines += [""] + rollout_lines(dev, max(3, a.repeats // 6))
    lines += [""] + training_lines(dev, max(3, a.repeats // 6))
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
