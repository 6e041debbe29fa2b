"""Time of one batch of action clips from the device-resident sampler against a per-frame host route, with one replayed
cfg4 step in the same process for scale.  GPU box.

    python tools/action_sampler_time.py --out profiles/action_sampler.txt

Batch 8, 3 frames per clip, K = 2048 (low resolution 128), depth frames of 3 000 - 10 000 points.  HIP events on the
sampler's stream for the device route, wall clock (with a device synchronisation) for the host route, median of --reps
alternating repeats after warm-up:
  new        ops.frame_subset + ops.action_gather + one FPS over the 24 clouds + ops.clip_gather_low, also each by itself
  per-frame  the reference loader's work, frame by frame, without its numba FPS (not installed here): np.random.choice
             and the fp64 gather / scale / centre in numpy on the host, one upload and one FPS launch per frame
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import tpgan_amd  # noqa: F401
from tpgan_amd import configs, ops


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    return a, b


def median_ms(pairs):
    return float(np.median([a.elapsed_time(b) for a, b in pairs]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    torch.backends.cudnn.enabled = False
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    hip = ops.backend_for(torch.zeros(1, device=dev))
    B, T, K = a.batch, 3, 2048
    M = K // 16
    lines = []

    np.random.seed(0)
    clip = configs.make_clip("cfg4", device=dev)
    stepper = configs.graphed_step("cfg4", configs.build_models("cfg4", dev, capturable=True), clip,
                                   amp_dtype=torch.bfloat16)
    for i in range(6):
        stepper(*clip, 12 + i)
    torch.cuda.synchronize()
    step_ms = median_ms([timed(lambda i=i: stepper(*clip, 12 + (i % 2)), st) for i in range(40)])
    torch.cuda.synchronize()
    lines.append(f"replayed cfg4 step (bf16, median over alternating iterations with and without the discriminator updates): {step_ms:.3f} ms")

    rng = np.random.default_rng(1)
    gen = torch.Generator().manual_seed(0)
    count = rng.integers(3000, 10001, size=(T, B))
    first = np.concatenate([[0], np.cumsum(count.reshape(-1))[:-1]]).reshape(T, B)
    host_points = np.stack([rng.integers(0, 240, int(count.sum())), rng.integers(0, 320, int(count.sum())),
                            rng.integers(400, 600, int(count.sum()))], 1).astype(np.float32)
    points = torch.from_numpy(host_points).to(dev)
    keep = {}

    def draws():
        halves = torch.randint(2 ** 32, (T * B, 2), generator=gen).numpy().astype(np.uint64)
        scales = 0.9 + 0.2 * torch.rand((B, 3), dtype=torch.float64, generator=gen).numpy()
        return (halves[:, 1] << np.uint64(32)) | halves[:, 0], scales, torch.randint(K, (T * B,), generator=gen)

    def sel(seeds):
        keep["sub"] = ops.frame_subset(count.reshape(-1), seeds, K, device=dev).view(T, B, K)

    def gat(scales):
        keep["high"], _ = ops.action_gather(points, first, count, keep["sub"], scales, "train")

    def fps(starts):
        start = starts.to(torch.int32).to(dev, non_blocking=True)
        keep["fps"] = hip.fps(keep["high"].view(T * B, K, 3), M, start, False)

    def low():
        keep["low"], _ = ops.clip_gather_low(keep["high"].view(1, T * B, K, 3), keep["fps"])

    def new():
        seeds, scales, starts = draws()
        sel(seeds), gat(scales), fps(starts), low()

    def old():
        _, scales, starts = draws()
        high, lo = [], []
        for b in range(B):
            v = []
            for t in range(T):
                n = int(count[t, b])
                r = np.random.choice(n, size=K, replace=False)
                q = host_points[first[t, b]:first[t, b] + n][r].astype(np.float64)
                q[:, 1] = -q[:, 1]
                v.append((q * scales[b]) / 300.0)
            c = v[T // 2].mean(0)
            for t in range(T):
                h = torch.from_numpy((v[t] - c).astype(np.float32)).to(dev)
                i = hip.fps(h.view(1, K, 3), M, starts[t * B + b:t * B + b + 1].to(torch.int32).to(dev), False)
                high.append(h)
                lo.append(h[i[0].long()])
        keep["old"] = (torch.stack(high), torch.stack(lo))

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(5):
        new(), old()
    torch.cuda.synchronize()
    t_new, t_wall, t_old, parts = [], [], [], {k: [] for k in ("sel", "gat", "fps", "low")}
    for _ in range(a.reps):
        t_new.append(timed(new, st))
        t_old.append(wall(old))
        t_wall.append(wall(new))
        seeds, scales, starts = draws()
        parts["sel"].append(timed(lambda: sel(seeds), st))
        parts["gat"].append(timed(lambda: gat(scales), st))
        parts["fps"].append(timed(lambda: fps(starts), st))
        parts["low"].append(timed(low, st))
        torch.cuda.synchronize()
    m_new, m_wall, m_old = median_ms(t_new), float(np.median(t_wall)), float(np.median(t_old))
    lines.append(f"frames of {int(count.min())} - {int(count.max())} points ({int(count.sum())} in the batch), K = {K}, low = {M}")
    lines.append(f"  frame_subset {median_ms(parts['sel']):.3f}   action_gather {median_ms(parts['gat']):.3f}   "
                 f"fps (24 clouds, one launch) {median_ms(parts['fps']):.3f}   clip_gather_low {median_ms(parts['low']):.3f}")
    lines.append(f"  new batch: {m_new:.3f} ms on the stream, {m_wall:.3f} ms wall clock with a synchronisation "
                 f"= {100 * m_new / step_ms:.1f} % of the cfg4 step")
    lines.append(f"  per-frame host route: {m_old:.3f} ms wall clock = {m_old / m_wall:.1f} x the new batch's wall clock, "
                 f"{100 * m_old / step_ms:.1f} % of the cfg4 step")
    text = "\n".join([f"action-clip sampler, batch {B}, 3 frames per clip, ms (median of {a.reps} alternating repeats)"]
                     + lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
