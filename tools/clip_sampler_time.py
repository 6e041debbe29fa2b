"""Time of one training batch from the device-resident clip sampler against the per-clip route it replaces, with one
replayed cfg2 step in the same process for scale.  GPU box.

    python tools/clip_sampler_time.py --out profiles/clip_sampler.txt

Batch 8, scenes of 20 000 / 40 000 / 80 000 particles (3 frames per clip), K = 4096 and 9216.  HIP events, median of
--reps alternating repeats after warm-up (new, old, new, old, ...):
  new      ops.patch_select + ops.clip_gather_high + the FPS entry + noise + ops.clip_gather_low, also each by itself
  per-clip the route before this sampler: ops.sample_patch_with_fps per clip (a torch.topk, a host-drawn seed, one FPS
           launch per clip) and torch indexing for the 12 arrays, stacked into the batch
"""
import argparse
import os
import sys

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
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    torch.backends.cudnn.enabled = False
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    hip = ops.backend_for(torch.zeros(1, device=dev))
    B, T, jitter = a.batch, 3, 0.003
    lines = []

    np.random.seed(0)
    clip = configs.make_clip("cfg2", device=dev)
    stepper = configs.graphed_step("cfg2", configs.build_models("cfg2", dev, capturable=True), clip,
                                   amp_dtype=torch.bfloat16)
    for i in range(6):
        stepper(*clip, 12 + i)
    torch.cuda.synchronize()
    step_ms = median_ms([timed(lambda i=i: stepper(*clip, 12 + (i % 2)), st) for i in range(40)])
    torch.cuda.synchronize()
    lines.append(f"replayed cfg2 step (bf16, median over alternating iterations with and without the discriminator updates): {step_ms:.3f} ms")
    lines.append(f"{'scene':>7} {'K':>6} | {'select':>8} {'gather-hi':>9} {'fps':>8} {'gather-lo':>9} | {'new batch':>9} "
                 f"{'per-clip':>9} {'ratio':>6} | new / step")

    rng = np.random.default_rng(1)
    gen = torch.Generator().manual_seed(0)
    for N in (20000, 40000, 80000):
        pos = torch.from_numpy((rng.uniform(0, 1, (B * T * N, 3)) * (N / 20000) ** (1 / 3)).astype(np.float32)).to(dev)
        vel = torch.from_numpy(rng.normal(0, 0.1, (B * T * N, 3)).astype(np.float32)).to(dev)
        count = np.full(B, N)
        frame_first = np.stack([np.arange(B) * T * N + t * N for t in range(T)])
        centroids = torch.stack([pos[f:f + N].double().mean(0).float() for f in frame_first[1]])
        crow = np.arange(B)
        for K in (4096, 9216):
            M = K // 8

            def draws():
                return (torch.randint(N, (B,), generator=gen).tolist(), torch.randint(K, (B,), generator=gen).tolist())

            keep = {}

            def sel(seeds):
                keep["patch"] = ops.patch_select(pos, frame_first[1], count, seeds, K)

            def ghi():
                keep["hp"], keep["hv"] = ops.clip_gather_high(pos, vel, frame_first, count, centroids, crow, keep["patch"])

            def fps(starts):
                start = torch.tensor(starts, dtype=torch.int32).to(dev)
                keep["fps"] = hip.fps(keep["hp"][1], M, start, False)

            def glo():
                noise = torch.randn((T, B, M, 3), device=dev)
                keep["low"] = ops.clip_gather_low(keep["hp"], keep["fps"], noise, jitter, vel, frame_first, count)

            def new():
                seeds, starts = draws()
                sel(seeds), ghi(), fps(starts), glo()

            def old():
                seeds, starts = draws()
                hp, hv, lp, lv = [[] for _ in range(T)], [[] for _ in range(T)], [[] for _ in range(T)], [[] for _ in range(T)]
                for b in range(B):
                    frames = [pos[frame_first[t, b]:frame_first[t, b] + N] for t in range(T)]
                    vels = [vel[frame_first[t, b]:frame_first[t, b] + N] for t in range(T)]
                    c = centroids[b]
                    r = ops.sample_patch_with_fps(frames[1] - c, K, seed_idx=seeds[b], initial_idx=starts[b])
                    for t in range(T):
                        h = frames[t][r["patch_idx"]] - c
                        hp[t].append(h)
                        hv[t].append(vels[t][r["patch_idx"]])
                        lp[t].append(h[r["fps_idx"]] + torch.randn((M, 3), device=dev) * jitter)
                        lv[t].append(vels[t][r["fps_idx"]])
                keep["old"] = [torch.stack(x) for lst in (hp, hv, lp, lv) for x in lst]

            for _ in range(5):
                new(), old()
            torch.cuda.synchronize()
            t_new, t_old, parts = [], [], {k: [] for k in ("sel", "ghi", "fps", "glo")}
            for _ in range(a.reps):
                t_new.append(timed(new, st))
                t_old.append(timed(old, st))
                seeds, starts = draws()
                parts["sel"].append(timed(lambda: sel(seeds), st))
                parts["ghi"].append(timed(ghi, st))
                parts["fps"].append(timed(lambda: fps(starts), st))
                parts["glo"].append(timed(glo, st))
                torch.cuda.synchronize()
            m_new, m_old = median_ms(t_new), median_ms(t_old)
            lines.append(f"{N:7d} {K:6d} | {median_ms(parts['sel']):8.3f} {median_ms(parts['ghi']):9.3f} "
                         f"{median_ms(parts['fps']):8.3f} {median_ms(parts['glo']):9.3f} | {m_new:9.3f} {m_old:9.3f} "
                         f"{m_old / m_new:6.1f} | {100 * m_new / step_ms:5.1f} %")
            print(lines[-1], flush=True)
    text = "\n".join([f"clip sampler, batch {B}, 3 frames per clip, ms (HIP events, median of {a.reps} alternating repeats)"]
                     + lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
