"""What a frame of the fluid simulator costs (`ops.pbf_substep`, csrc/pbf.hip; `tpgan_amd.simulate`).  GPU box.

Scenes of the default size (`simulate.random_scene(seed)`, seeds 1..), default substeps and iterations.  Every scene is
first advanced WARM frames so that the fluid has hit the floor and the neighbourhoods are those of a splash, not of the
start lattice.  Then, for one scene and for a batch of 24:
  wall      host clock around one frame that ends in a device synchronise, median of the timed frames
  kinds     HIP events around every launch kind (`ops.OpTimer`), in a pass of its own: ms per frame, and the share of the
            grid builds in their sum
and for the one scene the same frame through the host statement (`ops._pbf_substep_torch`) with a
scipy.spatial.cKDTree neighbour search, 16 threads: the baseline.  The host frame must EQUAL the device frame bit for bit,
or the tool fails.

    python tools/simulate_time.py [--frames 10 --warm 12 --batch 24] [--out profiles/simulate.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import tpgan_amd  # noqa: F401
from tpgan_amd import ops
from tpgan_amd import simulate as S

KINDS = ("pbf_predict", "pbf_grid", "pbf_lambda", "pbf_dp", "pbf_finish")
HOST_THREADS = 16


def frame(state, prm):
    x, v, lengths, lo, hi = state
    for _ in range(S.SUBSTEPS):
        x, v = ops.pbf_substep(x, v, lengths, lo, hi, 1.0 / (S.FPS * S.SUBSTEPS), prm)
    return x, v, lengths, lo, hi


def measure(scenes, warm, frames, dev, prm):
    """-> (median wall ms per frame, {kind: event ms per frame}, state before the timed frames, state after the first)."""
    state = S.pack(scenes, dev)
    for _ in range(warm):
        state = frame(state, prm)
    torch.cuda.synchronize(dev)
    start, first, wall = state, None, []
    for _ in range(frames):
        t = time.perf_counter()
        state = frame(state, prm)
        torch.cuda.synchronize(dev)
        wall.append((time.perf_counter() - t) * 1e3)
        first = first or state
    timer = ops.OpTimer()
    ops.set_timer(timer)
    try:
        for _ in range(frames):
            state = frame(state, prm)
        torch.cuda.synchronize(dev)
    finally:
        ops.set_timer(None)
    kinds = {k: r["total_ms"] / frames for k, r in timer.summary().items()}
    return statistics.median(wall), kinds, start, first


def kdtree_neighbours(p, h):
    """Candidate pairs from scipy's KD-tree, 16 workers: every pair within 1.001 h."""
    from scipy.spatial import cKDTree
    q = p.double().numpy()
    n, k = len(q), 64
    tree = cKDTree(q)
    while True:
        _, idx = tree.query(q, k=min(k, n), distance_upper_bound=1.001 * h, workers=HOST_THREADS)
        idx = idx.reshape(n, -1)
        if k >= n or (idx[:, -1] == n).all():                # every row has an empty slot: nothing was cut off
            break
        k *= 2
    valid = idx < n
    return torch.from_numpy(np.repeat(np.arange(n), valid.sum(1))), torch.from_numpy(idx[valid])


def host_frame(start, prm):
    """One frame of scene 0 by the host statement -> (seconds, x, v)."""
    x, v, lengths, lo, hi = start
    n = int(lengths[0])
    x, v = x[:1, :n].cpu(), v[:1, :n].cpu()
    box = ops.pbf_box(lo[:1], hi[:1], 1)
    torch.set_num_threads(HOST_THREADS)
    t = time.perf_counter()
    for _ in range(S.SUBSTEPS):
        x, v = ops._pbf_substep_torch(x, v, None, box, float(np.float32(1.0 / (S.FPS * S.SUBSTEPS))), prm, kdtree_neighbours)
    return time.perf_counter() - t, x, v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--warm", type=int, default=12)
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda", 0)
    prm = ops.PbfParams()
    scenes = [S.random_scene(s) for s in range(1, a.batch + 1)]
    counts = [len(s.particles()[0]) for s in scenes]
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True,
                                         stderr=subprocess.DEVNULL).strip()
    except Exception:
        commit = "working tree"
    lines = [f"# {torch.cuda.get_device_name(0)}; {commit} plus the fluid simulator; substeps {S.SUBSTEPS}, iters {prm.iters}; "
             f"{a.warm} frames of warm-up, then {a.frames} timed frames: wall = host clock + synchronise, median; kinds = HIP "
             "events in a pass of their own",
             f"scenes: seeds 1..{a.batch}, particles {counts[0]} (the single scene), batch total {sum(counts)}, "
             f"largest {max(counts)}"]
    table = {}
    for name, group in (("1 scene", scenes[:1]), (f"{a.batch} scenes", scenes)):
        wall, kinds, start, first = measure(group, a.warm, a.frames, dev, prm)
        table[name] = (wall, kinds)
        if name == "1 scene":
            host_s, hx, hv = host_frame(start, prm)
            n = counts[0]
            same = torch.equal(hx[0], first[0][0, :n].cpu()) and torch.equal(hv[0], first[1][0, :n].cpu())
            assert same, "the host statement's frame differs from the device's"
    names = list(table)
    lines.append(f"{'ms per frame':28s}" + "".join(f"{n:>14s}" for n in names))
    lines.append(f"{'wall':28s}" + "".join(f"{table[n][0]:14.3f}" for n in names))
    for k in KINDS:
        lines.append(f"{k:28s}" + "".join(f"{table[n][1].get(k, 0.0):14.3f}" for n in names))
    lines.append(f"{'sum of the kinds':28s}" + "".join(f"{sum(table[n][1].values()):14.3f}" for n in names))
    lines.append(f"{'share of the grid builds':28s}" +
                 "".join(f"{table[n][1].get('pbf_grid', 0.0) / sum(table[n][1].values()):14.3f}" for n in names))
    per_scene = table[names[1]][0] / a.batch
    lines.append(f"batch: {per_scene:.3f} ms per frame and scene; {sum(counts) / table[names[1]][0] / 1e3:.2f} M particle-frames/s")
    lines.append(f"host statement, scipy cKDTree neighbours, {HOST_THREADS} threads, the single scene's first timed frame: "
                 f"{host_s * 1e3:.0f} ms (one frame, not repeated), equal to the device's bit for bit; "
                 f"device / host = 1 / {host_s * 1e3 / table[names[0]][0]:.0f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
