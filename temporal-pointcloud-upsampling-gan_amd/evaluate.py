"""Scores a sequence of predicted frames against the true ones on the GPU.

    python -m tpgan_amd.evaluate --pred 'out/pcd_{i}.npy' --gt 'gt/data_{i}.npz' --count 200 --out scores.npz

Per frame one JSON line with `cd` (Chamfer distance per true point), `emd` and `mmd` (both in the frame's joint
normalisation, as `metrics.position_loss`) and `free_surface_diff` (`analysis.free_surface_particle_loss`), then one
line with their means.  Frame files are `.npy` arrays (N,3) or `.npz` archives with a `pos` entry.

EMD matches clouds of equal size.  Where a frame's two clouds differ in their number of points, it is taken on a
seeded random subset of `--emd_points` points of each (default: the largest multiple of 1024 not above the smaller
count, or the smaller count itself below 1024).

The matching takes at most `--emd_iters` rounds per frame (default: `metrics.round_cap`, the reference's 3000 up to 2048
points, scaled with the number of matched points beyond).  A frame that needs more ends the run with an error that
names the frame; raise `--emd_iters`, or match fewer points with `--emd_points`.
"""
import argparse
import json

import numpy as np
import torch

from . import analysis, metrics, ops
from .losses import chamfer_distance

KEYS = ("cd", "emd", "mmd", "free_surface_diff")


def load_frame(path):
    data = np.load(path)
    pos = data["pos"] if hasattr(data, "files") else data
    return np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)


def default_emd_points(n_pred, n_gt):
    small = min(n_pred, n_gt)
    return small // 1024 * 1024 if small >= 1024 else small


def frame_scores(pred, gt, emd_points=None, generator=None, emd_iters=None):
    """pred (N,3), gt (M,3) GPU tensors -> dict of the four scores (python numbers)."""
    ops._need(pred.dim() == 2 and gt.dim() == 2 and pred.shape[1] == 3 and gt.shape[1] == 3, "frames must be (N,3)")
    ops._need(pred.shape[0] > 0 and gt.shape[0] > 0, "frames must not be empty")
    p, g = pred[None], gt[None]
    cd = chamfer_distance(p, g) / g.shape[1]
    corner, h = metrics._joint_frame(p, g)
    pn, gn = (p - corner) / h, (g - corner) / h
    mmd = metrics.gaussian_mmd(pn, gn, blur=0.01)
    if pred.shape[0] != gt.shape[0] or emd_points is not None:
        m = default_emd_points(pred.shape[0], gt.shape[0]) if emd_points is None else int(emd_points)
        ops._need(1 <= m <= min(pred.shape[0], gt.shape[0]),
                  f"--emd_points must be in [1, {min(pred.shape[0], gt.shape[0])}], got {m}")
        pn = pn[:, torch.randperm(pred.shape[0], generator=generator)[:m].to(pred.device)]
        gn = gn[:, torch.randperm(gt.shape[0], generator=generator)[:m].to(gt.device)]
    emd = metrics.earth_mover_distance(pn, gn, eps=0.03,
                                       iters=metrics.round_cap(pn.shape[1], 3000) if emd_iters is None else emd_iters)
    return {"cd": float(cd), "emd": float(emd[0]), "mmd": float(mmd[0]),
            "free_surface_diff": int(analysis.free_surface_particle_loss(pred, gt))}


def parser():
    ap = argparse.ArgumentParser(prog="python -m tpgan_amd.evaluate",
                                 description="Chamfer distance, EMD, Gaussian MMD and free-surface difference per frame.")
    ap.add_argument("--pred", required=True, help="predicted frames, '{i}' = frame index, e.g. 'out/pcd_{i}.npy'")
    ap.add_argument("--gt", required=True, help="true frames, e.g. 'gt/data_{i}.npz' (entry 'pos')")
    ap.add_argument("--count", type=int, required=True, help="number of frames")
    ap.add_argument("--start", type=int, default=0, help="first frame index")
    ap.add_argument("--emd_points", type=int, default=None, help="points of each cloud that EMD is taken on")
    ap.add_argument("--emd_iters", type=int, default=None, help="cap on the rounds of a frame's matching")
    ap.add_argument("--seed", type=int, default=0, help="seed of the EMD subsets")
    ap.add_argument("--out", default=None, help="output .npz with the per-frame series")
    ap.add_argument("--device", default="cuda")
    return ap


def parse_args(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    for name in ("pred", "gt"):
        if "{i}" not in getattr(a, name):
            ap.error(f"--{name} must contain '{{i}}'")
    if a.count < 1:
        ap.error("--count must be at least 1")
    if a.start < 0:
        ap.error("--start must not be negative")
    if a.emd_points is not None and a.emd_points < 1:
        ap.error("--emd_points must be at least 1")
    if a.emd_iters is not None and a.emd_iters < 1:
        ap.error("--emd_iters must be at least 1")
    return a


def main(argv=None):
    a = parse_args(argv)
    dev = torch.device(a.device)
    gen = torch.Generator(device="cpu").manual_seed(a.seed)
    series = {k: [] for k in KEYS}
    for i in range(a.start, a.start + a.count):
        pred = torch.from_numpy(load_frame(a.pred.format(i=i))).to(dev)
        gt = torch.from_numpy(load_frame(a.gt.format(i=i))).to(dev)
        try:
            s = frame_scores(pred, gt, a.emd_points, gen, a.emd_iters)
        except RuntimeError as e:
            if "unassigned persons" not in str(e):
                raise
            raise SystemExit(f"frame {i}: {e}; raise --emd_iters or match fewer points with --emd_points")
        for k in KEYS:
            series[k].append(s[k])
        print(json.dumps({"frame": i, **s}), flush=True)
    means = {k: float(np.mean(series[k])) for k in KEYS}
    print(json.dumps({"frames": a.count, "mean": means}), flush=True)
    if a.out:
        np.savez(a.out, frame=np.arange(a.start, a.start + a.count), **{k: np.asarray(v) for k, v in series.items()})


if __name__ == "__main__":
    main()
