"""Particle density (`analysis.get_particle_density`, csrc/radius_reduce.hip on the uniform grid) beside the K = 64
radius search `tpg_frnn_grid_f32` on the same cloud: same grid build, same candidates, a K-best list on top.  GPU box.

For each cloud size: HIP-event time per call (the two alternating inside one window, median of the repeats after a
warm-up of every shape), the algorithmic bytes of the density -- 12 B (Nq + Np) read, 8 B Nq written -- and the
fraction of the HBM peak (8 TB/s, MI355X) those bytes over that time amount to.  Writes profiles/radius_reduce.txt
when --out is given.

    python tools/radius_reduce_time.py [--sizes 20000 65536] [--cutoff 0.0775] [--repeats 200] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import tpgan_amd  # noqa: F401
from tpgan_amd import analysis, ops
from tpgan_amd.synthetic import fluid_clip

HBM_PEAK = 8.0e12


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[20000, 65536])
    ap.add_argument("--cutoff", type=float, default=0.0775)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda", 0)
    lines = [f"# {torch.cuda.get_device_name(0)}; HIP events, {a.repeats} alternating repeats after warm-up, median "
             f"(min .. max); cutoff {a.cutoff}",
             f"{'N':>7} {'op':>28} {'us/call':>9} {'min':>8} {'max':>8} {'neighbours':>10} {'bytes':>9} {'of 8 TB/s':>9}"]
    for n in a.sizes:
        x = fluid_clip(1, n, 8, 1, seed=n, device=dev)[1][0][0].contiguous()
        xb = x.unsqueeze(0)
        runs = {"get_particle_density": lambda: analysis.get_particle_density(x, a.cutoff),
                "fixed_radius_neighbor_num": lambda: analysis.fixed_radius_neighbor_num(x, a.cutoff),
                "frnn_grid K=64": lambda: ops.neighbour_search(xb, xb, 64, r=a.cutoff)}
        for fn in runs.values():                                     # warm-up: code objects, workspaces
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(a.repeats):
            for k, fn in runs.items():
                times[k].append(event_ms(fn) * 1e3)
        mean_nbrs = float(analysis.fixed_radius_neighbor_num(x, a.cutoff).float().mean())
        for k, t in times.items():
            med = statistics.median(t)
            nbytes = 12 * (n + n) + (8 * n if k == "get_particle_density" else 0)
            frac = f"{nbytes / (med * 1e-6) / HBM_PEAK:9.5f}" if k == "get_particle_density" else f"{'':>9}"
            lines.append(f"{n:7d} {k:>28} {med:9.1f} {min(t):8.1f} {max(t):8.1f} {mean_nbrs:10.1f} "
                         f"{nbytes if k == 'get_particle_density' else 0:9d} {frac}")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
