"""Critical-path sensitivity of the graph-replayed step: replace ONE search op by a free stand-in
(indices of the right shape, wrong values), or leave a discriminator update out, and time the step.  The
difference to the real step is the most any optimisation of that part could buy; it is a measurement aid
only, nothing here is product code, and what it times is not a training step.

    python tools/what_if.py [fps] [knn] [ball_query] [skip_t | skip_s | skip_ts] [--config cfg4]

skip_t / skip_s / skip_ts: the temporal / spatial / both discriminator updates' forward and backward are not
issued (`GraphedFluidStep._update` is replaced by a stand-in that only stores a zero loss under the update's
key; their index plans and optimizer launches stay).  `profiles/r03_whatif_update_branches.txt` was recorded
with an environment switch inside the step (TPGAN_WHATIF_SKIP=t|s|ts under tools/ab_env.py), which is gone;
its figures are reproduced by running, alternately on one box,

    python tools/what_if.py            python tools/what_if.py skip_t
    python tools/what_if.py skip_s     python tools/what_if.py skip_ts

and the same with `--config cfg4`, and comparing the `ms_per_step` of the result lines.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                             # noqa: E402

import bench                                                             # noqa: E402
from tpgan_amd import ops                                                # noqa: E402
from tpgan_amd.gan_step_graph import GraphedFluidStep                    # noqa: E402


def free_fps(self, xyz, m, start=None, skip_origin=True):
    B, N, _ = xyz.shape
    step = max(N // m, 1)
    return (torch.arange(m, device=xyz.device, dtype=torch.int32) * step % N).expand(B, m).contiguous()


_cache = {}


def free_knn(self, p1, p2, len1, len2, K, r2, r=None):
    B, P1, D = p1.shape
    key = (B, P1, p2.shape[1], K)
    if key not in _cache:
        idx = (torch.arange(P1, device=p1.device).view(1, P1, 1) + torch.arange(K, device=p1.device).view(1, 1, K) * 7) % p2.shape[1]
        _cache[key] = (torch.full((B, P1, K), 0.01, device=p1.device), idx.expand(B, P1, K).contiguous())
    return _cache[key]


def free_bq(self, radius, nsample, xyz, new_xyz):
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    key = ("bq", B, N, S, nsample)
    if key not in _cache:
        idx = (torch.arange(S, device=xyz.device).view(1, S, 1) * (N // S) + torch.arange(nsample, device=xyz.device).view(1, 1, nsample)) % N
        _cache[key] = idx.to(torch.int32).expand(B, S, nsample).contiguous()
    return _cache[key]


def skip_updates(keys):
    """Stand-in for GraphedFluidStep._update: the updates that write `keys` report a zero loss and launch nothing."""
    real = GraphedFluidStep._update

    def update(self, dis, optim, branch, passes, plan, key, side, args=()):
        if key not in keys:
            return real(self, dis, optim, branch, passes, plan, key, side, args)
        self._keep[key] = torch.zeros((), device=self.dev)
    return update


SKIPS = {"skip_t": ("tempo_dis_loss",), "skip_s": ("spatial_dis_loss",), "skip_ts": ("tempo_dis_loss", "spatial_dis_loss")}


def main():
    which, config = sys.argv[1:], []
    if "--config" in which:                                   # passed on to bench.py
        i = which.index("--config")
        config, which = which[i:i + 2], which[:i] + which[i + 2:]
    if "fps" in which:
        ops.HipBackend.fps = free_fps
    if "knn" in which:
        ops.HipBackend.knn = free_knn
    if "ball_query" in which:
        ops.HipBackend.ball_query = free_bq
    for mode, keys in SKIPS.items():
        if mode in which:
            GraphedFluidStep._update = skip_updates(keys)
    sys.argv = [sys.argv[0], "--steps", "30", "--warmup", "3", "--no-extra"] + config
    print("stand-ins:", which or "none")
    bench.main()


if __name__ == "__main__":
    main()
