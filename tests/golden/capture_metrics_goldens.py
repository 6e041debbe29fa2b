"""Generates tests/golden/metrics.npz by running the REFERENCE's own `position_loss` functions in the build container.

    TPGAN_REFERENCE=<checkout of the reference> python tests/golden/capture_metrics_goldens.py

Same recipe as capture_analysis_goldens.py: the reference checkout (read-only, imported unmodified; never copied, never
shipped) on `sys.path` in this container only, `pytorch3d` / `frnn` / `chamferdist` resolved to this repo's
import-compatible modules with the oracle as their CPU backend, `dgl`, `numba` and `open3d` the inert import shims of
tests/golden/_import_shims.  Never run by a test.

What runs: train_fluid/analysis_helper.py `position_loss(masked_pos, pos_pred, pos_gt)` at B = 1, n = 1024, and
train_action/analysis_helper.py `position_loss(pos_pred, pos_gt)` at n = 2048.

Both rest on two packages that are not available: the `emd` auction extension and `geomloss`.  This script places
RECORDING STAND-INS for them in `sys.modules` (the shim files stay as they are and are shadowed):
  emd.forward       records xyz1, xyz2, eps and iters as they arrive, and fills `dist` / `assignment` in place from
                    scipy.optimize.linear_sum_assignment on the float64 squared distances (the optimal matching)
  geomloss.SamplesLoss  records the constructor's blur and the two clouds, and returns the Gaussian MMD of
                    tpgan_amd.metrics.gaussian_mmd evaluated by the statement of tests/test_metrics_cpu.py (the
                    canonical fp32 squared distance and exponent, float64 exponential and sums)
The reference's wrapper moves its tensors to 'cuda'; there is no GPU in the build container, so `Tensor.cuda` and the
`device=` argument of `torch.zeros` are made no-ops in this process.

So the fixture pins the reference's PYTHON -- the shift to the joint minimum corner, the scale h, the divisors, the
scalars it passes -- not the two absent packages.  `cycle_consistency` needs DGL and cannot be captured.

What is stored: the inputs, the tensors and scalars that reached both stand-ins, the returned cd / emd / mmd and the
optimal sum of squared distances.
"""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("TPGAN_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
if not REFERENCE:
    raise SystemExit("set TPGAN_REFERENCE (or pass the path) to a checkout of the reference")

sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(HERE, "_import_shims"))
sys.path.insert(2, os.path.join(ROOT, "tests"))
warnings.simplefilter("ignore")

import tpgan_amd  # noqa: E402
from oracle import torch_backend  # noqa: E402
from scipy.optimize import linear_sum_assignment  # noqa: E402
from test_metrics_cpu import mmd_statement  # noqa: E402
from tpgan_amd.synthetic import action_clip, fluid_clip  # noqa: E402

tpgan_amd.install_compat()
torch_backend.install()
sys.path.insert(3, REFERENCE)

RECORD = {}

# ---- the stand-ins -----------------------------------------------------------------------------------------------
emd_mod = types.ModuleType("emd")


def _emd_forward(xyz1, xyz2, dist, assignment, *rest):
    eps, iters = rest[-2:]                                    # the reference calls it positionally; the rest is scratch
    RECORD["emd_xyz1"], RECORD["emd_xyz2"] = xyz1.numpy().copy(), xyz2.numpy().copy()
    RECORD["emd_eps"], RECORD["emd_iters"] = np.float64(eps), np.int64(iters)
    total = 0.0
    for b in range(xyz1.shape[0]):
        a, c = xyz1[b].double().numpy(), xyz2[b].double().numpy()
        cost = ((a[:, None, :] - c[None, :, :]) ** 2).sum(-1)
        rows, cols = linear_sum_assignment(cost)
        assignment[b] = torch.from_numpy(cols.astype(np.int32))
        dist[b] = torch.from_numpy(cost[rows, cols].astype(np.float32))
        total += cost[rows, cols].sum()
    RECORD["emd_optimum"] = np.float64(total)


emd_mod.forward = _emd_forward
geomloss_mod = types.ModuleType("geomloss")


class SamplesLoss:
    def __init__(self, loss="sinkhorn", scaling=0.5, blur=0.05, **kw):
        assert loss == "gaussian"
        self.blur = blur

    def __call__(self, x, y):
        RECORD["mmd_x"], RECORD["mmd_y"] = x.numpy().copy(), y.numpy().copy()
        RECORD["mmd_blur"] = np.float64(self.blur)
        return torch.tensor([mmd_statement(a, b, self.blur)[0] for a, b in zip(x.numpy(), y.numpy())])


geomloss_mod.SamplesLoss = SamplesLoss
sys.modules["emd"], sys.modules["geomloss"] = emd_mod, geomloss_mod

# no GPU in the build container: the reference's `.cuda()` / device='cuda' become no-ops in this process
torch.Tensor.cuda = lambda self, *a, **k: self
_zeros = torch.zeros
torch.zeros = lambda *a, **k: _zeros(*a, **{key: v for key, v in k.items() if key != "device"})


def load(name, sub):
    folder = os.path.join(REFERENCE, sub)
    sys.path.insert(0, folder)
    try:
        spec = importlib.util.spec_from_file_location(name, os.path.join(folder, "analysis_helper.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(folder)
    return mod


def main():
    out = {}
    # fluid: a frame against the next one of the same synthetic flow; the "masked" cloud is a subset of the prediction
    _, high = fluid_clip(1, 1024, 8, 2, seed=71)
    pred, gt = high[0].clone(), high[1].clone()
    masked = pred[:, torch.randperm(1024, generator=torch.Generator().manual_seed(72))[:768]].clone()
    out["fluid/masked_pos"], out["fluid/pos_pred"], out["fluid/pos_gt"] = masked.numpy(), pred.numpy(), gt.numpy()
    ref = load("ref_fluid_analysis_helper", "train_fluid")
    RECORD.clear()
    cd, emd, mmd = ref.position_loss(masked.clone(), pred.clone(), gt.clone())
    out.update({f"fluid/{k}": v for k, v in RECORD.items()})
    out["fluid/cd"], out["fluid/emd"], out["fluid/mmd"] = (np.float64(float(v)) for v in (cd, emd, mmd))
    # action: two frames of a synthetic action clip (1/8 of the points are exact repeats)
    _, high = action_clip(1, 2048, 16, 2, seed=73)
    pred, gt = high[0].clone(), high[1].clone()
    out["action/pos_pred"], out["action/pos_gt"] = pred.numpy(), gt.numpy()
    ref = load("ref_action_analysis_helper", "train_action")
    RECORD.clear()
    cd, emd = ref.position_loss(pred.clone(), gt.clone())
    out.update({f"action/{k}": v for k, v in RECORD.items()})
    out["action/cd"], out["action/emd"] = np.float64(float(cd)), np.float64(float(emd))
    path = os.path.join(HERE, "metrics.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print(f"metrics: {os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays")
    for k, v in out.items():
        v = np.asarray(v)
        print(f"  {k}: {v.dtype} {v.shape}" + (f" = {v}" if v.ndim == 0 else ""))


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
