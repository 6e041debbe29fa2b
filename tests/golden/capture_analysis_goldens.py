"""Generates tests/golden/analysis.npz by running the REFERENCE's own analysis functions in the build container.

    python tests/golden/capture_analysis_goldens.py

Same recipe as capture_goldens.py: `/root/reference` (read-only, imported unmodified; never copied, never shipped) on
`sys.path` in this container only, `pytorch3d` / `frnn` / `chamferdist` resolved to this repo's import-compatible
modules, `dgl`, `numba`, `open3d`, `emd` and `geomloss` inert import shims (tests/golden/_import_shims).  With the
`numba` shim the reference's `calc_dns` runs as plain Python, so the clouds are small.

What runs (train_fluid/analysis_helper.py, train_utils.py): get_particle_density, get_particle_density_of_two_pcd,
particle_dns2grid_dns, fixed_radius_neighbor_num, get_free_surface_particles, free_surface_particle_loss and
sample_patch_with_fps(return_free_surface_particles=True).  analysis_helper.py:278 calls get_free_surface_particles
without importing it (the reference's notebooks have it in scope through `from train_utils import *`); the name is put
into the imported module's namespace here, the file itself is untouched.

What is stored: arrays only -- the seeded clouds, and every function's output in the dtype it returns.  Before the
fixture is written, the share of queries whose COUNT the tests may not compare (a stored point within 4e-6 r of the rim,
tests/test_analysis_cpu.py) is checked against the 0.5 % cap for every case; a case above it wants another seed.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = "/root/reference"

sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "_import_shims"))

import tpgan_amd  # noqa: E402

tpgan_amd.install_compat()
sys.path.insert(2, REFERENCE)
sys.path.insert(3, os.path.join(REFERENCE, "train_fluid"))
sys.path.insert(4, os.path.join(ROOT, "tests"))
warnings.simplefilter("ignore")

import analysis_helper as ref_an  # noqa: E402
import train_utils as ref_tu  # noqa: E402

from test_analysis_cpu import CUTOFFS, MAX_EXCLUDED, RADII, excluded  # noqa: E402
from tpgan_amd.synthetic import fluid_clip  # noqa: E402

ref_an.get_free_surface_particles = ref_tu.get_free_surface_particles

SEED_A, SEED_B, SEED_PATCH = 61, 62, 7


def cloud(n, seed):
    _, high = fluid_clip(1, n, 8, 1, seed=seed)
    return high[0][0].numpy().astype(np.float32)


def check_share(tag, query, pos, r):
    share = excluded(query, pos, r).mean()
    print(f"  {tag} r={r}: excluded share {100 * share:.3f} %")
    assert share <= MAX_EXCLUDED, f"{tag} r={r}: {share:.4f} of the queries sit on the rim: pick another seed"


def main():
    out = {}
    a, b = cloud(2048, SEED_A), cloud(4096, SEED_B)
    for tag, pos in (("a", a), ("b", b)):
        out[f"{tag}/pos"] = pos
        for r in RADII:
            check_share(tag, pos, pos, r)
            out[f"{tag}/nbr_num/{r}"] = ref_tu.fixed_radius_neighbor_num(pos, r)
        for r in (0.025, 0.0775):
            out[f"{tag}/surface/{r}"] = ref_tu.get_free_surface_particles(pos, r)
        for c in CUTOFFS:
            out[f"{tag}/density/{c}"] = ref_an.get_particle_density(pos, c)
            print(f"  {tag} cutoff={c}: mean density {out[f'{tag}/density/{c}'].mean():.3f}, "
                  f"mean count {out[f'{tag}/nbr_num/{c}'].mean():.1f}")
    # a regular 8 x 8 x 8 lattice that extends beyond the fluid (the ball of cloud b has radius 0.248)
    ax = np.linspace(-0.4, 0.4, 8, dtype=np.float32)
    lattice = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    out["lattice/pos"] = lattice
    for c in CUTOFFS:
        check_share("lattice", lattice, b, c)
        out[f"lattice/two_pcd/{c}"] = ref_an.get_particle_density_of_two_pcd(lattice, b, c)
        out[f"lattice/grid_dns/{c}"] = ref_an.particle_dns2grid_dns(lattice, b, c)
    # free_surface_particle_loss at its radius 0.025: a jittered copy of b against b
    rng = np.random.RandomState(3)
    pred = (b + rng.normal(0.0, 0.004, b.shape)).astype(np.float32)
    check_share("pred", pred, pred, 0.025)
    out["pred/pos"] = pred
    out["loss/free_surface"] = np.int64(ref_an.free_surface_particle_loss(pred.copy(), b.copy()))
    # the patch sampler's default: surface points of the 2048-point patch at 3.1 * 0.025 / h
    np.random.seed(SEED_PATCH)
    ret, patch, fps_idx = ref_tu.sample_patch_with_fps(b, 1.0, sample_num=2048, return_free_surface_particles=True,
                                                       return_patch_and_fps_idx=True)
    np.random.seed(SEED_PATCH)
    out["patch/seed_idx"] = np.int64(np.random.choice(b.shape[0]))
    assert int(patch[0]) == int(out["patch/seed_idx"])
    check_share("patch", ret["patch_pos"], ret["patch_pos"], 3.1 * 0.025)
    out["patch/h"] = np.float64(1.0)
    out["patch/idx"] = np.asarray(patch, dtype=np.int64)
    out["patch/fps_idx"] = np.asarray(fps_idx, dtype=np.int64)
    out["patch/surface_points"] = ret["surface_points"]
    path = os.path.join(HERE, "analysis.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print(f"analysis: {os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays")
    for k, v in out.items():
        print(f"  {k}: {np.asarray(v).dtype} {np.asarray(v).shape}")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
