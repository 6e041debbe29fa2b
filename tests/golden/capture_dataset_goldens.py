"""Generates tests/golden/dataset.npz by running the REFERENCE's own dataset class in the build container.

    python tests/golden/capture_dataset_goldens.py

Same recipe as capture_analysis_goldens.py: `/root/reference` (read-only, imported unmodified; never copied, never
shipped) on `sys.path` in this container only, the inert import shims of tests/golden/_import_shims (with the `numba`
shim the reference's FPS loop runs as plain Python).

What runs: train_fluid/tempo_dataset.py `SiamData(root, 2, 5, sample_num=4096, jitter=0.0).__getitem__(idx)` on a toy
dataset written to a temporary directory: 2 cases x 5 steps of ~6000 persistent particles (a jittered lattice of
spacing 0.025 in a ball centred at (1, 0.5, 2)) moved by a smooth velocity field.  Frame s of a case is
`pos0 + float32(s * 0.025) * vel` in float32 numpy (`frame()` below, which tests/test_data_cpu.py imports nothing from:
it restates the line); only pos0 and vel are stored, ~290 KB in all.

What is stored per kept item: the clip index, its three file keys, the seed particle, the reference's `patch_idx` and
`fps_idx` (recorded by wrapping `sample_patch_with_fps` in tempo_dataset's namespace; the file is untouched), the
relative gap between the K-th and (K+1)-th float64 distance, h, and the reference's float32 centroid of the centre
frame: the 12 arrays the item returned are gathers of the frames by the two index lists, the positions minus that
centroid, which is checked here array by array before the centroid is stored in their place.

Conditions (checked here, not in the tests):
  * the KD-tree ranks float64 distances, the sampler fp32 d2 (relative error a few 2^-24): the two can only disagree about
    membership if the K-th and (K+1)-th neighbour are closer than that, so only items whose relative gap is >= 1e-6 are
    kept, and fewer than 3 kept items is an error;
  * every kept item must reproduce under this file's own numpy statement of the sampler (`restate`): same patch set;
    and, with the reference's patch order and first FPS pick, the same FPS picks on the patch centred with the
    float64-accumulated centroid, velocities equal, positions within 16 * 2^-24 * max|pos|.  The position bound is a
    condition on the REFERENCE's centroid: `np.mean(pos, axis=0)` of an (N,3) float32 array adds the rows one after
    the other in float32 (numpy sums pairwise only along the contiguous axis), so its error over ~6000 rows is of the
    order of sqrt(N) roundings of the running sum and can exceed the bound; an item whose reference centroid does is
    dropped like one that fails the gap condition (the figure is printed), never the bound widened.
"""
import os
import sys
import tempfile
import warnings

import numpy as np

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
warnings.simplefilter("ignore")

import tempo_dataset as ref_ds  # noqa: E402

CASES, STEPS, SPACING, K = 2, 5, 0.025, 4096
CENTRE = np.array([1.0, 0.5, 2.0])
MIN_GAP = 1e-6
ITEMS = (0, 1, 2, 3, 4, 5)
NAMES = ("highres_pos_left", "highres_pos", "highres_pos_right", "highres_vel_left", "highres_vel", "highres_vel_right",
         "lowres_pos_left", "lowres_pos", "lowres_pos_right", "lowres_vel_left", "lowres_vel", "lowres_vel_right")


def make_case(rng, radius):
    ax = np.arange(-radius, radius + SPACING, SPACING)
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    g = g[(g ** 2).sum(1) <= radius ** 2]
    g = g + rng.uniform(-0.3, 0.3, g.shape) * SPACING
    pos0 = (g + CENTRE).astype(np.float32)
    w = rng.normal(0.0, 1.0, 3)
    vel = (np.cross(w, g) + 0.3 * np.sin(7.0 * g[:, [1, 2, 0]]) + rng.normal(0.0, 0.02, g.shape)).astype(np.float32)
    return pos0, vel


def frame(pos0, vel, s):
    return pos0 + np.float32(s * SPACING) * vel


def fps_numpy(pts, k, first):
    """Dataset-side FPS in fp32: squared distances (dx*dx + dy*dy) + dz*dz, arg-max ties to the smallest index."""
    idx = np.zeros(k, np.int64)
    idx[0] = first
    d = pts - pts[first]
    best = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    for i in range(1, k):
        idx[i] = int(np.argmax(best))
        d = pts - pts[idx[i]]
        best = np.minimum(best, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return idx


def restate(frames, vels, seed, patch_ref, fps_first):
    """The sampler's rule in numpy on one clip: (patch by the fp32 rule, outputs on the reference's patch order)."""
    centre = frames[1]
    d = centre - centre[seed]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    patch = np.lexsort((np.arange(len(d2)), d2))[:K]
    c = centre.astype(np.float64).mean(0).astype(np.float32)
    high = [f[patch_ref] - c for f in frames]
    fps = fps_numpy(high[1], K // 8, fps_first)
    hv = [v[patch_ref] for v in vels]
    # (the reference's low-resolution velocities index the whole scene with the patch-local FPS picks)
    return patch, fps, high + hv + [h[fps] for h in high] + [v[fps] for v in vels]


def main():
    rng = np.random.RandomState(2024)
    cases = [make_case(rng, r) for r in (0.285, 0.29)]
    out = {"spacing": np.float64(SPACING), "case_steps": np.int64(STEPS), "sample_num": np.int64(K)}
    recorded = {}
    plain = ref_ds.sample_patch_with_fps

    def recording(*a, **kw):
        ret = plain(*a, **kw)
        recorded["patch"], recorded["fps"] = np.asarray(ret[1]), np.asarray(ret[2])
        return ret

    ref_ds.sample_patch_with_fps = recording
    with tempfile.TemporaryDirectory() as tmp:
        for c, (pos0, vel) in enumerate(cases):
            print(f"case{c + 1}: {pos0.shape[0]} particles")
            out[f"case{c + 1}/pos0"], out[f"case{c + 1}/vel"] = pos0, vel
            os.makedirs(os.path.join(tmp, f"case{c + 1}"))
            for s in range(STEPS):
                np.savez(os.path.join(tmp, f"case{c + 1}", f"data_{s}.npz"), pos=frame(pos0, vel, s), vel=vel)
        ds = ref_ds.SiamData(tmp, CASES, STEPS, sample_num=K, jitter=0.0)
        out["len"] = np.int64(len(ds))
        keys = []
        for idx in range(len(ds)):
            case, step = idx // STEPS + 1, idx % (STEPS - 2)
            keys.append([f"case{case}/data_{step + t}.npz" for t in range(3)])
        out["keys"] = np.array(keys)
        kept = []
        for idx in ITEMS:
            np.random.seed(100 + idx)
            item = ds[idx]
            patch, fps = recorded["patch"], recorded["fps"]
            case, step = idx // STEPS, idx % (STEPS - 2)
            pos0, vel = cases[case]
            frames = [frame(pos0, vel, step + t) for t in range(3)]
            seed = int(patch[0])
            d = np.sort(np.sqrt(((frames[1].astype(np.float64) - frames[1][seed].astype(np.float64)) ** 2).sum(1)))
            assert d[0] == 0.0 and d[1] > 0.0, "the seed must be a unique point"
            gap = (d[K] - d[K - 1]) / d[K - 1]
            print(f"item {idx}: seed {seed}, relative gap {gap:.3e}")
            if gap < MIN_GAP:
                print("  dropped: K-th and (K+1)-th neighbour too close for an fp32 / float64 comparison")
                continue
            mine_patch, mine_fps, mine = restate(frames, [vel] * 3, seed, patch, int(fps[0]))
            assert np.array_equal(np.sort(mine_patch), np.sort(patch)), f"item {idx}: patch set differs"
            assert np.array_equal(mine_fps, fps), f"item {idx}: FPS picks differ"
            bound = 16 * 2.0 ** -24 * max(np.abs(f).max() for f in frames)
            worst = 0.0
            for name, a, b in zip(NAMES, mine, item[:12]):
                assert a.dtype == np.float32 and np.asarray(b).dtype == np.float32, name
                if "vel" in name:
                    assert np.array_equal(a, b), f"item {idx}: {name}"
                else:
                    worst = max(worst, float(np.abs(a - b).max()))
            print(f"  positions: largest difference {worst:.3e}, bound {bound:.3e}")
            if worst > bound:
                print("  dropped: the reference's own float32 centroid is further than the bound from the exact one")
                continue
            kept.append(idx)
            out[f"item{idx}/seed"] = np.int64(seed)
            out[f"item{idx}/patch_idx"] = patch.astype(np.int32)
            out[f"item{idx}/fps_idx"] = fps.astype(np.int32)
            out[f"item{idx}/gap"] = np.float64(gap)
            out[f"item{idx}/h"] = np.float32(item[12])
            # The 12 arrays are gathers of the frames by the two stored index lists, the positions minus the reference's
            # float32 centroid of the centre frame (normalize_point_cloud; jitter 0 adds exact zeros): store that
            # centroid instead of 12 arrays, after checking that it does rebuild every one of them exactly.
            m = ref_ds.normalize_point_cloud(frames[1].copy())[1].astype(np.float32).reshape(3)
            rebuilt = [f[patch] - m for f in frames]
            rebuilt = rebuilt + [vel[patch]] * 3 + [h[fps] for h in rebuilt] + [vel[fps]] * 3
            for name, a, b in zip(NAMES, rebuilt, item[:12]):
                assert np.array_equal(a, np.asarray(b)), f"item {idx}: {name} is not the gather it is stored as"
            out[f"item{idx}/centroid_ref"] = m
    ref_ds.sample_patch_with_fps = plain
    if len(kept) < 3:
        raise SystemExit(f"only {len(kept)} items pass the gap condition: pick other seeds")
    out["items"] = np.array(kept, np.int64)
    path = os.path.join(HERE, "dataset.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print(f"dataset: {os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays, items {kept}")


if __name__ == "__main__":
    main()
