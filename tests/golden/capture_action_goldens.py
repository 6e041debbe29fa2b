"""Generates tests/golden/action_dataset.npz by running the REFERENCE's own action dataset class in the build container.

    TPGAN_REFERENCE=<checkout of the reference> python tests/golden/capture_action_goldens.py

Same recipe as capture_dataset_goldens.py: the reference checkout (read-only, imported unmodified; never copied, never
shipped) on `sys.path` in this container only, the inert import shims of tests/golden/_import_shims (with the `numba`
shim the reference's FPS loop runs as plain Python).  Never run by a test.

What runs: train_action/msr_dataset.py `MSRAction3D(root, frames_per_clip=3, num_points=256, train=...)` in train and in
test mode (the latter with return_idx=True) on a toy dataset in the MSR layout written to a temporary directory: four
videos (two train subjects, two test subjects) of 4 or 5 frames of 100, 256 or 300 points -- fewer than, exactly and more
than num_points -- with UNIQUE INTEGER coordinates in [0, 400), stored as float64 (the reference divides the frames in
place, so they must be floating point; integer values make the fp32 copy the loader keeps exact).  `os.listdir` is
wrapped to list the directory in sorted order while the dataset is built: that is the order data.ActionSequences
documents, and it makes the video indices here independent of the file system.

What is recorded per item, by wrapping np.random.choice / np.random.uniform / np.random.randint and the module's
`farthest_point_sampling` name (the files are untouched): the per-frame subsets as the reference builds them (the
`np.arange` repeats followed by the drawn residue), the scales (train), the FPS' first picks and the FPS picks; and the
item's own outputs: high (T,K,3) and low (T,K/16,3) float32, the float64 centres (test), label and video index.

Conditions (checked here, not in the tests): every item must reproduce under this file's own numpy statement of the
sampler (`restate`) -- with the centroid summed in numpy's order EXACTLY (same operations, same order), and with the
centroid summed in the device kernel's order (256 strided partial sums folded by a halving tree) within one fp32 ulp,
with the same FPS picks.
"""
import os
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("TPGAN_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
if not REFERENCE:
    raise SystemExit("set TPGAN_REFERENCE (or pass the path) to a checkout of the reference")

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, "_import_shims"))
sys.path.insert(1, REFERENCE)
sys.path.insert(2, os.path.join(REFERENCE, "train_action"))
warnings.simplefilter("ignore")

import msr_dataset as ref_ds  # noqa: E402

K, T = 256, 3
VIDEOS = (("a01_s01_e01_sdepth.npz", (300, 100, 256, 300)),
          ("a03_s05_e02_sdepth.npz", (256, 300, 300, 100, 100)),
          ("a02_s06_e01_sdepth.npz", (100, 300, 256, 100)),
          ("a03_s10_e01_sdepth.npz", (300, 300, 100, 256, 300)))


def make_frame(rng, n):
    cells = rng.choice(400 ** 3, size=n, replace=False)
    return np.stack(np.unravel_index(cells, (400, 400, 400)), 1).astype(np.float64)


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


def tree_mean(v):
    """The device kernel's summation order: thread t adds rows t, t + 256, ...; the 256 partial sums fold by halves."""
    part = np.zeros((256, 3))
    for t in range(256):
        for row in v[t::256]:
            part[t] = part[t] + row
    d = 128
    while d > 0:
        part[:d] = part[:d] + part[d:2 * d]
        d //= 2
    return part[0] / v.shape[0]


def restate(frames, subsets, scales, starts, train, mean):
    """The sampler's rule in numpy on one clip.  frames: T float32 (n,3) arrays as the loader stores them."""
    v = []
    for f, r in zip(frames, subsets):
        q = f[r].astype(np.float64)
        q[:, 1] = -q[:, 1]
        v.append((q * (scales if train else np.ones(3))) / 300.0)
    cs = [mean(v[T // 2])] * T if train else [mean(x) for x in v]
    high = [(x - c).astype(np.float32) for x, c in zip(v, cs)]
    fps = [fps_numpy(h, K // 16, s) for h, s in zip(high, starts)]
    return high, fps, [h[i] for h, i in zip(high, fps)], cs


def main():
    rng = np.random.RandomState(2025)
    out = {"num_points": np.int64(K), "frames_per_clip": np.int64(T), "names": np.array([n for n, _ in VIDEOS])}
    videos = {}
    rec = {"choice": [], "uniform": [], "randint": [], "fps": []}
    plain = (np.random.choice, np.random.uniform, np.random.randint, ref_ds.farthest_point_sampling, os.listdir)

    def wrap(name, fn):
        def recording(*a, **kw):
            ret = fn(*a, **kw)
            rec[name].append(np.asarray(ret[0] if name == "fps" else ret).copy())
            return ret
        return recording

    with tempfile.TemporaryDirectory() as tmp:
        for v, (name, sizes) in enumerate(VIDEOS):
            frames = [make_frame(rng, n) for n in sizes]
            videos[name] = frames
            out[f"video{v}/count"] = np.array(sizes, np.int64)
            out[f"video{v}/points"] = np.concatenate(frames).astype(np.int16)
            assert np.array_equal(out[f"video{v}/points"].astype(np.float64), np.concatenate(frames))
            arr = np.empty(len(frames), dtype=object)
            for i, f in enumerate(frames):
                arr[i] = f
            np.savez(os.path.join(tmp, name), point_clouds=arr)
        os.listdir = lambda p: sorted(plain[4](p))
        sets = {"train": ref_ds.MSRAction3D(tmp, frames_per_clip=T, num_points=K, train=True),
                "test": ref_ds.MSRAction3D(tmp, frames_per_clip=T, num_points=K, train=False, return_idx=True)}
        os.listdir = plain[4]
    np.random.choice, np.random.uniform, np.random.randint = (wrap(n, f) for n, f in zip(("choice", "uniform", "randint"), plain))
    ref_ds.farthest_point_sampling = wrap("fps", plain[3])
    worst = 0.0
    for split, ds in sets.items():
        train = split == "train"
        names = [n for n, _ in VIDEOS if (int(n.split("_")[1][1:]) <= 5) == train]
        out[f"{split}/len"] = np.int64(len(ds))
        out[f"{split}/index_map"] = np.array(ds.index_map, np.int64)
        out[f"{split}/labels"] = np.array(ds.labels, np.int64)
        out[f"{split}/num_classes"] = np.int64(ds.num_classes)
        for idx in range(len(ds)):
            for lst in rec.values():
                lst.clear()
            np.random.seed(300 + idx + (0 if train else 50))
            item = ds[idx]
            video, t = ds.index_map[idx]
            frames = [videos[names[video]][t + i].astype(np.float32) for i in range(T)]
            subsets = []
            for f, r in zip(frames, rec["choice"]):         # rebuild r as the reference concatenates it
                n = f.shape[0]
                subsets.append(r if n > K else np.concatenate([np.arange(n)] * (K // n) + [r]))
                assert len(subsets[-1]) == K
            scales = rec["uniform"][0] if train else None
            starts = [int(s) for s in rec["randint"]]
            fps_ref = [np.asarray(f) for f in rec["fps"]]
            assert len(subsets) == T and len(starts) == T and len(fps_ref) == T and len(rec["uniform"]) == int(train)
            ref_high, ref_low = [np.asarray(a) for a in item[0]], [np.asarray(a) for a in item[1]]
            high, fps, low, cs = restate(frames, subsets, scales, starts, train, lambda v: np.mean(v, axis=0))
            for a, b, c, d, e, f in zip(high, ref_high, low, ref_low, fps, fps_ref):
                assert a.dtype == b.dtype == np.float32 and np.array_equal(a, b) and np.array_equal(c, d)
                assert np.array_equal(e, f)
            if not train:
                for c, d in zip(cs, item[2]):
                    assert np.array_equal(c, np.asarray(d))
            high2, fps2, low2, cs2 = restate(frames, subsets, scales, starts, train, tree_mean)
            for a, b, e, f in zip(high2, ref_high, fps2, fps_ref):
                assert (np.abs(a - b) <= np.spacing(np.abs(b))).all(), f"{split} item {idx}: more than one ulp"
                assert np.array_equal(e, f), f"{split} item {idx}: FPS picks differ under the device's summation order"
                worst = max(worst, float(np.abs(a.astype(np.float64) - b).max()))
            key = f"{split}/item{idx}"
            out[f"{key}/subsets"] = np.stack(subsets).astype(np.int32)
            if train:
                out[f"{key}/scales"] = np.asarray(scales, np.float64)
            out[f"{key}/starts"] = np.array(starts, np.int64)
            out[f"{key}/fps_idx"] = np.stack(fps_ref).astype(np.int32)
            out[f"{key}/high"] = np.stack(ref_high)
            out[f"{key}/low"] = np.stack(ref_low)
            out[f"{key}/label"] = np.int64(item[-2] if not train else item[2])
            if not train:
                out[f"{key}/centres"] = np.stack([np.asarray(c, np.float64) for c in item[2]])
                out[f"{key}/index"] = np.int64(item[4])
            print(f"{key}: video {video} t {t}, counts {[f.shape[0] for f in frames]}, label {int(out[f'{key}/label'])}")
    np.random.choice, np.random.uniform, np.random.randint, ref_ds.farthest_point_sampling = plain[:4]
    print(f"largest |difference| between the two summation orders' outputs and the reference: {worst:.3e}")
    path = os.path.join(HERE, "action_dataset.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print(f"action_dataset: {os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
