"""Action clips from depth videos, on the host: the numpy statement of the subset rule with known answers that pin its
hash, ActionSequences' host logic, the sampler against the reference's own dataset class (tests/golden/
action_dataset.npz; capture_action_goldens.py) and under the prefetcher, and the argument checks of the two new entries.

The numpy statement of both rules lives here (`subset`, `gather`), and a test-local subclass of the oracle backend adds
them as `frame_subset` / `action_gather` for CPU tensors, so that the sampler's host code runs without a device; the
kernels themselves are compared with the same statements in tests/test_action_data_gpu.py.

The fixture stores the toy videos' frames (integer coordinates), and per item of the reference's train and test dataset
the recorded per-frame subsets, scales, FPS starts and picks and the item's outputs.
"""
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "action_dataset.npz")
STEP_GOLDEN = os.path.join(HERE, "golden", "step_action.npz")


# ---- the rules in numpy -----------------------------------------------------------------------------------------------
def mix(h):
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x7FEB352D)
    h = h ^ (h >> np.uint32(15))
    h = h * np.uint32(0x846CA68B)
    return h ^ (h >> np.uint32(16))


def keys(n, seed):
    """key(j) = mix(mix(j * 0x9E3779B1 + seed_lo) ^ seed_hi), uint32 arithmetic, wrapping."""
    seed = int(seed)
    lo, hi = np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32)
    with np.errstate(over="ignore"):
        return mix(mix(np.arange(n, dtype=np.uint32) * np.uint32(0x9E3779B1) + lo) ^ hi)


def subset(n, K, seed):
    """The K smallest by (key, j) if n > K, else 0..n-1 repeated K // n times and then the K % n smallest."""
    order = np.lexsort((np.arange(n), keys(n, seed)))
    if n > K:
        return order[:K].astype(np.int32)
    return np.concatenate([np.arange(n)] * (K // n) + [order[:K % n]]).astype(np.int32)


def gather(points, frame_first, count, idx, scale, per_frame):
    """fp64: q = point, y negated; v = (q * scale) / 300; minus the mean over the K rows of the middle frame (train) or
    of the frame itself (test); one rounding to fp32.  -> high (T,B,K,3) float64 BEFORE that rounding, centres (T,B,3)."""
    T, B, K = idx.shape
    v = np.empty((T, B, K, 3))
    for t in range(T):
        for b in range(B):
            rows = frame_first[t, b] + np.clip(idx[t, b], 0, count[t, b] - 1)
            q = points[rows].astype(np.float64)
            q[:, 1] = -q[:, 1]
            v[t, b] = (q * (np.ones(3) if scale is None else scale[b])) / 300.0
    c = v.mean(2) if per_frame else np.broadcast_to(v[T // 2].mean(1), (T, B, 3))
    return v - c[:, :, None, :], c


def within_one_ulp(got, want64):
    """|got - want| <= spacing(|want| rounded to fp32): a different fp64 summation order moves the centroid by ~1e-13,
    which after the single rounding to fp32 can flip the result by at most one ulp."""
    want = want64.astype(np.float32)
    return got.dtype == np.float32 and bool((np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))).all())


@pytest.fixture()
def numpy_backend():
    """The oracle backend for CPU tensors plus the two new ops as the numpy statements above."""
    import tpgan_amd.ops as ops
    from oracle.torch_backend import OracleBackend

    class Backend(OracleBackend):
        def frame_subset(self, count, seed, K, device):
            return torch.from_numpy(np.stack([subset(int(n), K, s) for n, s in zip(count, seed)]))

        def action_gather(self, points, frame_first, count, idx, scale, per_frame):
            high, c = gather(points.numpy(), frame_first, count, idx.numpy(), scale, per_frame)
            return (torch.from_numpy(high.astype(np.float32)),
                    torch.from_numpy(np.ascontiguousarray(c.astype(np.float32))) if per_frame else None)

    ops.register_backend("cpu", Backend())
    yield
    ops.unregister_backend("cpu")


# ---- fixtures on disk -------------------------------------------------------------------------------------------------
def save_video(root, name, frames):
    arr = np.empty(len(frames), dtype=object)
    for i, f in enumerate(frames):
        arr[i] = f
    np.savez(os.path.join(root, name), point_clouds=arr)


def write_golden_dataset(root, g=None):
    g = g if g is not None else np.load(GOLDEN)
    os.makedirs(root, exist_ok=True)
    for v, name in enumerate(g["names"].tolist()):
        ends = np.cumsum(g[f"video{v}/count"])
        save_video(root, name, np.split(g[f"video{v}/points"].astype(np.float64), ends[:-1]))
    return g


def write_random_dataset(root, sizes_per_video, seed=0):
    """Depth-like integer coordinates (x, y in a 240 x 320 image, z around 500), train subjects only."""
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    for v, sizes in enumerate(sizes_per_video):
        frames = [np.stack([rng.integers(0, 240, n), rng.integers(0, 320, n), rng.integers(400, 600, n)], 1)
                  .astype(np.float64) for n in sizes]
        save_video(root, f"a{v + 1:02d}_s{v % 5 + 1:02d}_e01_sdepth.npz", frames)


def _batches(sampler, n):
    return [sampler.sample() for _ in range(n)]


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


# ---- the rule's known answers -------------------------------------------------------------------------------------------
def _z_and_correlation(seeds, n=3000, K=2048):
    counts, corr = np.zeros(n), []
    for s in seeds:
        r = subset(n, K, s)
        counts[r] += 1
        corr.append(np.corrcoef(np.arange(K), r)[0, 1])
    p = K / n
    z = (counts - len(seeds) * p) / np.sqrt(len(seeds) * p * (1 - p))
    return float(np.abs(z).max()), float(np.mean(corr))


def test_subset_rule_known_answers():
    seeds = np.random.default_rng(0).integers(0, 2 ** 63, size=256, dtype=np.uint64)
    r = subset(700, 2048, seeds[1])
    assert r.shape == (2048,) and np.array_equal(r[:1400], np.tile(np.arange(700), 2))
    assert r[1398:1403].tolist() == [698, 699, 325, 168, 545]
    assert len(np.unique(keys(40000, seeds[0]))) == 40000
    assert np.array_equal(subset(2048, 2048, seeds[2]), np.arange(2048))
    assert len(np.unique(subset(3000, 2048, seeds[3]))) == 2048
    z, corr = _z_and_correlation(seeds)
    print(f"256 random seeds: largest inclusion z-score {z:.3f}, mean position/index correlation {corr:+.4f}")
    assert z == pytest.approx(3.657, abs=1e-3) and z < 5.5
    assert corr == pytest.approx(-0.0038, abs=1e-4) and abs(corr) < 0.01
    z, _ = _z_and_correlation(range(1, 257))
    print(f"seeds 1..256: largest inclusion z-score {z:.3f}")
    assert z == pytest.approx(3.594, abs=1e-3) and z < 5.5


# ---- host logic -----------------------------------------------------------------------------------------------------------
def test_sequences_follow_the_reference_s_index_map(tmp_path):
    from tpgan_amd.data import ActionSequences
    g = write_golden_dataset(str(tmp_path))
    open(os.path.join(str(tmp_path), "README.txt"), "w").write("not a video\n")
    names = g["names"].tolist()
    for split, train in (("train", True), ("test", False)):
        seq = ActionSequences(str(tmp_path), train=train, frames_per_clip=3, device="cpu")
        want = sorted(n for n in names if (int(n.split("_")[1][1:]) <= 5) == train)
        assert seq.names == want
        assert len(seq) == int(g[f"{split}/len"])
        assert [list(seq.clip(i)) for i in range(len(seq))] == g[f"{split}/index_map"].tolist()
        assert seq.labels == g[f"{split}/labels"].tolist() and seq.num_classes == int(g[f"{split}/num_classes"])
        assert seq.points.dtype == torch.float32 and seq.points.shape == (int(seq.count.sum()), 3)
        with pytest.raises(IndexError):
            seq.clip(len(seq))
        # frames back to back in (video, frame) order
        off = 0
        for name in want:
            v = names.index(name)
            pts = g[f"video{v}/points"].astype(np.float32)
            assert np.array_equal(seq.points[off:off + len(pts)].numpy(), pts)
            off += len(pts)
        assert np.array_equal(seq.first, np.concatenate([[0], np.cumsum(seq.count)[:-1]]))
    seq2 = ActionSequences(str(tmp_path), train=True, frames_per_clip=2, step_between_clips=2, device="cpu")
    assert [seq2.clip(i) for i in range(len(seq2))] == [(0, 0), (1, 0), (1, 2)]
    assert seq2.frame_rows(2).tolist() == [4 + 2, 4 + 4]


def test_file_names_split_and_sorted_order(tmp_path):
    from tpgan_amd.data import ActionSequences
    root = str(tmp_path)
    frame = np.arange(12, dtype=np.float64).reshape(4, 3)
    for name in ("a12_s05_e03_sdepth.npz", "a02_s01_e01_sdepth.npz", "a07_s06_e01_sdepth.npz", "a20_s10_e02_sdepth.npz"):
        save_video(root, name, [frame] * 3)
    train = ActionSequences(root, train=True, device="cpu")
    test = ActionSequences(root, train=False, device="cpu")
    assert train.names == ["a02_s01_e01_sdepth.npz", "a12_s05_e03_sdepth.npz"] and train.labels == [1, 11]
    assert test.names == ["a07_s06_e01_sdepth.npz", "a20_s10_e02_sdepth.npz"] and test.labels == [6, 19]
    assert train.num_classes == 12 and test.num_classes == 20 and len(train) == 2 and len(test) == 2
    assert len(ActionSequences(root, train=True, frames_per_clip=4, device="cpu")) == 0       # videos too short: no clip


def test_an_empty_frame_is_an_error(tmp_path):
    from tpgan_amd.data import ActionSequences
    frame = np.arange(12, dtype=np.float64).reshape(4, 3)
    save_video(str(tmp_path), "a01_s01_e01_sdepth.npz", [frame, np.zeros((0, 3)), frame])
    with pytest.raises(ValueError, match=r"a01_s01_e01_sdepth\.npz: frame 1 is empty"):
        ActionSequences(str(tmp_path), device="cpu")
    with pytest.raises(ValueError, match="no test video"):
        ActionSequences(str(tmp_path), train=False, device="cpu")


# ---- the golden ---------------------------------------------------------------------------------------------------------
def check_golden_items(device, root):
    """With the reference's recorded subsets / scales / FPS starts fed in, the sampler reproduces the reference's items:
    high and centres within one fp32 ulp, the FPS picks equal, low the exact gather of high, label and index equal."""
    from tpgan_amd.data import ActionClipSampler, ActionSequences
    g = write_golden_dataset(root)
    K, T = int(g["num_points"]), int(g["frames_per_clip"])
    for split, train in (("train", True), ("test", False)):
        seq = ActionSequences(root, train=train, frames_per_clip=T, device=device)
        sampler = ActionClipSampler(seq, 1, K)
        assert len(seq) >= 3
        for idx in range(len(seq)):
            key = f"{split}/item{idx}"
            out = sampler.sample(indices=[idx], subset_idx=torch.from_numpy(g[f"{key}/subsets"]).to(device).view(T, 1, K),
                                 scales=g[f"{key}/scales"].reshape(1, 3) if train else None,
                                 initial_idx=g[f"{key}/starts"].reshape(T, 1))
            assert len(out) == (2 * T + 1 if train else 3 * T + 2)
            fps = sampler.last["fps_idx"][:, 0].cpu().numpy()
            assert np.array_equal(fps, g[f"{key}/fps_idx"]), f"{key}: FPS picks"
            for t in range(T):
                high, low = out[t][0].cpu().numpy(), out[T + t][0].cpu().numpy()
                want = g[f"{key}/high"][t]
                err = float(np.abs(high - want).max())
                print(f"{key} frame {t}: max |difference| of high {err:.3e}")
                assert within_one_ulp(high, want.astype(np.float64)), f"{key}: high, frame {t}"
                assert np.array_equal(low, high[fps[t]]), f"{key}: low is not the gather of high"
                assert within_one_ulp(low, g[f"{key}/low"][t].astype(np.float64))
                if not train:
                    assert within_one_ulp(out[2 * T + t][0].cpu().numpy(), g[f"{key}/centres"][t]), f"{key}: centre {t}"
            label = out[2 * T] if train else out[3 * T]
            assert label.dtype == torch.int64 and not label.is_cuda and label.tolist() == [int(g[f"{key}/label"])]
            if not train:
                assert out[3 * T + 1].tolist() == [int(g[f"{key}/index"])] and out[3 * T + 1].dtype == torch.int64


def test_sampler_reproduces_the_reference_items(numpy_backend, tmp_path):
    check_golden_items(torch.device("cpu"), str(tmp_path))


def test_same_seed_same_batches_and_prefetch_equals_plain(numpy_backend, tmp_path):
    from tpgan_amd.data import ActionClipSampler, ActionSequences, prefetch
    write_golden_dataset(str(tmp_path))
    for train in (True, False):
        seq = ActionSequences(str(tmp_path), train=train, device="cpu")

        def make(seed):
            return ActionClipSampler(seq, 3, 64, generator=torch.Generator().manual_seed(seed))
        a, b, c = _batches(make(5), 3), _batches(make(5), 3), _batches(make(6), 3)
        assert all(_equal(x, y) for x, y in zip(a, b)) and not any(_equal(x, y) for x, y in zip(a, c))
        out = a[0]
        assert len(out) == (7 if train else 11)
        for j in range(6):
            assert out[j].shape == (3, 64 if j < 3 else 4, 3) and out[j].dtype == torch.float32
        it = prefetch(make(5))
        states = []
        for want in a:
            states.append(it.resume_state)
            assert _equal(next(it), want)
        again = make(1)
        again.generator.set_state(states[2])                                    # what a checkpoint after batch 2 holds
        assert _equal(again.sample(), a[2])
        # the draws: the subset is the rule on the drawn seeds' frames, low the gather by the FPS picks
        s = make(9)
        out = s.sample()
        sub, fps = s.last["subset_idx"].numpy(), s.last["fps_idx"].long()
        for t in range(3):
            assert torch.equal(out[3 + t], torch.gather(out[t], 1, fps[t].unsqueeze(-1).expand(-1, -1, 3)))
            for b, i in enumerate(s.last["indices"]):
                n = int(seq.count[seq.frame_rows(i)[t]])
                assert sub[t, b].min() >= 0 and sub[t, b].max() < n
                if n <= 64:
                    assert np.array_equal(sub[t, b][:n], np.arange(n))
                else:
                    assert len(np.unique(sub[t, b])) == 64


# ---- argument checks ------------------------------------------------------------------------------------------------------
def test_ops_validate_their_arguments(numpy_backend):
    import tpgan_amd.ops as ops
    idx = ops.frame_subset([700, 3000], [1, 2 ** 64 - 1], 2048, device="cpu")
    assert idx.dtype == torch.int32 and idx.shape == (2, 2048)
    assert np.array_equal(idx[1].numpy(), subset(3000, 2048, 2 ** 64 - 1))
    with pytest.raises(RuntimeError, match="at least one point"):
        ops.frame_subset([700, 0], [1, 2], 2048, device="cpu")
    with pytest.raises(RuntimeError, match="K must be positive"):
        ops.frame_subset([700], [1], 0, device="cpu")
    with pytest.raises(RuntimeError, match=r"\[0, 2\^64\)"):
        ops.frame_subset([700], [-1], 16, device="cpu")
    with pytest.raises(RuntimeError, match="seeds must have shape"):
        ops.frame_subset([700], [1, 2], 16, device="cpu")
    with pytest.raises(RuntimeError, match=r"\[0, 2\^64\)"):
        ops.frame_subset([700], [1.5], 16, device="cpu")
    assert ops.frame_subset(torch.tensor([700]), np.array([7], np.uint64), 16, device="cpu").shape == (1, 16)
    pts = torch.arange(300, dtype=torch.float32).view(100, 3)
    first, count = np.array([[0], [40]]), np.array([[40], [60]])
    sub = torch.zeros(2, 1, 16, dtype=torch.int32)
    high, c = ops.action_gather(pts, first, count, sub, None, "test")
    assert high.shape == (2, 1, 16, 3) and c.shape == (2, 1, 3) and float(high.abs().max()) < 1e-12   # one point, 16 times
    assert ops.action_gather(pts, first, count, sub, np.ones((1, 3)), "train")[1] is None
    with pytest.raises(RuntimeError, match="non-empty slice"):
        ops.action_gather(pts, first, np.array([[40], [61]]), sub)
    with pytest.raises(RuntimeError, match="no scale"):
        ops.action_gather(pts, first, count, sub, np.ones((1, 3)), "test")
    with pytest.raises(RuntimeError, match="scale must be"):
        ops.action_gather(pts, first, count, sub, np.array([[1.0, np.inf, 1.0]]))
    with pytest.raises(RuntimeError, match="int tensor"):
        ops.action_gather(pts, first, count, sub.long())
    with pytest.raises(RuntimeError, match="mode"):
        ops.action_gather(pts, first, count, sub, None, "eval")


def test_new_entries_reject_bad_arguments_before_any_launch(hip_lib):
    """The C-ABI's own checks (no GPU here): conditions on the host tables are TPG_ERR_ARG with nothing launched, K above
    the LDS sort's capacity TPG_ERR_UNSUPPORTED, empty work TPG_OK."""
    import ctypes as C
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)

    def ints(*v):
        return C.cast((C.c_int32 * len(v))(*v), C.c_void_p)

    def seeds(*v):
        return C.cast((C.c_uint64 * len(v))(*v), C.c_void_p)

    def select(count=(700, 3000), K=2048, F=2, idx=p):
        return hip_lib.tpg_frame_subset(ints(*count), seeds(*range(len(count))), F, K, idx, None)
    assert select(count=(700, 0)) == -1 and select(count=(-5, 10)) == -1 and select(K=0) == -1 and select(K=-1) == -1
    assert select(idx=None) == -1 and select(F=-1) == -1
    assert select(K=hip_lib.tpg_patch_select_max_k() + 1) == -3
    assert select(F=0) == 0

    def gather(first=(0, 100, 200), count=(100, 100, 100), scale=None, mode=0, T=3, P=300, high=p, centre=None):
        sc = None if scale is None else C.cast((C.c_double * 3)(*scale), C.c_void_p)
        return hip_lib.tpg_action_gather_f32(p, P, ints(*first), ints(*count), p, sc, mode, T, 1, 16, high, centre, None)
    assert gather(first=(0, 100, 201)) == -1 and gather(first=(-1, 100, 200)) == -1 and gather(count=(100, 0, 100)) == -1
    assert gather(mode=2) == -1 and gather(high=None) == -1 and gather(scale=(1.0, float("nan"), 1.0)) == -1
    assert gather(mode=1) == -1                          # the test split returns its centres
    assert gather(mode=1, centre=p, scale=(1.0, 1.0, 1.0)) == -1 and gather(mode=0, centre=p) == -1
    assert gather(T=9, first=(0,) * 9, count=(100,) * 9) == -3 and gather(T=0) == 0


# ---- the trainer (run on the GPU by tests/test_action_data_gpu.py) ------------------------------------------------------
def _params(ckpt):
    return [ckpt[k][n] for k in ("sr_net", "tempo_dis", "spatial_dis") for n in sorted(ckpt[k])]


def check_trainer(tmp_path, device, iters, resume_at, num_points):
    """Train `iters` iterations with a checkpoint after every one; resume from iteration `resume_at` in a second log
    directory and run to `iters`: the eleven keys, weights_only loading, and parameters and Adam moments equal bit for
    bit."""
    from tpgan_amd import train, train_action
    data = os.path.join(str(tmp_path), "data")
    write_random_dataset(data, [(1500, 2048, 2600, 900), (3000, 2049, 700, 2500, 1800)])
    common = ["--data_dir", data, "--batch_size", "2", "--num_points", str(num_points), "--amp", "none", "--device", device,
              "--ckpt_every", "1", "--log_every", "1", "--iters", str(iters), "--seed", "1", "--dump_visualization"]
    a, b = os.path.join(str(tmp_path), "a"), os.path.join(str(tmp_path), "b")
    assert train_action.main(common + ["--log_dir", a]) == 0
    ck = os.path.join(a, "model_ckpt")
    assert open(os.path.join(ck, "latest_checkpoint.txt")).readline().strip() == f"tpugan_checkpoint{iters}.ckpt"
    full = torch.load(os.path.join(ck, f"tpugan_checkpoint{iters}.ckpt"), map_location="cpu", weights_only=True)
    assert set(full) == set(train.CKPT_KEYS) and len(train.CKPT_KEYS) == 11 and full["n_iter"] == iters
    first = torch.load(os.path.join(ck, "tpugan_checkpoint1.ckpt"), map_location="cpu", weights_only=True)
    assert any(not torch.equal(x, y) for x, y in zip(_params(first), _params(full))), "parameters did not move"
    assert train_action.main(common + ["--log_dir", b, "--resume", "--path_to_resume",
                                       os.path.join(ck, f"tpugan_checkpoint{resume_at}.ckpt")]) == 0
    again = torch.load(os.path.join(b, "model_ckpt", f"tpugan_checkpoint{iters}.ckpt"), map_location="cpu",
                       weights_only=True)
    for x, y in zip(_params(full), _params(again)):
        assert torch.equal(x, y)
    for k in ("sr_optim", "tempo_optim", "spatial_optim"):
        assert full[k]["state"].keys() == again[k]["state"].keys()
        for i, st in full[k]["state"].items():
            for name, v in st.items():
                assert torch.equal(torch.as_tensor(v), torch.as_tensor(again[k]["state"][i][name])), (k, i, name)
    return full


def test_trainer_flags_are_the_reference_s_plus_ours():
    from tpgan_amd import train_action
    opt = train_action.parse_args([])
    assert (opt.lr, opt.iters, opt.ckpt_every, opt.batch_size, opt.in_node_feats, opt.node_embedding) == \
        (3e-4, 80000, 5000, 4, 3, 128)
    assert (opt.R, opt.w, opt.freeze_D, opt.resume, opt.path_to_resume, opt.log_dir) == (2.0, 2.0, False, False, "", "./")
    assert (opt.seed, opt.amp, opt.device, opt.log_every, opt.num_points) == (1, "bf16", "cuda", 100, 2048)
    assert train_action.parse_args(["--dump_visualization", "--data_dir", "x"]).data_dir == "x"
    assert int(np.load(STEP_GOLDEN)["high"].shape[2]) <= 2048
