"""The action-clip sampler on the GPU: tpg_frame_subset and tpg_action_gather_f32 against the numpy statements of their
rules (tests/test_action_data_cpu.py), the sampler with the side-stream prefetcher, the reference's dataset golden on
the HIP path, and the trainer end to end with a bit-exact resume."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_action_data_cpu import (STEP_GOLDEN, _equal, check_golden_items, check_trainer, gather, keys,  # noqa: E402
                                  subset, within_one_ulp, write_random_dataset)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def seeds_for(n):
    return np.random.default_rng(n).integers(0, 2 ** 64, size=n, dtype=np.uint64)


# n = 1023 .. 1025: one candidate per thread of the selecting workgroup, and one more; n = K: the identity; n = K + 1:
# the smallest real selection; 40 000: a large depth frame; K = 64 and 4096: other sizes of the LDS sort
@pytest.mark.parametrize("n,K", [(1, 2048), (700, 2048), (1023, 2048), (1024, 2048), (1025, 2048), (2048, 2048),
                                 (2049, 2048), (3000, 2048), (40000, 2048), (65, 64), (5000, 4096)])
def test_frame_subset_equals_the_rule(dev, n, K):
    import tpgan_amd.ops as ops
    seed = seeds_for(3)[n % 3]
    got = ops.frame_subset([n], [seed], K, device=dev).cpu().numpy()
    assert got.shape == (1, K) and got.dtype == np.int32
    assert np.array_equal(got[0], subset(n, K, seed))
    if n == K:
        assert np.array_equal(got[0], np.arange(K))


def test_frame_subset_of_all_but_one_point(dev):
    """n = K + 1 (65 and 64): every key but the largest survives, so in each pass the rank asked of the histogram is the
    last or the last but one of its entries and the bin found is the last or the last but one that is occupied."""
    import tpgan_amd.ops as ops
    n, K = 65, 64
    seeds = seeds_for(5)
    got = ops.frame_subset([n] * len(seeds), seeds, K, device=dev).cpu().numpy()
    for f, seed in enumerate(seeds):
        assert np.array_equal(got[f], subset(n, K, seed)), f
        assert np.array_equal(np.setdiff1d(np.arange(n), got[f]), [np.argmax(keys(n, seed))]), f


def test_frame_subset_ragged_batch_equals_single_calls_and_repeats(dev):
    import tpgan_amd.ops as ops
    rng = np.random.default_rng(33)
    count = rng.integers(1, 9000, size=33)                                       # 33 frames: two launch groups
    count[[0, 5, 32]] = (2048, 1, 4096)
    seeds = seeds_for(33)
    got = ops.frame_subset(count, seeds, 2048, device=dev).cpu().numpy()
    for f in range(33):
        assert np.array_equal(got[f], subset(int(count[f]), 2048, seeds[f])), f
    for f in (0, 7, 31, 32):
        assert np.array_equal(got[f], ops.frame_subset(count[f:f + 1], seeds[f:f + 1], 2048, device=dev).cpu().numpy()[0])
    assert np.array_equal(got, ops.frame_subset(count, seeds, 2048, device=dev).cpu().numpy())   # two runs, the same bits


def test_frame_subset_error_statuses_write_nothing(dev):
    import tpgan_amd.ops as ops
    hip = ops.backend_for(torch.zeros(1, device=dev))
    idx = ops.frame_subset([3000, 700], [1, 2], 2048, device=dev)
    keep = idx.clone()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(count, K):
        count = np.array(count, np.int32)
        seed = np.array([5, 6], np.uint64)
        return hip.lib.tpg_frame_subset(count.ctypes.data, seed.ctypes.data, 2, K, C.c_void_p(idx.data_ptr()), stream)
    assert call([3000, 0], 2048) == -1 and call([-1, 700], 2048) == -1 and call([3000, 700], 0) == -1
    assert call([30000, 700], hip.lib.tpg_patch_select_max_k() + 1) == -3
    torch.cuda.synchronize()
    assert torch.equal(idx, keep)
    with pytest.raises(RuntimeError, match="ARG"):
        hip.frame_subset(np.array([0], np.int32), np.array([1], np.uint64), 16, dev)
    with pytest.raises(RuntimeError, match="UNSUPPORTED"):
        hip.frame_subset(np.array([9], np.int32), np.array([1], np.uint64), 16385, dev)


def _clips(rng, T, B, K, lo, hi):
    """Ragged frames of unique-ish integer coordinates up to 400, back to back, with the subsets of the rule."""
    count = rng.integers(lo, hi, size=(T, B))
    first = np.concatenate([[0], np.cumsum(count.reshape(-1))[:-1]]).reshape(T, B) + 7      # (7 unused rows in front)
    P = int(count.sum()) + 11
    points = rng.integers(0, 401, size=(P, 3)).astype(np.float32)
    idx = np.stack([subset(int(n), K, s) for n, s in zip(count.reshape(-1), seeds_for(T * B))]).reshape(T, B, K)
    return points, first, count, idx.astype(np.int32)


@pytest.mark.parametrize("T,B,K,lo,hi", [(3, 5, 2048, 500, 6000), (2, 33, 64, 20, 200)])
def test_action_gather_both_modes(dev, T, B, K, lo, hi):
    """fp64 numpy statement rounded to fp32, one-ulp bound (a different fp64 summation order moves the centroid by about
    1e-13; after the single rounding that flips a result by at most one fp32 ulp); two runs give equal bits."""
    import tpgan_amd.ops as ops
    rng = np.random.default_rng(T * B)
    points, first, count, idx = _clips(rng, T, B, K, lo, hi)
    idx[0, 0, 3] = 2 ** 30                                                       # clamped into the frame
    pts, sub = torch.from_numpy(points).to(dev), torch.from_numpy(idx).to(dev)
    scale = rng.uniform(0.9, 1.1, size=(B, 3))
    for mode, sc in (("train", scale), ("train", None), ("test", None)):
        high, centre = ops.action_gather(pts, first, count, sub, sc, mode)
        want, c = gather(points, first, count, idx, sc, mode == "test")
        assert high.shape == (T, B, K, 3) and high.is_contiguous() and high.dtype == torch.float32
        got = high.cpu().numpy()
        ulps = np.abs(got.astype(np.float64) - want.astype(np.float32)) / np.spacing(np.abs(want.astype(np.float32)))
        print(f"{mode}, scale {sc is not None}: largest difference {ulps.max():.2f} ulp, {int((ulps > 0).sum())} of {ulps.size} differ")
        assert within_one_ulp(got, want), mode
        assert np.abs(want).max() > 0.3                                          # (the clouds are ~1 wide: not vacuous)
        if mode == "test":
            assert centre.shape == (T, B, 3) and within_one_ulp(centre.cpu().numpy(), c)
        else:
            assert centre is None
        again, centre2 = ops.action_gather(pts, first, count, sub, sc, mode)
        assert torch.equal(again, high) and (centre is None or torch.equal(centre2, centre))


@pytest.fixture(scope="module")
def videos(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("action_videos"))
    write_random_dataset(root, [(1500, 2048, 2600, 900, 3100), (3000, 2049, 700, 2500), (5000, 4000, 10000)], seed=4)
    return root


def test_sampler_and_prefetch_on_the_gpu(dev, videos):
    from tpgan_amd.data import ActionClipSampler, ActionSequences, prefetch
    seq = ActionSequences(videos, train=True, device=dev)
    T, B, K, M = 3, 4, 2048, 128

    def make():
        return ActionClipSampler(seq, B, K, generator=torch.Generator().manual_seed(21))
    s = make()
    plain = [s.sample() for _ in range(6)]
    out = plain[0]
    assert len(out) == 2 * T + 1 and out[6].shape == (B,) and out[6].dtype == torch.int64 and not out[6].is_cuda
    for j, t in enumerate(out[:6]):
        assert t.shape == (B, K if j < T else M, 3) and t.dtype == torch.float32 and t.device == dev and t.is_contiguous()
    s2 = make()
    out2 = s2.sample()
    assert _equal(out2, out)                                                     # same seed, same bits
    fps, sub, scales = s2.last["fps_idx"].long(), s2.last["subset_idx"].cpu().numpy(), s2.last["scales"]
    assert fps.shape == (T, B, M) and sub.shape == (T, B, K) and scales.shape == (B, 3)
    assert ((scales >= 0.9) & (scales < 1.1)).all() and scales.dtype == np.float64
    points = seq.points.cpu().numpy()
    rows = np.stack([seq.frame_rows(i) for i in s2.last["indices"]], 1)
    want, _ = gather(points, seq.first[rows], seq.count[rows], sub, scales, False)
    for t in range(T):
        assert torch.equal(out2[T + t], torch.gather(out2[t], 1, fps[t].unsqueeze(-1).expand(-1, -1, 3)))
        assert within_one_ulp(out2[t].cpu().numpy(), want[t])                    # rows of the clip's own frame, transformed
        for b in range(B):
            n = int(seq.count[rows[t, b]])
            assert sub[t, b].min() >= 0 and sub[t, b].max() < n
            assert len(np.unique(sub[t, b])) == min(n, K)
        assert out2[6].tolist() == [seq.labels[seq.clip(i)[0]] for i in s2.last["indices"]]
    # the prefetcher on its side stream while the main stream is kept busy
    a = torch.randn(4096, 4096, device=dev)
    it = prefetch(make())
    got = []
    for _ in range(6):
        for _ in range(4):
            a = (a @ a).clamp_(-1, 1)
        batch = next(it)
        got.append([t.clone() for t in batch])             # consumed on the main stream, after the hand-off
    torch.cuda.synchronize()
    for x, y in zip(got, plain):
        assert _equal(x, y)


def test_golden_items_on_the_hip_path(dev, tmp_path):
    check_golden_items(dev, str(tmp_path))


def test_trainer_end_to_end_with_bit_exact_resume(dev, tmp_path, capsys):
    """12 iterations at the step_action golden's cloud size (the smallest the three action networks are known to run at),
    batch 2, bf16 off, checkpoint round trip, and a run resumed from iteration 7 equal to the uninterrupted one bit for
    bit on parameters and Adam moments."""
    num_points = int(np.load(STEP_GOLDEN)["high"].shape[2])
    assert num_points <= 2048
    check_trainer(tmp_path, "cuda", 12, 7, num_points)
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["n_iter"] for l in lines][:12] == list(range(1, 13))
    assert all(np.isfinite(v) for l in lines for v in l.values())
