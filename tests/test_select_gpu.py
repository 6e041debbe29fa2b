"""The two samplers' kernels at their launch-group, digit and capacity edges (the cases of tests/select_cases.py, whose
properties tests/test_select_cpu.py asserts): tpg_patch_select_f32 and tpg_frame_subset against the numpy rules of
tests/select_rule.py, the two clip gathers against their torch compositions with more than 32 clips per call and with
indices the header says are clamped, and both samplers end to end with more than 32 clips.  Every comparison is exact."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import select_cases as cases  # noqa: E402
from select_rule import patch_rule, subset  # noqa: E402
from test_action_data_cpu import _equal, write_random_dataset  # noqa: E402
from test_data_cpu import write_dataset  # noqa: E402

pytestmark = pytest.mark.gpu
PATCH_CASES = cases.patch_cases()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def select(dev, scenes, seeds, K):
    import tpgan_amd.ops as ops
    count = [len(s) for s in scenes]
    first = np.concatenate([[0], np.cumsum(count)[:-1]])
    pts = torch.from_numpy(np.concatenate(scenes)).to(dev)
    return ops.patch_select(pts, first, count, seeds, K).cpu().numpy()


# ---- patch select -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PATCH_CASES))
def test_patch_select_equals_the_rule(dev, name):
    scenes, seeds, K = PATCH_CASES[name]
    got = select(dev, scenes, seeds, K)
    assert got.shape == (len(scenes), K) and got.dtype == np.int32
    for b, (pts, seed) in enumerate(zip(scenes, seeds)):
        assert np.array_equal(got[b], patch_rule(pts, seed, K)), (name, b)
        if K == len(pts):
            assert np.array_equal(np.sort(got[b]), np.arange(K)), (name, b)                # K = N: a permutation
    if name == "all_identical":
        assert np.array_equal(got[0], np.arange(K))


@pytest.mark.parametrize("name", list(cases.GROUPS))
def test_patch_select_groups_equal_single_calls_and_repeat(dev, name):
    """Scenes on both sides of every launch-group boundary give what they give alone, and two runs the same bits."""
    scenes, seeds, K = PATCH_CASES[name]
    got = select(dev, scenes, seeds, K)
    for b in sorted({0, 31, 32, 33, len(scenes) - 1} & set(range(len(scenes)))):
        assert np.array_equal(got[b], select(dev, [scenes[b]], [seeds[b]], K)[0]), b
    assert np.array_equal(got, select(dev, scenes, seeds, K))


# ---- clip gathers -------------------------------------------------------------------------------------------------------
def clamped(idx, n):
    """The library's clamp of an index into [0, n): anything outside becomes n - 1 (csrc/tpg_common.hpp,
    tpg_clamp_idx; negative indices included)."""
    return torch.where((idx >= 0) & (idx < n), idx, n - 1)


def clip_tables(rng, T, B):
    """Per clip a scene of its own size (300 .. 900 points, all different), T frames of it anywhere in the store (every
    (t,b) another first row, in shuffled order) and a centroid row of its own: a clip that reads the table row of the
    same slot of another launch group reads other points."""
    count = rng.permutation(np.arange(300, 901))[:B]
    order = rng.permutation(T * B)
    size = np.repeat(count[None, :], T, 0).reshape(-1)
    start = np.empty(T * B, np.int64)
    start[order] = np.concatenate([[0], np.cumsum(size[order])[:-1]]) + 5
    crow = rng.permutation(B + 7)[:B]
    return count, start.reshape(T, B), crow, int(size.sum()) + 9


def gathers(dev, rng, T, B, K, M, with_vel, with_noise, patch=None, fps=None, jitter=0.003):
    """Both gathers through the public ops, and their torch compositions on the clamped indices."""
    import tpgan_amd.ops as ops
    count, frame_first, crow, P = clip_tables(rng, T, B)
    g = torch.Generator().manual_seed(int(rng.integers(2 ** 31)))
    pos = (torch.rand(P, 3, generator=g) + torch.tensor([1.0, 0.5, 2.0])).to(dev)
    vel = torch.randn(P, 3, generator=g).to(dev) if with_vel else None
    centroids = (torch.rand(B + 7, 3, generator=g) + 1.0).to(dev)
    if patch is None:
        patch = torch.stack([torch.randperm(int(n), generator=g)[:K] for n in count]).int()
    if fps is None:
        fps = torch.randint(K, (B, M), generator=g).int()
    patch, fps = patch.to(dev), fps.to(dev)
    noise = torch.randn(T, B, M, 3, generator=g).to(dev) if with_noise else None
    hp, hv = ops.clip_gather_high(pos, vel, frame_first, count, centroids, crow, patch)
    lp, lv = ops.clip_gather_low(hp, fps, noise, jitter, vel, frame_first, count)
    n = torch.as_tensor(count, device=dev).view(B, 1)
    first = torch.as_tensor(frame_first, device=dev).view(T, B, 1)
    rows = first + clamped(patch.long(), n).view(1, B, K)
    want_hp = pos[rows] - centroids[torch.as_tensor(crow, device=dev)].view(1, B, 1, 3)
    assert hp.shape == (T, B, K, 3) and torch.equal(hp, want_hp) and (hv is None) == (vel is None)
    sel = clamped(fps.long(), K).view(1, B, M, 1).expand(T, B, M, 3)
    want_lp = torch.gather(want_hp, 2, sel)
    if with_noise:
        want_lp = want_lp + noise * float(np.float32(jitter))
    assert lp.shape == (T, B, M, 3) and torch.equal(lp, want_lp) and (lv is None) == (vel is None)
    if with_noise:
        assert not torch.equal(lp, torch.gather(want_hp, 2, sel))
    if with_vel:
        assert torch.equal(hv, vel[rows])
        assert torch.equal(lv, vel[first + clamped(fps.long(), n).view(1, B, M)])
    # every clip's rows are its own: no two clips of the batch share a first row, a count or a centroid
    assert len(set(frame_first.reshape(-1).tolist())) == T * B and len(set(count.tolist())) == B == len(set(crow.tolist()))


@pytest.mark.parametrize("B,T,M,with_vel,with_noise", [(33, 8, 300, True, True), (65, 1, 1, False, False),
                                                        (65, 8, 1, True, False), (33, 1, 300, False, True)])
def test_gathers_equal_the_torch_compositions_beyond_one_group(dev, B, T, M, with_vel, with_noise):
    """K = 257: one lane past a workgroup of 256; M = 300 likewise, M = 1 a single lane; 8 frames: the tables' last row."""
    gathers(dev, np.random.default_rng(B * T + M), T, B, 257, M, with_vel, with_noise)


def test_gather_low_at_the_action_trainer_s_shape(dev):
    """ActionClipSampler's call: T * B = 48 frames as 48 "clips" of one frame, no velocities, no noise."""
    import tpgan_amd.ops as ops
    g = torch.Generator().manual_seed(48)
    T, B, K, M = 3, 16, 256, 16
    high = torch.randn(T, B, K, 3, generator=g).to(dev)
    fps = torch.stack([torch.randperm(K, generator=g)[:M] for _ in range(T * B)]).int().to(dev)
    low, none = ops.clip_gather_low(high.view(1, T * B, K, 3), fps)
    assert none is None and low.shape == (1, T * B, M, 3)
    assert torch.equal(low.view(T, B, M, 3), torch.gather(high, 2, fps.long().view(T, B, M, 1).expand(T, B, M, 3)))


def test_gathers_clamp_their_indices_as_the_header_states(dev):
    """patch entries -1, count[b] and 2^30 land inside the clip's scene, fps entries -5, K + 3 and 2^30 inside the patch
    for the positions and inside the scene for the velocities (K + 3 < count[b]: that one is a valid scene row), in the
    first launch group, in a later one and in the last slot of each.  In-range reads by contract."""
    rng = np.random.default_rng(2 ** 30)
    T, B, K, M = 2, 34, 257, 40
    count = clip_tables(np.random.default_rng(2 ** 30), T, B)[0]                          # the counts `gathers` will draw
    g = torch.Generator().manual_seed(1)
    patch = torch.stack([torch.randperm(int(n), generator=g)[:K] for n in count]).int()
    fps = torch.randint(K, (B, M), generator=g).int()
    for b in (0, 31, 32, 33):
        patch[b, [0, 100, 256]] = torch.tensor([-1, int(count[b]), 2 ** 30], dtype=torch.int32)
        fps[b, [0, 7, 39]] = torch.tensor([-5, K + 3, 2 ** 30], dtype=torch.int32)
        assert K + 3 < count[b]
    gathers(dev, rng, T, B, K, M, True, True, patch=patch, fps=fps)


# ---- frame subset -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K", cases.SUBSET)
def test_frame_subset_equals_the_rule(dev, n, K):
    import tpgan_amd.ops as ops
    seed = cases.subset_seed(n, K)
    got = ops.frame_subset([n], [seed], K, device=dev).cpu().numpy()
    assert got.shape == (1, K) and got.dtype == np.int32
    assert np.array_equal(got[0], subset(n, K, seed))


def test_frame_subset_batch_of_three_groups_equals_single_calls_and_repeats(dev):
    import tpgan_amd.ops as ops
    count, seeds, K = cases.subset_batch()
    got = ops.frame_subset(count, seeds, K, device=dev).cpu().numpy()
    for f in range(len(count)):
        assert np.array_equal(got[f], subset(int(count[f]), K, seeds[f])), f
    for f in (0, 31, 32, 63, 64):
        assert np.array_equal(got[f], ops.frame_subset(count[f:f + 1], seeds[f:f + 1], K, device=dev).cpu().numpy()[0]), f
    assert np.array_equal(got, ops.frame_subset(count, seeds, K, device=dev).cpu().numpy())


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_action_sampler_with_33_frames_per_batch(dev, tmp_path):
    """Batch 11 of 3 frames: the low-resolution gather sees 33 "clips", two launch groups."""
    from tpgan_amd.data import ActionClipSampler, ActionSequences
    write_random_dataset(str(tmp_path), [(300, 256, 520, 90, 257), (400, 255, 70, 350), (600, 500, 1000)], seed=11)
    seq = ActionSequences(str(tmp_path), train=True, device=dev)
    T, B, K, M = 3, 11, 256, 16

    def make():
        return ActionClipSampler(seq, B, K, generator=torch.Generator().manual_seed(33))
    s = make()
    out = s.sample()
    assert len(out) == 2 * T + 1 and _equal(make().sample(), out)                          # same seed, same bits
    fps, sub = s.last["fps_idx"].long(), s.last["subset_idx"].cpu().numpy()
    assert fps.shape == (T, B, M) and sub.shape == (T, B, K)
    rows = np.stack([seq.frame_rows(i) for i in s.last["indices"]], 1)
    for t in range(T):
        assert out[t].shape == (B, K, 3) and out[T + t].shape == (B, M, 3)
        assert torch.equal(out[T + t], torch.gather(out[t], 1, fps[t].unsqueeze(-1).expand(-1, -1, 3)))
        for b in range(B):
            n = int(seq.count[rows[t, b]])
            assert sub[t, b].min() >= 0 and sub[t, b].max() < n and len(np.unique(sub[t, b])) == min(n, K)


def test_clip_sampler_with_33_clips_per_batch(dev, tmp_path):
    """The fluid sampler's four calls with two launch groups (the toy dataset has 6 clips; a batch draws with
    replacement, and every clip of the batch has a seed point of its own): clips 0, 31 and 32 are the rule's patch of
    their scene and the gathers of their own frames, as the batch-4 test of tests/test_data_gpu.py checks them."""
    from tpgan_amd.data import ClipSampler, FluidSequences
    g = write_dataset(str(tmp_path))
    seq = FluidSequences(str(tmp_path), 2, int(g["case_steps"]), device=dev)
    B, K = 33, 4096
    indices = [i % len(seq) for i in range(B)]
    seeds = [(997 * b + 13) % int(seq.count[seq.clip(i)[0]]) for b, i in enumerate(indices)]

    def make():
        return ClipSampler(seq, B, K, jitter=0.003, generator=torch.Generator().manual_seed(21))
    s = make()
    out = s.sample(indices=indices, seed_idx=seeds)
    assert len(out) == 13 and out[12].shape == (B,) and s.last["indices"] == indices
    assert _equal(make().sample(indices=indices, seed_idx=seeds), out)
    fps, patch = s.last["fps_idx"].long(), s.last["patch_idx"].long()
    assert patch.shape == (B, K) and fps.shape == (B, K // 8)
    for f in range(3):
        low = torch.gather(out[f], 1, fps.unsqueeze(-1).expand(-1, -1, 3))
        assert float((out[6 + f] - low).abs().max()) < 6 * 0.003 and not torch.equal(out[6 + f], low)
        for b in (0, 31, 32):
            case, step = seq.clip(indices[b])
            frame = seq.pos[seq.frame_first[case, step + f]:][:seq.count[case]]
            vel = seq.vel[seq.frame_first[case, step + f]:][:seq.count[case]]
            assert torch.equal(out[f][b], frame[patch[b]] - seq.centroids[case * seq.case_steps + step + 1])
            assert torch.equal(out[3 + f][b], vel[patch[b]])
            assert torch.equal(out[9 + f][b], vel[fps[b]])
    for b in (0, 31, 32):
        case, step = seq.clip(indices[b])
        centre = seq.pos[seq.frame_first[case, step + 1]:][:seq.count[case]].cpu().numpy()
        assert np.array_equal(patch[b].cpu().numpy(), patch_rule(centre, seeds[b], K)), b
