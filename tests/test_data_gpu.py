"""The batched clip sampler on the GPU: tpg_patch_select_f32 against a numpy statement of its rule, the two gather
entries against their torch compositions, the reference's dataset golden on the HIP path, the sampler with the
side-stream prefetcher, and the trainer end to end with a bit-exact resume."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from select_rule import patch_rule as rule  # noqa: E402
from test_data_cpu import _equal, check_golden_items, check_trainer, write_dataset  # noqa: E402

pytestmark = pytest.mark.gpu


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


def ball(rng, n, centre=(1.0, 0.5, 2.0)):
    v = rng.normal(size=(n, 3))
    v *= (rng.uniform(size=(n, 1)) ** (1 / 3)) / np.linalg.norm(v, axis=1, keepdims=True)
    return (0.4 * v + np.asarray(centre)).astype(np.float32)


@pytest.mark.parametrize("N,K", [(N, K) for N in (4097, 20000, 65536, 200000) for K in (4096, 9216, 11264) if K <= N])
def test_patch_select_equals_the_rule(dev, N, K):
    rng = np.random.default_rng(N + K)
    pts = ball(rng, N)
    seed = int(rng.integers(N))
    got = select(dev, [pts], [seed], K)[0]
    assert np.array_equal(got, rule(pts, seed, K)) and got[0] == seed


def test_patch_select_ragged_batch_equals_single_calls_and_repeats(dev):
    rng = np.random.default_rng(7)
    sizes = [4096, 5000, 20000, 33333, 65537, 9000, 131072, 4100]
    scenes = [ball(rng, n, centre=rng.uniform(-2, 2, 3)) for n in sizes]
    seeds = [int(rng.integers(n)) for n in sizes]
    got = select(dev, scenes, seeds, 4096)
    for b, (s, sd) in enumerate(zip(scenes, seeds)):
        assert np.array_equal(got[b], rule(s, sd, 4096)), b
        assert np.array_equal(got[b], select(dev, [s], [sd], 4096)[0]), b
    assert np.array_equal(got, select(dev, scenes, seeds, 4096))               # two runs, the same bits


@pytest.mark.parametrize("K", [4096, 9216])
def test_patch_select_k_equals_n(dev, K):
    pts = ball(np.random.default_rng(K), K)
    got = select(dev, [pts], [17], K)[0]
    assert np.array_equal(got, rule(pts, 17, K)) and np.array_equal(np.sort(got), np.arange(K))


def test_patch_select_ties_are_decided_by_index(dev):
    rng = np.random.default_rng(11)
    K = 4096
    pts = ball(rng, 12000)
    seed = 6000
    pts[[5, 9000, 11999]] = pts[seed]                  # exact duplicates of the seed: index 5 comes first
    order = rule(pts, seed, K)
    near = pts[order[K - 100]].copy()
    far = rule(pts, seed, 12000)[-300:]                # 300 far points become copies of the (K-99)-th neighbour: a block
    pts[far] = near                                    # of 301 duplicates that starts 100 ranks before K and straddles it
    got = select(dev, [pts], [seed], K)[0]
    want = rule(pts, seed, K)
    assert np.array_equal(got, want) and list(got[:4]) == [5, seed, 9000, 11999]
    block = np.append(far, order[K - 100])
    assert np.isin(got, block).sum() == 100 and np.array_equal(got[-100:], np.sort(block)[:100])
    # a lattice: massive distance ties everywhere
    ax = np.arange(28, dtype=np.float32) * np.float32(0.025)
    lat = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    for sd in (0, 13 * 28 * 28 + 13 * 28 + 13):
        assert np.array_equal(select(dev, [lat], [sd], K)[0], rule(lat, sd, K)), sd
    # 999-padded dummies: 3000 identical far points after 5000 real ones, and a seed among the dummies
    pad = np.concatenate([ball(rng, 5000), np.full((3000, 3), 999.0, np.float32)])
    for sd in (10, 6000):
        assert np.array_equal(select(dev, [pad], [sd], 6000)[0], rule(pad, sd, 6000)), sd


def test_patch_select_ties_across_chunks_of_a_three_chunk_scene(dev):
    """2 * 1024 + 1 points, K = 1025: the whole first chunk of 1024 candidates, then ONE of the middle chunk, and the
    third chunk's single candidate stays out.  Every point is 0.5 or 2 from the seed along one axis (d2 = 4^-1 or 4^1,
    exact in fp32), and everything after the first chunk is at the far distance: the K-th distance has ties in all three
    chunks, of which the first chunk's and the first of the middle chunk's are taken."""
    rng = np.random.default_rng(2049)
    N, K = 2 * 1024 + 1, 1025
    far = np.ones(N, bool)
    far[1:1024] = rng.uniform(size=1023) < 0.5
    step = np.zeros((N, 3), np.float32)
    step[np.arange(N), rng.integers(3, size=N)] = np.where(far, 2.0, 0.5) * rng.choice([-1.0, 1.0], size=N)
    step[0] = 0.0
    pts = (np.asarray((1.0, 0.5, 2.0), np.float32) + step).astype(np.float32)
    got = select(dev, [pts], [0], K)[0]
    assert np.array_equal(got, rule(pts, 0, K))
    near = np.flatnonzero(~far)
    assert got[0] == 0 and np.array_equal(got[1:1 + len(near)], near) and got[-1] == 1024 and 2048 not in got


def test_patch_select_non_finite_coordinates(dev):
    """NaN distances rank after every finite one and after +inf, tied among themselves, by index."""
    rng = np.random.default_rng(3)
    pts = ball(rng, 5000)
    pts[100, 1] = np.nan
    pts[7, 0] = np.inf
    pts[4000] = np.nan
    pts[300, 2] = -np.inf
    got = select(dev, [pts], [50], 5000)[0]
    assert np.array_equal(got, rule(pts, 50, 5000))
    assert list(got[-4:]) == [7, 300, 100, 4000]
    assert np.array_equal(select(dev, [pts], [50], 4996)[0], rule(pts, 50, 4996))


def test_patch_select_error_statuses(dev):
    import tpgan_amd.ops as ops
    hip = ops.backend_for(torch.zeros(1, device=dev))
    pts = torch.rand(6000, 3, device=dev)
    one = lambda v: np.array([v], np.int32)                                       # noqa: E731
    idx = hip.patch_select(pts, one(0), one(6000), one(5), 4096)
    keep = idx.clone()
    for first, count, seed, K, msg in ((0, 6000, 6000, 4096, "ARG"), (0, 4000, 0, 4096, "ARG"), (1, 6000, 0, 4096, "ARG"),
                                       (0, 6000, 0, 0, "ARG")):
        with pytest.raises(RuntimeError, match=msg):
            hip.patch_select(pts, one(first), one(count), one(seed), K)
    big = torch.rand(20000, 3, device=dev)
    with pytest.raises(RuntimeError, match="UNSUPPORTED"):
        hip.patch_select(big, one(0), one(20000), one(0), 16385)
    torch.cuda.synchronize()
    assert torch.equal(idx, keep)


@pytest.mark.parametrize("with_vel,with_noise", [(True, True), (False, False), (True, False), (False, True)])
def test_gathers_equal_the_torch_compositions(dev, with_vel, with_noise):
    import tpgan_amd.ops as ops
    g = torch.Generator().manual_seed(5)
    T, B, K, M, P = 3, 5, 4096, 512, 60000
    pos = (torch.rand(P, 3, generator=g) + torch.tensor([1.0, 0.5, 2.0])).to(dev)
    vel = torch.randn(P, 3, generator=g).to(dev) if with_vel else None
    count = np.array([7000, 9000, 5000, 8000, 6000])
    frame_first = np.stack([np.array([0, 7000, 30000, 16000, 40000]) + t * count for t in range(T)])
    centroids = (torch.rand(11, 3, generator=g) + 1.0).to(dev)
    crow = [3, 0, 10, 7, 3]
    patch = torch.stack([torch.randperm(int(n), generator=g)[:K] for n in count]).int().to(dev)
    fps = torch.stack([torch.randperm(K, generator=g)[:M] for _ in count]).int().to(dev)
    noise = torch.randn(T, B, M, 3, generator=g).to(dev) if with_noise else None
    hp, hv = ops.clip_gather_high(pos, vel, frame_first, count, centroids, crow, patch)
    lp, lv = ops.clip_gather_low(hp, fps, noise, 0.003, vel, frame_first, count)
    rows = torch.as_tensor(frame_first, device=dev).view(T, B, 1) + patch.long().view(1, B, K)
    want_hp = pos[rows] - centroids[torch.tensor(crow, device=dev)].view(1, B, 1, 3)
    assert torch.equal(hp, want_hp) and (hv is None) == (vel is None)
    sel = fps.long().view(1, B, M, 1).expand(T, B, M, 3)
    want_lp = torch.gather(want_hp, 2, sel)
    if with_noise:
        want_lp = want_lp + noise * float(np.float32(0.003))
    assert torch.equal(lp, want_lp) and (lv is None) == (vel is None)
    if with_vel:
        assert torch.equal(hv, vel[rows])
        assert torch.equal(lv, vel[torch.as_tensor(frame_first, device=dev).view(T, B, 1) + fps.long().view(1, B, M)])


def test_golden_dataset_items_on_the_hip_path(dev, tmp_path):
    check_golden_items(dev, tmp_path)


def test_clip_sampler_and_prefetch_on_the_gpu(dev, tmp_path):
    from tpgan_amd.data import ClipSampler, FluidSequences, prefetch
    g = write_dataset(str(tmp_path))
    seq = FluidSequences(str(tmp_path), 2, int(g["case_steps"]), device=dev)

    def make():
        return ClipSampler(seq, 4, 4096, jitter=0.003, generator=torch.Generator().manual_seed(21))
    s = make()
    plain = [s.sample() for _ in range(6)]
    out = plain[0]
    assert len(out) == 13 and out[12].shape == (4,) and not out[12].is_cuda
    for j, t in enumerate(out[:12]):
        assert t.shape == (4, 4096 if j < 6 else 512, 3) and t.dtype == torch.float32 and t.device == dev and t.is_contiguous()
    # low = high rows + noise * jitter, every frame by the centre frame's lists
    s2 = make()
    out2 = s2.sample()
    assert _equal(out2, out)
    fps, patch = s2.last["fps_idx"].long(), s2.last["patch_idx"].long()
    for f in range(3):
        rows = torch.gather(out2[f], 1, fps.unsqueeze(-1).expand(-1, -1, 3))
        assert float((out2[6 + f] - rows).abs().max()) < 6 * 0.003 and not torch.equal(out2[6 + f], rows)
        for b, idx in enumerate(s2.last["indices"]):
            case, step = seq.clip(idx)
            frame = seq.pos[seq.frame_first[case, step + f]:][:seq.count[case]]
            vel = seq.vel[seq.frame_first[case, step + f]:][:seq.count[case]]
            assert torch.equal(out2[f][b], frame[patch[b]] - seq.centroids[case * seq.case_steps + step + 1])
            assert torch.equal(out2[3 + f][b], vel[patch[b]])
    # the prefetcher on its side stream while the main stream is kept busy
    a = torch.randn(4096, 4096, device=dev)
    it = prefetch(make())
    got = []
    for _ in range(6):
        for _ in range(4):
            a = (a @ a).clamp_(-1, 1)
        batch = next(it)
        got.append([t.clone() for t in batch])         # consumed on the main stream, after the hand-off
    torch.cuda.synchronize()
    for x, y in zip(got, plain):
        assert _equal(x, y)


def test_trainer_end_to_end_with_bit_exact_resume(dev, tmp_path, capsys):
    """14 iterations (both the n_iter <= 10 regime and the regular one), bf16 off, checkpoint round trip, and a run
    resumed from iteration 9 equal to the uninterrupted one bit for bit on parameters and Adam moments."""
    import json
    check_trainer(tmp_path, "cuda", 14, 9)
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["n_iter"] for l in lines][:14] == list(range(1, 15))
    assert all(np.isfinite(v) for l in lines for v in l.values())
