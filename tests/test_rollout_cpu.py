"""Sequence upsampling (tpgan_amd.rollout, ops.context_expand) without a GPU.

1. The two-int32 state (last frame with a hit, last frame with a NaN) decides exactly what the reference's clamp to
   {0, 0.6}, 25-frame mean and `> 0.01` decide (upsampling_network.py:159-174), over thousands of random frames.
2. Under the oracle backend, `upsample_sequence` / `SequenceUpsampler` at several chunk sizes and across several
   `push` calls equal a per-frame loop of the reference's formula on `net.body(feature, None)`."""
import numpy as np
import pytest
import torch

import tpgan_amd  # noqa: F401
from tpgan_amd import ops
from tpgan_amd.rollout import SequenceUpsampler, default_chunk, upsample_sequence
from tpgan_amd.srnet import NoMaskSRNet, SRNet
from tpgan_amd.synthetic import fluid_clip

F32_06 = np.float32(0.6)


def literal_keeps(masks):
    """The reference's running average, literally: (F, N) raw masks -> (F, N) keep decisions."""
    hist, keeps = [], []
    for m in masks:
        c = m.view(1, -1, 1)
        c = torch.where(c < 0.6, torch.zeros_like(c), c)
        c = torch.where(c > 0.6, torch.full_like(c, 0.6), c)
        if len(hist) >= 25:
            hist = hist[-24:]
        hist.append(c)
        keeps.append((torch.mean(torch.cat(hist, dim=0), dim=0) > 0.01).view(-1))
    return torch.stack(keeps)


def random_masks(frames, n, seed, p_hit=0.03, p_nan=0.004):
    """Raw masks with sparse hits (windows lapse), exact 0.6 and its float neighbours, NaN, +-inf, negatives, and
    whole all-zero / all-hit frames."""
    rng = np.random.default_rng(seed)
    m = rng.uniform(-1.0, 0.59, size=(frames, n)).astype(np.float32)
    u = rng.uniform(size=(frames, n))
    specials = np.array([F32_06, np.nextafter(F32_06, np.float32(1)), np.float32(np.inf), np.float32(7.5)], np.float32)
    hit = u < p_hit
    m[hit] = rng.choice(specials, size=int(hit.sum()))
    near = (u >= p_hit) & (u < p_hit + 0.01)
    m[near] = rng.choice(np.array([np.nextafter(F32_06, np.float32(0)), np.float32(-np.inf), np.float32(0.0),
                                   np.float32(-0.0)], np.float32), size=int(near.sum()))
    m[(u >= 0.5) & (u < 0.5 + p_nan)] = np.nan
    kind = rng.uniform(size=frames)
    m[kind < 0.03] = 0.0                                            # all-zero frames
    m[(kind >= 0.03) & (kind < 0.06)] = F32_06                      # all-hit frames
    return torch.from_numpy(m)


@pytest.mark.parametrize("frames,seed,chunks", [(1200, 0, (1,)), (900, 1, (7, 25, 64)), (60, 2, (60,)),
                                                (400, 3, (3, 1, 100, 24, 26))])
def test_state_form_equals_the_literal_running_average(frames, seed, chunks):
    masks = random_masks(frames, 64, seed)
    want = literal_keeps(masks)
    assert want.any() and not want.all()
    state, t, got = ops.context_state(64, "cpu"), 0, []
    while t < frames:
        for c in chunks:
            if t >= frames:
                break
            got.append(ops.context_keep(masks[t:t + c], state, t))
            t += got[-1].shape[0]
    got = torch.cat(got)
    assert torch.equal(got, want)
    # the window's start: frames before 24 see every earlier frame, later ones only the last 25
    assert frames < 25 or torch.equal(got[:24], want[:24])


def test_state_marks_nan_and_hits():
    masks = torch.tensor([[0.6, np.nan, 0.0], [0.0, 0.0, 0.59999996]], dtype=torch.float32)
    state = ops.context_state(3, "cpu")
    keep = ops.context_keep(masks, state, 5)
    assert keep.tolist() == [[True, False, False], [True, False, False]]
    assert state.tolist() == [[5, ops.CONTEXT_NONE, ops.CONTEXT_NONE], [ops.CONTEXT_NONE, 5, ops.CONTEXT_NONE]]
    late = ops.context_keep(torch.zeros(1, 3), state, 5 + 25)       # 25 frames later the hit has left the window
    assert late.tolist() == [[False, False, False]]


def test_context_expand_torch_form_matches_the_reference_expansion():
    """The composition for backends without the kernel: the reference's expand_pos_with_masking per frame."""
    torch.manual_seed(0)
    T, N, r = 5, 37, 4
    pos, edge = torch.randn(T, N, 3), torch.randn(T, N * r, 3)
    edge[0, 3] = float("inf")
    edge[1, 9] = float("nan")
    masks = random_masks(T, N, 7, p_hit=0.4)
    net = SRNet(3, 16, upsample_ratio=r)
    state = ops.context_state(N, "cpu")
    pts, offsets = ops._context_expand_torch(pos, edge, masks, state, 0)
    keeps = literal_keeps(masks)
    for t in range(T):
        _, want = net.expand_pos_with_masking(pos[t:t + 1], edge[t:t + 1].view(1, N, 3 * r),
                                              keeps[t].float().view(1, N, 1), hard_masking=True)
        got = pts[offsets[t]:offsets[t + 1]]
        assert got.shape == want[0].shape
        assert np.array_equal(got.numpy().view(np.int32), want[0].numpy().view(np.int32))


def test_cpu_tensors_need_a_backend():
    ops.unregister_backend("cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.context_expand(torch.zeros(1, 4, 3), torch.zeros(1, 8, 3), torch.zeros(1, 4),
                           ops.context_state(4, "cpu"), 0)


def test_default_chunk():
    assert default_chunk(1) == 64 and default_chunk(10 ** 7) == 1
    assert all(1 <= default_chunk(n) <= 64 for n in (1024, 4096, 16384, 65536))


# ------------------------------------------------------------------------------------- sequences through a model
N_PTS = 96


def _sequence(frames, in_feats, seed):
    low, _, vel, _ = fluid_clip(1, N_PTS * 8, 8, frames, seed=seed, with_vel=True)
    pos = torch.cat(low)                                            # (T, N, 3)
    feats = pos if in_feats == 3 else torch.cat([pos, torch.cat(vel) * 0.025], -1)
    return feats.contiguous(), pos.contiguous()


def _mixed_net(in_feats, feats):
    """Random weights; the mask head's bias moved so that the raw masks straddle 0.6 (mixed per-point decisions)."""
    torch.manual_seed(in_feats)
    net = SRNet(in_feats, 128).eval()
    last = net.filter_block.decoder[1]
    with torch.no_grad():
        last.bias.zero_()                                           # pre-activations z of the last layer, exactly:
        pos_part = net.body(feats, None)[1]
        last.weight.neg_()                                          # relu(z) - relu(-z)
        z = pos_part - net.body(feats, None)[1]
        last.weight.neg_()
        k = 1.0 / float(z.std())                                    # raw masks spread ~1 around 0.6 ...
        u = torch.unique(z.double())
        lo, hi = 17 * len(u) // 20, 19 * len(u) // 20              # ... with 0.6 in the widest gap of the top
        i = lo + int(torch.argmax(u[lo + 1:hi + 1] - u[lo:hi])) + 1  # decile but one (a hit keeps 25 frames)
        k = max(k, 1e-3 / float(u[i] - u[i - 1]))                  # every raw mask >= 5e-4 away from 0.6
        last.weight.mul_(k)
        last.bias.fill_(float(0.6 - k * (u[i - 1] + u[i]) / 2))
    return net


def literal_rollout(net, feats, pos):
    """The reference's forward_with_context, one frame at a time, on body(feature, None) -> list, masks."""
    hist, outs, masks = [], [], []
    for t in range(pos.shape[0]):
        edge, mask = net.body(feats[t:t + 1], None)
        masks.append(mask.view(-1))
        c = torch.where(mask < 0.6, torch.zeros_like(mask), mask)
        c = torch.where(c > 0.6, torch.full_like(c, 0.6), c)
        if len(hist) >= 25:
            hist = hist[-24:]
        hist.append(c)
        _, out = net.expand_pos_with_masking(pos[t:t + 1], edge, torch.mean(torch.cat(hist, 0), 0), hard_masking=True)
        outs.append(out)
    return outs, torch.stack(masks)


def _compare(got, want, masks):
    assert (masks - 0.6).abs().min() > 1e-4, "a mask lies at the decision threshold: pick another seed"
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape
        assert torch.allclose(g, w, rtol=0, atol=2e-5)


@pytest.mark.parametrize("in_feats", [3, 6])
def test_upsample_sequence_equals_the_per_frame_formula(oracle_cpu, in_feats):
    feats, pos = _sequence(34, in_feats, seed=11 + in_feats)
    net = _mixed_net(in_feats, feats)
    with torch.no_grad():
        want, masks = literal_rollout(net, feats, pos)
    keeps = literal_keeps(masks)
    assert keeps.any() and not keeps.all()
    counts = [N_PTS + 7 * int(k.sum()) for k in keeps]
    assert [w.shape[1] for w in want] == counts
    for chunk in (1, 7, 32):
        _compare(upsample_sequence(net, feats, pos, chunk=chunk), want, masks)
    up = SequenceUpsampler(net, chunk=4)                            # several pushes carry the state
    got = []
    for a, b in ((0, 3), (3, 20), (20, 21), (21, 34)):
        got += up.push(feats[a:b], pos[a:b])
    _compare(got, want, masks)
    up.reset()
    _compare(up.push(feats[:10], pos[:10]), want[:10], masks[:10])


def test_nomask_sequence_equals_per_frame_forward(oracle_cpu):
    feats, pos = _sequence(9, 3, seed=5)
    torch.manual_seed(3)
    net = NoMaskSRNet(3, 128).eval()
    with torch.no_grad():
        want = [net(feats[t:t + 1], pos[t:t + 1])[0] for t in range(9)]
    for chunk in (1, 4, None):
        got = upsample_sequence(net, feats, pos, chunk=chunk)
        assert len(got) == 9
        for g, w in zip(got, want):
            assert g.shape == w.shape == (1, N_PTS * 8, 3)
            assert torch.allclose(g, w, rtol=0, atol=2e-5)


def test_sequence_keeps_its_point_count(oracle_cpu):
    feats, pos = _sequence(2, 3, seed=1)
    up = SequenceUpsampler(SRNet(3, 128).eval(), chunk=1)
    up.push(feats, pos)
    with pytest.raises(ValueError, match="point count"):
        up.push(feats[:, :50].contiguous(), pos[:, :50].contiguous())
