"""Sequence upsampling on the MI355X: the fused context-mask kernel (csrc/rollout.hip) bit for bit against a numpy
restatement of the reference's formula, and `SequenceUpsampler` / the rollout CLI against the per-frame loop."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tpgan_amd  # noqa: F401
from tpgan_amd import ops
from tpgan_amd.rollout import SequenceUpsampler, upsample_sequence
from tpgan_amd.srnet import SRNet
from tpgan_amd.synthetic import fluid_clip, force_all_keep

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
F32_06 = np.float32(0.6)
NONE = ops.CONTEXT_NONE


# ------------------------------------------------------------------------------------------------ numpy oracle
def np_context_expand(pos, edge, masks, first):
    """The reference's clamp / 25-frame mean / `> 0.01` / expand / `expanded[hard]`, frame by frame, for the frames
    `first` .. of the raw masks (all frames from 0 give the history) -> (points, offsets, state (2, N))."""
    F, N = masks.shape
    r = edge.shape[1] // N
    with np.errstate(invalid="ignore"):
        c = np.where(masks < F32_06, np.float32(0), masks)
        c = np.where(c > F32_06, F32_06, c).astype(np.float32)
        pts, offsets = [], [0]
        for t in range(first, F):
            keep = c[max(0, t - 24):t + 1].mean(axis=0, dtype=np.float32) > np.float32(0.01)
            k = t - first
            e = edge[k].reshape(N, r, 3) * keep.astype(np.float32)[:, None, None]
            expanded = pos[k][:, None, :] + e
            hard = np.repeat(keep[:, None], r, axis=1)
            hard[:, 0] = True
            pts.append(expanded[hard])
            offsets.append(offsets[-1] + int(hard.sum()))
    return np.concatenate(pts).reshape(-1, 3), np.array(offsets, np.int64), np_state(masks)


def np_state(masks):
    """(2, N): the last frame with m >= 0.6 and the last frame with m NaN (CONTEXT_NONE: none)."""
    frames = np.arange(masks.shape[0], dtype=np.int64)[:, None]
    with np.errstate(invalid="ignore"):
        hit = np.where(masks >= F32_06, frames, NONE).max(axis=0, initial=NONE)
    nan = np.where(np.isnan(masks), frames, NONE).max(axis=0, initial=NONE)
    return np.stack([hit, nan]).astype(np.int32)


def synthetic_masks(F, N, seed):
    """Sparse hits (exact 0.6, its upper neighbour, inf), values just below 0.6, -inf, NaN, negatives, and whole
    all-zero / all-hit frames."""
    rng = np.random.default_rng(seed)
    m = rng.uniform(-1.0, 0.59, size=(F, N)).astype(np.float32)
    u = rng.uniform(size=(F, N))
    m[u < 0.03] = rng.choice(np.array([F32_06, np.nextafter(F32_06, np.float32(1)), np.inf, 3.0], np.float32),
                             size=int((u < 0.03).sum()))
    near = (u >= 0.03) & (u < 0.04)
    m[near] = rng.choice(np.array([np.nextafter(F32_06, np.float32(0)), -np.inf, 0.0, -0.0], np.float32),
                         size=int(near.sum()))
    m[(u >= 0.5) & (u < 0.504)] = np.nan
    kind = rng.uniform(size=F)
    m[kind < 0.03] = 0.0
    m[(kind >= 0.03) & (kind < 0.06)] = F32_06
    return m


def synthetic_inputs(F, N, r, seed):
    rng = np.random.default_rng(seed + 1)
    pos = rng.standard_normal((F, N, 3)).astype(np.float32)
    edge = rng.standard_normal((F, N * r, 3)).astype(np.float32)
    special = rng.uniform(size=edge.shape) < 0.002                  # inf / NaN in edge, on kept and dropped points
    edge[special] = rng.choice(np.array([np.inf, -np.inf, np.nan], np.float32), size=int(special.sum()))
    return pos, edge, synthetic_masks(F, N, seed)


def same_bits(a, b):
    """Equal bit for bit, NaN payloads aside (numpy's default NaN is not the GPU's)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int32), b[~nb].view(np.int32))


def run_kernel(pos, edge, masks, state, t0):
    out, offsets = ops.context_expand(torch.from_numpy(pos).to(DEV), torch.from_numpy(edge).to(DEV),
                                      torch.from_numpy(masks).to(DEV), state, t0)
    offsets = offsets.cpu().numpy()
    return out[:offsets[-1]].cpu().numpy(), offsets


CASES = [(N, T, (2, 8, 16)[(i + j) % 3]) for i, N in enumerate((1, 63, 64, 65, 4097, 20000))
         for j, T in enumerate((1, 7, 25, 64))] + [(4097, 25, 2), (4097, 25, 16), (65, 64, 8), (63, 7, 16)]


@pytest.mark.parametrize("N,T,r", CASES)
def test_kernel_bit_exact_against_numpy(N, T, r):
    history = 30 if N * T <= 4097 * 25 else 3                       # frames before the chunk (window start > 0)
    F = history + T
    pos, edge, masks = synthetic_inputs(T, N, r, seed=N * 131 + T * 7 + r)
    all_masks = np.concatenate([synthetic_masks(history, N, seed=N + 5), masks])
    want_pts, want_off, want_state = np_context_expand(pos, edge, all_masks, history)
    # the state of the history frames, as a previous call would have left it
    state = torch.from_numpy(np_state(all_masks[:history])).to(DEV).contiguous()
    pts, off = run_kernel(pos, edge, masks, state, history)
    assert np.array_equal(off, want_off)
    assert same_bits(pts, want_pts)
    assert np.array_equal(state.cpu().numpy(), want_state)
    assert F == all_masks.shape[0] and want_off[-1] > N * T       # some points kept


@pytest.mark.parametrize("N,r", [(65, 8), (4097, 16), (20000, 2)])
def test_state_carried_across_launches_equals_one_launch(N, r):
    T = 64
    pos, edge, masks = synthetic_inputs(T, N, r, seed=N + r)
    one = ops.context_state(N, DEV)
    pts1, off1 = run_kernel(pos, edge, masks, one, 0)
    many, pts, offs, t0 = ops.context_state(N, DEV), [], [0], 0
    for c in (1, 5, 17, 25, 16):
        p, o = run_kernel(pos[t0:t0 + c], edge[t0:t0 + c], masks[t0:t0 + c], many, t0)
        pts.append(p)
        offs += list(offs[-1] + o[1:])
        t0 += c
    assert t0 == T
    assert np.array_equal(np.array(offs), off1)
    assert same_bits(np.concatenate(pts), pts1)
    assert torch.equal(one, many)
    want_pts, want_off, want_state = np_context_expand(pos, edge, masks, 0)
    assert np.array_equal(off1, want_off) and same_bits(pts1, want_pts)
    assert np.array_equal(one.cpu().numpy(), want_state)


def test_kernel_rejects_bad_arguments(hip_lib):
    assert hip_lib.tpg_context_expand_f32(None, None, None, 1, 8, 17, 0, None, None, None, None, None) == -3
    assert hip_lib.tpg_context_expand_f32(None, None, None, 1, 8, 1, 0, None, None, None, None, None) == -3
    assert hip_lib.tpg_context_expand_f32(None, None, None, 1, 8, 8, -1, None, None, None, None, None) == -1
    assert hip_lib.tpg_context_expand_f32(None, None, None, 0, 8, 8, 0, None, None, None, None, None) == 0
    with pytest.raises(RuntimeError, match="ratio"):
        ops.context_expand(torch.zeros(1, 4, 3, device=DEV), torch.zeros(1, 4, 3, device=DEV),
                           torch.zeros(1, 4, device=DEV), ops.context_state(4, DEV), 0)


# ------------------------------------------------------------------------------------- the upsampler on a model
def mixed_net(in_feats, feats, seed):
    """Random weights; the mask head's last layer rescaled so that the raw masks spread ~1 and 0.6 sits in the widest
    gap of the values of the top decile but one (mixed per-point decisions; a hit keeps a point for 25 frames)."""
    torch.manual_seed(seed)
    net = SRNet(in_feats, 128).to(DEV).eval()
    last = net.filter_block.decoder[1]
    with torch.no_grad():
        last.bias.zero_()                                           # pre-activations z of the last layer, exactly:
        pos_part = torch.cat([net.body(feats[t:t + 1], None)[1] for t in range(feats.shape[0])])
        last.weight.neg_()                                          # relu(z) - relu(-z)
        z = pos_part - torch.cat([net.body(feats[t:t + 1], None)[1] for t in range(feats.shape[0])])
        last.weight.neg_()
        k = 1.0 / float(z.std())
        u = torch.unique(z.double())
        lo, hi = 17 * len(u) // 20, 19 * len(u) // 20
        i = lo + int(torch.argmax(u[lo + 1:hi + 1] - u[lo:hi])) + 1
        k = max(k, 1e-3 / float(u[i] - u[i - 1]))                  # every raw mask >= 5e-4 away from 0.6
        last.weight.mul_(k)
        last.bias.fill_(float(0.6 - k * (u[i - 1] + u[i]) / 2))
    return net


def sequence(frames, n, in_feats, seed):
    low, _, vel, _ = fluid_clip(1, n * 8, 8, frames, seed=seed, device=DEV, with_vel=True)
    pos = torch.cat(low).contiguous()
    feats = pos if in_feats == 3 else torch.cat([pos, torch.cat(vel) * 0.025], -1).contiguous()
    return feats, pos


def literal_loop(net, feats, pos):
    """Per-frame reference formula on body(feature, None) -> outputs, raw masks (T, N)."""
    hist, outs, masks = [], [], []
    with torch.no_grad():
        for t in range(pos.shape[0]):
            edge, mask = net.body(feats[t:t + 1], None)
            masks.append(mask.view(-1))
            c = torch.where(mask < 0.6, torch.zeros_like(mask), mask)
            c = torch.where(c > 0.6, torch.full_like(c, 0.6), c)
            hist = hist[-24:] if len(hist) >= 25 else hist
            hist.append(c)
            outs.append(net.expand_pos_with_masking(pos[t:t + 1], edge, torch.mean(torch.cat(hist, 0), 0), True)[1])
    return outs, torch.stack(masks)


def close(a, b, tol=2e-4):
    """tests/test_golden_models.py's tolerance for the GPU generator (forward_frames)."""
    a, b = a.detach().float().cpu().numpy(), b.detach().float().cpu().numpy()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float(np.abs(a - b).max(initial=0.0)) <= tol * max(1.0, float(np.abs(b).max(initial=0.0)))


def compare(got, want, masks=None):
    if masks is not None:
        assert float((masks - 0.6).abs().min()) > 1e-4, "a mask lies at the decision threshold: pick another seed"
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape                                   # keep decisions and counts exact
        close(g, w)


@pytest.mark.parametrize("frames,n,mode", [(40, 4096, "keep"), (40, 4096, "mixed"), (6, 20000, "keep"),
                                           (6, 20000, "mixed")])
def test_upsampler_equals_forward_with_context_loop(frames, n, mode):
    feats, pos = sequence(frames, n, 3, seed=n + frames)
    if mode == "keep":
        torch.manual_seed(1)
        net = force_all_keep(SRNet(3, 128)).to(DEV).eval()
    else:
        net = mixed_net(3, feats, seed=2)
    want, hist = [], []
    with torch.no_grad():
        for t in range(frames):
            out, hist = net.forward_with_context(feats[t:t + 1], pos[t:t + 1], hist)
            want.append(out)
        masks = torch.stack([net.body(feats[t:t + 1], None)[1].view(-1) for t in range(frames)])
    if mode == "keep":
        assert all(w.shape[1] == 8 * n for w in want)
    else:
        keeps = [w.shape[1] for w in want]
        assert min(keeps) > n and max(keeps) < 8 * n, keeps
    compare(upsample_sequence(net, feats, pos), want, None if mode == "keep" else masks)
    up = SequenceUpsampler(net, chunk=3)
    compare(up.push(feats[:4], pos[:4]) + up.push(feats[4:], pos[4:]), want)


def test_upsampler_in_feats_6_follows_the_reference_body():
    feats, pos = sequence(30, 2048, 6, seed=6)
    net = mixed_net(6, feats, seed=6)
    want, masks = literal_loop(net, feats, pos)
    compare(upsample_sequence(net, feats, pos, chunk=8), want, masks)


def test_chunk_invariance():
    feats, pos = sequence(70, 1024, 3, seed=70)
    net = mixed_net(3, feats, seed=7)
    base = upsample_sequence(net, feats, pos, chunk=1)
    for chunk in (16, 64):
        compare(upsample_sequence(net, feats, pos, chunk=chunk), base)


def test_cli_end_to_end(tmp_path):
    frames, n = 30, 512
    feats, pos = sequence(frames, n, 6, seed=30)
    net = mixed_net(6, feats, seed=30)
    rng = np.random.default_rng(0)
    shift = rng.uniform(-2, 2, size=(frames, 1, 3)).astype(np.float32)    # frames away from the origin
    vel = (feats[..., 3:] / 0.025).cpu().numpy()
    for i in range(frames):
        np.savez(tmp_path / f"data_{i}.npz", pos=pos[i].cpu().numpy() + shift[i], vel=vel[i])
    ckpt = tmp_path / "tpugan_vel_checkpoint.ckpt"
    torch.save({"sr_net": net.state_dict(), "n_iter": 0}, ckpt)
    out = tmp_path / "out"
    cmd = [sys.executable, "-m", "tpgan_amd.rollout", "--checkpoint", str(ckpt), "--frames",
           str(tmp_path / "data_{i}.npz"), "--count", str(frames), "--in-feats", "6", "--chunk", "8", "--out", str(out)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    # the in-process loop: the demo notebook's normalisation, the reference formula per frame
    from tpgan_amd.rollout import load_frames
    f, p, cents, hs = load_frames(str(tmp_path / "data_{i}.npz"), range(frames), 6)
    want, _ = literal_loop(net, f.to(DEV), p.to(DEV))
    for i in range(frames):
        got = np.load(out / f"pcd_{i}.npy")
        expect = want[i][0].cpu().numpy() * hs[i] + cents[i]
        assert got.shape == expect.shape
        assert np.abs(got - expect).max() <= 2e-4 * max(1.0, np.abs(expect).max())
