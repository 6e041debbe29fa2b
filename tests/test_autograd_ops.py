"""The layer every caller goes through -- the torch.autograd.Function classes of tpgan_amd.ops and the four drop-in
modules under compat/ -- against plain fp64 PyTorch statements of the same operations, differentiated by
torch.autograd.  The statements are written from the docstrings and include/tpgan_ops.h and share no code with ops.py.

One body per case, two devices: "cpu" runs the Python layer over the oracle backend (no GPU needed), "cuda" runs the
HIP kernels through the very same layer.  Search results (kNN / radius / three-nn / ball-query indices) are pinned
bit-exact elsewhere; here they are taken from oracle.ref_ops on the same inputs, asserted equal, and values and
gradients are compared in fp64 on top of them.

Tolerances are derived, not tuned:
  * pure gathers: equality;
  * an fp32 sum of n terms, each made with c roundings: |got - want| <= (n + c) 2^-24 sum|term_i| elementwise, the sum
    of magnitudes taken in fp64 through the same scatter;
  * BatchNorm / head / spectral norm: TOL = 1e-5 of the tensor's largest magnitude (BASELINE.json);
  * a value stored in bf16: 2^-7 |ref| + 1e-5 max|ref| on top.
Every element of every compared tensor is compared.  Inputs of LeakyReLU / max cases are conditioned so that no fp64
pre-activation lies within 1e-4 of the kink and the two largest of every (group, channel) are 1e-3 of the scale apart;
both are asserted on the reference before anything runs."""
import sys
import types
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_ops as R

U32 = 2.0 ** -24
TOL = 1e-5
DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
GPU_ONLY = [pytest.param("cuda", marks=pytest.mark.gpu)]


def _on(request, device):
    """Make `device` usable: the oracle backend for CPU tensors, the HIP library for the GPU."""
    if device == "cpu":
        request.getfixturevalue("oracle_cpu")
    else:
        assert torch.cuda.is_available()
    return torch.device(device)


def _rng(*key):
    return np.random.default_rng(list(key))


def _t(a, dev, grad=False, dtype=torch.float32):
    t = torch.from_numpy(np.array(a)) if isinstance(a, np.ndarray) else a.detach().cpu().clone()    # never the caller's memory
    t = t.to(dtype).to(dev)
    return t.requires_grad_(True) if grad else t


def _d(t, grad=False):
    """The fp64 CPU carrier of the values a tensor holds (exact for fp32 and bf16)."""
    return t.detach().cpu().double().requires_grad_(grad)


def _cmp_sum(got, want, absum, n, c, what, bf16=False):
    """fp32 sum of n terms of c roundings each (n: number or tensor of per-element counts)."""
    got, want = got.detach().cpu().double(), want.detach().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bound = (torch.as_tensor(n, dtype=torch.float64) + c) * U32 * absum.detach().double()
    if bf16:
        bound = bound + 2.0 ** -7 * want.abs() + 1e-5 * want.abs().max()
    err = (got - want).abs()
    assert bool((err <= bound).all()), (what, float((err - bound).max()), float(err.max()))


def _cmp_tol(got, want, what, bf16=False, tol=TOL, extra=None):
    """TOL of the tensor's largest magnitude, floored at 1 as tests/test_ops_gpu.py takes it."""
    got, want = got.detach().cpu().double(), want.detach().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bound = tol * max(1.0, float(want.abs().max()))
    if extra is not None:
        bound = bound + extra
    if bf16:
        bound = bound + 2.0 ** -7 * want.abs() + 1e-5 * want.abs().max()
    err = (got - want).abs()
    assert bool((err <= bound).all()), (what, float(err.max()), float(want.abs().max()))


def _exact(got, want, what):
    got, want = got.detach().cpu().double(), want.detach().double()
    assert got.shape == want.shape and bool((got == want).all()), what


def _lrelu(z, slope):
    return torch.where(z > 0, z, z * slope)


# ---------------------------------------------------------------------------------------------------------------
# 1. gather_operation / gather_rows / grouping_operation / three_interpolate
# ---------------------------------------------------------------------------------------------------------------
def _upstream(kind, shape, rng):
    """-> (the tensor handed to backward, or None for out.sum().backward(); its fp64 values)."""
    if kind == "expanded":
        return None, torch.ones(shape, dtype=torch.float64)
    g = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    if kind == "transposed":
        g = g.transpose(-1, -2).contiguous().transpose(-1, -2)          # same values, last two strides swapped
        assert not g.is_contiguous() or g.shape[-1] == 1 or g.shape[-2] == 1
    elif kind == "bf16":
        g = g.bfloat16()
    return g, g.double()


def _backward(out, leaves, g, dev):
    if g is None:
        out.sum().backward(retain_graph=True)
        grads = [l.grad.clone() for l in leaves]
    else:
        grads = [x.clone() for x in torch.autograd.grad(out, leaves, g.to(dev), retain_graph=True)]
    for l in leaves:
        l.grad = None
    return grads


# (B, C, N, S, K): small, S = K = 1 with one channel, C = 128, and the workload's N = 4096 / S = 1024 / K = 32
GATHER_SHAPES = [(2, 3, 50, 7, 4), (1, 1, 33, 1, 1), (2, 128, 64, 16, 5), (2, 3, 4096, 1024, 32)]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("upstream", ["random", "expanded", "transposed", "bf16"])
@pytest.mark.parametrize("repeat", [False, True])
@pytest.mark.parametrize("B,C,N,S,K", GATHER_SHAPES)
@pytest.mark.parametrize("op", ["gather_operation", "gather_rows", "grouping_operation"])
def test_gathers_match_fp64(request, device, op, B, C, N, S, K, repeat, upstream):
    from tpgan_amd import ops
    dev = _on(request, device)
    rng = _rng(1, B, C, N, S, K, int(repeat))
    ishape = (B, S, K) if op == "grouping_operation" else (B, S)
    idx = np.full(ishape, N // 2, np.int32) if repeat else rng.integers(0, N, ishape).astype(np.int32)
    f = rng.standard_normal((B, N, C) if op == "gather_rows" else (B, C, N)).astype(np.float32)
    x = _t(f, dev, grad=True)
    out = getattr(ops, op)(x, _t(idx, dev, dtype=torch.int32))
    # the fp64 statement
    xr = _d(x, grad=True)
    li = torch.from_numpy(idx).long()
    if op == "gather_rows":
        ref = torch.gather(xr, 1, li[:, :, None].expand(B, S, C))
    else:
        ref = torch.gather(xr, 2, li.reshape(B, 1, -1).expand(B, C, -1)).reshape((B, C) + ishape[1:])
    assert out.dtype == torch.float32
    _exact(out, ref, "forward")
    g, g64 = _upstream(upstream, tuple(ref.shape), _rng(2, B, C, N, S, K))
    (want,) = torch.autograd.grad(ref, xr, g64, retain_graph=True)
    (absum,) = torch.autograd.grad(ref, xr, g64.abs(), retain_graph=True)
    (hits,) = torch.autograd.grad(ref, xr, torch.ones_like(ref))
    (got,) = _backward(out, [x], g, dev)
    assert got.dtype == torch.float32
    # a scatter of `hits` terms per element, the terms are the upstream values themselves (c = 0)
    _cmp_sum(got, want, absum, hits, 0, "grad features")
    # these scatters add with float atomics (csrc/ball_group.hip): a second backward agrees within the same bound
    (again,) = _backward(out, [x], g, dev)
    _cmp_sum(again, want, absum, hits, 0, "grad features, second backward")


def _three_case(rng, B, n, m):
    u = rng.uniform(-0.25, 0.25, (B, n, 3)).astype(np.float32)
    k = rng.uniform(-0.25, 0.25, (B, m, 3)).astype(np.float32)
    return u, k


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("upstream", ["random", "expanded", "transposed", "bf16"])
@pytest.mark.parametrize("B,C,n,m", [(2, 3, 50, 7), (1, 1, 1, 3), (2, 128, 64, 16), (3, 5, 300, 3), (2, 3, 4096, 1024)])
def test_three_interpolate_matches_fp64(request, device, B, C, n, m, upstream):
    from tpgan_amd import ops
    dev = _on(request, device)
    rng = _rng(3, B, C, n, m)
    u, k = _three_case(rng, B, n, m)
    dist, idx = ops.three_nn(_t(u, dev), _t(k, dev))
    rd2, ri = R.three_nn(u, k)
    assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), ri)
    # the distance is the square root of the oracle's squared distance: one fp32 operation, which torch's vectorised
    # square root delivers within one ulp (2^-23 relative) rather than correctly rounded
    root = torch.from_numpy(rd2).double().sqrt()
    assert dist.dtype == torch.float32 and bool(((dist.cpu().double() - root).abs() <= 2.0 ** -23 * root).all())
    # the usual inverse-distance weights (pointnet2's PointnetFPModule)
    w = 1.0 / (dist + 1e-8)
    w = (w / w.sum(2, keepdim=True)).contiguous()
    f = rng.standard_normal((B, C, m)).astype(np.float32)
    x = _t(f, dev, grad=True)
    out = ops.three_interpolate(x, idx, w)
    xr, wr = _d(x, grad=True), _d(w)
    li = torch.from_numpy(ri).long()
    picked = torch.gather(xr, 2, li.reshape(B, 1, n * 3).expand(B, C, n * 3)).reshape(B, C, n, 3)
    ref = (picked * wr[:, None]).sum(3)
    # three products (one rounding each) and their sum
    _cmp_sum(out, ref, (picked.abs() * wr[:, None]).sum(3), 3, 1, "forward")
    g, g64 = _upstream(upstream, tuple(ref.shape), _rng(4, B, C, n, m))
    (want,) = torch.autograd.grad(ref, xr, g64, retain_graph=True)
    (absum,) = torch.autograd.grad(ref, xr, g64.abs(), retain_graph=True)          # the weights are positive
    hits = torch.zeros(B, m, dtype=torch.float64).scatter_add_(1, li.reshape(B, -1), torch.ones(B, n * 3, dtype=torch.float64))
    (got,) = _backward(out, [x], g, dev)
    # `hits` terms g * w per element (c = 1), float atomics: the second backward is held to the same bound
    _cmp_sum(got, want, absum, hits[:, None, :], 1, "grad features")
    (again,) = _backward(out, [x], g, dev)
    _cmp_sum(again, want, absum, hits[:, None, :], 1, "grad features, second backward")


# ---------------------------------------------------------------------------------------------------------------
# 2. chamfer_nn and the loss built on it
# ---------------------------------------------------------------------------------------------------------------
def _chamfer_clouds(kind, rng):
    if kind == "ragged":                     # N != M
        s, t = rng.uniform(-1, 1, (2, 37, 3)), rng.uniform(-1, 1, (2, 90, 3))
    elif kind == "one_target_for_many":      # every source is nearest to target 4; the targets are far apart
        t = rng.uniform(-1, 1, (2, 9, 3)) * 10
        s = t[:, 4:5] + 0.01 * rng.standard_normal((2, 60, 3))
    elif kind == "duplicates":
        s, t = rng.uniform(-1, 1, (2, 40, 3)), rng.uniform(-1, 1, (2, 25, 3))
        s[:, 7] = s[:, 3]; s[:, 8] = s[:, 3]; t[:, 5] = t[:, 2]; t[0, 9] = s[0, 3]      # ... and one exact hit
    elif kind == "single":                   # B = 1, N = 1
        s, t = rng.uniform(-1, 1, (1, 1, 3)), rng.uniform(-1, 1, (1, 5, 3))
    else:                                    # the workload's size
        s, t = rng.uniform(-0.25, 0.25, (2, 4096, 3)), rng.uniform(-0.25, 0.25, (2, 1024, 3))
    return s.astype(np.float32), t.astype(np.float32)


def _chamfer_ref(s, t, i1, i2, g1, g2):
    """d1[b,i] = |s_i - t_{i1[i]}|^2, d2[b,j] = |t_j - s_{i2[j]}|^2 and the gradients of sum g1 d1 + sum g2 d2, with
    the per-element sum of the magnitudes of the terms 2 g (a - b) and their number."""
    B, N, _ = s.shape
    M = t.shape[1]
    e1, e2 = i1[:, :, None].expand(B, N, 3), i2[:, :, None].expand(B, M, 3)
    d1 = ((s - torch.gather(t, 1, e1)) ** 2).sum(2)
    d2 = ((t - torch.gather(s, 1, e2)) ** 2).sum(2)
    gs, gt = torch.autograd.grad([d1, d2], [s, t], [g1, g2])
    a1 = (2 * g1[:, :, None] * (s - torch.gather(t, 1, e1))).abs().detach()
    a2 = (2 * g2[:, :, None] * (t - torch.gather(s, 1, e2))).abs().detach()
    abs_s = a1 + torch.zeros(B, N, 3, dtype=torch.float64).scatter_add_(1, e2, a2)
    abs_t = a2 + torch.zeros(B, M, 3, dtype=torch.float64).scatter_add_(1, e1, a1)
    n_s = 1 + torch.zeros(B, N, dtype=torch.float64).scatter_add_(1, i2, torch.ones(B, M, dtype=torch.float64))
    n_t = 1 + torch.zeros(B, M, dtype=torch.float64).scatter_add_(1, i1, torch.ones(B, N, dtype=torch.float64))
    return d1, d2, gs, gt, abs_s, abs_t, n_s[:, :, None], n_t[:, :, None]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("zero", [None, "g1", "g2"])
@pytest.mark.parametrize("kind", ["ragged", "one_target_for_many", "duplicates", "single", "workload"])
def test_chamfer_nn_matches_fp64(request, device, kind, zero):
    from tpgan_amd import ops
    dev = _on(request, device)
    rng = _rng(5, len(kind))
    s, t = _chamfer_clouds(kind, rng)
    _, ri1, _, ri2 = R.chamfer_fwd(s, t)
    if kind == "one_target_for_many":
        assert (ri1 == 4).all()
    src, tgt = _t(s, dev, grad=True), _t(t, dev, grad=True)
    d1, d2, i1, i2 = ops.chamfer_nn(src, tgt)
    assert i1.dtype == torch.int64 and np.array_equal(i1.cpu().numpy(), ri1) and np.array_equal(i2.cpu().numpy(), ri2)
    assert not i1.requires_grad and not i2.requires_grad
    # the two upstream gradients differ, and one of them may be all zeros
    g1 = torch.from_numpy(rng.standard_normal(d1.shape).astype(np.float32)) * (0.0 if zero == "g1" else 1.0)
    g2 = torch.from_numpy(rng.uniform(0.5, 2.0, d2.shape).astype(np.float32)) * (0.0 if zero == "g2" else 1.0)
    sr, tr = _d(src, grad=True), _d(tgt, grad=True)
    rd1, rd2, gs, gt, abs_s, abs_t, n_s, n_t = _chamfer_ref(sr, tr, torch.from_numpy(ri1), torch.from_numpy(ri2),
                                                            g1.double(), g2.double())
    # three squares of a difference: n = 3 terms of c = 2 roundings
    _cmp_sum(d1, rd1, rd1, 3, 2, "d1")
    _cmp_sum(d2, rd2, rd2, 3, 2, "d2")
    got = torch.autograd.grad([d1, d2], [src, tgt], [g1.to(dev), g2.to(dev)], retain_graph=True)
    # terms 2 g (a - b): the difference, the product with g, the doubling and the accumulation's own rounding (c = 4)
    _cmp_sum(got[0], gs, abs_s, n_s, 4, "grad src")
    _cmp_sum(got[1], gt, abs_t, n_t, 4, "grad tgt")
    # the backward is a gather over an inverted index (no float atomics): the same bits every time
    again = torch.autograd.grad([d1, d2], [src, tgt], [g1.to(dev), g2.to(dev)])
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("reduction", ["mean", "sum", None])
@pytest.mark.parametrize("bidirectional", [True, False])
def test_losses_chamfer_distance_matches_fp64(request, device, bidirectional, reduction):
    from tpgan_amd import losses
    dev = _on(request, device)
    s, t = _chamfer_clouds("ragged", _rng(6))
    _, ri1, _, ri2 = R.chamfer_fwd(s, t)
    src, tgt = _t(s, dev, grad=True), _t(t, dev, grad=True)
    got = losses.chamfer_distance(src, tgt, bidirectional=bidirectional, reduction=reduction)
    sr, tr = _d(src, grad=True), _d(tgt, grad=True)
    want, scale = _chamfer_loss_ref(sr, tr, ri1, ri2, bidirectional, False, reduction)
    up = torch.from_numpy(_rng(7).uniform(0.5, 2.0, tuple(want.shape)).astype(np.float32))
    # a sum of N + M distances of 3 squares each
    _cmp_sum(got, want, want, s.shape[1] + t.shape[1] + 3, 2, "loss")
    gs, gt = torch.autograd.grad(got, [src, tgt], up.to(dev))
    rs, rt = torch.autograd.grad(want, [sr, tr], up.double())
    B = s.shape[0]
    g1 = (up.double() * scale).reshape(-1, 1).expand(B, s.shape[1])
    g2 = g1[:, :1].expand(B, t.shape[1]) * (1.0 if bidirectional else 0.0)
    _, _, rs2, rt2, abs_s, abs_t, n_s, n_t = _chamfer_ref(_d(src, True), _d(tgt, True), torch.from_numpy(ri1),
                                                          torch.from_numpy(ri2), g1, g2)
    assert torch.allclose(rs, rs2, rtol=1e-12, atol=0) and torch.allclose(rt, rt2, rtol=1e-12, atol=0)
    _cmp_sum(gs, rs, abs_s, n_s, 5, "grad src")          # c: the reduction's factor 1 / B on top of the 4
    _cmp_sum(gt, rt, abs_t, n_t, 5, "grad tgt")


def _chamfer_loss_ref(sr, tr, i1, i2, bidirectional, reverse, reduction):
    """chamferdist 1.0 as compat/chamferdist's docstring states it: the squared nearest-neighbour distance per point,
    summed over the points of a cloud, then `reduction` over the batch.  -> (loss, d loss / d (per-cloud sum))."""
    B, N, _ = sr.shape
    M = tr.shape[1]
    e1 = torch.as_tensor(i1)[:, :, None].expand(B, N, 3)
    e2 = torch.as_tensor(i2)[:, :, None].expand(B, M, 3)
    fwd = ((sr - torch.gather(tr, 1, e1)) ** 2).sum(2).sum(1)
    bwd = ((tr - torch.gather(sr, 1, e2)) ** 2).sum(2).sum(1)
    per_cloud = fwd + bwd if bidirectional else (bwd if reverse else fwd)
    if reduction == "mean":
        return per_cloud.mean(), 1.0 / B
    if reduction == "sum":
        return per_cloud.sum(), 1.0
    return per_cloud, 1.0


# ---------------------------------------------------------------------------------------------------------------
# 3. attach_dist_grad: differentiable distances of pytorch3d.ops.knn_points and of a radius search
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def compat():
    """The four drop-in modules, imported the way INTEGRATION.md section 1 says; gone again after this module."""
    import tpgan_amd
    saved = list(sys.path)
    ours = ("pointnet2_ops", "pytorch3d", "frnn", "chamferdist")
    assert not any(m.split(".")[0] in ours for m in sys.modules)
    cdir = tpgan_amd.install_compat()
    import chamferdist
    import frnn
    import pointnet2_ops
    import pointnet2_ops.pointnet2_utils as pn2
    import pytorch3d.ops as p3d
    for mod in (chamferdist, frnn, pointnet2_ops, pn2, p3d):
        assert mod.__file__.startswith(cdir), mod.__file__
    yield types.SimpleNamespace(pn2=pn2, p3d=p3d, frnn=frnn, chamferdist=chamferdist, pointnet2_ops=pointnet2_ops)
    sys.path[:] = saved
    for name in list(sys.modules):
        if name.split(".")[0] in ours:
            del sys.modules[name]


def _dist_ref(p1r, p2r, idx, filled, w):
    """sum_k w |p1 - p2[idx]|^2 over the filled slots; an empty slot holds a CONSTANT (include/tpgan_ops.h: "missing
    slots dist 0 / idx 0" for kNN, -1 / -1 for a radius search), so it adds nothing to either gradient -- decided
    from the header: the 0 of a (0, 0) slot is not |p1 - p2[0]|^2, it is the value 0 with index 0.
    -> (dists of the filled slots, grads, sum of the terms' magnitudes, number of terms) per element of p1 and p2."""
    B, P1, K = idx.shape
    D, P2 = p1r.shape[2], p2r.shape[1]
    safe = torch.where(filled, idx, torch.zeros_like(idx))
    e = safe.reshape(B, P1 * K, 1).expand(B, P1 * K, D)
    diff = p1r[:, :, None, :] - torch.gather(p2r, 1, e).reshape(B, P1, K, D)
    dists = (diff ** 2).sum(3) * filled
    loss = (dists * w).sum()
    a = (2 * (w * filled)[..., None] * diff).abs().detach()
    abs1 = a.sum(2)
    abs2 = torch.zeros(B, P2, D, dtype=torch.float64).scatter_add_(1, e, a.reshape(B, P1 * K, D))
    n1 = filled.double().sum(2)[:, :, None].expand(B, P1, D)
    n2 = torch.zeros(B, P2, dtype=torch.float64).scatter_add_(1, safe.reshape(B, -1), filled.double().reshape(B, -1))
    return dists, loss, abs1, abs2, n1, n2[:, :, None].expand(B, P2, D)


KNN_CASES = [
    # (B, P1, P2, D, K, lengths1, lengths2)
    (2, 40, 55, 3, 8, None, None),
    (2, 30, 44, 32, 5, None, None),
    (3, 20, 24, 3, 6, [20, 7, 1], [24, 9, 13]),           # ragged
    (2, 12, 9, 3, 16, None, None),                        # K > P2: (0, 0) slots without lengths
    (2, 12, 16, 3, 8, [12, 5], [3, 16]),                  # K > a cloud's length
    (1, 9, 6, 32, 8, [4], [6]),
    (2, 1024, 4096, 3, 32, None, None),                   # the workload's size
]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("needs", ["both", "p1", "p2"])
@pytest.mark.parametrize("B,P1,P2,D,K,len1,len2", KNN_CASES)
def test_knn_points_dists_are_differentiable(request, compat, device, B, P1, P2, D, K, len1, len2, needs):
    dev = _on(request, device)
    rng = _rng(8, B, P1, P2, D, K)
    a = rng.standard_normal((B, P1, D)).astype(np.float32)
    b = rng.standard_normal((B, P2, D)).astype(np.float32)
    l1 = None if len1 is None else np.asarray(len1, np.int64)
    l2 = None if len2 is None else np.asarray(len2, np.int64)
    rd, ri = R.knn(a, b, K, l1, l2)
    p1, p2 = _t(a, dev, grad=needs != "p2"), _t(b, dev, grad=needs != "p1")
    res = compat.p3d.knn_points(p1, p2, None if l1 is None else _t(l1, dev, dtype=torch.int64),
                                None if l2 is None else _t(l2, dev, dtype=torch.int64), K=K)
    assert res.idx.dtype == torch.int64 and np.array_equal(res.idx.cpu().numpy(), ri)
    assert np.array_equal(res.dists.detach().cpu().numpy(), rd)
    n1 = np.full(B, P1) if l1 is None else l1
    n2 = np.full(B, P2) if l2 is None else l2
    filled = torch.from_numpy((np.arange(K)[None, None, :] < n2[:, None, None]) &
                              (np.arange(P1)[None, :, None] < n1[:, None, None]))
    assert bool((torch.from_numpy(ri)[~filled] == 0).all()) and bool((torch.from_numpy(rd)[~filled] == 0).all())
    w = torch.from_numpy(rng.uniform(0.5, 2.0, (B, P1, K)).astype(np.float32))        # non-zero on the empty slots too
    p1r, p2r = _d(p1, grad=True), _d(p2, grad=True)
    dists, loss, abs1, abs2, c1, c2 = _dist_ref(p1r, p2r, torch.from_numpy(ri), filled, w.double())
    _cmp_sum(res.dists, dists, dists, D, 2, "dists")
    leaves, refs = [], []
    if needs != "p2":
        leaves.append(p1); refs.append((p1r, abs1, c1, "grad p1"))
    if needs != "p1":
        leaves.append(p2); refs.append((p2r, abs2, c2, "grad p2"))
    got = torch.autograd.grad((res.dists * w.to(dev)).sum(), leaves)
    want = torch.autograd.grad(loss, [r[0] for r in refs])
    for g, wnt, (_, absum, n, what) in zip(got, want, refs):
        _cmp_sum(g, wnt, absum, n, 4, what)         # 2 w (a - b): difference, 2 w, product, + the sum's own (c = 4)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("D,K", [(3, 8), (32, 4), (3, 40)])
def test_knn_points_in_itself_sums_both_terms(request, compat, device, D, K):
    """p2 is p1: ONE tensor receives the query term and the neighbour term."""
    dev = _on(request, device)
    rng = _rng(9, D, K)
    B, P = 2, 33
    a = rng.standard_normal((B, P, D)).astype(np.float32)
    rd, ri = R.knn(a, a, K)
    p = _t(a, dev, grad=True)
    dists, idx, _ = compat.p3d.knn_points(p, p, K=K)
    assert np.array_equal(idx.cpu().numpy(), ri)
    filled = torch.from_numpy(np.broadcast_to(np.arange(K)[None, None, :] < P, (B, P, K)).copy())
    w = torch.from_numpy(rng.uniform(0.5, 2.0, (B, P, K)).astype(np.float32))
    pr = _d(p, grad=True)
    _, loss, abs1, abs2, c1, c2 = _dist_ref(pr, pr, torch.from_numpy(ri), filled, w.double())
    (got,) = torch.autograd.grad((dists * w.to(dev)).sum(), [p])
    (want,) = torch.autograd.grad(loss, [pr])
    _cmp_sum(got, want, abs1 + abs2, c1 + c2 + 1, 4, "grad p")       # + 1: the two terms are added by autograd


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("needs", ["both", "p1", "p2"])
@pytest.mark.parametrize("B,P1,P2,K,r,len1,len2", [(2, 50, 70, 8, 0.35, None, None), (2, 50, 70, 8, 0.35, [50, 11], [9, 70]),
                                                   (1, 10, 10, 4, 1e-3, None, None), (2, 512, 2048, 16, 0.08, None, None)])
def test_radius_search_dists_are_differentiable(request, compat, device, B, P1, P2, K, r, len1, len2, needs):
    """-1 slots contribute nothing to either gradient (frnn's dists are -1 there, a constant)."""
    from tpgan_amd import ops
    dev = _on(request, device)
    rng = _rng(10, B, P1, P2, K)
    a = rng.uniform(-0.5, 0.5, (B, P1, 3)).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, (B, P2, 3)).astype(np.float32)
    l1 = None if len1 is None else np.asarray(len1, np.int64)
    l2 = None if len2 is None else np.asarray(len2, np.int64)
    rd, ri = R.knn(a, b, K, l1, l2, r)
    assert (ri < 0).any()
    p1, p2 = _t(a, dev, grad=needs != "p2"), _t(b, dev, grad=needs != "p1")
    t1 = None if l1 is None else _t(l1, dev, dtype=torch.int64)
    t2 = None if l2 is None else _t(l2, dev, dtype=torch.int64)
    d, i, nn, grid = compat.frnn.frnn_grid_points(p1, p2, t1, t2, K=K, r=r)
    assert np.array_equal(i.cpu().numpy(), ri) and np.array_equal(d.cpu().numpy(), rd)
    dists = ops.attach_dist_grad(p1, p2, d, i, t1, t2)
    filled = torch.from_numpy(ri >= 0)
    w = torch.from_numpy(rng.uniform(0.5, 2.0, (B, P1, K)).astype(np.float32))
    p1r, p2r = _d(p1, grad=True), _d(p2, grad=True)
    ref, loss, abs1, abs2, c1, c2 = _dist_ref(p1r, p2r, torch.from_numpy(ri), filled, w.double())
    _exact(dists, torch.from_numpy(rd), "values pass through")
    _cmp_sum(torch.where(filled.to(dev), dists, torch.zeros_like(dists)), ref, ref, 3, 2, "dists")
    leaves = ([p1] if needs != "p2" else []) + ([p2] if needs != "p1" else [])
    refs = ([(p1r, abs1, c1)] if needs != "p2" else []) + ([(p2r, abs2, c2)] if needs != "p1" else [])
    got = torch.autograd.grad((dists * w.to(dev)).sum(), leaves)
    want = torch.autograd.grad(loss, [x[0] for x in refs])
    for g, wnt, (_, absum, n) in zip(got, want, refs):
        _cmp_sum(g, wnt, absum, n, 4, "grad")


# ---------------------------------------------------------------------------------------------------------------
# 4. spectral_normalize / spectral_normalize_many
# ---------------------------------------------------------------------------------------------------------------
def _sn_ref(W64, u, v, training, eps=1e-12):
    """oracle/ref_ops.py and include/tpgan_ops.h: in training mode v <- normalise(W^T u) FIRST, then u <- normalise(W v)
    with the new v, then sigma = u . W v with both new vectors; the result is W / sigma with u and v CONSTANTS of the
    differentiation (torch.nn.utils.spectral_norm's forward pre-hook, one power iteration)."""
    with torch.no_grad():
        if training:
            t = W64.t() @ u
            v = t / t.norm().clamp_min(eps)
            s = W64 @ v
            u = s / s.norm().clamp_min(eps)
    sigma = u @ (W64 @ v)
    return W64 / sigma, u, v


def _sn_inputs(rng, R_, Cn):
    W = rng.standard_normal((R_, Cn)).astype(np.float32)
    u = rng.standard_normal(R_).astype(np.float32)
    v = rng.standard_normal(Cn).astype(np.float32)
    return W, u / np.linalg.norm(u), v / np.linalg.norm(v)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("R_,Cn", [(64, 6), (128, 131), (256, 515), (256, 259), (1, 64), (64, 256)])
def test_spectral_normalize_matches_fp64(request, device, R_, Cn, training):
    from tpgan_amd import ops
    dev = _on(request, device)
    rng = _rng(11, R_, Cn)
    W, u, v = _sn_inputs(rng, R_, Cn)
    shape = (R_, Cn // 3, 3) if Cn % 3 == 0 else (R_, Cn)            # a conv weight: flattened behind the first axis
    Wd, ud, vd = _t(W.reshape(shape), dev, grad=True), _t(u, dev), _t(v, dev)
    out = ops.spectral_normalize(Wd, ud, vd, training)
    assert out.shape == shape
    Wr = _d(Wd.reshape(R_, Cn), grad=True)
    ref, ur, vr = _sn_ref(Wr, torch.from_numpy(u).double(), torch.from_numpy(v).double(), training)
    _cmp_tol(out.reshape(R_, Cn), ref, "W / sigma")
    _cmp_tol(ud, ur, "u")
    _cmp_tol(vd, vr, "v")
    if not training:
        assert np.array_equal(ud.cpu().numpy(), u) and np.array_equal(vd.cpu().numpy(), v)
    G = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    (got,) = torch.autograd.grad(out, Wd, G.to(dev))
    (want,) = torch.autograd.grad(ref, Wr, G.double().reshape(R_, Cn))
    _cmp_tol(got.reshape(R_, Cn), want, "grad W")


class _SNModule:
    def __init__(self, W, u, v, dev):
        self.weight_orig, self.weight_u, self.weight_v = _t(W, dev, grad=True), _t(u, dev), _t(v, dev)


# on the GPU both routes of the batched forward: rows of a weight over several workgroups, and one workgroup per weight
SN_ROUTES = [("cpu", None), pytest.param("cuda", "split", marks=pytest.mark.gpu),
             pytest.param("cuda", "one", marks=pytest.mark.gpu)]


@pytest.mark.parametrize("device,route", SN_ROUTES)
@pytest.mark.parametrize("training", [True, False])
def test_spectral_normalize_many_matches_fp64(request, device, route, training):
    """A weight used several times in one forward: each use is one more power iteration from the previous use's
    vectors, and the weight's gradient is the sum over its uses (every use with its own upstream gradient)."""
    from tpgan_amd import ops
    dev = _on(request, device)
    rng = _rng(12)
    shapes, uses = [(64, 6), (256, 515), (128, 131), (1, 64)], [2, 3, 1, 2]
    inputs = [_sn_inputs(rng, *s) for s in shapes]
    mods = [_SNModule(W, u, v, dev) for W, u, v in inputs]
    be = ops.backend_for(mods[0].weight_orig)
    prev = ops.SN_SPLIT[0]
    try:
        if route is not None:                   # the switch is read when a plan is made
            ops.SN_SPLIT[0] = route == "split"
            be._sn_plans.clear()
        outs = ops.spectral_normalize_many(mods, uses, training)
        if route is not None:
            plan = next(iter(be._sn_plans.values()))
            assert (plan["split"] is not None) == (route == "split")
        Gs = [[torch.from_numpy(rng.standard_normal(s).astype(np.float32)) for _ in range(k)] for s, k in zip(shapes, uses)]
        flat_out = [o for per in outs for o in per]
        flat_g = [g.to(dev) for per in Gs for g in per]
        got = torch.autograd.grad(flat_out, [m.weight_orig for m in mods], flat_g)
    finally:
        ops.SN_SPLIT[0] = prev
        if route is not None:
            be._sn_plans.clear()
    for m, (W, u, v), k, per, gs, g in zip(mods, inputs, uses, outs, Gs, got):
        assert len(per) == k
        Wr = torch.from_numpy(W).double().requires_grad_(True)
        ur, vr = torch.from_numpy(u).double(), torch.from_numpy(v).double()
        total = 0.0
        for o, G in zip(per, gs):
            ref, ur, vr = _sn_ref(Wr, ur, vr, training)
            _cmp_tol(o, ref, "W / sigma")
            total = total + (ref * G.double()).sum()
        (want,) = torch.autograd.grad(total, Wr)
        _cmp_tol(g, want, "grad W")
        _cmp_tol(m.weight_u, ur, "u")
        _cmp_tol(m.weight_v, vr, "v")


# ---------------------------------------------------------------------------------------------------------------
# 5. row_bn_act / row_act_max
# ---------------------------------------------------------------------------------------------------------------
def _bn_ref(x, gamma, beta, mode, nseg, eps, rm, rv, shift, momentum):
    """BatchNorm over rows, fp64.  mode "train": batch statistics (biased variance) per segment of equal consecutive
    rows; running statistics updated segment after segment with the UNBIASED variance, `shift` entering the running
    mean only.  mode "eval": the running statistics, the mean less `shift` (x lacks that constant).  mode "identity":
    no statistics.  -> (z, new running mean, new running variance)."""
    C = x.shape[1]
    g = torch.ones(C, dtype=torch.float64) if gamma is None else gamma
    b = torch.zeros(C, dtype=torch.float64) if beta is None else beta
    if mode == "identity":
        return x * g + b, rm, rv
    if mode == "eval":
        mean = rm if shift is None else rm - shift
        return (x - mean) / torch.sqrt(rv + eps) * g + b, rm, rv
    zs = []
    for xs in x.chunk(nseg, 0):
        Ps = xs.shape[0]
        mean, var = xs.mean(0), xs.var(0, unbiased=False)
        zs.append((xs - mean) / torch.sqrt(var + eps) * g + b)
        if rm is not None:
            with torch.no_grad():
                rm = (1 - momentum) * rm + momentum * (mean + (0 if shift is None else shift))
                rv = (1 - momentum) * rv + momentum * var * Ps / (Ps - 1)
    return torch.cat(zs, 0), rm, rv


def _conditioned(x, zfn, slope, K, rnd):
    """Nudge x (values kept representable: `rnd`) until no pre-activation zfn(x) lies within 2e-4 of the kink and, with
    K, the two largest activations of every (group, channel) are 2e-3 of the scale apart; the test asserts the halves
    of these margins on its reference."""
    for _ in range(200):
        z = zfn(x.double())
        near = (z.abs() < 2e-4) & (slope != 1.0)
        if K:
            a = _lrelu(z, slope).reshape(-1, K, z.shape[1])
            top = a.topk(min(2, K), dim=1)
            if K > 1:
                close = (top.values[:, 0] - top.values[:, 1]) < 2e-3 * a.abs().max()
                bump = torch.zeros_like(a, dtype=torch.bool).scatter_(1, top.indices[:, :1], close[:, None])
                near = near | bump.reshape(z.shape)
        if not bool(near.any()):
            return x
        # away from the kink on the side z is on; the largest of a near-tie upwards (gamma > 0 in every case here)
        step = 0.03 * (x.double().abs() + 0.05)
        if K > 1:
            step = step * torch.where(bump.reshape(z.shape) | (z >= 0), 1.0, -1.0)
        else:
            step = step * torch.where(z >= 0, 1.0, -1.0)
        x = rnd(torch.where(near, x.double() + step, x.double()))
    raise AssertionError("could not condition the input")


def _assert_conditioned(z, slope, K):
    """On the fp64 reference alone: a bad seed fails here, loudly."""
    if slope != 1.0:
        assert float(z.abs().min()) >= 1e-4, "a pre-activation within 1e-4 of the LeakyReLU kink"
    if K > 1:
        a = _lrelu(z, slope).reshape(-1, K, z.shape[1])
        top = a.topk(2, dim=1).values
        assert float((top[:, 0] - top[:, 1]).min()) >= 1e-3 * float(a.abs().max()), "near-tie under the max over K"


def _stored_y_allowance(z, g, x, gamma, beta, base, nseg, K, slope, eps):
    """With K > 0 and a bf16 output, the backward's reduction takes the arg-max row's pre-activation from the STORED
    output (csrc/rowbn.hip, rowbn_bwd_reduce_max_kernel: z = y > 0 ? y : y / slope, xhat = (z - beta) / gamma) instead of
    gathering x: y went through one rounding to bf16, so z is off by up to 2^-8 |z| (oracle.ref_ops.BF16_REL) and xhat by
    that over |gamma|.  Propagated in fp64 through the formulas the reduction feeds, per segment s of Ps rows:
        dgamma = sum g' xhat                      -> E_s = 2^-8 sum_groups |g'| |z| / |gamma|, summed over the segments
        dx     = gamma rstd (g' - c1 - xhat c2)   -> |gamma rstd xhat| E_s / Ps      (training statistics only)
    This is on top of TOL and the output's own bf16 ulp.  Without it the case train / nseg 3 / K 4 / 96 x 16 / bf16 missed
    on the MI355X: |dx - ref| up to 7.3e-3 at max|ref| = 3.66 (a segment has 8 groups: the roundings do not average
    out), which is 2^-9 of the largest value and inside this allowance.  No gamma: nothing is reduced, no allowance."""
    if gamma is None:
        return {}
    P, C = z.shape
    G = P // K
    zk = z.reshape(G, K, C)
    top = _lrelu(zk, slope).argmax(1, keepdim=True)
    zmax = zk.gather(1, top)[:, 0]
    gg = g * torch.where(zmax > 0, 1.0, slope)
    e_seg = (2.0 ** -8 * gg.abs() * zmax.abs() / gamma.double().abs()).reshape(nseg, G // nseg, C).sum(1)     # (nseg, C)
    out = {"dgamma": e_seg.sum(0)}
    if base == "train":
        Ps = P // nseg
        rstd = torch.stack([1.0 / torch.sqrt(xs.var(0, unbiased=False) + eps) for xs in x.chunk(nseg, 0)])    # (nseg, C)
        per_row = (rstd * e_seg / Ps).repeat_interleave(Ps, 0)
        out["dx"] = (z - beta.double()).abs() * per_row
    return out


_F32, _BF16 = torch.float32, torch.bfloat16

ROWBN_CASES = [
    # (mode, nseg, K, P, C, slope, affine, x dtype, out dtype, upstream, who needs grad)
    ("train", 1, 0, 96, 8, 0.2, True, _F32, _F32, "random", "all"),
    ("train", 3, 0, 96, 16, 0.2, True, _F32, _F32, "random", "all"),
    ("train", 1, 4, 96, 8, 0.2, True, _F32, _F32, "random", "all"),
    ("train", 3, 8, 192, 16, 0.0, True, _F32, _F32, "random", "all"),
    ("train", 1, 0, 64, 8, 1.0, True, _F32, _F32, "random", "all"),
    ("train", 1, 0, 64, 8, 0.2, True, _F32, _F32, "expanded", "all"),
    ("train", 1, 0, 64, 8, 0.2, False, _F32, _F32, "random", "all"),
    ("train", 1, 16, 2048, 64, 0.2, True, _F32, _F32, "transposed", "all"),
    ("train", 1, 0, 96, 8, 0.2, True, _F32, _F32, "random", "x"),           # gamma / beta without requires_grad
    ("train", 1, 4, 96, 8, 0.2, True, _F32, _F32, "random", "affine"),      # x without requires_grad
    ("train", 1, 0, 96, 8, 0.2, True, _F32, _BF16, "bf16", "all"),
    ("train", 3, 4, 96, 16, 0.2, True, _BF16, _BF16, "bf16", "all"),
    ("train", 1, 32, 8 * 1024 * 32 // 8, 128, 0.2, True, _BF16, _BF16, "bf16", "all"),     # a set-abstraction tail
    ("eval", 1, 0, 96, 8, 0.2, True, _F32, _F32, "random", "all"),
    ("eval", 1, 4, 96, 8, 0.2, True, _F32, _F32, "transposed", "all"),
    ("eval_shift", 1, 0, 96, 8, 0.2, True, _F32, _F32, "random", "all"),
    ("eval_shift", 1, 4, 96, 16, 0.2, True, _BF16, _BF16, "bf16", "all"),
    ("train_shift", 3, 0, 96, 8, 0.2, True, _F32, _F32, "random", "all"),
    ("identity", 1, 0, 96, 8, 0.2, False, _F32, _F32, "random", "x"),
    ("identity", 1, 20, 640, 128, 0.2, False, _F32, _F32, "random", "x"),                 # row_act_max
    ("identity", 1, 4, 96, 16, 0.2, False, _F32, _BF16, "bf16", "x"),
]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("mode,nseg,K,P,C,slope,affine,xdt,odt,upstream,needs", ROWBN_CASES)
def test_row_bn_act_matches_fp64(request, device, mode, nseg, K, P, C, slope, affine, xdt, odt, upstream, needs):
    from tpgan_amd import ops
    dev = _on(request, device)
    rng = _rng(13, nseg, K, P, C, len(mode))
    eps, momentum = 1e-5, 0.1
    shifted = mode.endswith("_shift")
    base = mode.split("_")[0]
    gamma = torch.from_numpy(rng.uniform(0.5, 1.5, C).astype(np.float32)) if affine else None
    beta = torch.from_numpy((0.3 * rng.standard_normal(C)).astype(np.float32)) if affine else None
    rm0 = torch.from_numpy((0.2 * rng.standard_normal(C)).astype(np.float32)) if base != "identity" else None
    rv0 = torch.from_numpy(rng.uniform(0.5, 2.0, C).astype(np.float32)) if base != "identity" else None
    shift = torch.from_numpy((0.5 * rng.standard_normal(C)).astype(np.float32)) if shifted else None
    d64 = lambda t: None if t is None else t.double()
    rnd = (lambda t: t.to(xdt).double())
    x0 = rnd(torch.from_numpy(rng.standard_normal((P, C)) * rng.uniform(0.5, 2.0, C) + rng.standard_normal(C)))
    zfn = lambda xx: _bn_ref(xx, d64(gamma), d64(beta), base, nseg, eps, d64(rm0), d64(rv0), d64(shift), momentum)[0]
    x0 = _conditioned(x0, zfn, slope, K, rnd)
    # ---- the reference, and the conditions on it
    xr = x0.clone().requires_grad_(True)
    gr = None if gamma is None else gamma.double().requires_grad_(True)
    br = None if beta is None else beta.double().requires_grad_(True)
    z, rm_ref, rv_ref = _bn_ref(xr, gr, br, base, nseg, eps, d64(rm0), d64(rv0), d64(shift), momentum)
    _assert_conditioned(z.detach(), slope, K)
    ref = _lrelu(z, slope)
    if K:
        ref = ref.reshape(P // K, K, C).max(1).values
    # ---- the op
    x = _t(x0, dev, grad=needs != "affine", dtype=xdt)
    g_ = None if gamma is None else _t(gamma, dev, grad=needs != "x")
    b_ = None if beta is None else _t(beta, dev, grad=needs != "x")
    rm, rv = (None, None) if rm0 is None else (_t(rm0, dev), _t(rv0, dev))
    nbt = torch.tensor(5, dtype=torch.int64, device=dev)
    sh = None if shift is None else _t(shift, dev)
    if base == "identity" and K:
        y = ops.row_act_max(x, slope, K, odt)
    else:
        y = ops.row_bn_act(x, g_, b_, rm, rv, base == "train", momentum, eps, slope, K, odt, nbt, nseg, sh)
    assert y.dtype == odt and y.shape == ref.shape
    _cmp_tol(y, ref, "y", bf16=odt == _BF16)
    # running statistics and the counter
    if base == "train":
        _cmp_tol(rm, rm_ref, "running mean")
        _cmp_tol(rv, rv_ref, "running var")
        assert int(nbt) == 5 + nseg
    else:
        assert int(nbt) == 5
        if rm is not None:
            assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0)
    # ---- gradients
    g, g64 = _upstream(upstream, tuple(ref.shape), _rng(14, P, C))
    if g is not None and g.dtype != odt:
        g = g.to(odt)
        g64 = g.double()
    leaves = ([x] if needs != "affine" else []) + ([g_, b_] if (affine and needs != "x") else [])
    refs = ([xr] if needs != "affine" else []) + ([gr, br] if (affine and needs != "x") else [])
    names = (["dx"] if needs != "affine" else []) + (["dgamma", "dbeta"] if (affine and needs != "x") else [])
    got = _backward(y, leaves, g, dev)
    want = torch.autograd.grad(ref, refs, g64)
    extra = _stored_y_allowance(z.detach(), g64, x0, gamma, beta, base, nseg, K, slope, eps) if (K and odt == _BF16) else {}
    for a, w, name in zip(got, want, names):
        assert a.dtype == (xdt if name == "dx" else _F32)
        _cmp_tol(a, w, name, bf16=(name == "dx" and xdt == _BF16), extra=extra.get(name))
    if affine and needs == "x":
        assert g_.grad is None and b_.grad is None


# ---------------------------------------------------------------------------------------------------------------
# 6. row_combine (GATHER / SUB / EDGE) and head_bn_act
# ---------------------------------------------------------------------------------------------------------------
def _spread(rng, B, N, C, dtype):
    """Rows whose every channel differs by >= 2^-5 between any two rows of a cloud (values exact in bf16 up to
    N = 256): the EDGE mode's LeakyReLU never sees a difference near its kink."""
    perm = np.stack([np.stack([rng.permutation(N) for _ in range(C)], 1) for _ in range(B)])
    return torch.from_numpy((perm - N // 2) * 2.0 ** -5).to(dtype)


# prepared inverse: GPU only (the oracle backend has no invert_index; NeighbourList.with_inverse is a no-op there)
RC_DEVICES = [("cpu", False), pytest.param("cuda", False, marks=pytest.mark.gpu),
              pytest.param("cuda", True, marks=pytest.mark.gpu)]


@pytest.mark.parametrize("device,inverse", RC_DEVICES)
@pytest.mark.parametrize("q_grad", [True, False])
@pytest.mark.parametrize("idt,odt,upstream", [(_F32, _F32, "random"), (_F32, _F32, "expanded"), (_F32, _F32, "transposed"),
                                              (_F32, _BF16, "bf16"), (_BF16, _BF16, "bf16")])
@pytest.mark.parametrize("mode,B,N,S,K,C", [("GATHER", 2, 40, 13, 5, 8), ("SUB", 2, 40, 13, 5, 8), ("EDGE", 2, 40, 40, 5, 8),
                                            ("GATHER", 1, 7, 1, 1, 16), ("SUB", 2, 1024, 256, 32, 64),
                                            ("EDGE", 2, 256, 256, 20, 64), ("SUB", 1, 9, 6, 4, 8)])
def test_row_combine_matches_fp64(request, device, inverse, mode, B, N, S, K, C, idt, odt, upstream, q_grad):
    from tpgan_amd import ops
    dev = _on(request, device)
    rng = _rng(15, B, N, S, K, C, len(mode))
    slope = 0.2
    idx = rng.integers(0, N, (B, S, K)).astype(np.int32)
    if (N, S) == (9, 6):
        idx[:] = 3                                        # one source row hit by every slot
    if mode == "EDGE":                                    # no self edges: QE[idx] - QE[s] = 0 sits ON the kink
        idx = np.where(idx == np.arange(S)[None, :, None], (idx + 1) % N, idx).astype(np.int32)
    U0 = torch.from_numpy(rng.standard_normal((B, N, C))).to(idt)
    Q0 = None if mode == "GATHER" else (_spread(rng, B, N, C, idt) if mode == "EDGE"
                                        else torch.from_numpy(rng.standard_normal((B, S, C))).to(idt))
    U = _t(U0, dev, grad=True, dtype=idt)
    Q = None if Q0 is None else _t(Q0, dev, grad=q_grad, dtype=idt)
    it = _t(idx, dev, dtype=torch.int32)
    nl = ops.attach_inverse(it, N) if inverse else it
    if inverse:
        assert nl.inverse is not None
    out = ops.row_combine(U, Q, nl, getattr(ops, "ROW_" + mode), slope, odt)
    # ---- the fp64 statement (include/tpgan_ops.h): U[idx] | U[idx] - QE[s] | U[idx] + lrelu(QE[idx] - QE[s])
    Ur, Qr = _d(U, grad=True), (None if Q is None else _d(Q, grad=True))
    e = torch.from_numpy(idx).long().reshape(B, S * K, 1).expand(B, S * K, C)
    pick = lambda t: torch.gather(t, 1, e).reshape(B, S, K, C)
    if mode == "GATHER":
        ref, mag, n, c = pick(Ur), pick(Ur).abs(), 1, 0
    elif mode == "SUB":
        ref, mag, n, c = pick(Ur) - Qr[:, :, None], pick(Ur).abs() + Qr[:, :, None].abs(), 2, 0
    else:
        diff = pick(Qr) - Qr[:, :, None]
        assert float(diff.detach().abs().min()) >= 1e-4
        ref = pick(Ur) + _lrelu(diff, slope)
        mag, n, c = pick(Ur).abs() + pick(Qr).abs() + Qr[:, :, None].abs(), 3, 1       # c: the slope's product
    assert out.dtype == odt and out.shape == ref.shape
    if mode == "GATHER" and idt == odt:
        _exact(out, ref, "forward")
    else:
        _cmp_sum(out, ref, mag, n, c, "forward", bf16=odt == _BF16)
    g, g64 = _upstream(upstream, tuple(ref.shape), _rng(16, B, S, K, C))
    if g is not None and g.dtype != odt:
        g = g.to(odt)
        g64 = g.double()
    leaves = [U] + ([Q] if (Q is not None and q_grad) else [])
    refs = [Ur] + ([Qr] if (Q is not None and q_grad) else [])
    want = torch.autograd.grad(ref, refs, g64, retain_graph=True)
    absum = [a.abs() for a in torch.autograd.grad(ref if mode != "EDGE" else pick(Ur) + pick(Qr) + Qr[:, :, None], refs,
                                                  g64.abs())]
    # number of terms per element: the slots that hit a source row (U), the K slots of a centre (QE), both for EDGE
    hits = torch.zeros(B, N, dtype=torch.float64).scatter_add_(1, torch.from_numpy(idx).long().reshape(B, -1),
                                                               torch.ones(B, S * K, dtype=torch.float64))[:, :, None]
    counts = [hits] + ([K if mode == "SUB" else hits + K] if len(refs) == 2 else [])
    got = _backward(out, leaves, g, dev)
    for a, w, s_, n_, name in zip(got, want, absum, counts, ["grad U", "grad QE"]):
        assert a.dtype == idt
        _cmp_sum(a, w, s_, n_, 1, name, bf16=idt == _BF16)        # c = 1: the slope's product (EDGE), 0 otherwise
    if Q is not None and not q_grad:
        assert Q.grad is None
    # the backward gathers over the inverted index in a fixed order: the same bits every time
    again = _backward(out, leaves, g, dev)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def _head_ref(h, gamma, beta, eps, slope, mask):
    B = h.shape[0]
    mean, var = h.mean(0), h.var(0, unbiased=False)
    z = (h - mean) / torch.sqrt(var + eps)
    if gamma is not None:
        z = z * gamma + beta
    y = _lrelu(z, slope)
    return z, (y if mask is None else y * mask), mean, var * B / (B - 1)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("upstream", ["random", "expanded", "transposed"])
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("B,C", [(2, 16), (16, 64), (8, 256)])
def test_head_bn_act_matches_fp64(request, device, B, C, masked, affine, upstream):
    from tpgan_amd import ops
    dev = _on(request, device)
    rng = _rng(17, B, C, int(masked), int(affine))
    slope = 0.2
    bn = torch.nn.BatchNorm1d(C, affine=affine)
    with torch.no_grad():
        bn.running_mean.copy_(torch.from_numpy(0.2 * rng.standard_normal(C)))
        bn.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 2.0, C)))
        if affine:
            bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, C)))
            bn.bias.copy_(torch.from_numpy(0.3 * rng.standard_normal(C)))
    rm0, rv0 = bn.running_mean.clone().double(), bn.running_var.clone().double()
    gam, bet = (bn.weight.detach().double(), bn.bias.detach().double()) if affine else (None, None)
    bn = bn.to(dev)
    mask = torch.from_numpy(((rng.uniform(size=(B, C)) < 0.7) / 0.7).astype(np.float32)) if masked else None
    rnd = lambda t: t.float().double()
    hraw = rng.standard_normal((B, C)) + rng.standard_normal(C)
    if B == 2:
        # two rows: rstd = 2 / |h0 - h1| multiplies every rounding of the backward, so the rows are kept 0.5 .. 2 apart
        # per channel (a well-conditioned problem: the bound is about the kernel, not about dividing by nearly nothing)
        gap = rng.uniform(0.5, 2.0, C) * rng.choice([-1.0, 1.0], C)
        hraw = np.stack([hraw[0] + gap / 2, hraw[0] - gap / 2])
    h0 = _conditioned(rnd(torch.from_numpy(hraw)),
                      lambda hh: _head_ref(hh, gam, bet, bn.eps, slope, None)[0], slope, 0, rnd)
    hr = h0.clone().requires_grad_(True)
    gr, br = (gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)) if affine else (None, None)
    z, ref, mean, uvar = _head_ref(hr, gr, br, bn.eps, slope, None if mask is None else mask.double())
    _assert_conditioned(z.detach(), slope, 0)
    h = _t(h0, dev, grad=True)
    y = ops.head_bn_act(h, bn, slope, None if mask is None else mask.to(dev))
    _cmp_tol(y, ref, "y")
    _cmp_tol(bn.running_mean, (1 - bn.momentum) * rm0 + bn.momentum * mean.detach(), "running mean")
    _cmp_tol(bn.running_var, (1 - bn.momentum) * rv0 + bn.momentum * uvar.detach(), "running var")
    assert int(bn.num_batches_tracked) == 1
    g, g64 = _upstream(upstream, tuple(ref.shape), _rng(18, B, C))
    leaves = [h] + ([bn.weight, bn.bias] if affine else [])
    got = _backward(y, leaves, g, dev)
    want = torch.autograd.grad(ref, [hr] + ([gr, br] if affine else []), g64)
    for a, w, name in zip(got, want, ["dh", "dgamma", "dbeta"]):
        _cmp_tol(a, w, name)


# ---------------------------------------------------------------------------------------------------------------
# 7. the drop-in modules
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", DEVICES)
def test_knn_points_contract(request, compat, device):
    dev = _on(request, device)
    rng = _rng(19)
    B, P1, P2, D, K = 3, 10, 12, 3, 6
    a, b = rng.standard_normal((B, P1, D)).astype(np.float32), rng.standard_normal((B, P2, D)).astype(np.float32)
    l2 = np.asarray([12, 4, 1], np.int64)
    p1, p2 = _t(a, dev), _t(b, dev)
    res = compat.p3d.knn_points(p1, p2, None, _t(l2, dev, dtype=torch.int64), K, -1, True, True)    # positional order
    assert type(res).__name__ == "KNN" and res._fields == ("dists", "idx", "knn")
    dists, idx, nn = res
    assert dists is res.dists and idx is res.idx and nn is res.knn
    assert idx.dtype == torch.int64 and dists.dtype == torch.float32 and dists.shape == idx.shape == (B, P1, K)
    rd, ri = R.knn(a, b, K, None, l2)
    assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(dists.cpu().numpy(), rd)
    # return_nn: p2[idx], zero in the slots beyond lengths2
    want = np.take_along_axis(b[:, None], ri[..., None].repeat(D, 3).reshape(B, P1 * K, D)[:, None], 2).reshape(B, P1, K, D)
    want = want * (np.arange(K)[None, None, :, None] < l2[:, None, None, None])
    assert nn.shape == (B, P1, K, D) and np.array_equal(nn.cpu().numpy(), want.astype(np.float32))
    # without lengths, K > P2: the empty slots are zero too; return_nn defaults to None, `version` / `return_sorted` accepted
    res2 = compat.p3d.knn_points(p1, p2, K=P2 + 3, version=2, return_nn=True, return_sorted=False)
    assert bool((res2.knn[:, :, P2:] == 0).all()) and bool((res2.idx[:, :, P2:] == 0).all())
    assert torch.equal(res2.knn[:, :, :P2], compat.p3d.knn_gather(p2, res2.idx)[:, :, :P2])
    assert compat.p3d.knn_points(p1, p2, K=2).knn is None
    with pytest.raises(ValueError):
        compat.p3d.knn_points(p1, p2[:2], K=2)
    with pytest.raises(ValueError):
        compat.p3d.knn_points(p1, _t(rng.standard_normal((B, P2, 4)).astype(np.float32), dev), K=2)


@pytest.mark.parametrize("device", DEVICES)
def test_frnn_grid_points_contract(request, compat, device):
    dev = _on(request, device)
    rng = _rng(20)
    B, P1, P2, K, r = 2, 30, 40, 8, 0.3
    a, b = rng.uniform(-0.5, 0.5, (B, P1, 3)).astype(np.float32), rng.uniform(-0.5, 0.5, (B, P2, 3)).astype(np.float32)
    p1, p2 = _t(a, dev), _t(b, dev)
    res = compat.frnn.frnn_grid_points(p1, p2, None, None, K, torch.tensor([r]), None, True, True, 2.0)
    assert isinstance(res, tuple) and len(res) == 4 and res[3] is None
    dists, idxs, nn, grid = res
    rd, ri = R.knn(a, b, K, None, None, r)
    assert idxs.dtype == torch.int64 and np.array_equal(idxs.cpu().numpy(), ri) and np.array_equal(dists.cpu().numpy(), rd)
    miss = ri < 0
    assert miss.any() and (~miss).any() and (rd[miss] == -1).all()
    want = np.where(miss[..., None], 0.0, np.take_along_axis(b, np.maximum(ri, 0).reshape(B, -1, 1).repeat(3, 2), 1)
                    .reshape(B, P1, K, 3)).astype(np.float32)
    assert np.array_equal(nn.cpu().numpy(), want)
    assert np.array_equal(compat.frnn.frnn_gather(p2, idxs).cpu().numpy(), want)
    assert compat.frnn.frnn_grid_points(p1, p2, K=K, r=r)[2] is None
    for bad in (dict(K=0, r=r), dict(K=65, r=r), dict(K=K, r=0.0), dict(K=K, r=-1.0), dict(K=K, r=torch.tensor([0.1, 0.2]))):
        with pytest.raises(ValueError):
            compat.frnn.frnn_grid_points(p1, p2, **bad)
    with pytest.raises(ValueError):
        compat.frnn.frnn_grid_points(p1, p2[:1], K=K, r=r)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("reduction", ["mean", "sum", None])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("bidirectional", [False, True])
def test_chamfer_distance_module_matches_fp64(request, compat, device, bidirectional, reverse, reduction):
    dev = _on(request, device)
    s, t = _chamfer_clouds("ragged", _rng(21))
    _, ri1, _, ri2 = R.chamfer_fwd(s, t)
    src, tgt = _t(s, dev, grad=True), _t(t, dev, grad=True)
    cd = compat.chamferdist.ChamferDistance()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = cd(src, tgt, bidirectional, reverse, reduction)               # positional order of chamferdist 1.0
    assert (len(caught) == 1) == (bidirectional and reverse)
    sr, tr = _d(src, grad=True), _d(tgt, grad=True)
    want, scale = _chamfer_loss_ref(sr, tr, ri1, ri2, bidirectional, reverse, reduction)
    assert got.shape == want.shape
    _cmp_sum(got, want, want, s.shape[1] + t.shape[1] + 3, 2, "loss")
    up = torch.from_numpy(_rng(22).uniform(0.5, 2.0, tuple(want.shape)).astype(np.float32))
    gs, gt = torch.autograd.grad(got, [src, tgt], up.to(dev))
    rs, rt = torch.autograd.grad(want, [sr, tr], up.double())
    B = s.shape[0]
    per = (up.double() * scale).reshape(-1, 1).expand(B, 1)
    g1 = per.expand(B, s.shape[1]) * (1.0 if (bidirectional or not reverse) else 0.0)
    g2 = per.expand(B, t.shape[1]) * (1.0 if (bidirectional or reverse) else 0.0)
    _, _, rs2, rt2, abs_s, abs_t, n_s, n_t = _chamfer_ref(_d(src, True), _d(tgt, True), torch.from_numpy(ri1),
                                                          torch.from_numpy(ri2), g1, g2)
    assert torch.allclose(rs, rs2, rtol=1e-12, atol=0) and torch.allclose(rt, rt2, rtol=1e-12, atol=0)
    _cmp_sum(gs, rs, abs_s, n_s, 5, "grad src")
    _cmp_sum(gt, rt, abs_t, n_t, 5, "grad tgt")


@pytest.mark.parametrize("device", DEVICES)
def test_chamfer_distance_module_exceptions(request, compat, device):
    dev = _on(request, device)
    cd = compat.chamferdist.ChamferDistance()
    a, b = torch.zeros(2, 5, 3, device=dev), torch.zeros(2, 6, 3, device=dev)
    with pytest.raises(TypeError):
        cd(a.cpu().numpy(), b)
    with pytest.raises(ValueError):
        cd(a[:1], b)
    with pytest.raises(ValueError):
        cd(a, torch.zeros(2, 6, 2, device=dev))
    with pytest.raises(ValueError):
        cd(a[0], b[0])
    with pytest.raises(ValueError):
        cd(a, b, reduction="max")


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("use_xyz,with_features", [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize("B,N,S,C,radius,nsample", [(2, 60, 9, 5, 0.4, 8), (2, 4096, 1024, 3, 0.06, 32)])
def test_query_and_group_matches_fp64(request, compat, device, B, N, S, C, radius, nsample, use_xyz, with_features):
    dev = _on(request, device)
    rng = _rng(23, B, N, S)
    p = rng.uniform(-0.5, 0.5, (B, N, 3)).astype(np.float32)
    q = (p[:, :S] + 0.01 * rng.standard_normal((B, S, 3))).astype(np.float32)
    f = rng.standard_normal((B, C, N)).astype(np.float32)
    ri = R.ball_query(radius, nsample, p, q)
    xyz, new_xyz = _t(p, dev, grad=True), _t(q, dev, grad=True)
    feat = _t(f, dev, grad=True) if with_features else None
    out = compat.pn2.QueryAndGroup(radius, nsample, use_xyz)(xyz, new_xyz, feat)
    xr, qr, fr = _d(xyz, True), _d(new_xyz, True), (_d(feat, True) if with_features else None)
    e = torch.from_numpy(ri).long().reshape(B, 1, S * nsample)
    group = lambda t: torch.gather(t, 2, e.expand(B, t.shape[1], S * nsample)).reshape(B, t.shape[1], S, nsample)
    gx = group(xr.transpose(1, 2)) - qr.transpose(1, 2)[..., None]
    ref = torch.cat([gx, group(fr)], 1) if (use_xyz and with_features) else (group(fr) if with_features else gx)
    assert out.shape == ref.shape
    nx = 3 if (use_xyz or not with_features) else 0
    _exact(out[:, nx:], ref[:, nx:], "grouped features")
    mag = group(xr.transpose(1, 2)).abs() + qr.transpose(1, 2)[..., None].abs()
    if nx:
        _cmp_sum(out[:, :nx], ref[:, :nx], mag.detach(), 2, 0, "grouped xyz - centre")
    g = torch.from_numpy(_rng(24, B, N, S).standard_normal(tuple(ref.shape)).astype(np.float32))
    leaves = ([xyz, new_xyz] if nx else []) + ([feat] if with_features else [])
    refs = ([xr, qr] if nx else []) + ([fr] if with_features else [])
    got = torch.autograd.grad(out, leaves, g.to(dev))
    want = torch.autograd.grad(ref, refs, g.double(), retain_graph=True)
    # magnitudes: the same linear map applied to |g| (the map's coefficients are +1 and, for the centres, -1)
    absum = [a.abs() for a in torch.autograd.grad(ref, refs, g.double().abs())]
    hits = torch.zeros(B, N, dtype=torch.float64).scatter_add_(1, e.reshape(B, -1), torch.ones(B, S * nsample, dtype=torch.float64))
    counts = ([hits[:, :, None], float(nsample)] if nx else []) + ([hits[:, None, :]] if with_features else [])
    for a, w, s_, n_ in zip(got, want, absum, counts):
        _cmp_sum(a, w, s_, n_, 0, "grad")
    if not nx:
        assert xyz.grad is None and new_xyz.grad is None
    if not with_features:
        with pytest.raises(AssertionError):
            compat.pn2.QueryAndGroup(radius, nsample, False)(xyz, new_xyz, None)


def test_group_all_three_branches(compat):
    """GroupAll is index-free tensor plumbing: no backend involved."""
    rng = _rng(25)
    xyz = torch.from_numpy(rng.standard_normal((2, 11, 3)).astype(np.float32))
    f = torch.from_numpy(rng.standard_normal((2, 4, 11)).astype(np.float32))
    both = compat.pn2.GroupAll()(xyz, None, f)
    assert both.shape == (2, 7, 1, 11) and torch.equal(both[:, :3, 0], xyz.transpose(1, 2)) and torch.equal(both[:, 3:, 0], f)
    assert torch.equal(compat.pn2.GroupAll(use_xyz=False)(xyz, None, f), f.unsqueeze(2))
    assert torch.equal(compat.pn2.GroupAll()(xyz, None), xyz.transpose(1, 2).unsqueeze(2))
    assert torch.equal(compat.pn2.GroupAll(False)(xyz, None, None), xyz.transpose(1, 2).unsqueeze(2))


def test_cpu_tensors_raise_without_a_backend(compat):
    """"CPU tensors raise (HIP only, no CPU fallback)" -- nobody has registered the oracle here."""
    x, f = torch.zeros(1, 8, 3), torch.zeros(1, 4, 8)
    i2, i3 = torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, 2, 2, dtype=torch.int32)
    calls = [lambda: compat.pn2.furthest_point_sample(x, 2), lambda: compat.pn2.gather_operation(f, i2),
             lambda: compat.pn2.ball_query(0.1, 2, x, x), lambda: compat.pn2.grouping_operation(f, i3),
             lambda: compat.pn2.three_nn(x, x), lambda: compat.pn2.three_interpolate(f, torch.zeros(1, 2, 3, dtype=torch.int32), torch.zeros(1, 2, 3)),
             lambda: compat.p3d.knn_points(x, x, K=2), lambda: compat.frnn.frnn_grid_points(x, x, K=2, r=0.1),
             lambda: compat.chamferdist.ChamferDistance()(x, x)]
    for call in calls:
        with pytest.raises(RuntimeError, match="HIP only"):
            call()


@pytest.mark.parametrize("device", DEVICES)
def test_pointnet2_argument_errors(request, compat, device):
    """wrong dtype and non-contiguous inputs raise RuntimeError.  Argument validation only:
    every call below is refused by the Python layer before any kernel (or the oracle) sees it."""
    dev = _on(request, device)
    x, f = torch.zeros(2, 8, 3, device=dev), torch.zeros(2, 4, 8, device=dev)
    i2 = torch.zeros(2, 2, dtype=torch.int32, device=dev)
    i3 = torch.zeros(2, 2, 3, dtype=torch.int32, device=dev)
    w3 = torch.zeros(2, 2, 3, device=dev)
    pn2 = compat.pn2
    bad = [
        lambda: pn2.gather_operation(f.double(), i2), lambda: pn2.gather_operation(f, i2.long()),
        lambda: pn2.gather_operation(f.transpose(1, 2), i2), lambda: pn2.gather_operation(f, i3),
        lambda: pn2.grouping_operation(f.half(), i3), lambda: pn2.grouping_operation(f, i3.long()),
        lambda: pn2.grouping_operation(f, i3.transpose(1, 2)), lambda: pn2.grouping_operation(f[:1], i3),
        lambda: pn2.three_interpolate(f, i3.long(), w3), lambda: pn2.three_interpolate(f, i3, w3.double()),
        lambda: pn2.three_interpolate(f.transpose(1, 2), i3, w3),
        lambda: pn2.three_nn(x.double(), x), lambda: pn2.three_nn(x, x.transpose(1, 2)),
        lambda: pn2.ball_query(0.1, 2, x.double(), x), lambda: pn2.ball_query(0.1, 2, x, x[:1]),
        lambda: pn2.furthest_point_sample(x.double(), 2), lambda: pn2.furthest_point_sample(x.transpose(1, 2), 2),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
        assert True, k


@pytest.mark.parametrize("device", GPU_ONLY)     # mixed devices and the library's own K limit need the GPU side
def test_mixed_device_and_k_limit_raise(request, compat, device):
    dev = _on(request, device)
    x, f = torch.zeros(1, 80, 3, device=dev), torch.zeros(1, 4, 80, device=dev)
    i2 = torch.zeros(1, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="same device"):
        compat.pn2.gather_operation(f, i2)
    with pytest.raises(RuntimeError, match="same device"):
        compat.pn2.ball_query(0.1, 2, x, x.cpu())
    with pytest.raises(RuntimeError, match="same device"):
        compat.p3d.knn_points(x, x.cpu(), K=2)
    with pytest.raises(ValueError):
        compat.chamferdist.ChamferDistance()(x, x.cpu())
    # K > 64: tpg_knn_f32 refuses it from its argument check (TPG_ERR_UNSUPPORTED), before any launch
    with pytest.raises(RuntimeError):
        compat.p3d.knn_points(x, x, K=65)
