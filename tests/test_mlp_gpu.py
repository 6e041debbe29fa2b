"""The fused MFMA tail-layer kernels (csrc/mlp_fused.hip) against a plain PyTorch fp32 statement of
the same op on the same (bf16-rounded) inputs.

Tolerances: the kernel multiplies bf16 operands exactly and accumulates in fp32 like the reference
product; the stored y is rounded once to bf16, so |y - y_ref| <= one bf16 ulp of |y_ref| (2^-8
relative) plus the fp32 summation-order noise; statistics are computed from the kernel's OWN
stored values and must match an fp64 recomputation from them to 1e-5."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import tpgan_amd.ops as ops
    return ops.backend_for(torch.zeros(1, device="cuda"))


def _layer_inputs(P, Cin, Cout, nseg, seed, with_bn=True):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(P, Cin, generator=g) * 0.7 + 0.3 * torch.randn(1, Cin, generator=g)).bfloat16().cuda()
    W = (torch.randn(nseg, Cout, Cin, generator=g) / Cin ** 0.5).cuda()
    if with_bn:
        ss = torch.stack([torch.rand(nseg, Cin, generator=g) + 0.5, 0.3 * torch.randn(nseg, Cin, generator=g)], 1).cuda()
    else:
        ss = None
    return x, W, ss


def _ref_fwd(x, W, ss, slope, nseg):
    P = x.shape[0] // nseg
    ys = []
    for s in range(nseg):
        a = x[s * P:(s + 1) * P].float()
        if ss is not None:
            # one rounding of the exact x*sc + sh, like the kernel's fma
            a = (a.double() * ss[s, 0].double() + ss[s, 1].double()).float()
        a = torch.where(a > 0, a, a * slope).bfloat16().float()
        ys.append(a @ W[s].bfloat16().float().t())
    return torch.cat(ys, 0)


@pytest.mark.parametrize("Cin,Cout", [(64, 64), (64, 128), (128, 64), (128, 128), (128, 256), (256, 128), (256, 256)])
@pytest.mark.parametrize("P,nseg", [(8 * 128 * 32, 1), (3 * 4096, 3), (1000, 1), (2 * 16 * 7, 2)])
def test_mlp_fwd_matches_torch(hip, Cin, Cout, P, nseg):
    x, W, ss = _layer_inputs(P, Cin, Cout, nseg, seed=Cin + Cout + P)
    rm, rv = torch.zeros(Cout, device="cuda"), torch.ones(Cout, device="cuda")
    nbt = torch.zeros((), dtype=torch.int64, device="cuda")
    gamma, beta = torch.rand(Cout, device="cuda") + 0.5, torch.randn(Cout, device="cuda") * 0.1
    y, ci = hip.mlp_fwd(x, ss, 0.01, W, nseg, 1e-5, 0.1, rm, rv, nbt, None, gamma, beta)
    mean, rstd = ci[:, 2], ci[:, 3]
    ref = _ref_fwd(x, W, ss, 0.01, nseg)
    err = (y.float() - ref).abs()
    # same bf16 operands, fp32 accumulation in another order, ONE rounding of y to bf16: within one
    # bf16 ulp (2^-7 relative: a sum that lands next to a rounding tie may go to the other neighbour)
    bound = ref.abs() * 2.0 ** -7 + 1e-5 * ref.abs().max()
    assert bool((err <= bound).all()), float((err - bound).max())
    # statistics of the stored tensor, per segment
    Ps = P // nseg
    yd = y.double().view(nseg, Ps, Cout)
    m_ref, v_ref = yd.mean(1), yd.var(1, unbiased=False)
    assert torch.allclose(mean.double(), m_ref, rtol=0, atol=1e-5 * float(m_ref.abs().max() + v_ref.sqrt().max()))
    assert torch.allclose(rstd.double(), (v_ref + 1e-5).rsqrt(), rtol=1e-5, atol=0)
    a = gamma * rstd
    assert torch.allclose(ci[:, 0], a) and torch.allclose(ci[:, 1], beta - mean * a, atol=1e-6)
    # running statistics chained segment after segment, unbiased variance, counter += nseg
    erm, erv = torch.zeros(Cout, dtype=torch.float64), torch.ones(Cout, dtype=torch.float64)
    for s in range(nseg):
        erm = 0.9 * erm + 0.1 * m_ref[s].cpu()
        erv = 0.9 * erv + 0.1 * (v_ref[s].cpu() * Ps / (Ps - 1))
    assert torch.allclose(rm.double().cpu(), erm, atol=1e-5) and torch.allclose(rv.double().cpu(), erv, rtol=1e-5, atol=1e-6)
    assert int(nbt) == nseg


def test_mlp_fwd_mean_shift_enters_the_running_mean_only(hip):
    """mean_shift (set_abstraction.py hands the conv biases left out of the product through it): the running mean tracks
    mean_s(y) + shift, chained segment by segment as (1 - m) rm + m (mean_s(y) + shift); mean, rstd and the folded
    constants are those of the launch without the shift, bit for bit; the running variance is unchanged by it."""
    P, nseg, Cin, Cout = 3 * 4096, 3, 64, 128
    x, W, ss = _layer_inputs(P, Cin, Cout, nseg, seed=11)
    shift = torch.randn(Cout, device="cuda")
    gamma, beta = torch.rand(Cout, device="cuda") + 0.5, torch.randn(Cout, device="cuda") * 0.1
    res = []
    for sh in (None, shift):
        rm, rv = torch.full((Cout,), 0.5, device="cuda"), torch.ones(Cout, device="cuda")
        y, ci, mean, rstd = hip.mlp_fwd(x, ss, 0.01, W, nseg, 1e-5, 0.1, rm, rv, None, sh, gamma, beta, mean_rstd=True)
        res.append((y, ci, mean, rstd, rm, rv))
    (y0, ci0, m0, r0, rm0, rv0), (y1, ci1, m1, r1, rm1, rv1) = res
    assert torch.equal(y0, y1) and torch.equal(ci0, ci1) and torch.equal(m0, m1) and torch.equal(r0, r1)
    assert torch.equal(rv0, rv1)
    ms = y1.double().view(nseg, P // nseg, Cout).mean(1).cpu()
    erm = torch.full((Cout,), 0.5, dtype=torch.float64)
    for s in range(nseg):
        erm = 0.9 * erm + 0.1 * (ms[s] + shift.double().cpu())
    assert torch.allclose(rm1.double().cpu(), erm, rtol=0, atol=1e-5), float((rm1.double().cpu() - erm).abs().max())


def test_mlp_fwd_statistics_survive_a_large_mean(hip):
    """|mean| / sigma = 1e3 in the OUTPUT: the pivoted, Chan-combined sums keep the variance."""
    P, Cin, Cout = 65536, 64, 128
    x = torch.ones(P, Cin).bfloat16().cuda()
    x[:, 0] = (torch.randn(P) * 0.01).bfloat16().cuda()             # the only varying input
    W = torch.zeros(1, Cout, Cin).cuda()
    W[0, :, 1] = 8.0                                                  # constant part: 8
    W[0, :, 0] = 1.0                                                  # varying part: sigma 0.01
    y, ci = hip.mlp_fwd(x, None, 1.0, W, 1, 1e-5, 0.0, None, None, None, None, None, None)
    mean, rstd = ci[:, 2], ci[:, 3]
    yd = y.double()
    assert torch.allclose(mean.double()[0], yd.mean(0), atol=1e-6)
    assert torch.allclose(rstd.double()[0], (yd.var(0, unbiased=False) + 1e-5).rsqrt(), rtol=1e-4)


def test_mlp_fwd_is_bitwise_reproducible(hip):
    x, W, ss = _layer_inputs(6 * 8192, 64, 128, 3, seed=5)
    a = hip.mlp_fwd(x, ss, 0.2, W, 3, 1e-5, 0.1, None, None, None, None, None, None)
    b = hip.mlp_fwd(x, ss, 0.2, W, 3, 1e-5, 0.1, None, None, None, None, None, None)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    # without statistics (a tail without BatchNorm): the same rows, no finalize
    y2, none = hip.mlp_fwd(x, ss, 0.2, W, 3, stats=False)
    assert none is None and torch.equal(y2, a[0])


# ------------------------------------------------------------------ the whole tail, forward + backward
def _ste_bf16(t):
    """bf16 rounding with a straight-through gradient: the reference rounds where the kernels round."""
    return t + (t.bfloat16().float() - t).detach()


def _ref_tail(x0, gammas, betas, Ws, slopes, K, nseg, eps=1e-5):
    outs = []
    P = x0.shape[0] // nseg
    for s in range(nseg):
        a = x0[s * P:(s + 1) * P]
        for l in range(len(gammas)):
            m, v = a.mean(0), a.var(0, unbiased=False)
            z = (a - m) * (gammas[l] * (v + eps).rsqrt()) + betas[l]
            a = torch.where(z > 0, z, z * slopes[l])
            if l < len(Ws):
                w = Ws[l][s] if Ws[l].dim() == 3 else Ws[l]
                a = _ste_bf16(_ste_bf16(a) @ _ste_bf16(w).t())       # operands and the stored product in bf16
        outs.append(a.view(P // K, K, -1).max(1)[0])
    return torch.cat(outs, 0)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-12))


@pytest.mark.parametrize("chain,K,P,nseg,per_seg_w", [
    ((64, 128), 32, 8 * 64 * 32, 1, False), ((64, 128), 32, 2 * 8 * 64 * 32, 2, True),
    ((128, 128), 32, 4096, 1, False), ((128, 256), 16, 3 * 2048, 3, True),
    ((256, 128, 256), 32, 2 * 4096, 2, True), ((256, 256, 256), 32, 4096, 1, False),
    ((64, 64, 128), 64, 4096, 1, False), ((128, 64), 8, 1000 * 8, 1, False),
    ((64, 128), 16, 7 * 320, 7, True), ((64, 128, 128), 16, 70 * 256, 70, True)])     # 70 segments: two sweeps of the finalize kernels
def test_mlp_tail_forward_backward(chain, K, P, nseg, per_seg_w):
    import tpgan_amd.ops as ops
    torch.manual_seed(sum(chain) + K)
    L = len(chain) - 1
    x0 = (torch.randn(P, chain[0]) * 0.8 + 0.2 * torch.randn(1, chain[0])).bfloat16().cuda()
    bns = [torch.nn.BatchNorm1d(c).cuda().train() for c in chain]
    for bn in bns:
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0, 0.2)
    Ws = [(torch.randn(*((nseg,) if per_seg_w else ()), chain[l + 1], chain[l]) / chain[l] ** 0.5).cuda().requires_grad_(True)
          for l in range(L)]
    slopes = [0.01] * (L + 1)
    assert ops.mlp_tail_supported(x0, chain, K)
    xk = x0.clone().requires_grad_(True)
    out = ops.mlp_tail(xk, bns, Ws, slopes, K, nseg)
    gout = torch.randn(out.shape, device="cuda").bfloat16()
    params = [xk] + Ws + [p for bn in bns for p in (bn.weight, bn.bias)]
    got = torch.autograd.grad(out, params, gout)
    xr = x0.float().clone().requires_grad_(True)
    ref = _ref_tail(xr, [bn.weight for bn in bns], [bn.bias for bn in bns], Ws, slopes, K, nseg)
    want = torch.autograd.grad(ref, [xr] + Ws + [p for bn in bns for p in (bn.weight, bn.bias)], gout.float())
    # forward: the stored output is one bf16 rounding of a value that went through L bf16 products
    err = float((out.float() - ref).abs().max() / ref.abs().max())
    assert err <= 2e-2, err
    # (a max-pool winner may differ where two rows are within rounding: compared in L2)
    names = ["dx0"] + [f"dW{l + 1}" for l in range(L)] + [f"{n}{l}" for l in range(L + 1) for n in ("dgamma", "dbeta")]
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        rel = _rel(g.float(), w)
        assert rel <= 3e-2, (name, rel)
    # running statistics moved like nn.BatchNorm's own forward (momentum 0.1, nseg updates)
    assert all(int(bn.num_batches_tracked) == nseg for bn in bns)
    assert all(not torch.equal(bn.running_mean, torch.zeros_like(bn.running_mean)) for bn in bns)


def test_mlp_tail_frozen_weights_need_no_weight_gradient():
    """The generator step back-propagates through FROZEN discriminators: data gradient only."""
    import tpgan_amd.ops as ops
    torch.manual_seed(0)
    x0 = torch.randn(4096, 64).bfloat16().cuda().requires_grad_(True)
    bns = [torch.nn.BatchNorm1d(c).cuda().train().requires_grad_(False) for c in (64, 128)]
    W = (torch.randn(128, 64) / 8).cuda()
    out = ops.mlp_tail(x0, bns, [W], [0.01, 0.01], 32)
    (gx,) = torch.autograd.grad(out, [x0], torch.randn_like(out))
    assert torch.isfinite(gx).all() and float(gx.abs().max()) > 0


def test_mlp_tail_is_bitwise_reproducible():
    import tpgan_amd.ops as ops
    torch.manual_seed(1)
    x0 = torch.randn(3 * 8192, 64).bfloat16().cuda()
    W = (torch.randn(3, 128, 64) / 8).cuda().requires_grad_(True)
    res = []
    for _ in range(2):
        bns = [torch.nn.BatchNorm1d(c).cuda().train() for c in (64, 128)]
        xk = x0.clone().requires_grad_(True)
        out = ops.mlp_tail(xk, bns, [W], [0.01, 0.01], 32, 3)
        g = torch.autograd.grad(out, [xk, W, bns[0].weight, bns[1].bias], torch.ones_like(out))
        res.append((out,) + tuple(g) + (bns[1].running_var.clone(),))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def _gather_tail_case(C, K, S, nseg, fused, table_dtype=torch.float32, inverse=False, need_u=True, need_q=True,
                      second=False):
    """row_combine(ROW_SUB) -> mlp_tail on fixed inputs, as the two ops (`fused` False) or as ops.gather_mlp_tail:
    -> [out, the gradients of whichever of U, Q is wanted, of W and of every BatchNorm affine, the running statistics]."""
    import tpgan_amd.ops as ops
    torch.manual_seed(C + K)
    B, N = 2 * nseg, 500
    U = torch.randn(B, N, C, device="cuda").to(table_dtype).requires_grad_(need_u)
    Q = torch.randn(B, S, C, device="cuda").to(table_dtype).requires_grad_(need_q)
    idx = torch.randint(0, N, (B, S, K), device="cuda", dtype=torch.int32)
    W = (torch.randn(128, C) / C ** 0.5).cuda().requires_grad_(True)
    bns = [torch.nn.BatchNorm1d(c).cuda().train() for c in (C, 128)]
    lst = ops.attach_inverse(idx, N) if inverse else idx
    if fused:
        out = ops.gather_mlp_tail(U, Q, lst, bns, [W], [0.01, 0.01], nseg).view(-1, 128)
    else:
        y = ops.row_combine(U, Q, lst, ops.ROW_SUB, out_dtype=torch.bfloat16)
        out = ops.mlp_tail(y.view(-1, C), bns, [W], [0.01, 0.01], K, nseg)
    loss = (out.float() * torch.linspace(-1, 1, out.numel(), device="cuda").view_as(out)).sum()
    if second:
        loss = loss + y.float().square().sum() * 1e-3
    wrt = [t for t in (U, Q) if t.requires_grad] + [W] + [p for bn in bns for p in (bn.weight, bn.bias)]
    stats = [t.clone() for bn in bns for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]
    return [out.detach()] + list(torch.autograd.grad(loss, wrt)) + stats


@pytest.mark.parametrize("C,K,S,nseg", [(64, 32, 256, 1), (64, 12, 300, 2), (128, 7, 96, 3)])
def test_tail_hands_its_row_sums_to_the_gather_that_fed_it(C, K, S, nseg):
    """A set-abstraction level is row_combine(ROW_SUB) -> fused tail.  As ONE node (ops.gather_mlp_tail) the tail's
    backward sums its input gradient over each group of K rows while writing it (tpg_mlp_bn_bwd_apply_rowsum) and the
    gather's backward takes those sums as the gradient of Q instead of reading the rows again: same bits as the two
    separate ops (the two-pass route) in the output, every gradient and the BatchNorms' running statistics.  On the
    separate ops a second consumer of the gathered rows adds its gradient to the tail's, as ever."""
    # (the inverted index keeps entry order: the scatter sums are reproducible, bits can be compared)
    two_pass = _gather_tail_case(C, K, S, nseg, fused=False)
    for a, b in zip(two_pass, _gather_tail_case(C, K, S, nseg, fused=True)):
        assert a.shape == b.shape and torch.equal(a, b)
    shared = _gather_tail_case(C, K, S, nseg, fused=False, second=True)
    assert all(torch.isfinite(t).all() for t in shared)
    assert not torch.equal(shared[2], two_pass[2])                       # Q's gradient
    if nseg > 1:
        return
    # the node's other routes, at the first shape: a NeighbourList with a prepared inverse (also against the bare
    # tensor), bf16 tables (plain last tail launch + the ROW_SUB backward), and fewer wanted gradients (with neither
    # table wanting one no input gradient is computed at all)
    for kw in (dict(inverse=True), dict(table_dtype=torch.bfloat16), dict(need_q=False), dict(need_u=False),
               dict(need_u=False, need_q=False)):
        want = _gather_tail_case(C, K, S, nseg, fused=False, **kw)
        got = _gather_tail_case(C, K, S, nseg, fused=True, **kw)
        assert len(got) == len(want) == 1 + kw.get("need_u", True) + kw.get("need_q", True) + 5 + 6, kw
        for a, b in zip(want, got):
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), kw
        if kw.get("inverse"):
            for a, b in zip(got, _gather_tail_case(C, K, S, nseg, fused=True)):
                assert torch.equal(a, b)


# ------------------------------------------------------------------ EdgeConv MLP: the tail without BatchNorm
@pytest.mark.parametrize("chain,K,P", [((64, 64, 128), 20, 512 * 20 * 6), ((128, 128, 256), 12, 512 * 12 * 4),
                                         ((128, 128, 256), 4, 1000 * 4), ((64, 128), 9, 9 * 333)])
def test_mlp_tail_plain_forward_backward(chain, K, P):
    """ops.mlp_tail_plain (identity statistics) against the PyTorch statement of the EdgeConv MLP
    (gcn_lib/pointnet/gcn.py:207-211): [conv -> LeakyReLU(0.2)]* -> max over the k neighbours."""
    import tpgan_amd.ops as ops
    torch.manual_seed(sum(chain) + K)
    L = len(chain) - 1
    x0 = torch.randn(P, chain[0]).bfloat16().cuda()
    Ws = [(torch.randn(chain[l + 1], chain[l]) / chain[l] ** 0.5).cuda().requires_grad_(True) for l in range(L)]
    slopes = [1.0] + [0.2] * L
    xk = x0.clone().requires_grad_(True)
    out = ops.mlp_tail_plain(xk, Ws, slopes, K)
    gout = torch.randn(out.shape, device="cuda").bfloat16()
    got = torch.autograd.grad(out, [xk] + Ws, gout)
    xr = x0.float().clone().requires_grad_(True)
    a = xr
    for l in range(L):
        a = _ste_bf16(_ste_bf16(a) @ _ste_bf16(Ws[l]).t())
        a = torch.where(a > 0, a, a * 0.2)
    ref = a.view(P // K, K, -1).max(1)[0]
    want = torch.autograd.grad(ref, [xr] + Ws, gout.float())
    err = float((out.float() - ref).abs().max() / ref.abs().max())
    assert err <= 2e-2, err
    for name, g, w in zip(["dx0"] + [f"dW{l + 1}" for l in range(L)], got, want):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        rel = _rel(g.float(), w)
        assert rel <= 3e-2, (name, rel)


def test_edgeconv_fused_tail_equals_the_separate_launches():
    """EdgeConv.forward_rows with the fused MFMA tail against the hipBLASLt + activation launches it
    replaces, bf16 autocast, same module: outputs and all gradients."""
    from tpgan_amd import graph_conv
    from tpgan_amd.graph_conv import EdgeConv
    torch.manual_seed(4)
    m = EdgeConv(64, 256, k=12, aggregate="max", mlp_layer=True, bn=False, insn=False).cuda()
    x = torch.randn(6, 512, 64, device="cuda")
    res = []
    for fused in (True, False):
        graph_conv.FUSED_EDGE_TAILS[0] = fused
        try:
            xi = x.clone().requires_grad_(True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = m.forward_rows(xi)
            g = torch.autograd.grad(y.float().square().sum(), [xi] + list(m.parameters()))
            res.append((y.float(),) + tuple(t.float() for t in g))
        finally:
            graph_conv.FUSED_EDGE_TAILS[0] = True
    for a, b in zip(*res):
        assert a.shape == b.shape and _rel(a, b) <= 3e-2, _rel(a, b)


# ------------------------------------------------------------ the 16 -> 16 -> 32 tail of the IDGCN EdgeConvs
def _small_tail_reference(h, W1, W2, s1, s2, K):
    z2 = F.leaky_relu(h.float() @ W1.t(), s1) @ W2.t()
    P = h.shape[0] // K
    return F.leaky_relu(z2.view(P, K, -1).max(1)[0], s2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("P,K", [(12288, 20), (12288, 10), (1000, 9), (37, 3), (5, 1)])
def test_small_tail_forward_backward(dtype, P, K):
    """csrc/mlp_small.hip against plain PyTorch fp32 on the same rows: output, gradient to the rows, both
    weight gradients.  The kernels compute in fp32 whatever the row type: fp32 rows to 1e-5 (north_star's
    tolerance), bf16 rows to the rounding of the stored output / gradient (2^-8)."""
    from tpgan_amd import ops
    torch.manual_seed(P + K)
    h = torch.randn(P * K, 16, device="cuda").to(dtype)
    W1 = (torch.randn(16, 16, device="cuda") * 0.3).requires_grad_(True)
    W2 = (torch.randn(32, 16, device="cuda") * 0.3).requires_grad_(True)
    g = torch.randn(P, 32, device="cuda").to(dtype)
    hi = h.clone().requires_grad_(True)
    y = ops.small_tail(hi, W1, W2, 0.2, 0.2, K)
    assert y.dtype == dtype and y.shape == (P, 32)
    gh, g1, g2 = torch.autograd.grad(y, [hi, W1, W2], g)
    hr = h.float().clone().requires_grad_(True)
    yr = _small_tail_reference(hr, W1, W2, 0.2, 0.2, K)
    rh, r1, r2 = torch.autograd.grad(yr, [hr, W1, W2], g.float())
    tol = 1e-5 if dtype == torch.float32 else 2.0 ** -7
    assert _rel(y.float(), yr) <= tol, _rel(y.float(), yr)
    assert _rel(gh.float(), rh) <= tol, _rel(gh.float(), rh)
    assert _rel(g1, r1) <= max(tol, 2e-5) and _rel(g2, r2) <= max(tol, 2e-5), (_rel(g1, r1), _rel(g2, r2))


def test_small_tail_routes_ties_to_the_first_maximum_and_is_reproducible():
    from tpgan_amd import ops
    torch.manual_seed(3)
    K, P = 12, 640
    base = torch.randn(P, 1, 16, device="cuda")
    h = base.expand(P, K, 16).reshape(P * K, 16).contiguous()            # K identical edges per point: every channel ties
    W1 = torch.randn(16, 16, device="cuda", requires_grad=True)
    W2 = torch.randn(32, 16, device="cuda", requires_grad=True)
    hi = h.clone().requires_grad_(True)
    y = ops.small_tail(hi, W1, W2, 0.2, 0.2, K)
    gh, g1, g2 = torch.autograd.grad(y.sum(), [hi, W1, W2])
    gh = gh.view(P, K, 16)
    assert float(gh[:, 1:].abs().max()) == 0.0 and float(gh[:, 0].abs().max()) > 0.0    # all of it on edge 0
    hi2 = h.clone().requires_grad_(True)
    gh2, g1b, g2b = torch.autograd.grad(ops.small_tail(hi2, W1, W2, 0.2, 0.2, K).sum(), [hi2, W1, W2])
    assert torch.equal(gh.reshape(-1, 16), gh2) and torch.equal(g1, g1b) and torch.equal(g2, g2b)


@pytest.mark.parametrize("amp", [False, True])
def test_idgcn_small_tails_equal_the_separate_launches(amp):
    """IDGCNLayer.forward_rows (two EdgeConvs with 16 -> 16 -> 32 tails) with the one-launch tails against the
    GEMM + activation launches they replace.  fp32: the two forms sum in different orders, outputs agree to 1e-4;
    a near-tie of the max over the neighbours may then pick another edge and move its share of a gradient
    (measured 6e-4 of a weight gradient's norm): 2e-3.  bf16 autocast: the unfused path rounds every
    intermediate to bf16, the fused one only its output (measured 3.1e-2 on one weight gradient): 5e-2."""
    from tpgan_amd import graph_conv
    from tpgan_amd.graph_conv import IDGCNLayer
    torch.manual_seed(6)
    m = IDGCNLayer(128, 128, bn=False, insn=False, residual=True).cuda()
    x = torch.randn(4, 512, 128, device="cuda")
    res = []
    for fused in (True, False):
        graph_conv.FUSED_EDGE_TAILS[0] = fused
        try:
            xi = x.clone().requires_grad_(True)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                y = m.forward_rows(xi)
            g = torch.autograd.grad(y.float().square().sum(), [xi] + list(m.parameters()))
            res.append((y.float(),) + tuple(t.float() for t in g))
        finally:
            graph_conv.FUSED_EDGE_TAILS[0] = True
    assert _rel(res[0][0], res[1][0]) <= (3e-2 if amp else 1e-4)
    for a, b in zip(*res):
        assert a.shape == b.shape and _rel(a, b) <= (5e-2 if amp else 2e-3), _rel(a, b)


# ------------------------------------------------------------------ row-wise linear layers (csrc/rowlinear.hip)
@pytest.mark.parametrize("P,Cin,Cout,nseg", [
    (12288, 3, 64, 1), (12288, 128, 128, 1), (12288, 128, 32, 1), (12288, 32, 16, 1), (12288, 96, 128, 1),
    (12288, 256, 64, 1), (12288, 256, 12, 1), (12288, 12, 24, 1), (12288, 24, 24, 1), (12288, 64, 1, 1),
    (65536, 6, 64, 2), (6144, 131, 128, 6), (4096, 259, 256, 2), (3072, 515, 256, 4), (8, 256, 256, 1),
    (8, 64, 1, 1), (1, 5, 7, 1), (33, 17, 19, 1), (100, 300, 130, 1), (256, 16, 16, 2), (4096, 256, 256, 1), (2048, 515, 256, 1)])
@pytest.mark.parametrize("din,dout", [("f32", "f32"), ("bf16", "bf16"), ("f32", "bf16")])
def test_row_linear_against_pytorch_fp32(P, Cin, Cout, nseg, din, dout):
    """tpg_rowlinear_fwd / dgrad / wgrad against plain PyTorch fp32 on the same (rounded) rows: the generator's and
    the discriminators' channel counts (3, 6, 12, 24, 96, 131, 259, 515, ...), segments with their own weights,
    bias and LeakyReLU in the epilogue, tiny P (the heads), ragged sizes.  fp32 in / out: 2e-5 of the output scale
    (fp32 products, another summation order); bf16: one rounding of the stored values."""
    import tpgan_amd.ops as ops
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}
    torch.manual_seed(P + Cin + Cout)
    dev = "cuda"
    assert ops.ROW_LINEAR[0] is False           # (off by default: slower than the library, see ops.ROW_LINEAR; the op itself is tested)
    x = torch.randn(P, Cin, device=dev).to(dt[din])
    W = (torch.randn(nseg, Cout, Cin, device=dev) / Cin ** 0.5)
    b = torch.randn(Cout, device=dev) * 0.3
    gy = torch.randn(P, Cout, device=dev).to(dt[dout])
    for slope, use_b in ((0.2, True), (1.0, False)):
        xa = x.clone().requires_grad_(True)
        Wa = (W if nseg > 1 else W[0]).clone().requires_grad_(True)
        ba = b.clone().requires_grad_(True) if use_b else None
        y = ops.row_linear(xa, Wa, ba, slope, nseg, dt[dout])
        assert y.dtype == dt[dout] and y.shape == (P, Cout)
        y.backward(gy)
        # reference: fp32 math on the same inputs
        xr = x.float().clone().requires_grad_(True)
        Wr = W.clone().requires_grad_(True)
        br = b.clone().requires_grad_(True) if use_b else None
        z = torch.bmm(xr.view(nseg, P // nseg, Cin), Wr.transpose(1, 2)).view(P, Cout)
        if use_b:
            z = z + br
        yr = torch.nn.functional.leaky_relu(z, slope) if slope != 1.0 else z
        # the kernel's backward takes lrelu' from the sign of the STORED output
        ys = y.detach().float()
        gz = gy.float() * torch.where(ys > 0, torch.ones_like(ys), torch.full_like(ys, slope)) if slope != 1.0 else gy.float()
        z.backward(gz)
        tol_y = 2e-5 if dout == "f32" else 8e-3
        assert float((y.float() - yr).abs().max()) <= tol_y * max(1.0, float(yr.abs().max())), (slope, float((y.float() - yr).abs().max()))
        tol_g = 2e-5 if din == "f32" else 8e-3
        assert float((xa.grad.float() - xr.grad).abs().max()) <= tol_g * max(1.0, float(xr.grad.abs().max()))
        gW = Wa.grad.view(nseg, Cout, Cin)
        assert float((gW - Wr.grad).abs().max()) <= 1e-4 * max(1.0, float(Wr.grad.abs().max())), float((gW - Wr.grad).abs().max())
        if use_b:
            assert float((ba.grad - br.grad).abs().max()) <= 1e-4 * max(1.0, float(br.grad.abs().max()))


def test_row_linear_declines_what_it_cannot_stage():
    """Channel counts whose 16-row chunk does not fit the weight-gradient kernel's LDS are reported unsupported (the
    host layer then keeps the library GEMM) instead of failing inside a launch."""
    import tpgan_amd.ops as ops
    x = torch.randn(256, 515, device="cuda")
    prev, ops.ROW_LINEAR[0] = ops.ROW_LINEAR[0], True
    try:
        assert ops.row_linear_supported(x, torch.randn(256, 515, device="cuda"))
        assert not ops.row_linear_supported(x, torch.randn(512, 515, device="cuda"))
        assert not ops.row_linear_supported(torch.randn(256, 2000, device="cuda"), torch.randn(64, 2000, device="cuda"))
    finally:
        ops.ROW_LINEAR[0] = prev


def test_row_linear_is_bitwise_reproducible():
    import tpgan_amd.ops as ops
    torch.manual_seed(1)
    x = torch.randn(12288, 96, device="cuda")
    W = torch.randn(128, 96, device="cuda").requires_grad_(True)
    b = torch.randn(128, device="cuda").requires_grad_(True)
    gy = torch.randn(12288, 128, device="cuda")
    res = []
    for _ in range(2):
        xa = x.clone().requires_grad_(True)
        y = ops.row_linear(xa, W, b, 0.2)
        res.append((y.detach().clone(),) + tuple(g.clone() for g in torch.autograd.grad(y, [xa, W, b], gy)))
    for a, c in zip(*res):
        assert torch.equal(a, c)


# ------------------------------------------------------------------ the tail's backward launches against the fp64 oracle
# Each backward entry of csrc/mlp_fused.hip, called directly, against its restatement in oracle.ref_ops (contractions in
# float64 on the GPU).  Elementwise launches: bit for bit.  Contractions: per element, against the `emulated` oracle (d
# rounded to bf16 exactly as d_out8 rounds it) within one bf16 rounding of the stored value + kappa * M, and against the
# `contract` oracle (d exact) within that + the rounding allowance of d (oracle.ref_ops.mlp_bwd_operands).
# kappa = ref_ops.MLP_KAPPA = 2^-15 = 512 fp32 unit roundoffs: the depth of the deepest fp32 summation chain of a
# launch, which every case asserts from the launch geometry (`_depths`); the planted-defect tests in
# tests/test_oracle_cpu.py show that these bounds reject one duplicated or dropped row at the grid's shapes.
_MLP_PAIRS = [(64, 64), (64, 128), (128, 64), (128, 128), (128, 256), (256, 128), (256, 256)]
# rows per segment, nseg, per-segment W, K (MAX mode)
_BWD_SHAPES = [(4096, 1, False, 32), (1000, 1, False, 8), (37, 1, False, 37), (65535, 1, False, 255),
               (2997, 3, True, 9), (192, 70, True, 3), (256, 2, False, 256)]
_WORST = {}


def _note(check, ratio):
    _WORST[check] = max(_WORST.get(check, 0.0), ratio)
    assert ratio <= 1.0, (check, ratio)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    if _WORST:
        print("\nlargest error / bound per check: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(_WORST.items())))


def _depths(hip, P, nseg, Cin, Cout):
    """Deepest fp32 summation chains of one dgrad / wgrad launch (the launchers' geometry, csrc/mlp_fused.hip)."""
    G = hip.lib.tpg_mlp_wgrad_workspace_bytes(P * nseg, Cin, Cout, nseg) // (4 * nseg * Cin * Cout)
    rows_wg = -(-(-(-P // 64)) // G) * 64
    h_w = rows_wg + 1 + -(-G // 4) + 3
    strips = 2 if (Cin == 64 and Cout <= 128) else 1
    smem = Cin * (Cout + 8) * 2 + 4 * (4 * Cout + Cin + 8 * Cin)
    slots = 256 if (smem > 60 * 1024 or Cin == 256) else 512
    tiles = -(-P // (64 * strips))
    Gd = min(tiles, max(16, slots // nseg))
    h_s = -(-tiles // Gd) * 4 * strips + 6          # a lane's rows, 2 shuffles, 4 waves (then fp64)
    return Cout + 2, h_w, h_s


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(got, ref64):
    """Kernel output == oracle value, bit for bit (ref64: float64 holding a value of got's type)."""
    return torch.equal(_bits(got), _bits(ref64.to(got.dtype)))


def _run_bwd_case(hip, Cin, Cout, P, nseg, per_seg, K, mode_max, slope_in=0.01, slope_out=0.01):
    from oracle import ref_ops as R
    kap = R.MLP_KAPPA
    for h in _depths(hip, P, nseg, Cin, Cout):
        assert h * R.U32 <= kap, h
    c = R.mlp_bwd_case(Cin, Cout, P, nseg, per_seg, K, mode_max, slope_out, seed=Cin * 7 + Cout + P + nseg, device="cuda")
    K = c["K"]
    # constants: the kernel's, equal to the oracle's bit for bit, then used by both
    ci_in = hip.mlp_consts(c["mean_in"], c["rstd_in"], c["gamma_in"], c["beta_in"], None, True, False)[0]
    ci_o, cb_o = hip.mlp_consts(c["mean_out"], c["rstd_out"], c["gamma_out"], c["beta_out"], c["c12_out"], True, True)
    r_ci, _ = R.mlp_consts(c["mean_in"], c["rstd_in"], c["gamma_in"], c["beta_in"], None)
    r_cio, r_cbo = R.mlp_consts(c["mean_out"], c["rstd_out"], c["gamma_out"], c["beta_out"], c["c12_out"])
    assert _same_bits(ci_in, r_ci) and _same_bits(ci_o, r_cio) and _same_bits(cb_o, r_cbo), "mlp_consts"
    if mode_max:
        ag = hip.mlp_max_prep(c["gout"], c["y"], cb_o, slope_out, nseg)
        assert _same_bits(ag, R.mlp_max_prep(c["gout"], c["y"], cb_o, slope_out, nseg)), "mlp_max_prep"
        # the by-product of the last BatchNorm's backward sums: the same bits
        *_, ag2 = hip.rowbn_bwd_sums(c["gout"], c["x_out"], c["arg"], c["y"], K, c["mean_out"], c["rstd_out"],
                                     c["gamma_out"], c["beta_out"], slope_out, True, nseg, want_cb=True)
        assert ag2 is not None and torch.equal(_bits(ag2), _bits(ag)), "rowbn_bwd_sums_consts ag"
        g_arg = ag
    else:
        g_arg = c["g_out"]
    args = (c["x_out"], g_arg, c["arg"], K, cb_o, c["x_in"], ci_in, slope_in)
    g_in, c12, cb_in, dgam, dbet = hip.mlp_dgrad(*args, c["W"], nseg, True)
    dW = hip.mlp_wgrad(*args, nseg)
    torch.cuda.synchronize()
    again = hip.mlp_dgrad(*args, c["W"], nseg, True)
    assert all(torch.equal(_bits(u), _bits(v)) for u, v in zip((g_in, c12, cb_in, dgam, dbet), again)), "dgrad repro"
    assert torch.equal(_bits(dW), _bits(hip.mlp_wgrad(*args, nseg))), "wgrad repro"
    assert _same_bits(cb_in, R.mlp_finalize_cb(ci_in, c12)), "finalize cb"
    for level, round_d in (("emulated", True), ("contract", False)):
        ops = R.mlp_bwd_operands(*args, nseg, round_d=round_d)
        dg, wg = R.mlp_dgrad_ref(ops, c["W"]), R.mlp_wgrad_ref(ops)
        _note(f"g_in/{level}", R.err_ratio(g_in, dg["g"], R.gin_bound(dg["g"], dg["M"], dg["R"], kap)))
        _note(f"dW/{level}", R.err_ratio(dW, wg["dW"], R.dw_bound(wg["M"], wg["R"], kap)))
        if round_d:
            S1, S2 = dg["S1"], dg["S2"]
            _note("c1", R.err_ratio(c12[:, 0], dg["c12"][:, 0], R.sums_bound(S1 / P, dg["c12"][:, 0], kap)))
            _note("c2", R.err_ratio(c12[:, 1], dg["c12"][:, 1], R.sums_bound(S2 / P, dg["c12"][:, 1], kap)))
            _note("dbeta", R.err_ratio(dbet, dg["dbeta"], R.sums_bound(S1.sum(0), dg["dbeta"], kap)))
            _note("dgamma", R.err_ratio(dgam, dg["dgamma"], R.sums_bound(S2.sum(0), dg["dgamma"], kap)))
        del ops, dg, wg
    if mode_max:
        # the tail's first BatchNorm on the kernel's own g_in / c12: both apply launches bit for bit
        dx = hip.mlp_bn_bwd_apply(g_in, c["x_in"], ci_in, c12, nseg)
        dx2, qneg = hip.mlp_bn_bwd_apply(g_in, c["x_in"], ci_in, c12, nseg, K)
        rdx, rq = R.mlp_bn_bwd_apply(g_in, c["x_in"], ci_in, c12, nseg, K)
        assert _same_bits(dx, rdx) and _same_bits(dx2, rdx) and _same_bits(qneg, rq), "mlp_bn_bwd_apply"


@pytest.mark.parametrize("P,nseg,per_seg,K,mode_max", [s + (m,) for s in _BWD_SHAPES for m in (False, True)
                                                      if m or s[3] != 256])
@pytest.mark.parametrize("Cin,Cout", _MLP_PAIRS)
def test_mlp_bwd_launches_match_fp64_oracle(hip, Cin, Cout, P, nseg, per_seg, K, mode_max):
    """The grid: every channel pair x DENSE / MAX x rows per segment 4096 (baseline), 1000 (partial last tile of the
    64- / 128-row tiles and of WG_ROWS), 37 (less than one tile), 65535 (several tiles per workgroup at the grid's cap,
    the deferred stores of 128 -> 256 over several tiles, a partial last tile, K = 255), 3 x 2997 (ragged segments with
    their own weights), 70 x 192 (two sweeps of the finalize kernels), 2 x 256 with K = 256 (MAX only: the ABI's limit,
    arg-max bytes 0..255).  slope_in = 0.01."""
    _run_bwd_case(hip, Cin, Cout, P, nseg, per_seg, K, mode_max)


@pytest.mark.parametrize("slope", [0.0, 1.0])
@pytest.mark.parametrize("mode_max", [False, True], ids=["dense", "max"])
@pytest.mark.parametrize("Cin,Cout", _MLP_PAIRS)
def test_mlp_bwd_launches_at_slopes_0_and_1(hip, Cin, Cout, mode_max, slope):
    """LeakyReLU slopes 0 (ReLU: y == 0 on the negative side, the gradient 0 either way) and 1 (no activation), for the
    input's activation and the max-prep slope, at 1000 rows, K = 8."""
    _run_bwd_case(hip, Cin, Cout, 1000, 1, False, 8, mode_max, slope_in=slope, slope_out=slope)


# ------------------------------------------------------------------ the tail's forward launch against the fp64 oracle
# tpg_mlp_fwd (mlp_fwd_kernel + mlp_stats_finalize_kernel), called directly, at its launch edges (tests/mlp_fwd_cases.py).
# Stored rows: the MFMA operands are restated bit for bit, the product is float64 on the GPU, and the stored bf16 value
# must lie in [bf16(y64 - kappa M), bf16(y64 + kappa M)] (rounding is monotone; for most elements both ends coincide).
# Statistics: from the kernel's OWN stored rows in float64, within bounds derived from the launch geometry
# (oracle.ref_ops.mlp_fwd_stats), the per-workgroup partials included; ci bit for bit from the kernel's mean / rstd.
# tests/test_oracle_cpu.py shows that these checks reject the planted defects at the grid's shapes.
import mlp_fwd_cases as FWD

_WORST_FWD = {}         # (Cin, Cout) -> check -> largest error / bound ("exact": the smallest bit-for-bit share of y)


def _note_fwd(pair, check, ratio):
    _WORST_FWD.setdefault(pair, {})[check] = max(_WORST_FWD.get(pair, {}).get(check, 0.0), ratio)
    _note("fwd " + check, ratio)


@pytest.fixture(scope="module", autouse=True)
def _report_worst_fwd():
    yield
    for (Cin, Cout), w in sorted(_WORST_FWD.items()):
        exact = w.pop("exact", None)
        print(f"\nfwd {Cin:3d} -> {Cout:3d}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(w.items())) +
              ("" if exact is None else f"; y checked bit for bit: >= {100.0 * (1.0 - exact):.1f} % of a case's elements"), end="")


def _fwd_launch(hip, c, slope, affine=True, running=True):
    """One call on fresh copies of the state it updates -> (y, ci, mean, rstd, running_mean, running_var, nbt, part)."""
    Cout = c["W"].shape[-2]
    rm, rv, nbt = (c[k].clone() if running else None for k in ("running_mean", "running_var", "num_batches_tracked"))
    y, ci, mean, rstd = hip.mlp_fwd(c["x"], c["ss"], slope, c["W"], c["nseg"], c["eps"], c["momentum"], rm, rv, nbt,
                                    c["mean_shift"] if running else None, c["gamma"] if affine else None,
                                    c["beta"] if affine else None, mean_rstd=True)
    G = hip.lib.tpg_mlp_fwd_blocks(c["x"].shape[0], c["x"].shape[1], Cout, c["nseg"])
    ws = hip._mlp_ws(c["x"], max(c["x"].shape[1], Cout), c["nseg"])
    part = ws[:c["nseg"] * G * 3 * Cout].view(c["nseg"], G, 3, Cout).clone()
    return y, ci, mean, rstd, rm, rv, nbt, part


def _run_fwd_case(hip, Cin, Cout, P, nseg, per_seg, edge=None, ss_kind="ss", slope=0.01, affine=True, running=True):
    from oracle import ref_ops as R
    kap = R.MLP_KAPPA
    geo = R.mlp_fwd_geometry(P, nseg, Cin, Cout)
    assert geo["G"] == hip.lib.tpg_mlp_fwd_blocks(P * nseg, Cin, Cout, nseg)
    if edge is not None:
        FWD.check_reaches(geo, edge)
    # the deepest fp32 chains: the k-loop's Cin products into one accumulator; a lane's rows, 2 shuffles, 4 waves
    assert Cin * R.U32 <= kap and (geo["lane_rows"] + 6) * R.U32 <= kap
    c = R.mlp_fwd_case(Cin, Cout, P, nseg, per_seg, ss_kind, seed=Cin * 7 + Cout + P + nseg, device="cuda")
    c = dict(c, running_mean=c["running_mean"] if running else None)
    y, ci, mean, rstd, rm, rv, nbt, part = _fwd_launch(hip, c, slope, affine, running)
    torch.cuda.synchronize()
    again = _fwd_launch(hip, c, slope, affine, running)
    for name, u, v in zip("y ci mean rstd rm rv nbt part".split(), (y, ci, mean, rstd, rm, rv, nbt, part), again):
        assert (u is None and v is None) or torch.equal(_bits(u) if u.is_floating_point() else u,
                                                        _bits(v) if v.is_floating_point() else v), ("repro", name)
    # without statistics: the same rows, no constants (and no finalize launch: nothing it writes is passed)
    y2, none = hip.mlp_fwd(c["x"], c["ss"], slope, c["W"], nseg, stats=False)
    assert none is None and torch.equal(_bits(y2), _bits(y)), "stats=False"
    ref = R.mlp_fwd_ref(c, slope)
    _note_fwd((Cin, Cout), "y", R.mlp_fwd_stored_ratio(y, ref, kap))
    lo, hi = R.mlp_fwd_stored_interval(ref, kap)
    _WORST_FWD[(Cin, Cout)]["exact"] = max(_WORST_FWD[(Cin, Cout)].get("exact", 0.0), float((lo != hi).double().mean()))
    del ref, lo, hi
    st = R.mlp_fwd_stats(y, c, geo)
    for k, v in R.mlp_fwd_stats_ratios(st, part, mean, rstd, rm, rv).items():
        _note_fwd((Cin, Cout), k, v)
    want_ci = R.mlp_consts(mean, rstd, c["gamma"] if affine else None, c["beta"] if affine else None, None)[0]
    assert _same_bits(ci, want_ci), "ci"
    if P == 1:
        assert torch.equal(rstd, torch.full_like(rstd, float(np.float32(1.0 / np.sqrt(np.float64(np.float32(1e-5)))))))
    if running:
        assert int(nbt) == int(c["num_batches_tracked"]) + nseg
    else:
        assert rm is None and rv is None and nbt is None


@pytest.mark.parametrize("P,nseg,per_seg,edge", FWD.SHAPES)
@pytest.mark.parametrize("Cin,Cout", FWD.PAIRS)
def test_mlp_fwd_launch_matches_fp64_oracle(hip, Cin, Cout, P, nseg, per_seg, edge):
    """The grid: every channel pair x the launch edges of tests/mlp_fwd_cases.py (several tiles per workgroup with uneven
    counts and a partial last tile, fewer rows than a tile, one row, the finalize's re-fetch path, two sweeps, dead lane
    groups, shared and per-segment weights); input constants as (nseg,2,Cin), slope 0.01, mean_shift, running
    statistics that start away from 0 / 1."""
    _run_fwd_case(hip, Cin, Cout, P, nseg, per_seg, edge)


@pytest.mark.parametrize("ss_kind,slope,affine,running", [
    (None, 0.01, True, True), ("ss", 0.0, True, True), ("ci", 0.2, True, True), ("ss", 1.0, True, True),
    ("ci", 0.01, False, True), ("ss", 0.2, True, False), (None, 0.0, False, False)],
    ids=["noss", "slope0", "ci-slope0.2", "slope1", "ci-noaffine", "norunning", "noss-slope0-bare"])
@pytest.mark.parametrize("nseg", [1, 3])
@pytest.mark.parametrize("Cin,Cout", FWD.PAIRS)
def test_mlp_fwd_launch_variants_match_fp64_oracle(hip, Cin, Cout, nseg, ss_kind, slope, affine, running):
    """At 1000 rows per segment: no input constants / (nseg,2,Cin) / a ci block (nseg,4,Cin), LeakyReLU slopes 0, 0.01,
    0.2 and 1, gamma and beta both None, no running statistics (per-segment weights at nseg = 3)."""
    _run_fwd_case(hip, Cin, Cout, 1000, nseg, nseg > 1, None, ss_kind, slope, affine, running)
