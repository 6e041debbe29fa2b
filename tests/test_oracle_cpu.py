"""Oracle (oracle/tpgref.c) against the independent brute-force statement and hand-built
known-answer cases.  The reference ships no tests or golden vectors for these ops
(SURVEY.md section 4), so op-level parity is UNPINNED; these cases pin the canonical rules."""
import numpy as np
import pytest

from oracle import bruteforce as BF
from oracle import ref_ops as R


def _cloud(rng, B, N, D=3, scale=0.25):
    return rng.uniform(-scale, scale, (B, N, D)).astype(np.float32)


@pytest.mark.parametrize("D,K", [(3, 20), (32, 9), (32, 20), (64, 12), (64, 4), (5, 7)])
def test_knn_matches_bruteforce(D, K):
    rng = np.random.default_rng(D * 100 + K)
    p = rng.standard_normal((2, 150, D)).astype(np.float32)
    p[0, 5] = p[0, 7]          # exact duplicates (MSR-style repeats)
    p[1, 10:14] = p[1, 3]
    d, i = R.knn(p, p, K)
    d2, i2 = BF.knn(p, p, K)
    assert np.array_equal(i, i2) and np.array_equal(d, d2)
    assert np.array_equal(i[:, :, 0][0][:5], np.arange(5))  # self is nn #0


def test_knn_duplicates_order_by_index():
    p2 = np.zeros((1, 6, 3), np.float32)
    p2[0, :, 0] = [1, 0, 1, 0, 1, 0]
    q = np.zeros((1, 1, 3), np.float32)
    d, i = R.knn(q, p2, 6)
    assert i[0, 0].tolist() == [1, 3, 5, 0, 2, 4]
    assert d[0, 0].tolist() == [0, 0, 0, 1, 1, 1]


def test_knn_999_dummies():
    rng = np.random.default_rng(3)
    p = _cloud(rng, 1, 64)
    p[0, 40:] = 999.0  # hard-masking pads (upsampling_network.py:149)
    d, i = R.knn(p, p, 8)
    d2, i2 = BF.knn(p, p, 8)
    assert np.array_equal(i, i2)
    assert i[0, 45].tolist() == list(range(40, 48))  # ties among identical dummies -> index order


def test_knn_ragged_and_short():
    rng = np.random.default_rng(4)
    p1, p2 = _cloud(rng, 3, 20), _cloud(rng, 3, 30)
    l1, l2 = np.array([20, 7, 0]), np.array([30, 4, 9])
    d, i = R.knn(p1, p2, 6, l1, l2)
    d2, i2 = BF.knn(p1, p2, 6, l1, l2)
    assert np.array_equal(i, i2) and np.array_equal(d, d2)
    assert (i[1, :7, 4:] == 0).all() and (d[1, :7, 4:] == 0).all()  # K > len2 -> zero pad
    assert (i[2] == 0).all()                                         # len1 == 0


@pytest.mark.parametrize("K,r", [(1, 0.0475), (16, 0.035), (32, 2.0), (8, 0.01)])
def test_frnn_matches_bruteforce(K, r):
    rng = np.random.default_rng(K)
    p1, p2 = _cloud(rng, 2, 64), _cloud(rng, 2, 300)
    d, i = R.knn(p1, p2, K, r=r)
    d2, i2 = BF.knn(p1, p2, K, r=r)
    assert np.array_equal(i, i2) and np.array_equal(d, d2)
    assert ((i == -1) == (d == -1)).all()


def test_frnn_strict_radius():
    q = np.zeros((1, 1, 3), np.float32)
    p2 = np.array([[[0.5, 0, 0], [0.25, 0, 0], [0.5000001, 0, 0]]], np.float32)
    d, i = R.knn(q, p2, 3, r=0.5)  # d^2 == r^2 is OUT (strict <)
    assert i[0, 0].tolist() == [1, -1, -1]
    assert d[0, 0].tolist() == [0.0625, -1, -1]


@pytest.mark.parametrize("N,m", [(500, 64), (64, 64), (10, 25)])
def test_fps_matches_bruteforce(N, m):
    rng = np.random.default_rng(N)
    x = _cloud(rng, 2, N)
    x[0, 3] = 0.0          # origin point: never eligible (|x|^2 <= 1e-3)
    x[1, :3] = 999.0       # dummies
    assert np.array_equal(R.fps(x, m), BF.fps(x, m))


def test_fps_known_answers():
    # 4 collinear points; start at 0; farthest from 0 is 3; then 1 vs 2: temp = min dist to {0,3}
    x = np.array([[[1, 0, 0], [2, 0, 0], [3.5, 0, 0], [5, 0, 0]]], np.float32)
    assert R.fps(x, 4)[0].tolist() == [0, 3, 2, 1]
    # duplicates: ties -> smallest index
    x = np.array([[[1, 0, 0], [3, 0, 0], [3, 0, 0], [3, 0, 0]]], np.float32)
    assert R.fps(x, 3)[0].tolist() == [0, 1, 0]  # tie 1/2/3 -> 1; then every temp is 0 -> smallest index
    # all points within the origin ball: nothing eligible -> index 0 repeated
    x = np.full((1, 5, 3), 0.01, np.float32)
    assert R.fps(x, 4)[0].tolist() == [0, 0, 0, 0]


def test_fps_more_samples_than_points_does_not_crash():
    rng = np.random.default_rng(0)
    x = _cloud(rng, 1, 8) + 1.0
    out = R.fps(x, 20)
    assert out.shape == (1, 20) and (out >= 0).all() and (out < 8).all()


@pytest.mark.parametrize("r,ns", [(0.1, 16), (0.15, 32), (0.6, 16), (0.005, 8)])
def test_ball_query_matches_bruteforce(r, ns):
    rng = np.random.default_rng(ns)
    x = _cloud(rng, 2, 400)
    q = x[:, ::5].copy()
    assert np.array_equal(R.ball_query(r, ns, x, q), BF.ball_query(r, ns, x, q))


def test_ball_query_known_answers():
    x = np.zeros((1, 6, 3), np.float32)
    x[0, :, 0] = [5, 0.1, 5, 0.2, 0.3, 5]
    q = np.zeros((1, 2, 3), np.float32)
    q[0, 1, 0] = 100.0
    idx = R.ball_query(1.0, 4, x, q)
    assert idx[0, 0].tolist() == [1, 3, 4, 1]   # index order; tail filled with FIRST hit
    assert idx[0, 1].tolist() == [0, 0, 0, 0]   # no hit -> zeros
    idx = R.ball_query(1.0, 2, x, q)
    assert idx[0, 0].tolist() == [1, 3]         # stops at nsample


def test_group_gather_roundtrip():
    rng = np.random.default_rng(1)
    f = rng.standard_normal((2, 7, 100)).astype(np.float32)
    idx = rng.integers(0, 100, (2, 30, 5)).astype(np.int32)
    idx[0, 0] = 7  # repeated index
    out = R.group_fwd(f, idx)
    assert np.array_equal(out, BF.group_fwd(f, idx))
    g = rng.standard_normal(out.shape).astype(np.float32)
    assert np.allclose(R.group_bwd(g, idx, 100), BF.group_bwd(g, idx, 100), atol=1e-5)
    gi = idx[:, :, 0].copy()
    assert np.array_equal(R.gather_fwd(f, gi), BF.gather_fwd(f, gi))
    gg = rng.standard_normal((2, 7, 30)).astype(np.float32)
    ref = np.zeros((2, 7, 100))
    for b in range(2):
        for c in range(7):
            np.add.at(ref[b, c], gi[b], gg[b, c])
    assert np.allclose(R.gather_bwd(gg, gi, 100), ref, atol=1e-5)


def test_chamfer_hand_computed():
    s = np.array([[[0, 0, 0], [1, 0, 0]]], np.float32)
    t = np.array([[[0, 0, 0.5], [1, 0, 0], [4, 0, 0]]], np.float32)
    d1, i1, d2, i2 = R.chamfer_fwd(s, t)
    assert d1[0].tolist() == [0.25, 0.0] and i1[0].tolist() == [0, 1]
    assert d2[0].tolist() == [0.25, 0.0, 9.0] and i2[0].tolist() == [0, 1, 1]
    gs, gt = R.chamfer_bwd(s, t, i1, i2, np.ones_like(d1), np.ones_like(d2))
    # d(sum)/ds0 = 2(s0-t0) [fwd] + 2(s0-t0) [bwd term of t0]
    assert np.allclose(gs[0, 0], [0, 0, -2.0])
    assert np.allclose(gs[0, 1], [-6.0, 0, 0])       # t2 pulls s1: -2(t2 - s1)
    assert np.allclose(gt[0, 2], [6.0, 0, 0])


def test_chamfer_matches_bruteforce_value_and_numeric_grad():
    rng = np.random.default_rng(5)
    s, t = _cloud(rng, 2, 40), _cloud(rng, 2, 55)
    d1, i1, d2, i2 = R.chamfer_fwd(s, t)
    val = d1.sum(1).mean() + d2.sum(1).mean()
    assert abs(val - BF.chamfer(s, t)) < 1e-5
    gs, _ = R.chamfer_bwd(s, t, i1, i2, np.full_like(d1, 0.5), np.full_like(d2, 0.5))
    eps = 1e-3
    s2 = s.copy(); s2[1, 3, 1] += eps
    num = (BF.chamfer(s2, t) - BF.chamfer(s, t)) / eps
    assert abs(num - gs[1, 3, 1]) < 5e-3


def test_three_nn_and_interpolate():
    rng = np.random.default_rng(6)
    u, k = _cloud(rng, 2, 30), _cloud(rng, 2, 50)
    d2, idx = R.three_nn(u, k)
    bd, bi = BF.three_nn(u, k)
    assert np.array_equal(idx, bi) and np.array_equal(d2, bd)
    f = rng.standard_normal((2, 4, 50)).astype(np.float32)
    w = rng.uniform(0, 1, (2, 30, 3)).astype(np.float32)
    out = R.three_interp_fwd(f, idx, w)
    ref = np.stack([(f[b][:, idx[b]] * w[b][None]).sum(-1) for b in range(2)])
    assert np.allclose(out, ref, atol=1e-5)
    g = rng.standard_normal(out.shape).astype(np.float32)
    gf = R.three_interp_bwd(g, idx, w, 50)
    ref = np.zeros((2, 4, 50))
    for b in range(2):
        for c in range(4):
            np.add.at(ref[b, c], idx[b].reshape(-1), (g[b, c][:, None] * w[b]).reshape(-1))
    assert np.allclose(gf, ref, atol=1e-5)


# ------------------------------------------------------------------ cubic interpolation (--use_vel)
@pytest.mark.parametrize("case", ["dense", "with_far_queries", "coincident"])
def test_cubic_interpolation_matches_the_reference_algorithm(case, oracle_cpu):
    """ops.cubic_interpolation (one fused search-and-sum per batch + the padding selection) against
    the reference's algorithm written out as an edge list (oracle/bruteforce.py): FRNN-32, unique,
    FRNN again, kNN-4 padding multigraph, DGL-style scatter sums.  PARITY UNPINNED against DGL itself
    (not installable here); the edge-list statement follows gcn_lib/interpolation.py line by line."""
    import torch
    import tpgan_amd.ops as ops
    rng = np.random.default_rng({"dense": 0, "with_far_queries": 1, "coincident": 2}[case])
    B, Np, Nq, F, cutoff = 2, 300, 96, 3, 0.16
    pos = rng.uniform(-0.3, 0.3, (B, Np, 3)).astype(np.float32)
    field = rng.standard_normal((B, Np, F)).astype(np.float32)
    query = rng.uniform(-0.3, 0.3, (B, Nq, 3)).astype(np.float32)
    if case == "with_far_queries":            # 999-dummies of a masked prediction: no hit -> padding active
        query[0, :7] = 999.0
        query[0, 7:20] = rng.uniform(0.36, 0.4, (13, 3))          # few hits
    if case == "coincident":
        query[:, :40] = pos[:, :40]                                # d = 0 exactly
    got = ops.cubic_interpolation(torch.from_numpy(query), torch.from_numpy(field), torch.from_numpy(pos), cutoff).numpy()
    for b in range(B):
        want = BF.cubic_interpolation(query[b], field[b], pos[b], cutoff)
        assert np.abs(got[b] - want).max() <= 1e-5 * max(1.0, np.abs(want).max()), (case, b)
    if case == "with_far_queries":
        assert np.all(got[0, :7] == 0.0)                           # no neighbours: 0 / (0 + 1e-6)
    # the per-sample 2-D signature of the reference
    one = ops.cubic_interpolation(torch.from_numpy(query[1]), torch.from_numpy(field[1]), torch.from_numpy(pos[1]), cutoff)
    assert np.array_equal(one.numpy(), got[1])


def test_dataset_fps_random_start_no_origin_skip(oracle_cpu):
    """sampling.py:50-106 restated in numpy (squared fp32 distances, argmax = first maximum, start
    index given, NO |x|^2 > 1e-3 rule) against the oracle's start variant and ops.farthest_point_sampling."""
    import torch
    import tpgan_amd.ops as ops
    rng = np.random.default_rng(4)
    pts = rng.standard_normal((2, 700, 3)).astype(np.float32) * 0.2
    pts[0, 5] = 0.0                                    # at the origin: eligible here, skipped by pointnet2's rule
    pts[1, :40] *= 0.05
    start = np.array([17, 300], np.int32)
    got = R.fps_start(pts, 64, start, skip_origin=False)
    for b in range(2):
        x = pts[b]
        idx = [int(start[b])]
        mind = ((x - x[idx[0]]) ** 2).sum(-1, dtype=np.float32)
        for _ in range(63):
            j = int(np.argmax(mind))
            idx.append(j)
            mind = np.minimum(mind, ((x - x[j]) ** 2).sum(-1, dtype=np.float32))
        assert np.array_equal(got[b], np.array(idx)), b
    t = ops.farthest_point_sampling(torch.from_numpy(pts), 64, initial_idx=start.tolist())
    assert np.array_equal(t.numpy(), got)
    one = ops.farthest_point_sampling(torch.from_numpy(pts[1]), 64, initial_idx=300)
    assert np.array_equal(one.numpy(), got[1])
    d = ops.sample_patch_with_fps(torch.from_numpy(pts[0]), 256, seed_idx=3, initial_idx=0)
    assert d["patch_pos"].shape == (256, 3) and d["ds_pos"].shape == (32, 3) and int(d["patch_idx"][0]) == 3


def test_dataset_fps_oracle_matches_the_reference_fixture():
    """f4 pinned to the reference: tests/golden/sampling_fps.npz holds the indices
    `/root/reference/sampling.py:50-106` itself returned (capture_goldens.py, numba shim) for
    three clouds incl. exact duplicates, a point at the origin and a run of repeats."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampling_fps.npz"))
    for tag in ("fluid", "dup", "origin"):
        pts, k, start = g[f"{tag}/pts"], int(g[f"{tag}/k"]), int(g[f"{tag}/start"])
        got = R.fps_start(pts[None], k, np.array([start], np.int32), skip_origin=False)[0]
        assert np.array_equal(got, g[f"{tag}/idx"]), tag


# ------------------------------------------------------------------ the fused MLP tail's backward, launch by launch
def _tail_autograd(x0, gammas, betas, Ws, slopes, K, nseg, eps):
    """BatchNorm1d(train) -> LeakyReLU -> Linear(no bias) -> ... -> BatchNorm1d -> LeakyReLU -> max over K, float64,
    nseg calls on equal consecutive row blocks (one weight per call or one for all)."""
    import torch
    import torch.nn.functional as F
    P = x0.shape[0] // nseg
    outs = []
    for s in range(nseg):
        a = x0[s * P:(s + 1) * P]
        for l in range(len(gammas)):
            z = F.batch_norm(a, None, None, gammas[l], betas[l], training=True, eps=eps)
            a = F.leaky_relu(z, slopes[l])
            if l < len(Ws):
                a = a @ (Ws[l][s] if Ws[l].dim() == 3 else Ws[l]).t()
        outs.append(a.view(P // K, K, -1).max(1)[0])
    return torch.cat(outs)


@pytest.mark.parametrize("chain", [(8, 16), (16, 8, 24)])
@pytest.mark.parametrize("nseg,per_seg", [(1, False), (3, False), (3, True)])
@pytest.mark.parametrize("K", [1, 7])
@pytest.mark.parametrize("slope", [0.01, 0.0])
def test_mlp_tail_backward_restatements_chain_to_autograd(chain, nseg, per_seg, K, slope):
    """The per-launch restatements of the fused tail's backward (oracle.ref_ops: mlp_consts, mlp_max_prep, the dgrad /
    wgrad contractions, the finalize's c12 / cb, mlp_bn_bwd_apply), with every rounding switched off, chained exactly as
    ops._MlpTail.backward chains the launches, against torch.autograd in float64 on the plain statement of the tail.
    This pins the folded constants (a, f*mu, e, f, c12) and both rank-one terms (e^T W, e (x) sum a_in) independently
    of any GPU: any algebra slip is O(1), rounding is off, so the bound is 1e-10 relative."""
    import torch
    A = R.FP64
    eps = 1e-5
    L = len(chain) - 1
    g = torch.Generator().manual_seed(sum(chain) * 10 + nseg + K)
    P = 9 * K if K > 1 else 40                     # rows per segment
    x0 = torch.randn(nseg * P, chain[0], generator=g, dtype=torch.float64) + torch.randn(chain[0], generator=g, dtype=torch.float64)
    gam = [torch.rand(c, generator=g, dtype=torch.float64) + 0.5 for c in chain]
    bet = [0.3 * torch.randn(c, generator=g, dtype=torch.float64) for c in chain]
    Ws = [torch.randn(*((nseg,) if per_seg else ()), chain[l + 1], chain[l], generator=g, dtype=torch.float64) / chain[l] ** 0.5
          for l in range(L)]
    slopes = [slope] * (L + 1)
    # ---- forward as the kernels fold it: statistics -> ci, x_{l+1} = W . lrelu(sc*x + sh)
    xs, cis, stats = [x0], [], []
    for l in range(L + 1):
        xv = xs[-1].view(nseg, P, -1)
        mean, rstd = xv.mean(1), 1.0 / torch.sqrt(xv.var(1, unbiased=False) + eps)
        stats.append((mean, rstd))
        cis.append(R.mlp_consts(mean, rstd, gam[l], bet[l], None, A)[0])
        if l < L:
            sc, sh = (R._rows(cis[-1][:, i], P) for i in (0, 1))
            z = xs[-1] * sc + sh
            a = torch.where(z > 0, z, z * slope)
            xs.append(torch.cat([a[s * P:(s + 1) * P] @ (Ws[l][s] if per_seg else Ws[l]).t() for s in range(nseg)]))
    sc, sh = (R._rows(cis[L][:, i], P) for i in (0, 1))
    z = xs[L] * sc + sh
    yk = torch.where(z > 0, z, z * slope).view(-1, K, chain[-1])
    out, arg = yk.max(1)
    if K > 1:        # no ties in the max (slope 0: tied zeros pass no gradient whichever row wins)
        top = yk.topk(2, 1)[0]
        assert ((top[:, 0] > top[:, 1]) | (top[:, 0] == 0)).all()
    gout = torch.randn(out.shape, generator=g, dtype=torch.float64)
    # ---- the last BatchNorm's backward sums (tpg_rowbn_bwd_sums_consts): gg lives on the arg-max rows
    full = torch.zeros(nseg * P // K, K, chain[-1], dtype=torch.float64)
    full.scatter_(1, arg[:, None], gout[:, None])
    mean, rstd = stats[L]
    xhat = (xs[L] - R._rows(mean, P)) * R._rows(rstd, P)
    gg = full.view(-1, chain[-1]) * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    s1, sx = gg.view(nseg, P, -1).sum(1), (gg * xhat).view(nseg, P, -1).sum(1)
    c12 = torch.stack([s1 / P, sx / P], 1)
    got = {f"dgamma{L}": sx.sum(0), f"dbeta{L}": s1.sum(0)}
    cb = R.mlp_consts(mean, rstd, gam[L], bet[L], c12, A)[1]
    gnext = R.mlp_max_prep(gout, out, cb, slope, nseg, A)
    argn, Kn = arg.to(torch.uint8), K
    for l in range(L, 0, -1):
        ops = R.mlp_bwd_operands(xs[l], gnext, argn, Kn, cb, xs[l - 1], cis[l - 1], slope, nseg, A, round_d=False)
        dW = R.mlp_wgrad_ref(ops)["dW"]
        got[f"dW{l}"] = dW if per_seg else dW.sum(0)
        dg = R.mlp_dgrad_ref(ops, Ws[l - 1])
        got[f"dgamma{l - 1}"], got[f"dbeta{l - 1}"] = dg["dgamma"], dg["dbeta"]
        c12 = dg["c12"]
        cb = R.mlp_finalize_cb(cis[l - 1], c12, A)
        gnext, argn, Kn = dg["g"], None, 0
    got["dx0"] = R.mlp_bn_bwd_apply(gnext, x0, cis[0], c12, nseg, 0, A)
    # ---- autograd on the plain statement
    leaves = [x0.clone().requires_grad_(True)] + [w.clone().requires_grad_(True) for w in Ws] + \
             [t.clone().requires_grad_(True) for t in gam + bet]
    ref = _tail_autograd(leaves[0], leaves[1 + L:2 + 2 * L], leaves[2 + 2 * L:], leaves[1:1 + L], slopes, K, nseg, eps)
    assert torch.allclose(ref, out, rtol=1e-12, atol=1e-12)
    grads = torch.autograd.grad(ref, leaves, gout)
    names = ["dx0"] + [f"dW{l + 1}" for l in range(L)] + [f"dgamma{l}" for l in range(L + 1)] + [f"dbeta{l}" for l in range(L + 1)]
    for name, w in zip(names, grads):
        rel = float((got[name] - w).abs().max() / w.abs().max())
        assert rel <= 1e-10, (name, rel)


def _emulated(case, nseg, cbo=None, arg=None):
    """The oracle's emulated level of one launch pair on a case of R.mlp_bwd_case (constants folded by the oracle)."""
    ci_in = R.mlp_consts(case["mean_in"], case["rstd_in"], case["gamma_in"], case["beta_in"], None)[0]
    cb_out = R.mlp_consts(case["mean_out"], case["rstd_out"], case["gamma_out"], case["beta_out"], case["c12_out"])[1]
    cb_out = cb_out if cbo is None else cbo
    K = case["K"]
    g_arg = R.mlp_max_prep(case["gout"], case["y"], cb_out, 0.01, nseg) if K else case["g_out"]
    ops = R.mlp_bwd_operands(case["x_out"], g_arg, case["arg"] if arg is None else arg, K, cb_out, case["x_in"], ci_in,
                             0.01, nseg)
    return ops, cb_out


@pytest.mark.parametrize("Cin,Cout,P,nseg,per_seg,K", [(64, 128, 4096, 1, False, 32), (128, 128, 2997, 3, True, 9)])
def test_mlp_bwd_bounds_reject_planted_defects(Cin, Cout, P, nseg, per_seg, K):
    """The per-element bounds that tests/test_mlp_gpu.py applies to tpg_mlp_dgrad / tpg_mlp_wgrad (R.gin_bound,
    R.dw_bound at kappa = R.MLP_KAPPA) accept the oracle's own output, stored as the kernels store it, and reject each
    defect planted into it at the shapes of the GPU grid -- the evidence that the bounds mean something.  The old
    test's L2 bound of 3e-2 lets the one-row defects through (asserted too)."""
    import torch
    kap = R.MLP_KAPPA
    case = R.mlp_bwd_case(Cin, Cout, P, nseg, per_seg, K, True, 0.01, seed=P + Cin)
    ops, cb_out = _emulated(case, nseg)
    dg, wg = R.mlp_dgrad_ref(ops, case["W"]), R.mlp_wgrad_ref(ops)
    g_ok, dW_ok = R.rbf16(R.r32(dg["g"])), R.r32(wg["dW"])           # stored as the kernels store them

    def g_ratio(g):
        return R.err_ratio(g, dg["g"], R.gin_bound(dg["g"], dg["M"], dg["R"], kap))

    def w_ratio(dW):
        return R.err_ratio(dW, wg["dW"], R.dw_bound(wg["M"], wg["R"], kap))

    def l2(a, b):
        return float((a - b).norm() / b.norm())
    assert g_ratio(g_ok) <= 1.0 and w_ratio(dW_ok) <= 1.0
    d, A, m = ops["d"], ops["a_in"], ops["m"]
    seg = nseg - 1
    last = seg * P + P - 1                         # the ragged last tile's last row (P % 64 != 0 at 2997)
    row = seg * P + P // 3

    def row_term(r):
        return torch.outer(d[r] + ops["e"][r // P], A[r])
    # one row counted twice; one row dropped
    for r in (row, last):
        dW = dW_ok.clone()
        dW[r // P] += row_term(r)
        assert w_ratio(dW) > 1.0, ("row twice", r)
        assert l2(dW, wg["dW"]) < 3e-2              # what the 3e-2 L2 bound of the tail tests let through
        dW = dW_ok.clone()
        dW[r // P] -= row_term(r)
        g = g_ok.clone()
        g[r] = 0.0
        assert w_ratio(dW) > 1.0 and g_ratio(g) > 1.0, ("row dropped", r)
    # segment s reading segment s+1's constants (nseg > 1), or a perturbation of the same size (nseg = 1: 2 %)
    cbo = cb_out.clone()
    if nseg > 1:
        cbo[0] = cb_out[1]
    else:
        cbo[0] = cb_out[0] * 1.02
    ops2, _ = _emulated(case, nseg, cbo=cbo)
    assert g_ratio(R.rbf16(R.r32(R.mlp_dgrad_ref(ops2, case["W"])["g"]))) > 1.0, "cb of segment s+1"
    assert w_ratio(R.r32(R.mlp_wgrad_ref(ops2)["dW"])) > 1.0, "cb of segment s+1"
    # the rank-one terms left out
    sA = torch.stack([A[s * P:(s + 1) * P].sum(0) for s in range(nseg)])
    assert w_ratio(dW_ok - ops["e"][:, :, None] * sA[:, None, :]) > 1.0, "e (x) sum a_in left out"
    Wb = R.rbf16(R._f64(case["W"])).view(-1, Cout, Cin)
    eW = torch.cat([(ops["e"][s] @ Wb[s if Wb.shape[0] > 1 else 0])[None].expand(P, Cin) for s in range(nseg)])
    assert g_ratio(R.rbf16(R.r32(dg["g"] - eW * m))) > 1.0, "e^T W left out"
    # one 16-channel output tile of dW zeroed
    dW = dW_ok.clone()
    dW[:, 16:32] = 0.0
    assert w_ratio(dW) > 1.0, "16-channel tile"
    # the arg-max of one group routed to k+1
    arg = case["arg"].clone()
    grp = (seg * P + P // 2) // K
    arg[grp] = (arg[grp].long() + 1) % K
    ops3, _ = _emulated(case, nseg, arg=arg)
    assert g_ratio(R.rbf16(R.r32(R.mlp_dgrad_ref(ops3, case["W"])["g"]))) > 1.0, "arg-max to k+1"
    # W left in fp32
    assert g_ratio(R.rbf16(R.r32(R.mlp_dgrad_ref(ops, case["W"], round_w=False)["g"]))) > 1.0, "W not rounded"


def test_mlp_wgrad_bound_rejects_a_duplicated_row_tile():
    """65535 rows of the 128 -> 256 layer (several tiles per workgroup, a partial last tile, K = 255): one 64-row tile
    counted twice must fail the per-element dW bound (it passes the old 3e-2 L2 bound)."""
    import torch
    P, K = 65535, 255
    case = R.mlp_bwd_case(128, 256, P, 1, False, K, True, 0.01, seed=7)
    ops, _ = _emulated(case, 1)
    wg = R.mlp_wgrad_ref(ops)
    bound = R.dw_bound(wg["M"], wg["R"], R.MLP_KAPPA)
    assert R.err_ratio(R.r32(wg["dW"]), wg["dW"], bound) <= 1.0
    rows = slice(64 * 500, 64 * 501)
    dup = (ops["d"][rows] + ops["e"][0]).t() @ ops["a_in"][rows]
    bad = wg["dW"][0] + dup
    assert R.err_ratio(bad[None], wg["dW"], bound) > 1.0
    assert float(dup.norm() / wg["dW"].norm()) < 3e-2


def test_mlp_contract_bound_rejects_an_uncentred_operand():
    """The channel of x_out with |mu| / sigma ~ 1e3 (R.mlp_bwd_case): were the MFMA operand formed uncentred again --
    the bf16 rounding taken on a*g - f*x, of size |f mu|, before f*mu is added back -- the contract-level dW bound
    would fail, while the kernels' centred operand (the emulated oracle) passes it."""
    import torch
    P, nseg = 4096, 1
    case = R.mlp_bwd_case(64, 128, P, nseg, False, 0, False, 0.01, seed=3)
    ci_in = R.mlp_consts(case["mean_in"], case["rstd_in"], case["gamma_in"], case["beta_in"], None)[0]
    cb = R.mlp_consts(case["mean_out"], case["rstd_out"], case["gamma_out"], case["beta_out"], case["c12_out"])[1]
    args = (case["x_out"], case["g_out"], None, 0, cb, case["x_in"], ci_in, 0.01, nseg)
    exact = R.mlp_bwd_operands(*args, round_d=False)
    wg = R.mlp_wgrad_ref(exact)
    bound = R.dw_bound(wg["M"], wg["R"], R.MLP_KAPPA)
    centred = R.mlp_bwd_operands(*args)
    assert R.err_ratio(R.r32(R.mlp_wgrad_ref(centred)["dW"]), wg["dW"], bound) <= 1.0
    a, fm, f = (R._rows(R._f64(cb)[:, i], P) for i in (0, 1, 3))
    x, g = R._f64(case["x_out"]), R._f64(case["g_out"])
    unc = dict(centred)
    unc["d"] = R.r32(R.rbf16(R.fma32(a, g, R.r32(-f * x))) + fm)
    assert R.err_ratio(R.r32(R.mlp_wgrad_ref(unc)["dW"]), wg["dW"], bound) > 1.0


# ------------------------------------------------------------------ the fused MLP forward: geometry, bounds, planted defects
def test_mlp_fwd_geometry_equals_the_launcher(hip_lib):
    """R.mlp_fwd_geometry against tpg_mlp_fwd_blocks over the whole grid of tests/mlp_fwd_cases.py (and a few row counts
    around the caps), and every shape reaches the launch edge its row names."""
    import mlp_fwd_cases as S
    for Cin, Cout in S.PAIRS:
        for P, nseg, _, edge in S.SHAPES:
            geo = R.mlp_fwd_geometry(P, nseg, Cin, Cout)
            assert geo["G"] == hip_lib.tpg_mlp_fwd_blocks(P * nseg, Cin, Cout, nseg), (Cin, Cout, P, nseg)
            assert int(geo["n_wg"].sum()) == P and int(geo["tiles_wg"].sum()) == geo["tiles"]
            S.check_reaches(geo, edge)
        for P, nseg in [(16384, 6), (32768, 1), (65, 1), (128 * 512 + 1, 1), (64 * 256, 2), (3000, 40)]:
            assert R.mlp_fwd_geometry(P, nseg, Cin, Cout)["G"] == hip_lib.tpg_mlp_fwd_blocks(P * nseg, Cin, Cout, nseg)
    assert hip_lib.tpg_mlp_fwd_blocks(4096, 64, 256, 1) == 0 and hip_lib.tpg_mlp_fwd_blocks(7, 64, 64, 2) == 0
    # the real configuration the issue names: six segments of 16384 rows leave the finalize's registers
    geo = R.mlp_fwd_geometry(16384, 6, 64, 128)
    assert (geo["fin_L"], geo["G"], geo["fits"]) == (8, 85, False)


def _stored_rows(P, nseg, C, seed):
    """bf16 rows as a forward launch might have stored them: per-channel and per-segment offsets, channel
    R.MLP_FWD_MU_CHANNEL at 8 + 2^-4 on one row in 61 (|mean| / sigma ~ 1e3)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(nseg * P, C, generator=g) + torch.randn(C, generator=g)
    y = y + (0.3 * torch.randn(nseg, C, generator=g)).repeat_interleave(P, 0)
    r = torch.arange(nseg * P) % P
    y[:, R.MLP_FWD_MU_CHANNEL] = 8.0 + (r % 61 == 0) * 2.0 ** -4
    return y.bfloat16()


def _stats_case(P, nseg, C, seed):
    import torch
    g = torch.Generator().manual_seed(seed + 1)
    return dict(nseg=nseg, P=P, eps=1e-5, momentum=0.1, mean_shift=torch.randn(C, generator=g),
                running_mean=0.5 * torch.randn(C, generator=g), running_var=torch.rand(C, generator=g) + 0.5)


def test_mlp_fwd_statistics_bounds_hold_for_the_kernels_arithmetic():
    """The forward epilogue's statistics restated op for op in fp32 (R.mlp_fwd_partials_emulated) and finalized in fp64
    lie within the bounds R.mlp_fwd_stats derives from the geometry alone, at every shape of the GPU grid and the
    geometry of every channel pair (8 stored channels stand for Cout: the bounds are per channel)."""
    import mlp_fwd_cases as S
    worst = {}
    for Cin, Cout in [(64, 128), (128, 256), (256, 256)]:           # 128-row tiles; 64-row tiles; the cap of 256
        for P, nseg, per_seg, edge in S.SHAPES:
            if not per_seg and (P, nseg, True, edge) in S.SHAPES:
                continue
            geo = R.mlp_fwd_geometry(P, nseg, Cin, Cout)
            case, y = _stats_case(P, nseg, 8, P + nseg), _stored_rows(P, nseg, 8, P + Cin)
            st = R.mlp_fwd_stats(y, case, geo)
            part = R.mlp_fwd_partials_emulated(y, case, geo)
            fin = R.mlp_fwd_finalize(part, case)
            for k, v in R.mlp_fwd_stats_ratios(st, part, **fin).items():
                worst[k] = max(worst.get(k, 0.0), v)
                assert v <= 1.0, (Cin, Cout, P, nseg, k, v)
            assert (geo["lane_rows"] + 6) * R.U32 <= R.MLP_KAPPA
            if P == 1:
                assert float(st["var"].abs().max()) == 0.0 and float(st["E_rstd"].max()) <= 2.1 * R.U32 * 1e5 ** 0.5
    print("\nemulated epilogue, largest error / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))


def test_mlp_fwd_bounds_reject_planted_defects():
    """Each defect planted into a correct float64-derived result of the forward at the GPU grid's shapes must fail the
    check that tests/test_mlp_gpu.py applies (the stored-value interval at kappa = R.MLP_KAPPA, the statistics bounds of
    R.mlp_fwd_stats); the unmodified result passes each."""
    import torch
    kap = R.MLP_KAPPA
    seen = []

    def rej(name, ratio):
        seen.append(f"{name}: {ratio:.3g}")
        assert ratio > 1.0, (name, ratio)
    # ---- 64 -> 128 at 70001 rows: 547 tiles of 128 rows on 512 workgroups, the first 35 walk two tiles
    Cin, Cout, P, nseg = 64, 128, 70001, 1
    geo = R.mlp_fwd_geometry(P, nseg, Cin, Cout)
    case = R.mlp_fwd_case(Cin, Cout, P, nseg, False, "ss", seed=1)
    ref = R.mlp_fwd_ref(case, 0.01)
    y_ok = R.rbf16(R.r32(ref["y"]))
    assert Cin * R.U32 <= kap and R.mlp_fwd_stored_ratio(y_ok, ref, kap) <= 1.0
    y = y_ok.clone()                                    # one row's product computed from the neighbouring row
    y[P // 2] = y_ok[P // 2 + 1]
    rej("y: a row's product from the neighbouring row", R.mlp_fwd_stored_ratio(y, ref, kap))
    G, BM = geo["G"], geo["BM"]                         # one k-step dropped on a workgroup's second tile
    assert geo["tiles_wg"][3] == 2
    rows = slice((3 + G) * BM, (4 + G) * BM)
    a = ref["a"].clone()
    a[rows, 32:64] = 0.0
    y = y_ok.clone()
    y[rows] = R.rbf16(R.r32(R.mlp_fwd_ref(case, 0.01, a=a)["y"][rows]))
    rej("y: one k-step dropped on a second tile", R.mlp_fwd_stored_ratio(y, ref, kap))
    T = Cout // 16                                      # two output channels swapped (column j*T + t read as t*16 + j)
    y = y_ok.clone()
    y[:, [1, T]] = y_ok[:, [T, 1]]
    rej("y: two output channels swapped", R.mlp_fwd_stored_ratio(y, ref, kap))
    # statistics of the stored rows
    st = R.mlp_fwd_stats(y_ok, case, geo)
    part_ok = torch.stack([st["part_mean"], st["part_M2"], st["part_n"]], 2)
    ok = R.mlp_fwd_finalize(R.r32(part_ok), case)
    assert max(R.mlp_fwd_stats_ratios(st, R.r32(part_ok), **ok).values()) <= 1.0
    emu = R.mlp_fwd_partials_emulated(y_ok, case, geo)
    assert max(R.mlp_fwd_stats_ratios(st, emu, **R.mlp_fwd_finalize(emu, case)).values()) <= 1.0
    tail = dict(case, P=P + 1)                          # the clamped tail row counted as a row
    y_t = torch.cat([y_ok, y_ok[-1:]])
    geo_t = R.mlp_fwd_geometry(P + 1, nseg, Cin, Cout)
    assert geo_t["G"] == G and geo_t["last_wg"] == geo["last_wg"]
    bad = R.mlp_fwd_partials_emulated(y_t, tail, geo_t)
    r = R.mlp_fwd_stats_ratios(st, bad, **R.mlp_fwd_finalize(bad, tail))
    for k in ("part_n", "part_mean", "mean", "rstd", "running_mean"):
        rej("a clamped tail row counted, " + k, r[k])
    bad = emu.clone()                                   # a partial's n off by one, nothing else
    bad[0, geo["last_wg"], 2] += 1.0
    rej("a partial's n off by one, part_n", R.mlp_fwd_stats_ratios(st, bad)["part_n"])
    bad = R.mlp_fwd_partials_emulated(y_ok, case, geo, pivot_zero=True)      # E[x^2] - E[x]^2 in fp32
    r = R.mlp_fwd_stats_ratios(st, bad, **R.mlp_fwd_finalize(bad, case))
    mu = R.MLP_FWD_MU_CHANNEL
    sig = float(st["var"][0, mu].sqrt())
    assert 300.0 < float(st["mean"][0, mu].abs()) / sig < 3000.0
    for k in ("part_M2", "rstd"):
        rej("no pivot, sums in fp32, " + k, r[k])
    rej("no pivot, part_M2 of the |mean| >> sigma channel",
        R.err_ratio(bad[:, :, 1, mu], st["part_M2"][..., mu], st["E_part_M2"][..., mu]))
    # ---- 70 segments of 1100 rows: the running chain in the wrong segment order across the two sweeps
    Cin, Cout, P, nseg = 64, 64, 1100, 70
    geo = R.mlp_fwd_geometry(P, nseg, Cin, Cout)
    case = R.mlp_fwd_case(Cin, Cout, P, nseg, True, "ci", seed=2)
    y_ok = R.rbf16(R.r32(R.mlp_fwd_ref(case, 0.01)["y"]))
    st = R.mlp_fwd_stats(y_ok, case, geo)
    emu = R.mlp_fwd_partials_emulated(y_ok, case, geo)
    assert max(R.mlp_fwd_stats_ratios(st, emu, **R.mlp_fwd_finalize(emu, case)).values()) <= 1.0
    fin = R.mlp_fwd_finalize(emu, case, order=list(range(64, 70)) + list(range(64)))
    r = R.mlp_fwd_stats_ratios(st, emu, **fin)
    assert r["mean"] <= 1.0 and r["rstd"] <= 1.0, r
    for k in ("running_mean", "running_var"):
        rej("second sweep's segments chained first, " + k, r[k])
    # ---- 3 x 2997 rows, one weight for all: segment 1 multiplied by a weight of its own
    Cin, Cout, P, nseg = 128, 128, 2997, 3
    case = R.mlp_fwd_case(Cin, Cout, P, nseg, False, None, seed=3)
    ref = R.mlp_fwd_ref(case, 0.2)
    y_ok = R.rbf16(R.r32(ref["y"]))
    assert R.mlp_fwd_stored_ratio(y_ok, ref, kap) <= 1.0
    other = R.mlp_fwd_case(Cin, Cout, P, nseg, True, None, seed=3)["W"]
    assert not torch.equal(other[1], case["W"][0])
    y = R.rbf16(R.r32(R.mlp_fwd_ref(case, 0.2, W=other)["y"]))
    rej("y: a shared weight read as per-segment", R.mlp_fwd_stored_ratio(y, ref, kap))
    print("\nplanted defects, error / bound: " + "; ".join(seen))
