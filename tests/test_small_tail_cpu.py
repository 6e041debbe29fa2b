"""The oracle of the 16 -> 16 -> 32 small tails (oracle.ref_ops.small_tail_*_ref) and the bounds that
tests/test_small_tail_gpu.py applies to csrc/mlp_small.hip, checked without a GPU: the restatement against
torch.autograd in float64, the CPU backend through ops.small_tail, the bounds against planted defects at the shapes of
the GPU grid, and the dyadic builder's exactness condition."""
import pytest
import torch
import torch.nn.functional as F

import small_tail_cases as S
from oracle import ref_ops as R


def _statement(h, W1, W2, s1, s2, K):
    """max_K lrelu(W2 lrelu(W1 h)) as plain PyTorch (float64 in, differentiable)."""
    z2 = F.leaky_relu(h @ W1.t(), s1) @ W2.t()
    return F.leaky_relu(z2.view(h.shape[0] // K, K, -1).max(1)[0], s2)


@pytest.mark.parametrize("P,K", [(37, 3), (1000, 9)])
@pytest.mark.parametrize("s1,s2", S.SMALL_B_SLOPES)
def test_small_tail_restatement_chains_to_autograd(oracle_cpu, P, K, s1, s2):
    """small_tail_bwd_ref, given the forward's arg and out, equals torch.autograd.grad of the plain float64 statement
    (random rows: no ties, no pre-activation at the kink): 1e-10 relative, any algebra slip is O(1).  ops.small_tail on
    CPU tensors (the oracle backend) returns the same values rounded once to fp32."""
    from tpgan_amd import ops
    c = S.random_case(P, K, s1, s2, False)
    f = c["fwd"]
    assert bool((f["z1"] != 0).all()) and bool((f["best"] != 0).all())
    leaves = [c[n].double().requires_grad_(True) for n in ("h", "W1", "W2")]
    ref = _statement(*leaves, R.slope32(s1), R.slope32(s2), K)
    assert torch.allclose(ref, f["out"], rtol=1e-12, atol=1e-12)
    want = torch.autograd.grad(ref, leaves, c["gout"].double())
    b = R.small_tail_bwd_ref(c["h"], f["out"], c["gout"], f["arg"], c["W1"], c["W2"], s1, s2, K)
    for name, w in zip(("gh", "dW1", "dW2"), want):
        rel = float((b[name] - w).abs().max() / w.abs().max())
        assert rel <= 1e-10, (name, rel)
    h = c["h"].clone().requires_grad_(True)
    W1, W2 = c["W1"].clone().requires_grad_(True), c["W2"].clone().requires_grad_(True)
    y = ops.small_tail(h, W1, W2, s1, s2, K)
    assert y.dtype == torch.float32 and torch.equal(y.detach().double(), R.r32(f["out"]))
    got = torch.autograd.grad(y, [h, W1, W2], c["gout"])
    # the backend's backward reads the sign of the STORED out: the same sign
    for name, g_ in zip(("gh", "dW1", "dW2"), got):
        assert torch.equal(g_.double(), R.r32(b[name])), name


def test_small_tail_cpu_backend_row_types_and_empty_input(oracle_cpu):
    """bf16 rows come back as bf16 (one rounding of the fp32 value), the weight gradients in the weights' type; a
    (0, 16) input gives a (0, 32) output and zero weight gradients."""
    from tpgan_amd import ops
    c = S.random_case(37, 3, 0.2, 0.2, True)
    h = c["h"].bfloat16().requires_grad_(True)
    W1, W2 = c["W1"].clone().requires_grad_(True), c["W2"].clone().requires_grad_(True)
    y = ops.small_tail(h, W1, W2, 0.2, 0.2, 3)
    assert y.dtype == torch.bfloat16 and torch.equal(y.detach().double(), R.rbf16(c["fwd"]["out"]))
    gh, g1, g2 = torch.autograd.grad(y.float().sum(), [h, W1, W2])
    assert gh.dtype == torch.bfloat16 and g1.dtype == torch.float32 and g2.shape == (32, 16)
    h0 = torch.zeros(0, 16, requires_grad=True)
    y0 = ops.small_tail(h0, W1, W2, 0.2, 0.2, 3)
    assert y0.shape == (0, 32)
    gh0, g1, g2 = torch.autograd.grad(y0.sum(), [h0, W1, W2])
    assert gh0.shape == (0, 16) and not g1.any() and not g2.any()


def test_small_tail_geometry_is_the_launchers(hip_lib):
    """The oracle's restatement of small_bwd_blocks against the library's own workspace size (one 768-float slab per
    wave, four waves per workgroup), and h_w at the grid's shapes."""
    for P in (1, 16, 17, 64, 65, 1000, 4099, 65535, 65536, 65537, 65589, 165000):
        assert hip_lib.tpg_small_tail_workspace_bytes(P, 2) == 4 * 768 * 4 * R.small_tail_geometry(P)[1], P
    assert R.small_tail_geometry(65589) == (4100, 1024)
    assert int(S.second_trip_points(65589).sum()) == 53 and not S.second_trip_points(65536).any()
    assert R.small_tail_depth(1000, 9) == 1 * 16 * 9 + 4 + 16 and R.small_tail_depth(65589, 2) == 2 * 16 * 2 + 256 + 16


class _Bounds:
    """The checks of tests/test_small_tail_gpu.py on one family-B case, the backward on the oracle's own arg / out."""

    def __init__(self, c):
        self.c, self.f = c, c["fwd"]
        self.b = self.bwd(self.f["arg"])

    def bwd(self, arg, h=None, W1=None, W2=None):
        c = self.c
        return R.small_tail_bwd_ref(c["h"] if h is None else h, self.f["out"], c["gout"], arg,
                                    c["W1"] if W1 is None else W1, c["W2"] if W2 is None else W2, c["s1"], c["s2"], c["K"])

    def out(self, v):
        return R.err_ratio(v, self.f["out"], R.small_stored_bound(self.f["out"], self.f["Eout"], self.c["bf16"]))

    def gh(self, v):
        return R.err_ratio(v, self.b["gh"], R.small_stored_bound(self.b["gh"], self.b["Egh"], self.c["bf16"]))

    def dW1(self, v):
        return R.err_ratio(v, self.b["dW1"], self.b["EdW1"])

    def dW2(self, v):
        return R.err_ratio(v, self.b["dW2"], self.b["EdW2"])


def _l2(a, b):
    return float((a - b).norm() / b.norm())


OLD_BF16_TOL = 2.0 ** -7          # test_small_tail_forward_backward's L2 tolerance for bf16 rows


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("P,K", [(1000, 9), (65589, 2)])
def test_small_tail_bounds_reject_planted_defects(P, K, bf16):
    """The per-element bounds accept the oracle's own output stored as the kernel stores it and reject each planted
    defect."""
    c = S.random_case(P, K, 0.2, 0.2, bf16)
    B = _Bounds(c)
    f, b = B.f, B.b
    h, arg = c["h"].double(), f["arg"]
    out_ok, gh_ok = S.stored(f["out"], bf16), S.stored(b["gh"], bf16)
    dW1_ok, dW2_ok = R.r32(b["dW1"]), R.r32(b["dW2"])
    assert B.out(out_ok) <= 1.0 and B.gh(gh_ok) <= 1.0 and B.dW1(dW1_ok) <= 1.0 and B.dW2(dW2_ok) <= 1.0
    second = S.second_trip_points(P)
    n0 = int(second.nonzero()[7]) if second.any() else P // 2          # a point of a second-trip tile where there is one
    e0 = n0 * K + int(arg[n0, 0])                                      # the edge its channel 0 routes to

    def terms(edges):
        return b["gz1"][edges].t() @ h[edges], b["gz2"][edges].t() @ b["a1"][edges]
    # one edge's gh row zeroed
    gh = gh_ok.clone()
    gh[e0] = 0.0
    assert B.gh(gh) > 1.0
    # one edge counted twice in dW1 and dW2
    t1, t2 = terms(slice(e0, e0 + 1))
    assert B.dW1(dW1_ok + t1) > 1.0 and B.dW2(dW2_ok + t2) > 1.0
    # one point's arg moved to j + 1
    arg2 = arg.clone()
    arg2[n0] = ((arg[n0].long() + 1) % K).to(torch.uint8)
    b2 = B.bwd(arg2)
    assert B.gh(S.stored(b2["gh"], bf16)) > 1.0
    assert B.dW1(R.r32(b2["dW1"])) > 1.0 and B.dW2(R.r32(b2["dW2"])) > 1.0
    # the upper 16 channels of dW2 zeroed
    dW2 = dW2_ok.clone()
    dW2[16:] = 0.0
    assert B.dW2(dW2) > 1.0
    # the points of the second-trip tiles left out of dW
    if second.any():
        t1, t2 = terms(second.repeat_interleave(K))
        assert B.dW1(dW1_ok - t1) > 1.0 and B.dW2(dW2_ok - t2) > 1.0
    # the last live point of the ragged tile left out
    assert P % 16 != 0
    last = slice((P - 1) * K, P * K)
    t1, t2 = terms(last)
    gh = gh_ok.clone()
    gh[last] = 0.0
    assert B.dW1(dW1_ok - t1) > 1.0 and B.dW2(dW2_ok - t2) > 1.0 and B.gh(gh) > 1.0
    # products formed from bf16-rounded operands (fp32 rows: the kernel's exact-fp32 claim)
    if not bf16:
        hb, W1b, W2b = R.rbf16(h), R.rbf16(c["W1"].double()), R.rbf16(c["W2"].double())
        fb = R.small_tail_fwd_ref(hb, W1b, W2b, c["s1"], c["s2"], K)
        bb = B.bwd(arg, hb, W1b, W2b)
        assert B.out(R.r32(fb["out"])) > 1.0 and B.gh(R.r32(bb["gh"])) > 1.0
        assert B.dW1(R.r32(bb["dW1"])) > 1.0 and B.dW2(R.r32(bb["dW2"])) > 1.0
        # while plain fp32 arithmetic in another order (PyTorch's) sits well inside
        y32 = _statement(c["h"], c["W1"], c["W2"], R.slope32(c["s1"]), R.slope32(c["s2"]), K)
        assert B.out(y32) <= 0.5


def test_small_tail_old_l2_tolerance_lets_one_row_defects_through():
    """At the older test's own largest shape, 12 288 x 20 bf16 rows: one edge's gh row zeroed, one edge counted twice in
    the weight gradients and one (point, channel) routed to j + 1 all pass its L2 tolerance of 2^-7 -- and fail the
    per-element bounds.  That gap is the one the bounds close."""
    P, K = 12288, 20
    c = S.random_case(P, K, 0.2, 0.2, True)
    B = _Bounds(c)
    b, arg = B.b, c["fwd"]["arg"]
    n0 = P // 2
    e0 = n0 * K + int(arg[n0, 0])
    gh = S.stored(b["gh"], True)
    assert B.gh(gh) <= 1.0 and _l2(gh, b["gh"]) < OLD_BF16_TOL
    gh[e0] = 0.0
    assert B.gh(gh) > 1.0 and _l2(gh, b["gh"]) < OLD_BF16_TOL
    dW1 = R.r32(b["dW1"]) + torch.outer(b["gz1"][e0], c["h"][e0].double())
    dW2 = R.r32(b["dW2"]) + torch.outer(b["gz2"][e0], b["a1"][e0])
    assert B.dW1(dW1) > 1.0 and B.dW2(dW2) > 1.0
    assert _l2(dW1, b["dW1"]) < OLD_BF16_TOL and _l2(dW2, b["dW2"]) < OLD_BF16_TOL
    arg2 = arg.clone()
    arg2[n0, 0] = (int(arg[n0, 0]) + 1) % K
    b2 = B.bwd(arg2)
    gh2 = S.stored(b2["gh"], True)
    assert B.gh(gh2) > 1.0 and _l2(gh2, b["gh"]) < OLD_BF16_TOL


def test_small_tail_dyadic_oracle_rejects_the_later_of_two_tied_edges():
    """Family A at (1000, 9): routing a tied (point, channel) to its LAST maximiser changes the oracle's arg, gh and
    both weight gradients, so the bit-for-bit comparison of the GPU file goes red."""
    c = S.dyadic_case(1000, 9, 0.25, 0.25)
    f, b, K = c["fwd"], c["bwd"], 9
    z2v = f["z2"].view(1000, K, 32)
    ks = torch.arange(K)[None, :, None]
    last = torch.where(z2v == f["best"][:, None], ks, -1).max(1)[0].to(torch.uint8)
    assert int((last != f["arg"]).sum()) == S.dyadic_events(c)[0] > 0
    b2 = R.small_tail_bwd_ref(c["h"], f["out"], c["gout"], last, c["W1"], c["W2"], 0.25, 0.25, K)
    assert not torch.equal(b2["gh"], b["gh"]) and not torch.equal(b2["dW1"], b["dW1"]) and not torch.equal(b2["dW2"], b["dW2"])


@pytest.mark.parametrize("P,K,s1,s2", S.SMALL_A_CASES)
def test_small_tail_dyadic_cases_are_exact_in_fp32(P, K, s1, s2):
    """The builder's condition on every case of the GPU grid (it raises where a sum could round), the events it must
    contain, and that the condition is not vacuous: the same case with gout scaled by 2^12 violates it."""
    c = S.dyadic_case(P, K, s1, s2)
    assert all(0 <= v < S.EXACT_UNITS for v in c["exact"].values()), c["exact"]
    if (P, K) == (1000, 9):
        ties, z0, b0 = S.dyadic_events(c)
        assert ties > 0 and z0 > 0 and b0 > 0, (ties, z0, b0)
        bad = dict(c, gout=c["gout"] * 4096.0)
        bb = R.small_tail_bwd_ref(c["h"], c["fwd"]["out"], bad["gout"], c["fwd"]["arg"], c["W1"], c["W2"], s1, s2, K)
        with pytest.raises(AssertionError):
            S.dyadic_exactness(bad, bb)
    if P == S.BIG:
        dense = S.dense_points(P)
        assert bool(dense[65536:].all()) and bool(dense[:64].all()) and bool((c["gout"][65536:] != 0).any(1).all())
        assert 0.01 < float((c["gout"][64:65536] != 0).double().mean()) < 0.02      # 2 % kept, a third of k / 4 is 0
