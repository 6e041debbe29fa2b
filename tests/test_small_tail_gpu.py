"""csrc/mlp_small.hip -- tpg_small_tail_fwd / tpg_small_tail_bwd, called directly -- per element against the float64
oracle (oracle.ref_ops.small_tail_fwd_ref / small_tail_bwd_ref) on the cases of tests/small_tail_cases.py.

Family A (dyadic inputs: every sum exact in fp32 in any order): out, arg, gh, dW1, dW2 bit for bit, a bf16 store being
one round-to-nearest-even of the exact value.  Family B (random inputs): every element within its derived first-order
bound (h_w, the depth of a weight-gradient element's fp32 chain, asserted from the launcher's geometry); the arg-max a
near-maximiser everywhere and the oracle's wherever the exact gap to the runner-up exceeds twice the bound; the backward
is given the kernel's own arg and out, as autograd gives them, and the oracle the same.  tests/test_small_tail_cpu.py
shows that these bounds reject one dropped edge, one misrouted arg-max, a skipped second trip and bf16-rounded operands.
The (65 589, 2) cases run the backward's second trip: 4100 tiles on 4096 waves, the last tile with 5 live points."""
import pytest
import torch

import small_tail_cases as S
from oracle import ref_ops as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
_WORST = {}


@pytest.fixture(scope="module")
def hip():
    import tpgan_amd.ops as ops
    return ops.backend_for(torch.zeros(1, device="cuda"))


def _note(check, ratio):
    _WORST[check] = max(_WORST.get(check, 0.0), ratio)
    assert ratio <= 1.0, (check, ratio)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    if _WORST:
        print("\nsmall tails, largest error / bound per check: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(_WORST.items())))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _is_exactly(got, ref64):
    """Kernel output == oracle value (ref64: float64 holding the exact value; fp32 holds it exactly, bf16 after one
    round-to-nearest-even).  Compared as numbers, i.e. bit for bit except that the two zeros are one value: the sign
    of an exact zero sum depends on what the sum starts from, in the kernel and in the float64 product alike."""
    ref = ref64.to(torch.float32)
    assert bool((ref.double() == ref64).all()), "the oracle's value is not an fp32 number"
    return got.shape == ref.shape and torch.equal(got.cpu(), ref.to(got.dtype))


def _dev(c, dtype):
    return tuple(c[n].cuda().to(dtype if n in ("h", "gout") else torch.float32) for n in ("h", "W1", "W2", "gout"))


def _depth(hip, P, K):
    """h_w from the launcher's own geometry (one 768-float slab per wave), equal to the oracle's restatement."""
    blocks = hip.lib.tpg_small_tail_workspace_bytes(P, K) // (4 * 768 * 4)
    tiles = -(-P // 16)
    h_w = -(-tiles // (4 * blocks)) * 16 * K + -(-(4 * blocks) // 16) + 16
    assert h_w == R.small_tail_depth(P, K), (h_w, P, K)
    return h_w


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("P,K,s1,s2", S.SMALL_A_CASES)
def test_small_tail_dyadic_bit_for_bit(hip, P, K, s1, s2, dtype):
    """Family A: shapes around one tile (16, 17), one forward workgroup (64, 65), K = 255 with planted maxima at edges
    0 and 254 and ties between edges 3 and 254, the second trip at 65 589; slopes 0, 1/4, 1/2, 1; exact ties between
    different edges go to the lowest j, z1 == 0 takes slope s1 and out == 0 takes s2 in the backward."""
    c = S.dyadic_case(P, K, s1, s2)
    f, b = c["fwd"], c["bwd"]
    h, W1, W2, gout = _dev(c, dtype)
    assert torch.equal(h.float().cpu(), c["h"]) and torch.equal(gout.float().cpu(), c["gout"])      # exact in bf16 too
    out, arg = hip.small_tail_fwd(h, W1, W2, s1, s2, K)
    assert out.dtype == dtype and out.shape == (P, 32) and arg.dtype == torch.uint8
    assert torch.equal(arg.cpu(), f["arg"]), "arg"
    assert _is_exactly(out, f["out"]), "out"
    gh, dW1, dW2 = hip.small_tail_bwd(h, out, gout, arg, W1, W2, s1, s2, K)
    assert _is_exactly(gh, b["gh"]), "gh"
    assert _is_exactly(dW1, b["dW1"]), "dW1"
    assert _is_exactly(dW2, b["dW2"]), "dW2"
    out2, arg2 = hip.small_tail_fwd(h, W1, W2, s1, s2, K)
    again = hip.small_tail_bwd(h, out2, gout, arg2, W1, W2, s1, s2, K)
    assert torch.equal(_bits(out2), _bits(out)) and torch.equal(arg2, arg)
    assert all(torch.equal(_bits(u), _bits(v)) for u, v in zip(again, (gh, dW1, dW2))), "second launch"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_small_tail_planted_arg_bytes_at_k_255(hip, dtype):
    """The backward at (5, 255) with arg = 254 everywhere, and alternating 0 / 254 within each packed word: whatever
    bytes it is given it routes by them (the oracle is given the same), bit for bit."""
    c = S.dyadic_case(5, 255, 0.25, 0.25)
    h, W1, W2, gout = _dev(c, dtype)
    out, _ = hip.small_tail_fwd(h, W1, W2, 0.25, 0.25, 255)
    for name, arg in (("254", torch.full((5, 32), 254, dtype=torch.uint8)),
                      ("0/254", (torch.arange(32) % 2 * 254).to(torch.uint8).expand(5, 32).contiguous())):
        b = R.small_tail_bwd_ref(c["h"], c["fwd"]["out"], c["gout"], arg, c["W1"], c["W2"], 0.25, 0.25, 255)
        S.dyadic_exactness(c, b)
        gh, dW1, dW2 = hip.small_tail_bwd(h, out, gout, arg.cuda(), W1, W2, 0.25, 0.25, 255)
        assert _is_exactly(gh, b["gh"]) and _is_exactly(dW1, b["dW1"]) and _is_exactly(dW2, b["dW2"]), name


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("s1,s2", S.SMALL_B_SLOPES)
@pytest.mark.parametrize("P,K", S.SMALL_B_SHAPES)
def test_small_tail_random_within_derived_bounds(hip, P, K, s1, s2, bf16):
    """Family B: every element of out, gh, dW1, dW2 within its bound; the arg-max rule in its two parts."""
    c = S.random_case(P, K, s1, s2, bf16)
    f = c["fwd"]
    h_w = _depth(hip, P, K)
    tag = "bf16" if bf16 else "f32"
    h, W1, W2, gout = _dev(c, torch.bfloat16 if bf16 else torch.float32)
    out, arg = hip.small_tail_fwd(h, W1, W2, s1, s2, K)
    _note(f"out/{tag}", R.err_ratio(out.cpu(), f["out"], R.small_stored_bound(f["out"], f["Eout"], bf16)))
    arg_c = arg.cpu()
    assert int(arg_c.max()) < K
    picked = f["z2"].view(P, K, 32).gather(1, arg_c.long()[:, None])[:, 0]
    assert bool((picked >= f["best"] - 2 * f["E2max"]).all()), "arg is not a near-maximiser"
    assert bool((arg_c == f["arg"])[c["gap2"]].all()), "arg differs from the oracle's where the gap decides"
    gh, dW1, dW2 = hip.small_tail_bwd(h, out, gout, arg, W1, W2, s1, s2, K)
    b = R.small_tail_bwd_ref(c["h"], out.cpu(), c["gout"], arg_c, c["W1"], c["W2"], s1, s2, K, h_w=h_w)
    assert float(b["flip"].double().mean()) <= 1e-3
    _note(f"gh/{tag}", R.err_ratio(gh.cpu(), b["gh"], R.small_stored_bound(b["gh"], b["Egh"], bf16)))
    _note(f"dW1/{tag}", R.err_ratio(dW1.cpu(), b["dW1"], b["EdW1"]))
    _note(f"dW2/{tag}", R.err_ratio(dW2.cpu(), b["dW2"], b["EdW2"]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_small_tail_point_depends_on_its_own_edges_only(hip, dtype):
    """The 37 points of family B's (37, 3) at row offset 21 of a 100-point array filled with other values: the same bits
    in out, arg and gh as alone (another tile, another lane, other neighbours in the matrix instruction's columns)."""
    K, off, n = 3, 21, 37
    c = S.random_case(n, K, 0.2, 0.2, dtype == torch.bfloat16)
    h, W1, W2, gout = _dev(c, dtype)
    g = torch.Generator().manual_seed(5)
    hb = (3.0 * torch.randn(100 * K, 16, generator=g)).cuda().to(dtype)
    gb = torch.randn(100, 32, generator=g).cuda().to(dtype)
    hb[off * K:(off + n) * K] = h
    gb[off:off + n] = gout
    out, arg = hip.small_tail_fwd(h, W1, W2, 0.2, 0.2, K)
    gh = hip.small_tail_bwd(h, out, gout, arg, W1, W2, 0.2, 0.2, K)[0]
    out_b, arg_b = hip.small_tail_fwd(hb, W1, W2, 0.2, 0.2, K)
    gh_b = hip.small_tail_bwd(hb, out_b, gb, arg_b, W1, W2, 0.2, 0.2, K)[0]
    assert torch.equal(_bits(out_b[off:off + n]), _bits(out)) and torch.equal(arg_b[off:off + n], arg)
    assert torch.equal(_bits(gh_b[off * K:(off + n) * K]), _bits(gh))


def test_small_tail_of_no_points(hip):
    """P = 0: a (0, 32) output and zero weight gradients (the launcher's memset path), through ops.small_tail."""
    from tpgan_amd import ops
    h = torch.zeros(0, 16, device="cuda", requires_grad=True)
    W1 = torch.randn(16, 16, device="cuda", requires_grad=True)
    W2 = torch.randn(32, 16, device="cuda", requires_grad=True)
    y = ops.small_tail(h, W1, W2, 0.2, 0.2, 4)
    assert y.shape == (0, 32)
    gh, g1, g2 = torch.autograd.grad(y.sum(), [h, W1, W2])
    assert gh.shape == (0, 16) and g1.shape == (16, 16) and g2.shape == (32, 16)
    assert not bool(g1.any()) and not bool(g2.any())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("wanted", [(True, False, False), (False, True, True), (True, True, True)], ids=["h", "weights", "all"])
def test_small_tail_through_autograd_equals_the_backend_calls(hip, dtype, wanted):
    """ops.small_tail on family B's (1000, 9) with an expanded incoming gradient (from .sum(); fp32 for bf16 rows): the
    wanted gradients equal the direct backend calls bit for bit, the others are None."""
    from tpgan_amd import ops
    c = S.random_case(1000, 9, 0.2, 0.2, dtype == torch.bfloat16)
    h, W1, W2, _ = _dev(c, dtype)
    leaves = [t.clone().requires_grad_(w) for t, w in zip((h, W1, W2), wanted)]
    y = ops.small_tail(*leaves, 0.2, 0.2, 9)
    out, arg = hip.small_tail_fwd(h, W1, W2, 0.2, 0.2, 9)
    assert y.dtype == dtype and torch.equal(_bits(y.detach()), _bits(out))
    y.float().sum().backward()
    ones = torch.ones(1000, 32, device="cuda", dtype=dtype)
    direct = hip.small_tail_bwd(h, out, ones, arg, W1, W2, 0.2, 0.2, 9)
    for leaf, w, d in zip(leaves, wanted, direct):
        if w:
            assert leaf.grad.dtype == leaf.dtype and torch.equal(_bits(leaf.grad), _bits(d))
        else:
            assert leaf.grad is None
