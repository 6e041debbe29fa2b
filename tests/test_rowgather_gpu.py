"""csrc/rowgather.hip per launch -- rowcombine_fwd / rowcombine_bwd in the modes GATHER, SUB and EDGE, the EdgeConv front
end rowcombine_edge_fwd / _bwd, and SUB's rowsum_neg -- against the FP64 twins of oracle.ref_ops (rowcombine_*_twin) on
the cases of tests/rowgather_cases.py, by the assertions of tests/rowgather_rule.py.

Dyadic family: bit for bit, sums included, in any summation order.  Random family: the forward bit for bit against the
fp32 restatement, every gradient element within its derived bound.  Both: two launches agree bit for bit, a cloud
launched alone equals its slice of the batch.  Every shape is the smallest that reaches its edge: both backward forms
at every chunk count that picks them, list lengths around the lane-group count and the 4-entry unroll, the second pass
of every grid-stride loop, the rounded-up forward grid under the XCD ordering, out-of-range indices, and the kink of
EDGE mode on every row (tests/test_rowgather_cpu.py asserts the geometry and shows that the rule rejects seven
planted defects)."""
import time

import pytest
import torch

import rowgather_cases as S
import rowgather_rule as Q

pytestmark = pytest.mark.gpu

FAMILIES = ["dyadic", "random"]
_WORST, _T0 = {}, [None]


@pytest.fixture(scope="module")
def hip():
    import tpgan_amd.ops as ops
    _T0[0] = time.time()
    return ops.backend_for(torch.zeros(1, device="cuda"))


def _note(check, ratio):
    _WORST[check] = max(_WORST.get(check, 0.0), ratio)
    assert ratio <= 1.0, (check, ratio)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _WORST:
        print("\nrow gather, random family, largest error / bound per check: " +
              ", ".join(f"{k} {v:.3g}" for k, v in sorted(_WORST.items())))
    if _T0[0] is not None:
        print(f"row gather, wall time of this file: {time.time() - _T0[0]:.1f} s")


def _groups(which):
    """Cases of one edge, mode and type pair share a test item: the collection between GPU tests (tests/conftest.py)
    costs more than a case's launches, one item per case more than doubles the file's time.
    -> {"wave-GATHER-ff": [case indices]}."""
    out = {}
    for i in which:
        s = S.SHAPES[i]
        out.setdefault(f"{s['id'].split('-')[0]}-{s['mode']}-{s['pair']}", []).append(i)
    return out


_FWD, _BWD = _groups(S.FWD), _groups(S.BWD)


def _each(group, family, check):
    for i in group:
        try:
            check(S.case(family, i, "cuda"))
        except AssertionError as e:
            raise AssertionError(f"{family} {S.IDS[i]}: {e}") from e


@pytest.mark.parametrize("group", list(_FWD), ids=list(_FWD))
@pytest.mark.parametrize("family", FAMILIES)
def test_rowgather_forward(hip, family, group):
    _each(_FWD[group], family, lambda c: Q.check_forward(hip, "cuda", c))


@pytest.mark.parametrize("group", list(_BWD), ids=list(_BWD))
@pytest.mark.parametrize("family", FAMILIES)
def test_rowgather_backward(hip, family, group):
    _each(_BWD[group], family, lambda c: Q.check_backward(hip, "cuda", c, _note))


def test_rowgather_through_autograd_equals_the_backend_calls(hip):
    """ops.row_combine on a kink case: output and both gradients equal the direct backend calls bit for bit."""
    from tpgan_amd import ops
    c = S.case("random", [i for i in S.SMALL if S.IDS[i].startswith("kink-EDGE-ff") and S.SHAPES[i]["C"] == 64][0], "cuda")
    t = Q.inputs(c, "cuda")
    U, QE = t["U"].clone().requires_grad_(True), t["QE"].clone().requires_grad_(True)
    out = ops.row_combine(U, QE, t["idx"], ops.ROW_EDGE, c["slope"], c["dout"])
    out.backward(t["g"])
    direct = Q.launch_bwd(hip, c, t)
    assert torch.equal(Q.bits(out.detach()), Q.bits(Q.launch_fwd(hip, c, t)))
    assert torch.equal(Q.bits(U.grad), Q.bits(direct["gU"])) and torch.equal(Q.bits(QE.grad), Q.bits(direct["gQE"]))
