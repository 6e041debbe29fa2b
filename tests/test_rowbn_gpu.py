"""csrc/rowbn.hip per launch -- the backend's phase entries rowbn_stats, rowbn_apply_max, rowbn_fwd (eval mode),
rowbn_bwd_sums (without and with y) and rowbn_bwd -- against the restatements of oracle.ref_ops (rowbn_*_ref) on the
cases of tests/rowbn_cases.py, by the assertions of tests/rowbn_rule.py.

Dyadic family: bit for bit, sums included (rstd within one ulp); planted exact ties pin the first-maximum rule, the run
offset `kb` and the first-run-wins combine; the arg-max byte reaches 254 and 255.  Random family: y and arg exact (the
apply launch is restated op for op), statistics per channel and sums / dx per element within the derived bounds.  Every
shape is the smallest that reaches its launch edge (rowbn_cases.SHAPES; tests/test_rowbn_cpu.py asserts the geometry and
shows that these criteria reject seven planted defects the former global tolerance accepts)."""
import time

import pytest
import torch

import rowbn_cases as S
import rowbn_rule as Q
from oracle import ref_ops as R

pytestmark = pytest.mark.gpu

FAMILIES = ["dyadic", "random"]
_WORST, _RSTD_OFF, _T0 = {}, [0, 0], [None]


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
        print("\nrow BatchNorm, random family, largest error / bound per check: " +
              ", ".join(f"{k} {v:.3g}" for k, v in sorted(_WORST.items())))
        print(f"row BatchNorm, dyadic family: rstd one ulp off in {_RSTD_OFF[0]} of {_RSTD_OFF[1]} elements")
    if _T0[0] is not None:
        print(f"row BatchNorm, wall time of this file: {time.time() - _T0[0]:.1f} s")


@pytest.mark.parametrize("i", S.INDEX, ids=S.IDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_rowbn_statistics(hip, family, i):
    c = S.case(family, i)
    off = Q.check_stats(hip, "cuda", c, _note)
    if family == "dyadic":
        _RSTD_OFF[0] += off
        _RSTD_OFF[1] += c["nseg"] * c["C"]


@pytest.mark.parametrize("i", S.INDEX, ids=S.IDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_rowbn_apply_with_given_statistics(hip, family, i):
    Q.check_apply(hip, "cuda", S.case(family, i))


@pytest.mark.parametrize("i", S.INDEX, ids=S.IDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_rowbn_backward(hip, family, i):
    Q.check_backward(hip, "cuda", S.case(family, i), _note)


@pytest.mark.parametrize("i", S.VARIANT_CASES, ids=[S.IDS[i] for i in S.VARIANT_CASES])
@pytest.mark.parametrize("variant", S.VARIANTS[1:])
@pytest.mark.parametrize("family", FAMILIES)
def test_rowbn_without_affine_and_with_misaligned_constants(hip, family, variant, i):
    """gamma / beta absent (ld_consts' defaults), and gamma / beta / mean_shift as views one float past a 16-byte
    boundary (ld_consts' scalar branch): all three launches."""
    c = S.case(family, i, variant)
    Q.check_stats(hip, "cuda", c, _note)
    Q.check_apply(hip, "cuda", c)
    Q.check_backward(hip, "cuda", c, _note)


@pytest.mark.parametrize("i", [i for i in S.INDEX if S.SHAPES[i][5] > 1], ids=[S.IDS[i] for i in S.INDEX if S.SHAPES[i][5] > 1])
def test_rowbn_segments_equal_the_oracle_run_per_segment(hip, i):
    Q.check_segments(hip, "cuda", S.case("dyadic", i))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("name", ["150x3x24-f32-f32-s1", "32x32x64-f32-f32-s1", "96x48x40-bf16-bf16-s2"])
def test_rowbn_through_autograd_equals_the_backend_calls(hip, name):
    """ops.row_bn_act (training mode) on a U = 1 case and two L > 1 cases: the output, the running statistics and the three
    gradients equal the direct backend calls bit for bit (the backward is handed the stored y, as the op saves it)."""
    from tpgan_amd import ops
    c = S.case("random", S.IDS.index(name))
    t = Q.inputs(c, "cuda")
    K, C, nseg = c["K"], c["C"], c["nseg"]
    x = t["x"].clone().requires_grad_(True)
    gamma, beta = t["gamma"].clone().requires_grad_(True), t["beta"].clone().requires_grad_(True)
    rm, rv = c["rm0"].clone().cuda(), c["rv0"].clone().cuda()
    nbt = torch.full((), 7, dtype=torch.int64, device="cuda")
    y = ops.row_bn_act(x, gamma, beta, rm, rv, True, S.MOMENTUM, S.EPS, c["slope"], K, c["dother"], nbt, nseg, t["mean_shift"])
    y.backward(t["gy"])
    rm2, rv2 = c["rm0"].clone().cuda(), c["rv0"].clone().cuda()
    nbt2 = torch.full((), 7, dtype=torch.int64, device="cuda")
    mean, rstd = torch.empty(nseg, C, device="cuda"), torch.empty(nseg, C, device="cuda")
    y2, arg = hip.rowbn_fwd(t["x"], K, S.EPS, S.MOMENTUM, True, rm2, rv2, t["gamma"], t["beta"], c["slope"], mean, rstd,
                            c["dother"], nbt2, nseg, t["mean_shift"])
    assert torch.equal(_bits(y.detach()), _bits(y2)) and int(nbt) == int(nbt2) == 7 + nseg
    assert torch.equal(_bits(rm), _bits(rm2)) and torch.equal(_bits(rv), _bits(rv2))
    dx, dg, db = hip.rowbn_bwd(t["gy"], t["x"], arg, K, True, mean, rstd, t["gamma"], t["beta"], c["slope"], True, y2, nseg)
    assert torch.equal(_bits(x.grad), _bits(dx)) and torch.equal(_bits(gamma.grad), _bits(dg))
    assert torch.equal(_bits(beta.grad), _bits(db))
    assert bool(torch.isfinite(dg).all()) and bool(torch.isfinite(dx.float()).all())
