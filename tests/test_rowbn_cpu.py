"""The row BatchNorm oracle (oracle.ref_ops.rowbn_*) and the criteria of tests/rowbn_rule.py, without a GPU:
the FP64 twins against torch.nn.BatchNorm1d -> leaky_relu -> max under torch.autograd in float64; the dyadic builder's
exactness condition; every launch-geometry claim of tests/rowbn_cases.py; the oracle's CPU backend through the same
assertions as the kernels; and seven planted defects that the new criteria reject (each with the factor by which it
exceeds its bound, or the number of elements that differ) while the former tolerance -- a fraction of the tensor's
largest magnitude -- accepts them."""
import pytest
import torch

import rowbn_cases as S
import rowbn_rule as Q
from oracle import ref_ops as R
from oracle.torch_backend import OracleBackend


@pytest.mark.parametrize("i", S.INDEX, ids=S.IDS)
def test_rowbn_shapes_reach_their_launch_edges(i):
    P, K, C, din, dother, nseg, _, claims = S.SHAPES[i]
    geo = R.rowbn_geometry(P, K, C, din, dother, nseg)
    assert claims and {k: geo[k] for k in claims} == claims
    assert P * nseg * C * (2 if din == S.BF16 else 4) < 40e6


def test_rowbn_geometry_of_the_model_shapes():
    """The shapes the suite already ran: U = 4 and no cut groups at K = 32 x 8 clouds, L = 64 at the GroupAll level."""
    g = R.rowbn_geometry(8 * 512 * 32, 32, 128, S.F32, S.F32)
    assert (g["U_fwd"], g["L_fwd"], g["grid_fwd"], g["G_stats"]) == (4, 1, 512, 256)
    g = R.rowbn_geometry(2 * 256, 256, 256, S.BF16, S.BF16)
    assert (g["L_fwd"], g["L_bwd"], g["U_fwd"], g["cpr"], g["rpi"]) == (64, 64, 4, 32, 8)
    assert R.rowbn_geometry(70, 0, 256, S.BF16, S.BF16, 70)["G_stats"] == 1      # tests/test_segments_gpu.py: G = 1


@pytest.mark.parametrize("i", S.SMALL, ids=[S.IDS[i] for i in S.SMALL])
def test_rowbn_dyadic_cases_are_exact_in_any_order(i):
    c = S.dyadic_case(i)
    assert c["exact"] and all(v < S.EXACT_UNITS for v in c["exact"].values())
    # exact in any order: the fp32 restatement of the sums equals the FP64 twin's, and the launch geometry is moot
    for name in ("c12", "dgamma", "dbeta"):
        assert Q.mismatches(c["bwd"][name], R.r32(c["bwd64"][name])) == 0, name
    assert Q.mismatches(c["stats"]["mean"], R.r32(c["stats64"]["mean"])) == 0
    bad = dict(c)
    bad["bwd"] = dict(c["bwd"], gg=c["bwd"]["gg"] / 3.0)
    with pytest.raises(AssertionError):
        S.dyadic_exactness(bad)
    big = dict(c, x=c["x"] * 2.0 ** 12)
    if c["P"] > 1:
        with pytest.raises(AssertionError):
            S.dyadic_exactness(big)


TWIN_CASES = [(S.IDS.index(n), v) for n, v in (("150x3x24-f32-f32-s1", "plain"), ("330x10x64-f32-f32-s3", "plain"),
                                               ("96x48x40-bf16-bf16-s2", "no_affine"), ("37x0x48-f32-f32-s1", "plain"),
                                               ("1x0x8-f32-f32-s3", "plain"), ("240x6x72-f32-f32-s1", "plain"))]


@pytest.mark.parametrize("i,variant", TWIN_CASES, ids=[f"{S.IDS[i]}-{v}" for i, v in TWIN_CASES])
def test_rowbn_fp64_twins_equal_torch_autograd(i, variant):
    """Statistics (with the running chain over the segments and mean_shift), y, and the three gradients of the FP64 twins
    (gather form and stored-output form) against torch in float64.  Channels whose rows all tie under the max
    (gamma == 0) are left out of dgamma: which row carries the gradient is then the first-maximum rule's choice."""
    c = S.random_case(i, variant)
    P, K, C, nseg = c["P"], c["K"], c["C"], c["nseg"]
    aff = c["gamma"] is not None
    x = c["x"].double().requires_grad_(True)
    bn = torch.nn.BatchNorm1d(C, eps=R.slope32(S.EPS), momentum=R.slope32(S.MOMENTUM), affine=aff).double()
    leaves = [x]
    if aff:
        bn.weight.data.copy_(c["gamma"].double())
        bn.bias.data.copy_(c["beta"].double())
        leaves += [bn.weight, bn.bias]
    bn.running_mean.copy_(c["rm0"].double())
    bn.running_var.copy_(c["rv0"].double())
    s64 = c["stats64"]
    tol = dict(rtol=1e-7, atol=1e-9)
    if P > 1:
        shift = 0.0 if c["mean_shift"] is None else c["mean_shift"].double()
        ys = [torch.nn.functional.leaky_relu(bn(x[s * P:(s + 1) * P] + shift), R.slope32(c["slope"]))
              for s in range(nseg)]
        y = torch.cat(ys)
        torch.testing.assert_close(s64["running_mean"], bn.running_mean, **tol)
        torch.testing.assert_close(s64["running_var"], bn.running_var, rtol=1e-6, atol=1e-9)
        assert s64["num_batches_tracked"] == 7 + nseg
    else:                                           # one row per segment: torch refuses; mean = x, var = 0 by hand
        xs = x.view(nseg, 1, C)
        z = (x - x.detach()) * (R.slope32(S.EPS) ** -0.5) * (bn.weight if aff else 1.0) + (bn.bias if aff else 0.0)
        y = torch.nn.functional.leaky_relu(z, R.slope32(c["slope"]))
        assert torch.equal(s64["mean"], xs[:, 0].detach()) and bool((s64["var"] == 0).all())
        assert bool((s64["running_var"] <= c["rv0"].double()).all())            # the unbiased-variance guard: + 0
    if K:
        y = y.view(-1, K, C).max(1)[0]
    f = R.rowbn_apply_ref(c["x"], K, s64["mean"], s64["rstd"], c["gamma"], c["beta"], c["slope"], nseg, ar=R.FP64)
    torch.testing.assert_close(f["y"], y.detach(), rtol=1e-6, atol=1e-7)
    gy = c["gy"].double()
    want = torch.autograd.grad(y, leaves, gy)
    consts = (s64["mean"], s64["rstd"], c["gamma"], c["beta"], c["slope"])
    forms = [None] + ([f["y"]] if K else [])
    for yy in forms:
        b = R.rowbn_bwd_sums_ref(gy, c["x"], f["arg"], yy, K, *consts, nseg, c["din"], c["dother"], ar=R.FP64)
        assert yy is None or bool(b["inv"].any())
        d = R.rowbn_bwd_apply_ref(gy, c["x"], f["arg"], K, *consts, b["c12"] if P > 1 else None, nseg, ar=R.FP64)
        scale = float(want[0].abs().max())
        # z == 0 exactly (a constant column without beta: the pivoted twin gets 0, torch's mean leaves +-1e-16): the
        # subgradient there is the kernel's convention (slope), not torch's to decide
        ok = f["z"] != 0
        torch.testing.assert_close(d["dx"][ok], want[0][ok], rtol=1e-5, atol=1e-6 * scale)
        if aff:
            keep = c["gamma"] != 0 if K else torch.ones(C, dtype=torch.bool)
            torch.testing.assert_close(b["dgamma"][keep], want[1][keep], rtol=1e-5, atol=1e-6 * float(want[1].abs().max()))
            torch.testing.assert_close(b["dbeta"], want[2], rtol=1e-5, atol=1e-6 * float(want[2].abs().max()))


def test_rowbn_fp32_restatements_stay_within_their_bounds_of_the_twins():
    """The derived bounds hold for the restatement itself (they are derived, not fitted to a kernel): every small random
    case, statistics, sums in both forms and dx."""
    worst = {}

    def note(k, r):
        worst[k] = max(worst.get(k, 0.0), r)
    for i in S.SMALL:
        c = S.random_case(i)
        for name in ("mean", "rstd", "running_mean", "running_var"):
            note("stats/" + name, R.err_ratio(c["stats"][name], c["stats64"][name], c["stats_bound"][name]))
        for tag, b, bound in (("sums", c["bwd"], c["sums_bound"]),) + ((("sums_y", c["bwd_y"], c["sums_bound_y"]),) if c["K"] else ()):
            for name in ("c12", "dgamma", "dbeta"):
                if torch.isfinite(b[name]).all():
                    note(f"{tag}/{name}", R.err_ratio(b[name], c["bwd64"][name], bound[name]))
        keep = ~c["kink"]
        bound = R.rowbn_dx_bound(c["dx64"], c["sums_bound"]["c12"], c["nseg"], c["bf_in"])
        note("dx", R.err_ratio(R.rowbn_stored(c["dx"]["dx"], c["bf_in"])[keep], c["dx64"]["dx"][keep], bound[keep]))
    print("\nrow BatchNorm, fp32 restatement against the FP64 twin, largest error / bound: " +
          ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("i", S.SMALL, ids=[S.IDS[i] for i in S.SMALL])
@pytest.mark.parametrize("family", ["dyadic", "random"])
def test_rowbn_oracle_backend_passes_the_kernels_assertions(family, i):
    """oracle.torch_backend: its phase entries are the restatements, its rowbn_fwd / rowbn_bwd the older float64 numpy
    forms (judged by the bounds in both families: their sums are not taken in the kernels' order)."""
    c = S.case(family, i)
    be = OracleBackend()

    def note(k, r):
        assert r <= 1.0, (k, r)
    Q.check_stats(be, "cpu", c, note)
    Q.check_apply(be, "cpu", c)
    Q.check_backward(be, "cpu", c, note, bitwise=False)
    if c["nseg"] > 1 and family == "dyadic":
        Q.check_segments(be, "cpu", c, backward=False)         # its rowbn_bwd sums in float64


_VAR = [i for i in S.VARIANT_CASES if i in S.SMALL]


@pytest.mark.parametrize("i", _VAR, ids=[S.IDS[i] for i in _VAR])
@pytest.mark.parametrize("variant", S.VARIANTS[1:])
@pytest.mark.parametrize("family", ["dyadic", "random"])
def test_rowbn_oracle_backend_without_affine_and_with_misaligned_constants(family, variant, i):
    c = S.case(family, i, variant)
    be = OracleBackend()

    def note(k, r):
        assert r <= 1.0, (k, r)
    Q.check_stats(be, "cpu", c, note)
    Q.check_apply(be, "cpu", c)
    Q.check_backward(be, "cpu", c, note, bitwise=False)


# ---- planted defects ---------------------------------------------------------------------------------------------
def _last_maximum(c):
    K, C = c["K"], c["C"]
    vk = c["fwd"]["v"].view(-1, K, C)
    ks = torch.arange(K)[None, :, None]
    return torch.where(vk == c["fwd"]["y"][:, None], ks, -1).max(1)[0].to(torch.uint8)


def _stats_defect(c, seg, rows, ch):
    """mean of segment `seg`, channel `ch` with the rows `rows` left out of sum d -> (defective mean, ratio to bound)."""
    P = c["P"]
    xs = c["x"][seg * P:(seg + 1) * P].double()
    miss = (xs[rows, ch] - xs[0, ch]).sum() / P
    mean = c["stats"]["mean"].clone()
    mean[seg, ch] = R.r32(mean[seg, ch] - miss)
    assert float(miss) != 0.0
    return mean, R.err_ratio(mean, c["stats64"]["mean"], c["stats_bound"]["mean"])


def test_rowbn_planted_defects_are_rejected():
    rows = []          # (defect, new criterion's figure, what the figure is, the old tolerance accepts it)
    # 1. the LAST maximum instead of the first: dyadic (72, 24, 24), planted ties
    c = S.dyadic_case(S.IDS.index("72x24x24-f32-f32-s1"))
    bad = _last_maximum(c)
    n = int((bad != c["arg"]).sum())
    rows.append(("last maximum instead of first", n, "arg bytes differ", bool((bad < c["K"]).all())))
    # 2. the arg of one run without its offset kb: dyadic (32, 32, 64), L = 8 runs of 4 rows
    c = S.dyadic_case(S.IDS.index("32x32x64-f32-f32-s1"))
    L, K = c["geo_fwd"]["L_fwd"], c["K"]
    bad = c["arg"].clone()
    sel = bad < K - K // L
    bad[sel] += K // L
    n = int((bad != c["arg"]).sum())
    assert L == 8
    rows.append(("arg off by one run", n, "arg bytes differ", bool((bad < K).all())))
    # 3. one partial of the second pair_sums block dropped: random (269, 0, 1024) x 33, L = 1, partial 8 of G = 9
    c = S.random_case(S.IDS.index("269x0x1024-f32-f32-s33"))
    geo = c["stats"]["geo"]
    assert (geo["G_stats"], geo["fin_L"], geo["rpi_stats"]) == (9, 1, 1)
    mean, ratio = _stats_defect(c, 5, torch.arange(8, c["P"], 9), 6)
    rows.append(("one partial of the second pair_sums block dropped", ratio, "x bound (mean)",
                 Q.old_ok(mean, c["stats64"]["mean"], Q.OLD_TOL["f32"])))
    # 4. one thread skips a row of its remainder loop: random (707, 0, 1024) x 4, 23 workgroups, thread of row 0
    c = S.random_case(S.IDS.index("707x0x1024-f32-f32-s4"))
    assert (c["stats"]["geo"]["G_stats"], c["stats"]["geo"]["per_stats"]) == (23, (30, 31))
    mean, ratio = _stats_defect(c, 0, torch.tensor([30 * 23]), 6)
    rows.append(("a remainder row skipped in one thread", ratio, "x bound (mean)",
                 Q.old_ok(mean, c["stats64"]["mean"], Q.OLD_TOL["f32"])))
    # 5. dx without the c2 term in one row: random (37, 0, 48), the channel of gamma 1e-3
    c = S.random_case(S.IDS.index("37x0x48-f32-f32-s1"))
    d = c["dx"]
    dx = R.rowbn_stored(d["dx"], False).clone()
    a, c1 = d["a"][0, 5], c["bwd"]["c12"][0, 0, 5]
    dx[11, 5] = R.r32(a * (d["gg"][11, 5] - c1))
    bound = R.rowbn_dx_bound(c["dx64"], c["sums_bound"]["c12"], 1, False)
    rows.append(("dx without the c2 term in one row", R.err_ratio(dx, c["dx64"]["dx"], bound), "x bound (dx)",
                 Q.old_ok(dx, c["dx64"]["dx"], Q.OLD_TOL["grad_f32"])))
    # 6. bf16 by truncation instead of round-to-nearest-even: random (185, 5, 40) bf16
    c = S.random_case(S.IDS.index("185x5x40-bf16-bf16-s1"))
    y32 = c["fwd"]["y"].float()
    trunc = (y32.view(torch.int32) & -65536).view(torch.float32).double()
    rows.append(("bf16 truncation instead of RNE", Q.mismatches(trunc, c["y"]), "y elements differ",
                 Q.old_ok(trunc, c["fwd64"]["y"], Q.OLD_TOL["bf16"])))
    # 7. the stored-output form where 1 / gamma overflows: gamma == 0 == beta and a denormal gamma
    c = S.random_case(S.IDS.index("150x3x24-f32-f32-s1"))
    b = R.rowbn_bwd_sums_ref(c["gy"], c["x"], c["arg"], c["y"], c["K"], c["mean"], c["rstd"], c["gamma"], c["beta"],
                             c["slope"], 1, c["din"], c["dother"], fixed_guard=False)
    nonfinite = int((~torch.isfinite(b["dgamma"])).sum())
    assert not bool(torch.isfinite(b["dgamma"][3])) and not bool(torch.isfinite(b["dgamma"][4]))
    assert bool(torch.isfinite(c["bwd_y"]["dgamma"]).all())
    rows.append(("1 / gamma = inf in the stored-output form", nonfinite, "dgamma channels not finite",
                 Q.old_ok(b["dgamma"], c["bwd64"]["dgamma"], Q.OLD_TOL["grad_f32"])))
    print("\nrow BatchNorm, planted defects (defect | new criterion | old tolerance accepts):")
    for name, fig, what, old in rows:
        print(f"  {name}: {fig:.4g} {what} | {old}")
    for name, fig, what, old in rows:
        assert fig > 1.0 if "bound" in what else fig > 0, name
    # the former tolerance accepts all but the NaN (which no former case could produce: none had |gamma| < 0.05)
    assert [old for *_, old in rows] == [True] * 6 + [False]
