"""The row-gather oracle (oracle.ref_ops.rowcombine_*) and the criteria of tests/rowgather_rule.py, without a GPU: every
launch-geometry claim of tests/rowgather_cases.py, the launcher's caps read out of csrc/rowgather.hip, the dyadic
builder's exactness condition, the FP64 twins against torch.autograd in float64 and against the stated convention at
the kink, the oracle's CPU backend through the same assertions as the kernels, the C ABI's refusal of C % NE != 0, and
seven planted defects that the new rule rejects -- with the factor by which each exceeds its bound (or the number of
elements that differ) and what the former criterion, a fraction of the tensor's largest magnitude, says to it."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import rowgather_cases as S
import rowgather_rule as Q
from oracle import ref_ops as R
from oracle.torch_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def find(name, mode, pair, **kw):
    hits = [i for i in S.INDEX if all(S.SHAPES[i][k] == v for k, v in dict(kw, mode=mode, pair=pair).items())
            and S.SHAPES[i]["id"].startswith(name + "-")]
    assert len(hits) == 1, (name, mode, pair, kw, hits)
    return hits[0]


@pytest.mark.parametrize("i", S.INDEX, ids=S.IDS)
def test_rowgather_shapes_reach_their_launch_edges(i):
    s = S.SHAPES[i]
    geo = S.geometry(s)
    print(f"\n{s['id']}: " + ", ".join(f"{k}={geo[k]}" for k in s["claims"]))
    assert s["claims"] and {k: geo[k] for k in s["claims"]} == s["claims"]
    esz = {"ff": (4, 4), "fb": (4, 2), "bb": (2, 2)}[s["pair"]]
    assert s["B"] * s["S"] * s["K"] * s["C"] * esz[1] < 71e6 and s["B"] * s["N"] * s["C"] * esz[0] < 71e6
    if s["idx"][0] == "ladder":
        assert s["N"] <= 128
    if s["big"] and geo["passes_fwd"] == 2:
        assert geo["total"] % (geo["wgs_launched"] * 256) != 0            # the second pass is partial


def test_rowgather_caps_are_the_launchers():
    text = open(os.path.join(ROOT, "temporal-pointcloud-upsampling-gan_amd", "csrc", "rowgather.hip")).read()
    for name in ("TPG_RC_FWD_U", "TPG_RC_FWD_CAP", "TPG_RC_BWD_CAP", "TPG_RC_BWD_WAVE_CAP"):
        m = re.search(r"#ifndef %s\s*\n#define %s (\d+)" % (name, name), text)
        assert m and int(m.group(1)) == getattr(R, name), name
    m = re.search(r"grid_for\(unsigned total, unsigned per_thread = 1u, unsigned cap = (\d+)u\)", text)
    assert m and int(m.group(1)) == R.TPG_RC_ROWSUM_CAP
    # the dispatch of the shapes the suite ran before: powers of two only
    for C in (8, 16, 64, 128):
        assert R.rowcombine_geometry(R.ROW_GATHER, 2, 512, 512, 20, C, S.F32, S.F32)["form"] == "wave"
    assert R.rowcombine_geometry(R.ROW_SUB, 3, 256, 256, 32, 256, S.F32, S.F32)["form"] == "thread"
    assert R.rowcombine_geometry(R.ROW_EDGE, 3, 512, 512, 10, 16, S.BF16, S.BF16)["form"] == "thread"
    g = R.rowcombine_geometry(R.ROW_SUB, 2, 16384, 4096, 32, 64, S.F32, S.BF16)
    assert (g["passes_fwd"], g["passes_bwd"], g["passes_rowsum"], g["wgs_launched"] % 8) == (1, 1, 1, 0)


_LADDERS = [i for i in S.SMALL if S.SHAPES[i]["idx"][0] == "ladder"]


@pytest.mark.parametrize("i", _LADDERS[::5], ids=[S.IDS[i] for i in _LADDERS[::5]])
def test_rowgather_dyadic_cases_are_exact_in_any_order(i):
    c = S.case("dyadic", i)
    assert 0 < c["exact"] < S.EXACT_UNITS
    names = [n for n in ("U", "QE", "Y", "g") if c.get(n) is not None]
    with pytest.raises(AssertionError):
        S.dyadic_exactness(dict(c, **{n: c[n] * 2.0 ** 12 for n in names}))
    with pytest.raises(AssertionError):
        S.dyadic_exactness(dict(c, g=c["g"] / 3.0))
    # exact in any order: the fp32 forward restatement is the twin, and fp32 sums in list order are the twin's
    if c["mode"] == "FRONT":
        out32 = R.rowcombine_edge_fwd_twin(c["Y"], c["idx"], c["slope_a"], c["slope"], torch.float32)
    else:
        out32 = R.rowcombine_fwd_twin(c["U"], c.get("QE"), c["idx"], S.MODE[c["mode"]], c["slope"], 1.0, torch.float32)
    assert Q.mismatches(S._stored32(out32, c["bf_out"]), c["out"]) == 0
    for t in (v for k, v in c["bwd"].items() if k != "L"):
        assert torch.equal(R.r32(t["v"]), t["v"])


def _direct(U, QE, idxc, mode, slope, slope_u):
    lr = torch.nn.functional.leaky_relu
    bi = torch.arange(U.shape[0])[:, None, None]
    u = U[bi, idxc]
    if mode == R.ROW_GATHER:
        return u
    if mode == R.ROW_SUB:
        return u - QE[:, :, None]
    return lr(u, slope_u) + lr(QE[bi, idxc] - QE[:, :, None], slope)


_TWIN = [("wave", "GATHER", "ff", dict(C=16)), ("thread", "SUB", "bb", dict(C=48)), ("wave", "EDGE", "fb", dict(C=64)),
         ("oor", "GATHER", "ff", {}), ("oor", "EDGE", "bb", {}), ("oor", "FRONT", "ff", {}), ("wave", "FRONT", "bb", dict(C=32)),
         ("kink", "EDGE", "ff", dict(C=8)), ("kink", "FRONT", "ff", dict(C=64))]


@pytest.mark.parametrize("name,mode,pair,kw", _TWIN, ids=[f"{a}-{b}-{c}" for a, b, c, _ in _TWIN])
def test_rowgather_fp64_twins_equal_torch_autograd(name, mode, pair, kw):
    """Forward and every gradient of the twins against a direct restatement under torch.autograd in float64, indices
    clamped beforehand.  torch's leaky_relu takes the slope at 0 as well, so the comparison holds ON the kink too."""
    c = S.case("random", find(name, mode, pair, **kw))
    C, sl, sa = c["C"], R.slope32(c["slope"]), R.slope32(c["slope_a"])
    idxc = c["idxc"].long()
    g = c["g"].double()
    tol = dict(rtol=1e-12, atol=1e-12)
    if mode == "FRONT":
        Y = c["Y"].double().requires_grad_(True)
        out = _direct(Y[:, :, C:], Y[:, :, :C], idxc, R.ROW_EDGE, sl, sa)
        torch.testing.assert_close(R.rowcombine_edge_fwd_twin(c["Y"], c["idx"], c["slope_a"], c["slope"]), out.detach(), **tol)
        (gY,) = torch.autograd.grad(out, Y, g)
        torch.testing.assert_close(c["bwd"]["gE"]["v"], gY[:, :, :C], **tol)
        torch.testing.assert_close(c["bwd"]["gA"]["v"], gY[:, :, C:], **tol)
        return
    U = c["U"].double().requires_grad_(True)
    QE = None if mode == "GATHER" else c["QE"].double().requires_grad_(True)
    out = _direct(U, QE, idxc, S.MODE[mode], sl, 1.0)
    torch.testing.assert_close(R.rowcombine_fwd_twin(c["U"], c.get("QE"), c["idx"], S.MODE[mode], c["slope"]), out.detach(), **tol)
    grads = torch.autograd.grad(out, [U] if QE is None else [U, QE], g)
    torch.testing.assert_close(c["bwd"]["gU"]["v"], grads[0], **tol)
    if QE is not None:
        torch.testing.assert_close(c["bwd"]["gQE"]["v"], grads[1], **tol)
    L = torch.stack([torch.bincount(idxc[b].reshape(-1), minlength=c["N"]) for b in range(c["B"])])
    assert torch.equal(c["bwd"]["L"], L.double()) and torch.equal(c["bwd"]["gU"]["n"][:, :, 0], L.double())


def test_rowgather_twins_follow_the_convention_at_the_kink():
    """Only self edges: d == 0 everywhere, lrelu' = slope on the neighbour side AND on the centre side, so gE == 0
    exactly; lrelu'(Y[:, C:]) = slope_a at +-0; terms and sum |term| counted per element."""
    Y = torch.tensor([[[1.0, -0.0, 0.0, -2.0], [3.0, 0.5, -0.0, 4.0]]])            # C = 2: E | node half
    idx = torch.tensor([[[0, 0], [1, 1]]], dtype=torch.int32)
    g = torch.tensor([[[[1.0, 2.0], [3.0, 4.0]], [[5.0, 6.0], [7.0, 8.0]]]])
    r = R.rowcombine_edge_bwd_twin(g, idx, Y, 0.5, 0.25)
    assert torch.equal(r["gE"]["v"], torch.zeros(1, 2, 2, dtype=torch.float64))
    assert torch.equal(r["gE"]["n"], torch.full((1, 2, 2), 4.0, dtype=torch.float64))
    assert torch.equal(r["gE"]["A"], 0.5 * torch.tensor([[[4.0, 6.0], [12.0, 14.0]]], dtype=torch.float64))
    assert torch.equal(r["gA"]["v"], torch.tensor([[[2.0, 3.0], [6.0, 14.0]]], dtype=torch.float64))
    bad = R.rowcombine_edge_bwd_twin(g, idx, Y, 0.5, 0.25, defect="nbr_ge")
    assert torch.equal(bad["gE"]["v"], 0.75 * torch.tensor([[[4.0, 6.0], [12.0, 14.0]]], dtype=torch.float64))
    # an out-of-range index reads row N - 1, in both directions
    f = R.rowcombine_fwd_twin(Y, None, torch.tensor([[[-1, 2], [7, 0]]], dtype=torch.int32), R.ROW_GATHER)
    assert torch.equal(f[0, 0, 0], Y[0, 1].double()) and torch.equal(f[0, 1, 0], Y[0, 1].double())


@pytest.mark.parametrize("i", S.SMALL, ids=[S.IDS[i] for i in S.SMALL])
@pytest.mark.parametrize("family", ["dyadic", "random"])
def test_rowgather_oracle_backend_passes_the_kernels_assertions(family, i):
    """oracle.torch_backend over oracle/tpgref.c (fp32, sums in (s, k) order; it does not clamp: pre-clamped indices)."""
    c = S.case(family, i)
    be = OracleBackend()

    def note(k, r):
        assert r <= 1.0, (k, r)
    if "fwd" in c["run"]:
        Q.check_forward(be, "cpu", c, clamp=True)
    if "bwd" in c["run"]:
        Q.check_backward(be, "cpu", c, note, clamp=True)


def test_rowgather_unsupported_channel_counts_are_refused_before_any_launch(hip_lib):
    """C % NE != 0: C = 4 with a bf16 side is TPG_ERR_UNSUPPORTED (-3) from every entry, no device touched."""
    buf = (ctypes.c_float * 80)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    for din, dout in ((1, 1), (0, 1), (1, 0)):
        for mode in (0, 1, 2):
            assert hip_lib.tpg_rowcombine_fwd(p, p, p, mode, din, dout, 1, 8, 8, 2, 4, 0.2, p, None) == -3
            assert hip_lib.tpg_rowcombine_bwd(p, p, p, p, p, mode, din, dout, 1, 8, 8, 2, 4, 0.2, p, p, None) == -3
        assert hip_lib.tpg_rowcombine_edge_fwd(p, p, din, dout, 1, 8, 2, 4, 0.2, 0.2, p, None) == -3
        assert hip_lib.tpg_rowcombine_edge_bwd(p, p, p, p, p, din, dout, 1, 8, 2, 4, 0.2, 0.2, p, None) == -3
    assert hip_lib.tpg_rowcombine_fwd(p, p, p, 0, 0, 0, 1, 8, 8, 2, 6, 0.2, p, None) == -3          # f32: C % 4


# ---- planted defects ---------------------------------------------------------------------------------------------
def _seq32(c):
    """The gradients of the oracle's fp32 backend BEFORE the store's rounding (sums in (s, k) order), as float32."""
    g, idx = c["g"].numpy(), c["idxc"].numpy()
    if c["mode"] == "FRONT":
        gY = R.rowcombine_edge_bwd(g, idx, c["Y"].numpy(), c["slope_a"], c["slope"])
        return dict(gE=torch.from_numpy(gY[:, :, :c["C"]].copy()), gA=torch.from_numpy(gY[:, :, c["C"]:].copy()))
    gU, gQ = R.rowcombine_bwd(g, idx, c["QE"].numpy() if c["mode"] == "EDGE" else None, S.MODE[c["mode"]], c["N"], c["slope"])
    return dict(gU=torch.from_numpy(gU), gQE=None if gQ is None else torch.from_numpy(gQ))


def _former_inputs(c):
    """The case as the former per-element test prepared it: no self edges, E spread (no ties), no exact zeros."""
    g = torch.Generator().manual_seed(9)
    own = torch.arange(c["N"], dtype=torch.int32)[None, :, None]
    idx = torch.where(c["idxc"] == own, (own + 1) % c["N"], c["idxc"])
    rows = {n: torch.randn(c[n].shape, generator=g) for n in ("QE", "Y") if c.get(n) is not None}
    return idx, rows


def test_rowgather_planted_defects_are_rejected():
    rows = []                # (defect, figure of the new rule, what the figure is, old_ok, old_ok on the former inputs)
    # 1. a bf16 store that truncates: random wave ladder, bf16 rows, G = 16
    c = S.case("random", find("wave", "GATHER", "bb", C=32))
    good = _seq32(c)["gU"]
    assert Q.judge(c, "gU", good.bfloat16()) <= 1.0
    trunc = (good.view(torch.int32) & -65536).view(torch.float32)
    rows.append(("bf16 store truncates", Q.judge(c, "gU", trunc), "x bound (gU)", Q.old_ok(trunc, c["bwd"]["gU"]["v"], True), None))
    # 2. >= on the neighbour side of the kink only: the kink case, f32, thread and wave form
    for C in (8, 64):
        c = S.case("random", find("kink", "EDGE", "ff", C=C))
        bad = R.rowcombine_bwd_twin(c["g"], c["idx"], c["QE"], R.ROW_EDGE, c["N"], c["slope"], defect="nbr_ge")["gQE"]["v"].float()
        idx_f, rows_f = _former_inputs(c)
        a = R.rowcombine_bwd_twin(c["g"], idx_f, rows_f["QE"], R.ROW_EDGE, c["N"], c["slope"], defect="nbr_ge")["gQE"]["v"]
        b = R.rowcombine_bwd_twin(c["g"], idx_f, rows_f["QE"], R.ROW_EDGE, c["N"], c["slope"])["gQE"]["v"]
        rows.append((f">= on the neighbour side of the kink (C = {C})", Q.judge(c, "gQE", bad), "x bound (gE)",
                     Q.old_ok(bad, c["bwd"]["gQE"]["v"], False), Q.old_ok(a.float(), b, False)))
    # 3. the entry at position 2G dropped from the lists of 2G + 1 entries: random wave ladder, f32, G = 16
    c = S.case("random", find("wave", "GATHER", "ff", C=16))
    G = c["geo"]["G"]
    bad = c["bwd"]["gU"]["v"].clone()
    hit = 0
    for b in range(c["B"]):
        offs, lst = R.rowcombine_lists(c["idx"][b], c["N"])
        for n in np.flatnonzero(np.diff(offs) == 2 * G + 1):
            e = int(lst[offs[n] + 2 * G])
            bad[b, n] -= c["g"][b].reshape(-1, c["C"])[e].double()
            hit += 1
    assert hit == c["B"]
    bad = bad.float()
    rows.append(("entry 2G of a list of 2G + 1 dropped", Q.judge(c, "gU", bad), "x bound (gU)",
                 Q.old_ok(bad, c["bwd"]["gU"]["v"], False), None))
    # 4. the rows of the wave form's second pass left unwritten (zeros): random, 65700 rows
    c = S.case("random", find("wave2", "GATHER", "ff"))
    bad = c["bwd"]["gU"]["v"].float().clone()
    flat = bad.view(-1, c["C"])
    assert float(flat[4 * c["geo"]["grid_bwd"]:].abs().max()) > 0
    flat[4 * c["geo"]["grid_bwd"]:] = 0.0
    rows.append(("second pass left unwritten", Q.judge(c, "gU", bad), "x bound (gU)", Q.old_ok(bad, c["bwd"]["gU"]["v"], False), None))
    # 5. the idle workgroups of a rounded-up forward grid wrap around and write the next row's value: dyadic, 65 -> 72.
    # Planted on a copy of the expected output: the figure only counts the overwritten elements that hold another
    # number.  The forward was compared bit for bit before as well, so the former column is False by definition, not
    # by measurement; what was missing is a shape whose grid has idle workgroups.
    c = S.case("dyadic", find("xcd", "GATHER", "ff"))
    geo = c["geo"]
    assert geo["cpr"] == 1 and geo["idle"] == 7
    bad = c["out"].clone().view(-1, c["C"])
    wrap = geo["wgs_launched"] * 256 - geo["total"]
    bad[:wrap] = c["out"].view(-1, c["C"])[1:wrap + 1]
    rows.append(("idle workgroups write a wrong row twice", Q.mismatches(bad.view_as(c["out"]), c["out"]), "elements differ (out)",
                 False, None))                          # the forward was held bit for bit before as well
    # 6. slope_a not applied where Y[:, C:] == 0: the front end, f32
    c = S.case("random", find("thread", "FRONT", "ff", C=4))
    bad = R.rowcombine_edge_bwd_twin(c["g"], c["idx"], c["Y"], c["slope_a"], c["slope"], defect="a_zero")["gA"]["v"].float()
    idx_f, rows_f = _former_inputs(c)
    a = R.rowcombine_edge_bwd_twin(c["g"], idx_f, rows_f["Y"], c["slope_a"], c["slope"], defect="a_zero")["gA"]["v"]
    b = R.rowcombine_edge_bwd_twin(c["g"], idx_f, rows_f["Y"], c["slope_a"], c["slope"])["gA"]["v"]
    rows.append(("slope_a left out where the node half is 0", Q.judge(c, "gA", bad), "x bound (gA)",
                 Q.old_ok(bad, c["bwd"]["gA"]["v"], False), Q.old_ok(a.float(), b, False)))
    # 7. the lane groups' partial sums rounded to bf16 before the fold: random wave ladder, bf16 rows, G = 16
    c = S.case("random", find("wave", "GATHER", "bb", C=32))
    G = c["geo"]["G"]
    bad = torch.zeros(c["B"], c["N"], c["C"])
    for b in range(c["B"]):
        offs, lst = R.rowcombine_lists(c["idx"][b], c["N"])
        gb = c["g"][b].reshape(-1, c["C"])
        for n in range(c["N"]):
            part = torch.zeros(G, c["C"])
            for j, e in enumerate(lst[offs[n]:offs[n + 1]]):
                part[j % G] += gb[int(e)]
            bad[b, n] = part.bfloat16().double().sum(0).float()
    bad = bad.bfloat16()
    rows.append(("lane-group partials rounded to bf16", Q.judge(c, "gU", bad), "x bound (gU)",
                 Q.old_ok(bad, c["bwd"]["gU"]["v"], True), None))
    print("\nrow gather, planted defects (defect | new rule | former criterion accepts | ... on the former test's inputs,"
          " where the defect cannot fire):")
    for name, fig, what, old, former in rows:
        print(f"  {name}: {fig:.4g} {what} | {old} | {'-' if former is None else former}")
    for name, fig, what, old, former in rows:
        assert fig > 1.0 if "bound" in what else fig > 0, name
    assert rows[0][3] is True and rows[7][3] is True    # 1, 7: the former criterion accepts them on these very tensors
    # 2, 6: on the former inputs (no self edges, no ties, no exact zeros) the defective and the correct twin are the
    # same numbers, so these hold by construction: they document why the former suite was blind to the kink, they are
    # no evidence about the criterion -- which, on the kink tensors themselves, rejects both (column three, False).
    assert rows[1][4] is True and rows[2][4] is True and rows[6][4] is True
    assert rows[1][3] is False and rows[2][3] is False and rows[6][3] is False
