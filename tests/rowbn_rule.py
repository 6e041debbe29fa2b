"""What a backend's row BatchNorm entries must return on a case of tests/rowbn_cases.py: the assertions that
tests/test_rowbn_gpu.py runs on the HIP kernels and tests/test_rowbn_cpu.py on the oracle's CPU backend (and on planted
defects).  One launch per check, every launch fed the ORACLE's upstream values (given statistics, the oracle's y and arg),
so that one kernel's error cannot hide behind another's.

dyadic family: bit for bit (as numbers: the two zeros are one value); rstd within one fp32 ulp.
random family: |got - FP64 twin| <= the derived bound per element / channel (`note` records the largest ratio); the
apply launch is elementwise and restated op for op, so y and arg are exact there too."""
import torch

import rowbn_cases as S
from oracle import ref_ops as R

OLD_TOL = {"f32": 1e-5, "bf16": 8e-3, "grad_f32": 2e-5, "grad_bf16": 1e-2}     # tests/test_ops_gpu.py::test_rowbn_matches_oracle


def old_ok(got, ref, tol):
    """The criterion the row BatchNorm tests used before: a fraction of the tensor's largest magnitude."""
    ref = R._f64(ref)
    err = (R._f64(got).cpu() - ref).abs().max()
    return bool(err <= tol * max(1.0, float(ref.abs().max())))


def mismatches(got, ref64):
    """Elements of `got` that are not the number ref64 holds (a NaN is never equal)."""
    assert tuple(got.shape) == tuple(ref64.shape), (got.shape, ref64.shape)
    return int((got.detach().cpu().double() != ref64.cpu()).sum())


def exactly(got, ref64, what):
    n = mismatches(got, ref64)
    assert n == 0, f"{what}: {n} of {ref64.numel()} elements differ from the oracle"


def ulps32(got, ref64):
    """Largest distance in fp32 ulps between got (fp32) and the fp32 numbers ref64 holds (same sign assumed)."""
    a = got.detach().cpu().float().contiguous().view(torch.int32).long()
    b = ref64.float().contiguous().view(torch.int32).long()
    return int((a - b).abs().max()) if a.numel() else 0


def off16(t, dev):
    """t as a view that starts one float past a 16-byte boundary (ld_consts' scalar branch)."""
    if t is None:
        return None
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=dev)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def inputs(c, dev):
    """The case's tensors on `dev` in their row types; constants misaligned for the `misaligned` variant."""
    put = (lambda t: off16(t, dev)) if c["variant"] == "misaligned" else (lambda t: None if t is None else t.to(dev))
    d = dict(x=c["x"].to(dev, c["din"]), gy=c["gy"].to(dev, c["dother"]), gamma=put(c["gamma"]), beta=put(c["beta"]),
             mean_shift=put(c["mean_shift"]), mean=c["mean"].to(dev).contiguous(), rstd=c["rstd"].to(dev).contiguous())
    assert torch.equal(d["x"].float().cpu(), c["x"]) and torch.equal(d["gy"].float().cpu(), c["gy"])
    if c["K"]:
        d["arg"] = c["arg"].to(dev)
        d["y"] = c["y"].float().to(dev, c["dother"])
    else:
        d["arg"] = d["y"] = None
    return d


def check_stats(be, dev, c, note, bitwise=True):
    """rowbn_stats: mean, rstd, running statistics, batch counter; two launches agree bit for bit.
    -> number of rstd elements one ulp off (dyadic)."""
    t = inputs(c, dev)
    s, s64, B, nseg = c["stats"], c["stats64"], c["stats_bound"], c["nseg"]
    outs = []
    for _ in range(2):
        rm, rv = c["rm0"].clone().to(dev), c["rv0"].clone().to(dev)
        nbt = torch.full((), 7, dtype=torch.int64, device=dev)
        mean, rstd = be.rowbn_stats(t["x"], S.EPS, S.MOMENTUM, rm, rv, nbt, nseg, t["mean_shift"])
        outs.append((mean.clone(), rstd.clone(), rm, rv, nbt))
    mean, rstd, rm, rv, nbt = outs[0]
    assert mean.shape == (nseg, c["C"]) and int(nbt) == s["num_batches_tracked"] == 7 + nseg
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(outs[0], outs[1])), "the statistics differ between two launches"
    off = 0
    if c["family"] == "dyadic" and bitwise:
        exactly(mean, s["mean"], "mean")
        exactly(rm, s["running_mean"], "running mean")
        exactly(rv, s["running_var"], "running var")
        assert ulps32(rstd, s["rstd"]) <= 1, "rstd more than one ulp from the oracle"
        off = mismatches(rstd, s["rstd"])
    else:
        for name, got in (("mean", mean), ("rstd", rstd), ("running_mean", rm), ("running_var", rv)):
            ref = s64[name]
            assert bool(torch.isfinite(got).all()), name
            note(f"stats/{name}", R.err_ratio(got.cpu(), ref, B[name]))
    return off


def check_apply(be, dev, c):
    """rowbn_apply_max with given statistics (and rowbn_fwd in eval mode for one segment): y the stored fp32 value,
    arg the first maximum, both families."""
    t = inputs(c, dev)
    K, nseg = c["K"], c["nseg"]
    y, arg = be.rowbn_apply_max(t["x"], K, t["mean"], t["rstd"], t["gamma"], t["beta"], c["slope"], c["dother"], nseg)
    assert y.dtype == c["dother"]
    if K:
        assert arg.dtype == torch.uint8
        n = int((arg.cpu() != c["arg"]).sum())
        assert n == 0, f"arg: {n} of {arg.numel()} are not the first maximum"
    else:
        assert arg is None
    exactly(y, c["y"], "y")
    if nseg == 1:
        y2, arg2 = be.rowbn_fwd(t["x"], K, S.EPS, S.MOMENTUM, False, None, None, t["gamma"], t["beta"], c["slope"],
                                t["mean"][0].contiguous(), t["rstd"][0].contiguous(), c["dother"])
        exactly(y2, c["y"], "y (eval)")
        assert not K or torch.equal(arg2.cpu(), c["arg"]), "arg (eval)"


def _sums(c, got, ref, ref64, bound, note, tag, bitwise):
    c12, dg, db = got
    names = (("c12", c12), ("dgamma", dg), ("dbeta", db))
    for name, g in names:
        if g is None:
            continue
        assert bool(torch.isfinite(g).all()), f"{tag}/{name} is not finite"
        if c["family"] == "dyadic" and bitwise:
            exactly(g, ref[name], f"{tag}/{name}")
        else:
            note(f"{tag}/{name}", R.err_ratio(g.cpu(), ref64[name], bound[name]))


def _dx(c, dx, ref, ref64, Ec12, note, tag, bitwise):
    assert dx.dtype == c["din"] and bool(torch.isfinite(dx.float()).all()), f"{tag}/dx is not finite"
    if c["gamma"] is not None:
        zero = c["gamma"] == 0
        assert not bool(dx[:, zero.to(dx.device)].any()), f"{tag}/dx is not 0 where gamma is 0"
    if c["family"] == "dyadic" and bitwise:
        exactly(dx, R.rowbn_stored(ref["dx"], c["bf_in"]), f"{tag}/dx")
        return
    bound = R.rowbn_dx_bound(ref64, Ec12, c["nseg"], c["bf_in"])
    got = dx.float().cpu().double()
    keep = ~c["kink"] if c["family"] == "random" else torch.ones_like(got, dtype=torch.bool)
    note(f"{tag}/dx", R.err_ratio(got[keep], ref64["dx"][keep], bound[keep]))
    # the former criterion, on every element (the excluded ones too): max(gtol, ytol) where y feeds the sums
    loose = c["bf_in"] or (tag.endswith("_y") and c["bf_other"])
    assert old_ok(got, ref64["dx"], OLD_TOL["grad_bf16" if loose else "grad_f32"]), f"{tag}/dx at the global tolerance"


def check_backward(be, dev, c, note, bitwise=True):
    """rowbn_bwd_sums without and with y (gather and stored-output form), rowbn_bwd without and with y; and
    (bitwise) the eval-mode backward, no batch terms, every case of both families."""
    t = inputs(c, dev)
    K, nseg, aff = c["K"], c["nseg"], c["gamma"] is not None
    head = (t["gy"], t["x"], t["arg"])
    consts = (t["mean"], t["rstd"], t["gamma"], t["beta"], c["slope"])
    dy = c["family"] == "dyadic"
    stored = dict(gamma=c["gamma"], beta=c["beta"], bf16=c["bf_other"])
    rb = c["sums_bound"] if not dy else (None if bitwise else R.rowbn_bwd_sums_bound(c["bwd64"], c["slope"]))
    _sums(c, be.rowbn_bwd_sums(*head, None, K, *consts, aff, nseg), c["bwd"], c["bwd64"], rb, note, "sums", bitwise)
    dx, dg, db = be.rowbn_bwd(*head, K, True, *consts, aff, None, nseg)
    _sums(c, (None, dg, db), c["bwd"], c["bwd64"], rb, note, "bwd", bitwise)
    _dx(c, dx, c["dx"], c["dx64"], None if rb is None else rb["c12"], note, "bwd", bitwise)
    if K and t["y"].dtype == t["gy"].dtype:
        rby = c["sums_bound_y"] if not dy else \
            (None if bitwise else R.rowbn_bwd_sums_bound(c["bwd64"], c["slope"], None, stored))
        _sums(c, be.rowbn_bwd_sums(*head, t["y"], K, *consts, aff, nseg), c["bwd_y"], c["bwd64"], rby, note, "sums_y", bitwise)
        dx, dg, db = be.rowbn_bwd(*head, K, True, *consts, aff, t["y"], nseg)
        _sums(c, (None, dg, db), c["bwd_y"], c["bwd64"], rby, note, "bwd_y", bitwise)
        _dx(c, dx, c["dx_y"], c["dx64"], None if rby is None else rby["c12"], note, "bwd_y", bitwise)
    if bitwise:
        # eval mode: no reduction, dx = a * gg elementwise, restated op for op: exact in both families; one segment with
        # statistics (C) as the op passes them, several with (nseg, C) as the launch allows
        mr = (t["mean"][0].contiguous(), t["rstd"][0].contiguous()) if nseg == 1 else (t["mean"], t["rstd"])
        dx, dg, db = be.rowbn_bwd(*head, K, False, *mr, t["gamma"], t["beta"], c["slope"], False, None, nseg)
        assert dg is None and db is None
        exactly(dx, R.rowbn_stored(c["dx_eval"]["dx"], c["bf_in"]), "eval/dx")


def check_segments(be, dev, c, backward=True):
    """A dyadic case of nseg > 1 segments equals the restatement run on each segment alone, in call order: statistics
    with the running chain, apply, backward sums (dgamma / dbeta added over the segments) and dx."""
    t = inputs(c, dev)
    P, K, C, nseg = c["P"], c["K"], c["C"], c["nseg"]
    assert nseg > 1 and c["family"] == "dyadic"
    G = P // K if K else P
    rm, rv = c["rm0"].clone().to(dev), c["rv0"].clone().to(dev)
    nbt = torch.full((), 7, dtype=torch.int64, device=dev)
    mean, rstd = be.rowbn_stats(t["x"], S.EPS, S.MOMENTUM, rm, rv, nbt, nseg, t["mean_shift"])
    y, arg = be.rowbn_apply_max(t["x"], K, t["mean"], t["rstd"], t["gamma"], t["beta"], c["slope"], c["dother"], nseg)
    aff = c["gamma"] is not None
    if backward:
        dx, dg, db = be.rowbn_bwd(t["gy"], t["x"], t["arg"], K, True, t["mean"], t["rstd"], t["gamma"], t["beta"],
                                  c["slope"], aff, None, nseg)
    rm_r, rv_r, n_r, dg_r, db_r = c["rm0"], c["rv0"], 7, 0.0, 0.0
    for s in range(nseg):
        xs, gs = c["x"][s * P:(s + 1) * P], c["gy"][s * G:(s + 1) * G]
        st = R.rowbn_stats_ref(xs, 1, S.EPS, S.MOMENTUM, c["din"], rm_r, rv_r, n_r, c["mean_shift"])
        rm_r, rv_r, n_r = st["running_mean"], st["running_var"], st["num_batches_tracked"]
        exactly(mean[s], st["mean"][0], f"mean of segment {s}")
        assert ulps32(rstd[s], st["rstd"][0]) <= 1
        consts = (c["mean"][s], c["rstd"][s], c["gamma"], c["beta"], c["slope"])
        f = R.rowbn_apply_ref(xs, K, *consts, 1)
        exactly(y[s * G:(s + 1) * G], R.rowbn_stored(f["y"], c["bf_other"]), f"y of segment {s}")
        if K:
            assert torch.equal(arg[s * G:(s + 1) * G].cpu(), f["arg"]), f"arg of segment {s}"
        if not backward:
            continue
        b = R.rowbn_bwd_sums_ref(gs, xs, f["arg"], None, K, *consts, 1, c["din"], c["dother"])
        d = R.rowbn_bwd_apply_ref(gs, xs, f["arg"], K, *consts, b["c12"], 1)
        exactly(dx[s * P:(s + 1) * P], R.rowbn_stored(d["dx"], c["bf_in"]), f"dx of segment {s}")
        dg_r, db_r = dg_r + b["dgamma"], db_r + b["dbeta"]
    exactly(rm, rm_r, "running mean after the chain")
    exactly(rv, rv_r, "running var after the chain")
    assert int(nbt) == n_r
    if aff and backward:
        exactly(dg, R.r32(dg_r), "dgamma over the segments")
        exactly(db, R.r32(db_r), "dbeta over the segments")
