"""What a backend's row-gather entries must return on a case of tests/rowgather_cases.py: the assertions that
tests/test_rowgather_gpu.py runs on the HIP kernels and tests/test_rowgather_cpu.py on the oracle's CPU backend (and on
planted defects).  One launch per check, every launch fed the TWIN's upstream values.

forward, both families: every stored element is the number the case holds (dyadic: the round-to-nearest-even of the
exact value; random: the fp32 restatement op for op, rounded once) -- as numbers: the two zeros are one value.
backward, dyadic: the same, sums included (they are exact in any order).
backward, random: |got - twin| <= oracle.ref_ops.rowcombine_bound per element -- depth * 2^-24 * sum |term|, a bf16
store's 2^-8 (|want| + that) on top, no additive slack, an element without terms exactly 0 (`note` records the
largest ratio per check).
both: two launches agree bit for bit; every cloud launched alone equals its slice of the batched launch bit for bit."""
import torch

import rowgather_cases as S
from oracle import ref_ops as R

OLD_TOL = {"f32": 1e-5, "bf16": 1e-2}          # tests/test_ops_gpu.py::test_rowcombine_fwd_exact_bwd_close


def old_ok(got, ref, bf16):
    """The criterion the row-gather gradients were held to before: a fraction of the tensor's largest magnitude."""
    ref = R._f64(ref).cpu()
    err = (R._f64(got).cpu() - ref).abs().max()
    return bool(err <= OLD_TOL["bf16" if bf16 else "f32"] * max(1.0, float(ref.abs().max())))


def mismatches(got, want32):
    """Elements of `got` (as stored) that are not the fp32 number want32 holds (a NaN is never equal)."""
    assert tuple(got.shape) == tuple(want32.shape), (got.shape, want32.shape)
    return int((got.detach().float() != want32.to(got.device)).sum())


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def inputs(c, dev, clamp=False, cloud=None):
    """The case's tensors on `dev` in their row types (clamp: indices clamped beforehand, for a backend that does not
    clamp; cloud: that cloud alone)."""
    cut = (lambda t: t) if cloud is None else (lambda t: t[cloud:cloud + 1].contiguous())
    t = dict(idx=cut(c["idxc" if clamp else "idx"]).to(dev))
    for name, dt in (("U", c["din"]), ("QE", c["din"]), ("Y", c["din"]), ("g", c["dout"])):
        if c.get(name) is not None:
            t[name] = cut(c[name]).to(dev, dt)
            assert torch.equal(t[name].float(), cut(c[name]).to(dev)), name     # the values ARE of the row type
    return t


def launch_fwd(be, c, t):
    if c["mode"] == "FRONT":
        return be.rowcombine_edge_fwd(t["Y"], t["idx"], c["slope_a"], c["slope"], c["dout"])
    return be.rowcombine_fwd(t["U"], t.get("QE"), t["idx"], S.MODE[c["mode"]], c["slope"], c["dout"])


def launch_bwd(be, c, t):
    """-> {name: tensor} under the twin's names (gU, gQE; the front end: gE, gA, the two halves of gY)."""
    C = c["C"]
    if c["mode"] == "FRONT":
        gY = be.rowcombine_edge_bwd(t["g"], t["idx"], t["Y"], c["slope_a"], c["slope"])
        assert gY.dtype == c["din"] and tuple(gY.shape) == (t["Y"].shape[0], c["N"], 2 * C)
        return dict(gE=gY[:, :, :C], gA=gY[:, :, C:])
    mode = S.MODE[c["mode"]]
    gU, gQ = be.rowcombine_bwd(t["g"], t["idx"], t["QE"] if c["mode"] == "EDGE" else None, mode, c["N"], c["slope"],
                               c["din"])
    assert gU.dtype == c["din"] and (gQ is None) == (mode == R.ROW_GATHER)
    return dict(gU=gU) if gQ is None else dict(gU=gU, gQE=gQ)


def judge(c, name, got, cloud=None):
    """One gradient tensor against the twin -> dyadic: the number of elements that differ; random: the largest
    error / bound (inf where an element with bound 0 differs)."""
    t = c["bwd"][name]
    if cloud is not None:
        t = {k: v[cloud:cloud + 1] for k, v in t.items()}
    assert tuple(got.shape) == tuple(t["v"].shape), (name, got.shape, t["v"].shape)
    if c["family"] == "dyadic":
        return mismatches(got, S._stored32(t["v"], c["bf_in"]))
    if not bool(torch.isfinite(got.float()).all()):
        return float("inf")
    return R.err_ratio(got.float(), t["v"], R.rowcombine_bound(t, c["bf_in"]))


def check_forward(be, dev, c, clamp=False):
    out = launch_fwd(be, c, inputs(c, dev, clamp))
    assert out.dtype == c["dout"] and tuple(out.shape) == (c["B"], c["S"], c["K"], c["C"])
    n = mismatches(out, c["out"])
    assert n == 0, f"forward: {n} of {out.numel()} elements differ from the oracle"


def check_backward(be, dev, c, note, clamp=False):
    t = inputs(c, dev, clamp)
    first, second = launch_bwd(be, c, t), launch_bwd(be, c, t)
    assert sorted(first) == sorted(k for k in c["bwd"] if k != "L" and (c["mode"] != "FRONT" or k != "gU"))
    for name, got in first.items():
        assert torch.equal(bits(got), bits(second[name])), f"{name} differs between two launches"
        fig = judge(c, name, got)
        if c["family"] == "dyadic":
            assert fig == 0, f"{name}: {fig} of {got.numel()} elements differ from the oracle"
        else:
            note(f"{c['mode']}/{name}/{'bf16' if c['bf_in'] else 'f32'}", fig)
    for b in range(c["B"]) if c["B"] > 1 else ():
        alone = launch_bwd(be, c, inputs(c, dev, clamp, cloud=b))
        for name, got in alone.items():
            assert torch.equal(bits(got), bits(first[name][b:b + 1])), f"{name} of cloud {b} depends on the batch"
