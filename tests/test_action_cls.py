"""set_abstraction.ActionCls against fixtures captured from the reference's own ActionCls (tests/golden/capture_cls_goldens.py
-> action_cls.npz), on the CPU over the oracle backend and on the GPU, in the manner of test_golden_models.py and at the
tolerances it applies to `action_tempo`: eval-mode logits 2e-5 (CPU) / 2e-4 (GPU), train-mode logits 5e-3 (training-mode
BatchNorm over a variance << eps on untrained nets), state after the train pass 5e-5 / 2e-4.

The last two tests are about the one-launch eval tails (`fused_eval`, ops.gather_mlp_max) inside ActionTempoDis(3).eval():
in fp32 the flag must change nothing and both settings meet discriminators.npz; under bf16 autocast the flag moves the five
tails behind a row gather onto the kernel, and both settings are held to the same bf16 bound (see the test).
"""
import numpy as np
import pytest
import torch

from test_golden_models import _capture_threads, _t, check_weights, close, cpu_dropout, load  # noqa: F401


def _renamed(name):
    return name[:-5] if name.endswith("_orig") else name


def run_action_cls(dev, tol, train_tol, state_tol):
    from tpgan_amd import set_abstraction as SA
    g = load("action_cls")
    clip = [_t(x, dev) for x in g["clip"]]

    def passes(m, prefix, seed):
        m.train()
        torch.manual_seed(seed)                           # same dropout draws as the reference run
        with cpu_dropout():
            close(m(list(clip), 2.0), g[f"{prefix}/train"], train_tol)
        check_weights(m, g, f"{prefix}/w_after", atol=state_tol)
        m.eval()
        with torch.no_grad():
            close(m(list(clip), 2.0), g[f"{prefix}/eval"], tol)

    torch.manual_seed(51)
    m = SA.ActionCls(3)
    check_weights(m, g, "cls/w")                          # same names, bit-identical seeded values
    assert all(x.fused_eval for x in m.modules() if isinstance(x, (SA._PointnetSAModuleBase, SA.FlowEmbedding)))
    m = m.to(dev)
    passes(m, "cls", 151)

    torch.manual_seed(52)
    src = SA.ActionTempoDis(3, sn=True)
    check_weights(src, g, "src/w")
    src = src.to(dev)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    buffers = {k for k, _ in m.named_buffers()}
    m.init_feature_extractor(src)
    check_weights(m, g, "init/w", atol=state_tol)         # (the running statistics come from this run's train pass)
    mine = dict(m.named_parameters())
    assert list(mine) == list(g["init/names"])
    assert [p.requires_grad for p in mine.values()] == list(g["init/requires_grad"])
    copied = set()
    for part in ("coarse_graining_module", "flow_module"):
        for name, p in getattr(src, part).named_parameters():
            key = f"{part}.{_renamed(name)}"
            if key in mine:
                assert torch.equal(mine[key], p) and not mine[key].requires_grad, key     # the UN-normalised weight_orig
                copied.add(key)
    assert any(k.endswith("0.weight") for k in copied) and len(copied) == sum(not r for r in g["init/requires_grad"])
    after = m.state_dict()
    for k in before:
        if k in buffers or k.startswith(("SA_pooling", "fc_layers")):
            assert torch.equal(before[k], after[k]), k                                       # untouched
            assert k in buffers or mine[k].requires_grad
    passes(m, "init", 152)


def test_action_cls_cpu(oracle_cpu):
    run_action_cls("cpu", 2e-5, 5e-3, 5e-5)


@pytest.mark.gpu
def test_action_cls_gpu():
    run_action_cls("cuda", 2e-4, 5e-3, 2e-4)


def test_fused_eval_defaults():
    from tpgan_amd import set_abstraction as SA
    kinds = (SA._PointnetSAModuleBase, SA.FlowEmbedding)
    for make in (lambda: SA.ActionTempoDis(3), SA.ActionSpatialDis, lambda: SA.FluidTempoDis(3), SA.FluidSpatialDis):
        m = make()
        levels = [x for x in m.modules() if isinstance(x, kinds)]
        assert levels and not any(x.fused_eval for x in levels)
        assert SA.set_fused_eval(m, True) is m and all(x.fused_eval for x in levels)
        SA.set_fused_eval(m, False)
        assert not any(x.fused_eval for x in levels)
    assert "fused_eval" not in "".join(SA.ActionCls(3).state_dict())


def _trained_action_tempo():
    """ActionTempoDis(3) in the state the golden's eval logits were taken in: seeded, one train pass, then eval."""
    from tpgan_amd import set_abstraction as SA
    g = load("discriminators")
    ahigh = [_t(x, "cuda") for x in g["action"]]
    torch.manual_seed(23)
    m = SA.ActionTempoDis(3)
    check_weights(m, g, "action_tempo/w")
    m = m.cuda().train()
    torch.manual_seed(103)
    with cpu_dropout():
        m(list(ahigh), 2.0)
    return m.eval(), ahigh, g["action_tempo/eval"]


@pytest.mark.gpu
def test_fused_eval_flag_keeps_the_fp32_eval_logits():
    """fp32 rows are not the kernel's: with the flag on or off the eval forward is today's, at the file's own 2e-4."""
    from tpgan_amd import set_abstraction as SA
    m, ahigh, want = _trained_action_tempo()
    assert not m.coarse_graining_module[0].fused_eval                     # the default stays off
    outs = []
    for flag in (False, True):
        SA.set_fused_eval(m, flag)
        with torch.no_grad():
            outs.append(m(list(ahigh), 2.0))
        close(outs[-1], want, 2e-4)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.gpu
def test_fused_eval_under_bf16_autocast(monkeypatch):
    """Under bf16 autocast the flag sends the two levels (frames stacked: one launch each) and the three flow-embedding
    calls of T = 3 through ops.gather_mlp_max; off, none.  Bound for BOTH settings against the reference's fp32 logits:
    a bf16 rounding is 2^-9 relative; about 20 of them lie in series between the clouds and the pooled feature (5 tails
    of 2-3 layers, their inputs and outputs), uncorrelated: sqrt(20) * 2^-9 = 2^-6.8 of the activation scale, which the
    untrained head passes on at O(1).  2^-5 of max(1, |logit|) leaves 3.5x for the max-pool picks that change."""
    import tpgan_amd.ops as ops
    from tpgan_amd import set_abstraction as SA
    m, ahigh, want = _trained_action_tempo()
    calls, feats = [], []
    real, pool = ops.gather_mlp_max, m.SA_pooling.forward_rows
    monkeypatch.setattr(ops, "gather_mlp_max", lambda *a, **k: (calls.append(a[0].shape), real(*a, **k))[1])
    monkeypatch.setattr(m.SA_pooling, "forward_rows", lambda xyz, f, *a: (feats.append(f.double()), pool(xyz, f, *a))[1])
    with torch.no_grad():
        m(list(ahigh), 2.0)                                              # fp32: the reference for the features below
    outs = {}
    for flag in (False, True):
        SA.set_fused_eval(m, flag)
        calls.clear()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            outs[flag] = m(list(ahigh), 2.0).float()
        assert len(calls) == (5 if flag else 0), calls
        err = float((outs[flag].cpu() - torch.from_numpy(want)).abs().max())
        print(f"fused_eval {flag}: max |logit - reference| {err:.3e}")
        close(outs[flag], want, 2.0 ** -5)
    # the flow module's output (B,256,256: what the five tails produce together) against the same module's fp32 forward:
    # the fused tails are held to the per-layer bf16 path's error, as the op is (rms <= 1.25 x, max-abs <= 2 x)
    e_layer, e_fused = (feats[1] - feats[0]).flatten(), (feats[2] - feats[0]).flatten()
    assert e_fused.numel() >= 10 ** 4
    rms = [float(e.pow(2).mean().sqrt()) for e in (e_fused, e_layer)]
    top = [float(e.abs().max()) for e in (e_fused, e_layer)]
    print(f"flow features: rms fused {rms[0]:.3e} per-layer {rms[1]:.3e}; max-abs fused {top[0]:.3e} per-layer {top[1]:.3e}")
    assert rms[0] <= 1.25 * rms[1] and top[0] <= 2.0 * top[1]
    # grad mode with parameters that want a gradient: the per-layer path, silently
    calls.clear()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        m(list(ahigh), 2.0)
    assert not calls
