"""FlowEmbedding's single and stacked entries are one body: with one segment they are the same computation."""
import copy

import pytest
import torch


def _run(flow, entry, dev, autocast):
    """One training-mode forward + backward of a copy of `flow` through `entry` on fixed inputs:
    -> [output, the gradients of both feature inputs and of every parameter, the buffers afterwards]."""
    flow = copy.deepcopy(flow).to(dev).train()       # the BatchNorms and the spectral-norm vectors move
    B, N, C, K = 2, 64, 64, 32
    g = torch.Generator().manual_seed(5)
    p1, p2 = (torch.rand(B, N, 3, generator=g).to(dev) for _ in range(2))
    f1, f2 = (torch.randn(B, N, C, generator=g).to(dev).requires_grad_(True) for _ in range(2))
    idx = torch.randint(0, N, (B, N, K), generator=g).to(torch.int32).to(dev)
    with torch.autocast(device_type=dev, dtype=torch.bfloat16, enabled=autocast):
        if entry == "single":
            out = flow.forward_rows(p1, p2, f1, f2, 0.1, idx)
        else:
            out = flow.forward_rows_stacked(p1, p2, f1, f2, idx, 1)
    assert out.shape == (B, N, 128) and out.dtype == (torch.bfloat16 if autocast else torch.float32)
    weight = torch.linspace(-1, 1, out.numel(), device=dev).view_as(out)
    params = [p for _, p in sorted(flow.named_parameters())]
    grads = torch.autograd.grad((out.float() * weight).sum(), [f1, f2] + params)
    assert all(torch.isfinite(t).all() for t in grads) and all(float(t.abs().max()) > 0 for t in grads)
    return [out.detach()] + list(grads) + [b.clone() for _, b in sorted(flow.named_buffers())]


def _single_equals_stacked(dev, autocast):
    from tpgan_amd import set_abstraction as SA
    torch.manual_seed(11)
    flow = SA.FlowEmbedding(64, [64, 64, 128], sn=True)
    single, stacked = _run(flow, "single", dev, autocast), _run(flow, "stacked", dev, autocast)
    assert len(single) == len(stacked)
    for a, b in zip(single, stacked):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.gpu
def test_flow_embedding_stacked_with_one_segment_equals_forward_rows():
    """Training mode under bf16 autocast (the fused tail behind the gather): equal bits."""
    _single_equals_stacked("cuda", True)


def test_flow_embedding_stacked_with_one_segment_equals_forward_rows_cpu(oracle_cpu):
    """The same on CPU tensors with the oracle backend: fp32 rows, the per-layer path."""
    _single_equals_stacked("cpu", False)
