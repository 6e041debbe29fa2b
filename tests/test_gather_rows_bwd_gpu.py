"""tpg_gather_rows_bwd_f32 with repeated centres: furthest point sampling repeats a pick once a cloud has no candidate
left (npoint = N with points the sampler skips, |x|^2 <= 1e-3), so several slots name one row.  Their gradients
are added in ascending slot order, each addition rounded in fp32: the same bits as that sum written out in numpy, run
after run.  With float atomics the order, and with three or more addends the last bits, changed from run to run, which
made the generator's update of a replayed step differ from the same step launched again."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,N,S,C", [(4, 1024, 1024, 3), (2, 300, 513, 3), (1, 64, 40, 6)])
def test_repeated_centres_are_summed_in_slot_order(B, N, S, C):
    import tpgan_amd.ops as ops
    rng = np.random.default_rng(S)
    idx = np.stack([rng.permutation(max(N, S))[:S] % N for _ in range(B)]).astype(np.int32)
    idx[:, S // 2::7] = idx[:, :1]                  # one row named by dozens of slots, far apart (other workgroups)
    idx[0, -5:] = idx[0, 1]
    g = (rng.standard_normal((B, S, C)) * np.exp(rng.uniform(-8, 8, (B, S, 1)))).astype(np.float32)
    want = np.zeros((B, N, C), dtype=np.float32)
    for b in range(B):
        for s in range(S):
            want[b, idx[b, s]] = want[b, idx[b, s]] + g[b, s]              # fp32, one rounding per addition
    x = torch.zeros(B, N, C, device="cuda", requires_grad=True)
    gd, id_ = torch.from_numpy(g).cuda(), torch.from_numpy(idx).cuda()
    for _ in range(5):
        (gx,) = torch.autograd.grad(ops.gather_rows(x, id_), x, gd)
        assert np.array_equal(gx.cpu().numpy().view(np.int32), want.view(np.int32))
