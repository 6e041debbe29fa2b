"""ops.gather_mlp_max (csrc/mlp_infer.hip: gather -> act -> GEMM -> affine + act [-> GEMM -> affine + act] -> max over K
in one launch) against its formula in fp64 torch, and against today's per-layer path on the same inputs.

Inputs of the first tests: U, Q are bf16 and the weights are bf16-representable, so neither path loses anything on its
operands and the fp64 formula is the exact answer both approximate.  The models hand over fp32 tables whose difference
must not be rounded away: the tests at the end of the file are about those, op and modules.
Where they round: the fused launch rounds act_0(U - Q) (exact in fp32) once to bf16, the hidden layer once to bf16 and the result once to bf16; the per-layer path rounds at the same
three places and, in addition, the difference before act_0 and every GEMM output before its affine.

Tolerances
  absolute: every rounding is 2^-9 relative on one operand or result; a layer's dot product of C such terms with
      independent signs grows like sqrt(C) * 2^-9 * |w| |x|, which the weights (unit row norm / sqrt(C)) bring back to
      2^-9 of the activation scale, times the next layer's scale (<= 1.5), two layers and the output rounding:
      a few 2^-9 of the largest output.  8 * 2^-9 = 2^-6 of max|ref| is asserted per case; a wrong channel, a dropped
      neighbour or a max taken before the affine is off by O(1) of that scale.
  relative to the per-layer path, pooled over all cases (>= 10^4 outputs): RMS error <= 1.25 x, max-abs error <= 2 x
      the per-layer path's (the fused path rounds at a subset of its places; the margins cover the finite sample).
"""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

B, N, S = 3, 70, 5                      # N no multiple of 16, 15 groups: the last workgroup is partly filled
CHAINS = [(64, 128), (128, 256), (64, 64, 128), (256, 128, 256), (256, 256, 256)]
KS = [16, 32, 64]
SLOPES = [0.0, 0.01]
CASES = list(itertools.product(CHAINS, KS, SLOPES))


def _inputs(chain, K, seed, n_clouds=B, n_src=N, n_groups=S):
    g = torch.Generator().manual_seed(seed)
    C0 = chain[0]
    U = (torch.randn(n_clouds, n_src, C0, generator=g) + 0.3 * torch.randn(1, 1, C0, generator=g)).bfloat16().cuda()
    Q = (0.5 * torch.randn(n_clouds, n_groups, C0, generator=g)).bfloat16().cuda()
    idx = torch.randint(0, n_src, (n_clouds, n_groups, K), generator=g, dtype=torch.int32).cuda()   # with repeats
    Ws, As, Cs = [], [], []
    for cin, cout in zip(chain[:-1], chain[1:]):
        Ws.append((torch.randn(cout, cin, generator=g) / cin ** 0.5).bfloat16().float().cuda())
        sign = torch.where(torch.rand(cout, generator=g) < 0.5, -1.0, 1.0)                           # mixed signs
        As.append(((torch.rand(cout, generator=g) + 0.5) * sign).cuda())
        Cs.append((0.3 * torch.randn(cout, generator=g)).cuda())
    return U, Q, idx, Ws, As, Cs


def _act(z, slope):
    return torch.maximum(z, slope * z)


def _formula_fp64(U, Q, idx, Ws, As, Cs, slopes):
    b = torch.arange(U.shape[0], device=U.device).view(-1, 1, 1)
    x = _act(U.double()[b, idx.long()] - Q.double().unsqueeze(2), slopes[0])                          # (B,S,K,C0)
    for W, a, c, sl in zip(Ws, As, Cs, slopes[1:]):
        x = _act((x @ W.double().t()) * a.double() + c.double(), sl)
    return x.max(dim=2)[0]


def _per_layer(U, Q, idx, Ws, As, Cs, slopes):
    """Today's eval path: row_combine -> [rows_matmul -> row_bn_act(training=False)]*, max fused into the last pair."""
    import tpgan_amd.ops as ops
    from tpgan_amd.graph_conv import rows_matmul
    K = idx.shape[2]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        x = ops.row_combine(U, Q, idx, ops.ROW_SUB, out_dtype=torch.bfloat16).view(-1, U.shape[2])
        x = ops.row_bn_act(x, None, None, None, None, False, 0.0, 0.0, slopes[0], 0, torch.bfloat16)
        for l, (W, a, c) in enumerate(zip(Ws, As, Cs)):
            x = rows_matmul(x, W)
            zero, one = torch.zeros_like(a), torch.ones_like(a)
            x = ops.row_bn_act(x, a, c, zero, one, False, 0.0, 0.0, slopes[l + 1], K if l == len(Ws) - 1 else 0,
                               torch.bfloat16)
    return x.view(U.shape[0], idx.shape[1], -1)


@pytest.fixture(scope="module")
def results():
    """Every case once: (inputs, fused, per-layer, fp64 formula)."""
    import tpgan_amd.ops as ops
    out = {}
    for n, (chain, K, slope) in enumerate(CASES):
        inp = _inputs(chain, K, seed=100 + n)
        slopes = [slope] * len(chain)
        with torch.no_grad():
            fused = ops.gather_mlp_max(*inp, slopes)
        out[(chain, K, slope)] = (inp, fused, _per_layer(*inp, slopes), _formula_fp64(*inp, slopes))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("chain,K,slope", CASES)
def test_fused_tail_matches_the_fp64_formula(results, chain, K, slope):
    inp, fused, _, ref = results[(chain, K, slope)]
    assert fused.shape == (B, S, chain[-1]) and fused.dtype == torch.bfloat16
    err = float((fused.double() - ref).abs().max())
    bound = 2.0 ** -6 * float(ref.abs().max())
    print(f"chain {chain} K {K} slope {slope}: max|err| {err:.3e} bound {bound:.3e}")
    assert err <= bound


def test_fused_tail_is_no_less_accurate_than_the_per_layer_path(results):
    ef = torch.cat([(f.double() - r).flatten() for _, f, _, r in results.values()])
    ep = torch.cat([(p.double() - r).flatten() for _, _, p, r in results.values()])
    assert ef.numel() >= 10 ** 4
    rms_f, rms_p = float(ef.pow(2).mean().sqrt()), float(ep.pow(2).mean().sqrt())
    max_f, max_p = float(ef.abs().max()), float(ep.abs().max())
    print(f"outputs {ef.numel()}: rms fused {rms_f:.4e} per-layer {rms_p:.4e} ratio {rms_f / rms_p:.3f}; "
          f"max-abs fused {max_f:.4e} per-layer {max_p:.4e} ratio {max_f / max_p:.3f}")
    assert rms_f <= 1.25 * rms_p
    assert max_f <= 2.0 * max_p


@pytest.mark.parametrize("chain,K", [((64, 64, 128), 64), ((128, 256), 32), ((256, 256, 256), 32), ((64, 128), 16)])
def test_every_neighbour_position_can_win(chain, K):
    """Group s gathers one common row at every position except s mod K, where it gathers another row: on the channels
    where that row wins, the maximum sits at position s mod K -- every strip, lane quarter and accumulator row holds the
    winner in one of the K groups, and a kernel that skipped the position would return the common row's value."""
    import tpgan_amd.ops as ops
    U, Q, _, Ws, As, Cs = _inputs(chain, K, seed=7, n_clouds=1, n_src=N, n_groups=K)
    idx = torch.zeros(1, K, K, dtype=torch.int32, device="cuda")
    s = torch.arange(K, device="cuda")
    idx[0, s, s] = (1 + s % (N - 1)).int()
    slopes = [0.01] * len(chain)
    with torch.no_grad():
        fused = ops.gather_mlp_max(U, Q, idx, Ws, As, Cs, slopes)
    ref = _formula_fp64(U, Q, idx, Ws, As, Cs, slopes)
    common = _formula_fp64(U, Q, torch.zeros_like(idx), Ws, As, Cs, slopes)
    wins = ref > common + 2.0 ** -4 * ref.abs().max()           # clearly decided by the odd position
    assert bool(wins.any(dim=2).all()), "every group needs a channel that its odd neighbour wins"
    err = (fused.double() - ref).abs()
    assert float(err.max()) <= 2.0 ** -6 * float(ref.abs().max())


def test_runs_are_bit_identical_and_the_tiling_does_not_show(results):
    import tpgan_amd.ops as ops
    for (chain, K, slope), (inp, fused, _, _) in results.items():
        if slope != 0.01:
            continue
        U, Q, idx, Ws, As, Cs = inp
        slopes = [slope] * len(chain)
        with torch.no_grad():
            again = ops.gather_mlp_max(U, Q, idx, Ws, As, Cs, slopes)
            assert torch.equal(again, fused)
            for b in range(B):
                alone = ops.gather_mlp_max(U[b:b + 1].contiguous(), Q[b:b + 1].contiguous(), idx[b:b + 1].contiguous(),
                                           Ws, As, Cs, slopes)
                assert torch.equal(alone[0], fused[b]), (chain, K, b)


def test_more_groups_than_the_grid_holds_at_once():
    """Waves walk groups with the grid's stride: 2 * 1030 groups make every workgroup of the (256,256,256) launch (one
    per CU) take a second round and leave the last round partly filled."""
    import tpgan_amd.ops as ops
    chain, K = (256, 256, 256), 32
    U, Q, idx, Ws, As, Cs = _inputs(chain, K, seed=11, n_clouds=2, n_src=N, n_groups=1030)
    slopes = [0.01] * 3
    with torch.no_grad():
        fused = ops.gather_mlp_max(U, Q, idx, Ws, As, Cs, slopes)
    ref = _formula_fp64(U, Q, idx, Ws, As, Cs, slopes)
    assert float((fused.double() - ref).abs().max()) <= 2.0 ** -6 * float(ref.abs().max())


def test_unsupported_shapes_and_bad_arguments():
    import tpgan_amd.ops as ops
    U, Q, idx, Ws, As, Cs = _inputs((64, 128), 16, seed=3)
    sup = ops.gather_mlp_max_supported
    assert sup(U, (64, 128), 16) and sup(U, (64, 64, 128), 64) and sup(U, (256, 256, 256), 256)
    assert not sup(U, (256, 256, 512), 32)            # the 512-wide pooling tails
    assert not sup(U, (64, 128), 20) and not sup(U, (64, 128), 272) and not sup(U, (64, 128), 0)
    assert not sup(U.float(), (64, 128), 16)          # fp32 rows
    assert sup(U.float(), (64, 128), 16, torch.bfloat16) and not sup(U, (64, 128), 16, torch.float32)   # fp32 TABLES, bf16 rows
    assert not sup(U.cpu(), (64, 128), 16)
    assert not sup(U, (128, 64), 16) and not sup(U, (64,), 16)
    sl = [0.01, 0.01]
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="bf16"):
            ops.gather_mlp_max(U.float(), Q, idx, Ws, As, Cs, sl)
        with pytest.raises(RuntimeError, match="not built"):
            ops.gather_mlp_max(U, Q, idx[:, :, :12].contiguous(), Ws, As, Cs, sl)
        with pytest.raises(RuntimeError, match="int32"):
            ops.gather_mlp_max(U, Q, idx.long(), Ws, As, Cs, sl)
        with pytest.raises(RuntimeError, match="Q must be"):
            ops.gather_mlp_max(U, Q[:, :3].contiguous(), idx, Ws, As, Cs, sl)
        with pytest.raises(RuntimeError, match="does not follow"):
            ops.gather_mlp_max(U, Q, idx, [Ws[0][:, :32].contiguous()], As, Cs, sl)
        with pytest.raises(RuntimeError, match="per output channel"):
            ops.gather_mlp_max(U, Q, idx, Ws, [As[0][:64]], Cs, sl)
        with pytest.raises(RuntimeError, match="slopes"):
            ops.gather_mlp_max(U, Q, idx, Ws, As, Cs, [0.01, 1.5])
        with pytest.raises(RuntimeError, match="one slope more"):
            ops.gather_mlp_max(U, Q, idx, Ws, As, Cs, [0.01])
    # the C entry refuses what it was not built for, before any launch
    hip = ops.backend_for(U)
    p = U.data_ptr()
    assert hip.lib.tpg_mlp_infer_fwd(p, p, p, 1, 1, 8, 8, 16, 64, 96, 0, p, None, p, p, None, None, 0.0, 0.0, 0.0, p, None) == -3
    assert hip.lib.tpg_mlp_infer_fwd(p, p, p, 1, 1, 8, 8, 20, 64, 128, 0, p, None, p, p, None, None, 0.0, 0.0, 0.0, p, None) == -3
    assert hip.lib.tpg_mlp_infer_fwd(p, p, p, 1, 1, 8, 8, 16, 64, 128, 0, p, None, p, p, None, None, 2.0, 0.0, 0.0, p, None) == -1
    assert hip.lib.tpg_mlp_infer_fwd(p, None, p, 1, 1, 8, 8, 16, 64, 128, 0, p, None, p, p, None, None, 0.0, 0.0, 0.0, p, None) == -1
    assert hip.lib.tpg_mlp_infer_fwd(p, p, p, 1, 1, 8, 8, 16, 64, 64, 128, p, None, p, p, None, None, 0.0, 0.0, 0.0, p, None) == -1
    assert hip.lib.tpg_mlp_infer_fwd(p, p, p, 7, 1, 8, 8, 16, 64, 128, 0, p, None, p, p, None, None, 0.0, 0.0, 0.0, p, None) == -1
    assert hip.lib.tpg_mlp_infer_fwd(p, p, p, 1, 0, 8, 8, 16, 64, 128, 0, p, None, p, p, None, None, 0.0, 0.0, 0.0, p, None) == 0


def test_inputs_that_require_grad_are_refused():
    import tpgan_amd.ops as ops
    U, Q, idx, Ws, As, Cs = _inputs((64, 128), 16, seed=5)
    Ws[0].requires_grad_(True)
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.gather_mlp_max(U, Q, idx, Ws, As, Cs, [0.0, 0.0])
    with torch.no_grad():                                          # the same call without a graph goes through
        assert ops.gather_mlp_max(U, Q, idx, Ws, As, Cs, [0.0, 0.0]).shape == (B, S, 128)
    Ws[0].requires_grad_(False)
    assert ops.gather_mlp_max(U, Q, idx, Ws, As, Cs, [0.0, 0.0]).shape == (B, S, 128)


# ---- fp32 tables: what the models hand over.  The difference U[idx] - Q must be taken BEFORE anything is rounded ------
def _offset_tables(chain, K, seed, offset):
    """fp32 tables whose entries are large against their differences: every row = a common per-channel level of
    magnitude `offset` plus an O(1) part, as the first conv gives for a cloud far from the origin or a BatchNorm with
    a large running mean folded in.  Rounded to bf16 first, a row would lose 2^-9 * offset, not 2^-9 * |U - Q|."""
    U, Q, idx, Ws, As, Cs = _inputs(chain, K, seed)
    g = torch.Generator().manual_seed(seed + 1)
    level = (offset * (1.0 + torch.rand(1, 1, chain[0], generator=g))).cuda()
    return (U.float() + level).contiguous(), (Q.float() + level).contiguous(), idx, Ws, As, Cs


@pytest.mark.parametrize("offset", [0.0, 40.0])
def test_fp32_tables_are_subtracted_before_they_are_rounded(offset):
    """Same bounds as on bf16 tables, against the per-layer path on the SAME fp32 tables (row_combine subtracts in fp32
    and rounds the difference once): rms <= 1.25 x, max-abs <= 2 x, pooled over all chains (>= 10^4 outputs), and the
    absolute 2^-6 of max|ref| per chain -- at offset 40 a kernel that rounded the tables first would be off by
    2^-9 * 40..80 = 0.08..0.16 per input element, an order of magnitude above both."""
    import tpgan_amd.ops as ops
    ef, ep = [], []
    for n, chain in enumerate(CHAINS):
        inp = _offset_tables(chain, 32, 300 + n, offset)
        slopes = [0.01] * len(chain)
        ref = _formula_fp64(*inp, slopes)
        with torch.no_grad():
            fused = ops.gather_mlp_max(*inp, slopes)
        layer = _per_layer(*inp, slopes)
        assert float((fused.double() - ref).abs().max()) <= 2.0 ** -6 * float(ref.abs().max()), chain
        ef.append((fused.double() - ref).flatten())
        ep.append((layer.double() - ref).flatten())
    ef, ep = torch.cat(ef), torch.cat(ep)
    assert ef.numel() >= 10 ** 4
    rms_f, rms_p = float(ef.pow(2).mean().sqrt()), float(ep.pow(2).mean().sqrt())
    max_f, max_p = float(ef.abs().max()), float(ep.abs().max())
    print(f"offset {offset}: rms fused {rms_f:.4e} per-layer {rms_p:.4e}; max-abs fused {max_f:.4e} per-layer {max_p:.4e}")
    assert rms_f <= 1.25 * rms_p and max_f <= 2.0 * max_p


def _shifted_statistics(module, seed):
    """Running statistics and affines a trained net would have: non-zero means, variances away from 1, mixed-sign weights."""
    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d)):
            n = m.num_features
            m.running_mean.copy_(2.0 * torch.randn(n, generator=g))
            m.running_var.copy_(0.5 + torch.rand(n, generator=g))
            m.weight.data.copy_((0.5 + torch.rand(n, generator=g)) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0))
            m.bias.data.copy_(0.3 * torch.randn(n, generator=g))
    return module


def _module_errors(run, module):
    """run() in fp32 (the reference: same module, no autocast) and under bf16 autocast with fused_eval off / on ->
    (errors of the fused path, errors of the per-layer path), flattened."""
    from tpgan_amd import set_abstraction as SA
    import tpgan_amd.ops as ops
    calls = []
    real = ops.gather_mlp_max
    ops.gather_mlp_max = lambda *a, **k: (calls.append(a[0].dtype), real(*a, **k))[1]
    try:
        with torch.no_grad():
            ref = run().double()
            out = {}
            for flag in (False, True):
                SA.set_fused_eval(module, flag)
                n = len(calls)
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    out[flag] = run().double()
                assert (len(calls) > n) == flag
    finally:
        ops.gather_mlp_max = real
    assert all(d == torch.float32 for d in calls)              # the models hand over fp32 tables
    return (out[True] - ref).flatten(), (out[False] - ref).flatten()


def test_model_tails_are_as_accurate_fused_as_per_layer_off_centre():
    """The eval forward of a set-abstraction level (single call and frames stacked) and of a flow embedding, on clouds 5
    units off the origin and with BatchNorm statistics of non-zero mean: the fused tails' error against the module's own
    fp32 forward is held to the per-layer bf16 path's on the same module (rms <= 1.25 x, max-abs <= 2 x; > 10^4
    outputs).  Before the kernel took fp32 tables the off-centre cloud alone made the fused error several times larger."""
    from tpgan_amd import set_abstraction as SA
    torch.manual_seed(3)
    g = torch.Generator().manual_seed(4)
    xyz = (0.5 * torch.randn(4, 256, 3, generator=g) + 5.0).cuda()
    level = _shifted_statistics(SA.SSGSetConv(npoint=64, radius=0.8, nsample=64, mlp=[3, 64, 64, 128], sn=False), 5).cuda().eval()
    fluid = _shifted_statistics(SA.SSGSetConv(npoint=64, radius=0.3, nsample=32, mlp=[3, 64, 128], sn=False,
                                              act_fn=torch.nn.LeakyReLU()), 6).cuda().eval()
    flow = _shifted_statistics(SA.FlowEmbedding(256, [256, 128, 256]), 7).cuda().eval()
    p1, p2 = xyz[:, :128].contiguous(), (xyz[:, 128:] + 0.05).contiguous()
    f1, f2 = torch.randn(4, 128, 256, generator=g).cuda(), torch.randn(4, 128, 256, generator=g).cuda()
    runs = [(level, lambda: level.forward_rows(xyz, xyz)[1].float()),
            (level, lambda: level.forward_rows_stacked(xyz, xyz, 2)[1].float()),
            (fluid, lambda: fluid.forward_rows(xyz, xyz)[1].float()),
            (flow, lambda: flow.forward_rows(p1, p2, f1, f2, 2.0).float())]
    ef, ep = [], []
    for module, run in runs:
        a, b = _module_errors(run, module)
        ef.append(a)
        ep.append(b)
        print(f"{type(module).__name__}: rms fused {float(a.pow(2).mean().sqrt()):.3e} per-layer {float(b.pow(2).mean().sqrt()):.3e}; "
              f"max-abs fused {float(a.abs().max()):.3e} per-layer {float(b.abs().max()):.3e}")
        assert float(a.pow(2).mean().sqrt()) <= 1.25 * float(b.pow(2).mean().sqrt())
        assert float(a.abs().max()) <= 2.0 * float(b.abs().max())
    assert sum(x.numel() for x in ef) >= 10 ** 4
