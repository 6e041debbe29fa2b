"""The parts of the one-launch eval tail that need no GPU: the C entry's argument checks, the packed weight layout that
include/tpgan_ops.h documents, and the decisions that keep everything else on the per-layer path."""
import ctypes as C

import torch


def test_entry_rejects_bad_arguments_before_any_launch(hip_lib):
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    fwd = hip_lib.tpg_mlp_infer_fwd

    def call(B=1, N=8, S=8, K=16, chain=(64, 128, 0), slopes=(0.0, 0.0, 0.0), U=p, W2=None, a2=None, dtype=1):
        return fwd(U, p, p, dtype, B, N, S, K, *chain, p, W2, p, p, a2, a2, *slopes, p, None)

    assert call(chain=(64, 96, 0)) == -3 and call(chain=(256, 256, 512)) == -3          # chains that are not built
    assert call(K=20) == -3 and call(K=272) == -3 and call(K=0) == -1
    assert call(slopes=(2.0, 0.0, 0.0)) == -1 and call(slopes=(0.0, -0.5, 0.0)) == -1
    assert call(dtype=2) == -1 and call(dtype=0, chain=(64, 96, 0)) == -3
    assert call(U=None) == -1 and call(N=0) == -1 and call(B=-1) == -1
    assert call(chain=(64, 64, 128)) == -1                                             # second weight missing
    assert call(B=0) == 0 and call(S=0) == 0                                           # empty work
    sup = hip_lib.tpg_mlp_infer_supported
    for chain in [(64, 128, 0), (128, 256, 0), (64, 64, 128), (256, 128, 256), (256, 256, 256)]:
        assert sup(*chain, 16) == 1 and sup(*chain, 256) == 1 and sup(*chain, 24) == 0
    assert sup(128, 64, 0, 32) == 0


def test_packed_weight_is_the_documented_fragment_order():
    import tpgan_amd.ops as ops
    Cout, Cin = 128, 64
    rows = torch.arange(Cout, dtype=torch.float32).view(-1, 1).expand(Cout, Cin).contiguous()   # bf16 holds 0..255 exactly
    cols = torch.arange(Cin, dtype=torch.float32).view(1, -1).expand(Cout, Cin).contiguous()
    T, KS = Cout // 16, Cin // 32
    for W, want in ((rows, lambda t, s, lq, li, e: li * T + t), (cols, lambda t, s, lq, li, e: 32 * s + 8 * lq + e)):
        packed = ops.pack_infer_weight(W)
        assert packed.dtype == torch.bfloat16 and packed.shape == (T, KS, 4, 16, 8) and packed.is_contiguous()
        flat = packed.float().flatten()
        for t in range(T):
            for s in range(KS):
                for lq in range(4):
                    for li in range(16):
                        at = ((t * KS + s) * 64 + lq * 16 + li) * 8
                        assert flat[at:at + 8].tolist() == [float(want(t, s, lq, li, e)) for e in range(8)]


def test_cpu_rows_and_other_shapes_stay_on_the_per_layer_path(oracle_cpu):
    import tpgan_amd.ops as ops
    from tpgan_amd import set_abstraction as SA
    U = torch.zeros(1, 8, 64, dtype=torch.bfloat16)
    assert not ops.gather_mlp_max_supported(U, (64, 128), 16)                          # not on the GPU
    level = SA.SSGSetConv(npoint=4, radius=1.0, nsample=16, mlp=[3, 64, 128], sn=False).eval()
    level.fused_eval = True
    xyz = torch.randn(2, 16, 3)
    assert level._eval_tail(level.groupers[0], level.mlps[0], [xyz, xyz]) is None      # CPU tensors: today's path
    with torch.no_grad():
        assert level.forward_rows(xyz, xyz)[1].shape == (2, 4, 128)
    tail = SA._parse_tail(list(level.mlps[0])[1:], training=False)
    assert tail is not None and [c.out_channels for c in tail[1]] == [128] and tail[2] == [0.0, 0.0]
