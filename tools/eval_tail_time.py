"""Eval-mode tails: the one-launch kernel (ops.gather_mlp_max, csrc/mlp_infer.hip) against the per-layer path it replaces,
accuracy and time, and the ActionCls.eval() forward end to end both ways.  GPU box.

    python tools/eval_tail_time.py --out profiles/eval_tail.txt

Shapes: the five tails behind a row gather at the sizes of one evaluation batch of tpgan_amd.classify (128 clips x 3
frames x 2048 points): level 1 on 384 clouds, level 2 on 384, flow depth 0 on 256 pairs, depth 1 on 128, plus the
(64,128) chain of the fluid discriminators' first level.  The neighbour lists are real ones (k nearest points of the
first S points of random clouds), so the gather has the locality of a ball query.
  per-layer  ops.row_combine (fp32 tables in, bf16 rows out) -> [rows_matmul (library GEMM) ->
             ops.row_bn_act(training=False)] per layer, the max over K fused into the last pair: what set_abstraction
             runs in eval mode with fused_eval off
  fused      one launch on the same fp32 tables, the weights' bf16 packing (two small launches per weight) included
Time: HIP events on the current stream, --warmup iterations of both first, then --reps alternating repeats, medians.
Accuracy: both against the formula in fp64, on 4 clouds of the same per-cloud shape (>= 10^4 outputs each).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import tpgan_amd  # noqa: F401
from tpgan_amd import ops
from tpgan_amd.graph_conv import rows_matmul
from tpgan_amd.set_abstraction import ActionCls, set_fused_eval
from tpgan_amd.synthetic import action_clip

# name, chain, clouds, N, S, K, slope
TAILS = [("level 1", (64, 64, 128), 384, 2048, 512, 64, 0.0),
         ("level 2", (128, 256), 384, 512, 256, 32, 0.0),
         ("flow depth 0", (256, 128, 256), 256, 256, 256, 32, 0.01),
         ("flow depth 1", (256, 256, 256), 128, 256, 256, 32, 0.01),
         ("fluid level 1", (64, 128), 96, 4096, 1024, 32, 0.01)]


def inputs(chain, B, N, S, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    C0 = chain[0]
    xyz = torch.randn(B, N, 3, device="cuda", generator=g)
    idx = ops.neighbour_search(xyz[:, :S].contiguous(), xyz, K)[1].to(torch.int32).contiguous()
    U = torch.randn(B, N, C0, device="cuda", generator=g)                  # fp32 tables, as the models hand them over
    Q = 0.5 * torch.randn(B, S, C0, device="cuda", generator=g)
    Ws, As, Cs = [], [], []
    for cin, cout in zip(chain[:-1], chain[1:]):
        Ws.append((torch.randn(cout, cin, device="cuda", generator=g) / cin ** 0.5).bfloat16().float())
        sign = torch.where(torch.rand(cout, device="cuda", generator=g) < 0.5, -1.0, 1.0)
        As.append((torch.rand(cout, device="cuda", generator=g) + 0.5) * sign)
        Cs.append(0.3 * torch.randn(cout, device="cuda", generator=g))
    return U, Q, idx, Ws, As, Cs, [(torch.zeros_like(a), torch.ones_like(a)) for a in As]


def per_layer(U, Q, idx, Ws, As, Cs, stats, slopes):
    K = idx.shape[2]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        x = ops.row_combine(U, Q, idx, ops.ROW_SUB, out_dtype=torch.bfloat16).view(-1, U.shape[2])
        x = ops.row_bn_act(x, None, None, None, None, False, 0.0, 0.0, slopes[0], 0, torch.bfloat16)
        for l, (W, a, c, (mean, var)) in enumerate(zip(Ws, As, Cs, stats)):
            x = rows_matmul(x, W)
            x = ops.row_bn_act(x, a, c, mean, var, False, 0.0, 0.0, slopes[l + 1],
                               K if l == len(Ws) - 1 else 0, torch.bfloat16)
    return x.view(U.shape[0], idx.shape[1], -1)


def fused(U, Q, idx, Ws, As, Cs, stats, slopes):
    with torch.no_grad():
        return ops.gather_mlp_max(U, Q, idx, Ws, As, Cs, slopes)


def formula_fp64(U, Q, idx, Ws, As, Cs, stats, slopes):
    act = lambda z, s: torch.maximum(z, s * z)                               # noqa: E731
    b = torch.arange(U.shape[0], device=U.device).view(-1, 1, 1)
    x = act(U.double()[b, idx.long()] - Q.double().unsqueeze(2), slopes[0])
    for W, a, c, sl in zip(Ws, As, Cs, slopes[1:]):
        x = act((x @ W.double().t()) * a.double() + c.double(), sl)
    return x.max(dim=2)[0]


def alternate_ms(fns, warmup, reps):
    """Median HIP-event time of each callable, run in turn `reps` times after `warmup` rounds."""
    st = torch.cuda.current_stream()
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    pairs = [[] for _ in fns]
    for _ in range(reps):
        for fn, lst in zip(fns, pairs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            fn()
            b.record(st)
            lst.append((a, b))
    torch.cuda.synchronize()
    return [float(np.median([a.elapsed_time(b) for a, b in lst])) for lst in pairs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clips", type=int, default=128, help="clips of the end-to-end forward")
    a = ap.parse_args()
    torch.backends.cudnn.enabled = False
    lines = [f"eval-mode tails, bf16 rows: per-layer path vs one fused launch (ms, median of {a.reps} alternating repeats "
             f"after {a.warmup} warm-up rounds; errors against the fp64 formula on 4 clouds)"]
    for n, (name, chain, B, N, S, K, slope) in enumerate(TAILS):
        slopes = [slope] * len(chain)
        small = inputs(chain, 4, N, S, K, seed=10 + n)
        ref = formula_fp64(*small, slopes)
        ef, ep = (fused(*small, slopes).double() - ref).flatten(), (per_layer(*small, slopes).double() - ref).flatten()
        acc = (f"rms {float(ef.pow(2).mean().sqrt()):.3e} / {float(ep.pow(2).mean().sqrt()):.3e}, "
               f"max-abs {float(ef.abs().max()):.3e} / {float(ep.abs().max()):.3e} (fused / per-layer, {ef.numel()} outputs)")
        del small, ref, ef, ep
        inp = inputs(chain, B, N, S, K, seed=20 + n)
        t_layer, t_fused = alternate_ms([lambda: per_layer(*inp, slopes), lambda: fused(*inp, slopes)], a.warmup, a.reps)
        rows = B * S * K
        flops = 2.0 * rows * sum(x * y for x, y in zip(chain[:-1], chain[1:]))
        lines.append(f"{name}: chain {chain}, {B} clouds x {N} points, {S} centres x {K} neighbours ({rows / 1e6:.1f} M rows)")
        lines.append(f"  per-layer {t_layer:.3f}   fused {t_fused:.3f}   ratio {t_layer / t_fused:.2f} x   "
                     f"fused = {flops / t_fused / 1e9:.0f} TFLOP/s of MFMA work")
        lines.append(f"  {acc}")
        del inp
        torch.cuda.empty_cache()

    # the classifier's eval forward end to end
    torch.manual_seed(0)
    model = ActionCls(3).cuda().eval()
    _, clip = action_clip(a.clips, 2048, 16, 3, seed=3, device="cuda")

    def forward(flag):
        set_fused_eval(model, flag)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return model(list(clip), 2.0)

    out_f, out_p = forward(True).float(), forward(False).float()
    t_p, t_f = alternate_ms([lambda: forward(False), lambda: forward(True)], a.warmup, max(a.reps // 2, 5))
    lines.append(f"ActionCls(3).eval() forward, {a.clips} clips x 3 frames x 2048 points, bf16 autocast, no_grad "
                 f"(FPS, searches and head included):")
    lines.append(f"  per-layer tails {t_p:.2f}   fused tails {t_f:.2f}   ratio {t_p / t_f:.2f} x   "
                 f"max |logit difference| {float((out_f - out_p).abs().max()):.3e} (untrained weights)")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
