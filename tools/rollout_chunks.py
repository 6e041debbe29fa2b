"""Sequence upsampling: the reference's per-frame `forward_with_context` loop (upsampling_network.py:159-174, the demo
notebooks' B = 1 rollout) against `tpgan_amd.rollout.SequenceUpsampler` at several chunk sizes.  GPU box.

For N low-resolution points per frame, fp32 and bf16 autocast, output left on the device or copied to the host frame by
frame (what the demo does before np.save): ms per frame, frames/s, the speedup over the loop and the peak memory.
Chunks whose T * N exceeds MAX_POINTS are skipped ("what fits").  The net is `force_all_keep` (every slot survives:
the largest output, the benchmark regime of SURVEY.md section 8d).

    python tools/rollout_chunks.py [--sizes 1024 4096 16384 65536] [--chunks 1 4 16 64] [--frames F]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import tpgan_amd  # noqa: F401
from tpgan_amd.rollout import SequenceUpsampler, default_chunk
from tpgan_amd.srnet import SRNet
from tpgan_amd.synthetic import fluid_clip, force_all_keep

MAX_POINTS = 1 << 20            # low-resolution points per chunk the table goes up to


def loop(net, feats, pos, host):
    hist, n = [], 0
    for t in range(pos.shape[0]):
        out, hist = net.forward_with_context(feats[t:t + 1], pos[t:t + 1], hist)
        n += out.cpu().shape[1] if host else out.shape[1]
    return n


def chunked(net, feats, pos, host, chunk):
    outs = SequenceUpsampler(net, chunk).push(feats, pos)
    return sum(o.cpu().shape[1] if host else o.shape[1] for o in outs)


def timed(fn, dtype):
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == "bf16"):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        n = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, n, torch.cuda.max_memory_allocated() / 2 ** 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096, 16384, 65536])
    ap.add_argument("--chunks", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--frames", type=int, default=0, help="frames per timed run (0: 64, 16 from 65536 points)")
    a = ap.parse_args()
    torch.backends.cudnn.enabled = False
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    net = force_all_keep(SRNet(3, 128)).to(dev).eval()
    print(f"{'N':>6} {'dtype':>5} {'output':>6} {'path':>10} {'chunk':>5} {'ms/frame':>9} {'frames/s':>9} "
          f"{'speedup':>7} {'peak GiB':>8}", flush=True)
    for n in a.sizes:
        chunks = [c for c in a.chunks if c * n <= MAX_POINTS]
        frames = a.frames or (16 if n >= 65536 else 64)
        frames = max(frames, max(chunks))
        low, _ = fluid_clip(1, n * 8, 8, frames, seed=n, device=dev)
        pos = torch.cat(low).contiguous()
        for dtype in ("fp32", "bf16"):
            for host in (False, True):
                runs = [("loop", None, lambda: loop(net, pos, pos, host))]
                runs += [("sequence", c, (lambda c=c: chunked(net, pos, pos, host, c))) for c in chunks]
                base, count = None, None
                for name, c, fn in runs:
                    w = c or 1                                       # warm-up: one chunk (GEMM plans, workspaces)
                    timed(lambda: (loop(net, pos[:w], pos[:w], host) if c is None
                                   else chunked(net, pos[:w], pos[:w], host, c)), dtype)
                    sec, got, peak = timed(fn, dtype)
                    assert count is None or got == count, (name, c, got, count)
                    count = got
                    ms = sec / frames * 1e3
                    base = base or ms
                    print(f"{n:6d} {dtype:>5} {'host' if host else 'device':>6} {name:>10} {c or 1:5d} {ms:9.3f} "
                          f"{1e3 / ms:9.1f} {base / ms:7.2f} {peak:8.2f}", flush=True)
        print(f"# {n} points: default chunk {default_chunk(n)}", flush=True)


if __name__ == "__main__":
    main()
