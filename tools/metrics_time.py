"""Earth mover's distance (`ops.emd_match`, csrc/emd.hip) and Gaussian row sums (csrc/gauss_sum.hip) on the GPU box:
rounds, launches and milliseconds, the threshold / batch table behind HipBackend's EMD defaults, and the distance of
the matching from scipy's optimum.

    python tools/metrics_time.py --out profiles/metrics.txt [--sizes 1024 4096 16384] [--batches 1 8] [--no-full-frame]

Every timed case runs in a child process of its own (`--case`, one JSON line back) under its own time limit.  The
child drives the matching's three steps itself (HipBackend.emd_begin / emd_batch / emd_end, the loop of
HipBackend.emd_match) so that it can count launches and give up between two batches after `--limit` seconds or at the
round cap, which is reported as "not finished"; the process limit on top is a backstop.  After a case that fails or is
killed nothing further is started.

Clouds: two consecutive frames of synthetic.py's fluid clip in their joint normalisation (metrics.position_loss), two
consecutive frames of its action clip, halved (metrics.action_position_loss).  Settings: "default" is
ops.EMD_DEFAULTS (eps 1e-4, 3 phases, scaling 4); "metric" is what the metrics pass (fluid eps 0.03, action eps 0.002,
phases from metrics.schedule_phases, round cap metrics.round_cap(n, 3000)).  The sweep rows force the threshold
(`narrow`, persons) and the wide rounds per batch (`every`); '-' is the shipped default, printed in the header.  Times are wall-clock around one synchronised call after a warm-up on a small
cloud: a call synchronises once per batch of launches by design.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clouds(kind, n, B, device):
    import torch
    from tpgan_amd import metrics
    from tpgan_amd.synthetic import action_clip, fluid_clip
    if kind == "fluid":
        _, high = fluid_clip(B, n, 8, 2, seed=n + B, device=device)
        corner, h = metrics._joint_frame(high[0], high[1])
        return ((high[0] - corner) / h).contiguous(), ((high[1] - corner) / h).contiguous()
    _, high = action_clip(B, n, 16, 2, seed=n + B, device=device)
    return (high[0] / 2.0).contiguous(), (high[1] / 2.0).contiguous()


def settings(kind, which):
    from tpgan_amd import metrics, ops
    if which == "default":
        d = ops.EMD_DEFAULTS
        return d["eps"], d["phases"], d["scaling"], lambda n: d["iters"]
    eps = 0.03 if kind == "fluid" else 0.002
    return eps, metrics.schedule_phases(eps), ops.EMD_DEFAULTS["scaling"], lambda n: metrics.round_cap(n, 3000)


def drive(hip, x1, x2, eps, iters, phases, scaling, narrow_at, wide, limit):
    """HipBackend.emd_match's loop with counters and a deadline -> (outputs or None, info)"""
    n = x1.shape[1]
    narrow_at = hip.emd_narrow_at(n) if narrow_at is None else max(0, min(narrow_at, n))
    wide = hip.EMD_CHECK_EVERY if wide is None else wide
    st = hip.emd_begin(x1, x2, phases)
    info = {"batches": 0, "launches": 1, "narrow_at": narrow_at}
    deadline = time.monotonic() + limit
    while True:
        rec, launches = hip.emd_batch(st, eps, iters, scaling, narrow_at, wide)
        info["batches"] += 1
        info["launches"] += launches
        status = rec[:, 3]
        if bool((status == 1).all()):
            info["launches"] += 1
            return hip.emd_end(st), info
        why = "the round cap %d" % iters if bool((status == 2).any()) else (
            "%.0f s" % limit if time.monotonic() > deadline else None)
        if why:
            b = int((status != 1).nonzero()[0])
            info["not_finished"] = (f"{why}: cloud {b} in phase {int(rec[b, 0])} with {int(rec[b, 2])} unassigned "
                                    f"persons after {int(rec[b, 1])} rounds")
            return None, info


def run_case(spec, limit):
    """child: 'emd:kind:which:n:B:narrow_at:check_every:gap' or 'gauss:n:B' -> one JSON line"""
    import numpy as np
    import torch
    import tpgan_amd  # noqa: F401
    from tpgan_amd import ops
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda", 0)
    hip = ops.backend_for(torch.zeros(1, device=dev))
    parts = spec.split(":")
    out = {"case": spec}
    if parts[0] == "gauss":
        n, B = int(parts[1]), int(parts[2])
        a, b = clouds("fluid", n, B, dev)
        ops.gaussian_row_sums(a, b, 0.01)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(5):
            ops.gaussian_row_sums(a, b, 0.01)
        ev[1].record()
        ev[1].synchronize()
        out["ms"] = ev[0].elapsed_time(ev[1]) / 5
    else:
        _, kind, which, n, B, narrow_at, check_every, gap = parts
        n, B = int(n), int(B)
        eps, phases, scaling, cap = settings(kind, which)
        w1, w2 = clouds(kind, 256, 1, dev)
        hip.emd_match(w1, w2, eps, 1_000_000, phases, scaling)                      # warm-up: code objects
        x1, x2 = clouds(kind, n, B, dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res, info = drive(hip, x1, x2, eps, cap(n), phases, scaling, None if narrow_at == "-" else int(narrow_at),
                          None if check_every == "-" else int(check_every), limit)
        torch.cuda.synchronize()
        out.update(ms=(time.perf_counter() - t0) * 1e3, **info)
        if res is not None:
            dist, assignment, _, rounds = res
            out["rounds"] = [int(r) for r in rounds.tolist()]
            if gap == "1":
                from scipy.optimize import linear_sum_assignment
                a, b = x1[0].double().cpu().numpy(), x2[0].double().cpu().numpy()
                cost = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
                r, c = linear_sum_assignment(cost)
                best = cost[r, c].sum()
                mine = cost[np.arange(n), assignment[0].cpu().numpy()].sum()
                out.update(optimum=best, total=mine, gap=(mine - best) / best, bound=n * eps / best)
    print("RESULT " + json.dumps(out), flush=True)


def child(spec, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "--case", spec, "--limit", str(limit)]
    try:
        res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=limit + 120)
    except subprocess.TimeoutExpired:
        return None, f"killed at the process limit of {limit + 120} s"
    for line in res.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:]), None
    return None, f"exit status {res.returncode}: {(res.stderr or res.stdout)[-300:]}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=None, help="(child) one case")
    ap.add_argument("--limit", type=float, default=90.0, help="seconds a matching may take")
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096, 16384])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--no-full-frame", action="store_true")
    ap.add_argument("--no-table", action="store_true")
    ap.add_argument("--only-table", action="store_true", help="the threshold / batch sweep alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.case:
        return run_case(a.case, a.limit)
    lines, stop = [], None

    def emit(text):
        lines.append(text)
        print(text, flush=True)

    def emd_row(kind, which, n, B, narrow_at="-", check_every="-", gap=False):
        nonlocal stop
        if stop:
            return
        spec = f"emd:{kind}:{which}:{n}:{B}:{narrow_at}:{check_every}:{int(gap)}"
        r, err = child(spec, a.limit)
        head = f"{kind:>6} {which:>7} {n:6d} {B:2d} {narrow_at:>6} {check_every:>5}"
        if r is None:
            stop = f"{spec}: {err}"
            emit(f"{head}  FAILED: {err}")
        elif "not_finished" in r:
            emit(f"{head}  not finished after {r['ms'] / 1e3:.1f} s, {r['launches']} launches, at {r['not_finished']}")
        else:
            rd = r["rounds"]
            tail = f" {r['gap']:10.3e} {r['bound']:10.3e}" if "gap" in r else ""
            emit(f"{head} {min(rd):7d} {max(rd):7d} {r['launches']:8d} {r['batches']:7d} {r['ms']:10.2f}{tail}")

    emit("# ops.emd_match: wall-clock ms of one call (one synchronisation per batch of launches), rounds per cloud,")
    emit("# kernel launches, batches of the host loop; gap = (sum of squared distances - scipy's optimum) / optimum for")
    from tpgan_amd.ops import HipBackend as H
    emit("# cloud 0, bound = n * eps / optimum.  narrow / every '-': the defaults, narrow_at = max(%d, %d / n) persons,"
         % (H.EMD_NARROW_MIN, H.EMD_NARROW_WORK))
    emit("# %d wide rounds per batch, %d narrow rounds per launch." % (H.EMD_CHECK_EVERY, H.EMD_NARROW_ROUNDS))
    emit(f"{'cloud':>6} {'setting':>7} {'n':>6} {'B':>2} {'narrow':>6} {'every':>5} {'rounds<':>7} {'rounds>':>7} "
         f"{'launches':>8} {'batches':>7} {'ms':>10} {'gap':>10} {'bound':>10}")
    if not a.only_table:
        for kind in ("fluid", "action"):
            for n in a.sizes:
                for B in a.batches:
                    emd_row(kind, "default", n, B, gap=(n <= 4096 and B == 1))
        for kind in ("fluid", "action"):
            for n in a.sizes:
                emd_row(kind, "metric", n, 1, gap=n <= 4096)
        if not a.no_full_frame:
            emit("# the reference's full frame, n = 79872, B = 1 (metric setting)")
            emd_row("fluid", "metric", 79872, 1)
    if not a.no_table:
        emit("# threshold sweep (fluid; default setting, 8 wide rounds per batch; the last block: metric setting)")
        for which, n, B in (("default", 1024, 8), ("default", 4096, 1), ("default", 16384, 1), ("metric", 79872, 1)):
            for narrow_at in (0, 16, 64, 256, 1024):
                emd_row("fluid", which, n, B, str(narrow_at), "8")
        emit("# wide rounds per batch (fluid, default setting, n = 1024, B = 8, default threshold)")
        for check_every in (2, 8, 32):
            emd_row("fluid", "default", 1024, 8, "-", str(check_every))
    if a.only_table:
        a.no_full_frame, a.sizes = True, []
    emit("# ops.gaussian_row_sums, sigma 0.01: HIP-event ms per call, mean of 5")
    for n in list(a.sizes) + ([] if a.no_full_frame else [79872]):
        for B in a.batches if n < 79872 else (1,):
            if stop:
                break
            r, err = child(f"gauss:{n}:{B}", a.limit)
            if r is None:
                stop = f"gauss:{n}:{B}: {err}"
                emit(f"gauss {n:6d} {B:2d}  FAILED: {err}")
            else:
                emit(f"gauss {n:6d} {B:2d} {r['ms']:10.3f} ms  {B * n * n / (r['ms'] * 1e-3) / 1e9:8.1f} G pairs/s")
    if stop:
        emit(f"# stopped: nothing was started after {stop}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
