"""What solid obstacles cost the fluid simulator (`ops.pbf_substep(obstacles=...)`, pbf_collide_kernel of csrc/pbf.hip).
GPU box.

The protocol of tools/simulate_time.py: scenes of the default size (`simulate.random_scene(seed)`, seeds 1..), default
substeps and iterations, WARM frames first, then the wall clock around one frame that ends in a device synchronise (median
of the timed frames) and, in a pass of their own, HIP events around every launch kind (`ops.OpTimer`).  Measured for one
scene and for a batch of 24, in the same run, in three columns each:
  0 obst        the scenes of tools/simulate_time.py: the untouched path, to be compared with profiles/simulate.txt
  3 obst, off   the scenes of the same seeds drawn with 3 obstacles (fluid bodies that no longer fit are gone, so these
                scenes hold fewer particles), simulated WITHOUT their table: the baseline of the next column
  3 obst        the same scenes with their table: (1 + iters) collide launches per substep more

Every measurement runs in a child process of its own under a time limit, one after the other; the first that fails or
runs out of time ends the run.

    python tools/obstacle_time.py [--frames 10 --warm 12 --batch 24] [--out profiles/obstacles.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("pbf_predict", "pbf_collide", "pbf_grid", "pbf_lambda", "pbf_dp", "pbf_finish")
OBSTACLES = 3
STEP_SECONDS = 240


def measure(scenes, warm, frames, obstacles, apply):
    """-> dict(wall ms per frame (median), kinds {kind: event ms per frame}, particle counts, obstacles per scene)."""
    import torch

    import tpgan_amd  # noqa: F401
    from tpgan_amd import ops
    from tpgan_amd import simulate as S
    dev = torch.device("cuda", 0)
    prm = ops.PbfParams()
    group = [S.random_scene(s, obstacles=obstacles) for s in range(1, scenes + 1)]
    x, v, lengths, lo, hi = S.pack(group, dev)
    table = S.obstacle_table(group, dev) if apply else None

    def frame(x, v):
        for _ in range(S.SUBSTEPS):
            x, v = ops.pbf_substep(x, v, lengths, lo, hi, 1.0 / (S.FPS * S.SUBSTEPS), prm, table)
        return x, v
    for _ in range(warm):
        x, v = frame(x, v)
    torch.cuda.synchronize(dev)
    wall = []
    for _ in range(frames):
        t = time.perf_counter()
        x, v = frame(x, v)
        torch.cuda.synchronize(dev)
        wall.append((time.perf_counter() - t) * 1e3)
    timer = ops.OpTimer()
    ops.set_timer(timer)
    try:
        for _ in range(frames):
            x, v = frame(x, v)
        torch.cuda.synchronize(dev)
    finally:
        ops.set_timer(None)
    assert bool(torch.isfinite(x).all())
    summary = timer.summary()
    return dict(wall=statistics.median(wall), spread=[min(wall), max(wall)],
                kinds={k: r["total_ms"] / frames for k, r in summary.items()},
                launches={k: r["launches"] / frames for k, r in summary.items()},
                counts=[len(s.particles()[0]) for s in group], obstacles=[len(s.obstacles) for s in group],
                device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--warm", type=int, default=12)
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", type=int, nargs=3, default=None, help=argparse.SUPPRESS)      # the child: scenes, obstacles, table on
    a = ap.parse_args()
    if a.one:
        print("RESULT " + json.dumps(measure(a.one[0], a.warm, a.frames, a.one[1], bool(a.one[2]))), flush=True)
        return 0
    columns = {}
    for scenes in (1, a.batch):
        for obstacles, apply in ((0, 0), (OBSTACLES, 0), (OBSTACLES, 1)):
            cmd = [sys.executable, os.path.abspath(__file__), "--frames", str(a.frames), "--warm", str(a.warm),
                   "--one", str(scenes), str(obstacles), str(apply)]
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_SECONDS)     # raises when it runs out
            if done.returncode != 0:
                sys.stderr.write(done.stdout + done.stderr)
                return done.returncode or 1
            line = [l for l in done.stdout.splitlines() if l.startswith("RESULT ")][-1]
            columns[f"{scenes} sc, {obstacles} obst" + (", off" if obstacles and not apply else "")] = json.loads(line[len("RESULT "):])
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True,
                                         stderr=subprocess.DEVNULL).strip()
    except Exception:
        commit = "working tree"
    names = list(columns)
    first = columns[names[0]]
    lines = [f"# {first['device']}; {commit} plus solid obstacles; substeps 4, iters 4; {a.warm} frames of warm-up, then "
             f"{a.frames} timed frames: wall = host clock + synchronise, median (min .. max below); kinds = HIP events in a "
             "pass of their own; every column in a process of its own",
             f"scenes: seeds 1..{a.batch}; particles " + ", ".join(f"{n}: {sum(columns[n]['counts'])}" for n in names)]
    lines.append(f"{'ms per frame':28s}" + "".join(f"{n:>18s}" for n in names))
    lines.append(f"{'wall':28s}" + "".join(f"{columns[n]['wall']:18.3f}" for n in names))
    lines.append(f"{'wall, min .. max':28s}" + "".join(f"{'%.3f .. %.3f' % tuple(columns[n]['spread']):>18s}" for n in names))
    for k in KINDS:
        lines.append(f"{k:28s}" + "".join(f"{columns[n]['kinds'].get(k, 0.0):18.3f}" for n in names))
    lines.append(f"{'sum of the kinds':28s}" + "".join(f"{sum(columns[n]['kinds'].values()):18.3f}" for n in names))
    lines.append(f"{'collide launches per frame':28s}" + "".join(f"{columns[n]['launches'].get('pbf_collide', 0.0):18.1f}" for n in names))
    for scenes in (1, a.batch):
        base, with_ = columns[f"{scenes} sc, {OBSTACLES} obst, off"], columns[f"{scenes} sc, {OBSTACLES} obst"]
        lines.append(f"{scenes} scene(s) of {sum(with_['counts'])} particles: wall with the table / without = "
                     f"{with_['wall'] / base['wall']:.3f} ({with_['wall'] - base['wall']:+.3f} ms per frame)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
