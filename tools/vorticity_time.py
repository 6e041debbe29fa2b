"""What vorticity confinement and a per-particle XSPH table add to a frame of the fluid simulator (`ops.pbf_substep`,
csrc/pbf.hip: finish_ex and vorticity).  GPU box.

The scheme of tools/simulate_time.py: scenes of the default size (`simulate.random_scene(seed)`, seeds 1..), default
substeps and iterations, every scene first advanced WARM plain frames.  Then, for one scene and for a batch of 24, the SAME
frame (from the same warm state) four ways -- plain, with a viscosity table, with confinement, with both -- alternating
frame by frame in one run, so that clocks and neighbours are shared and the plain frames of the same run are the yardstick:
  wall      host clock around one frame that ends in a device synchronise, median of the timed frames
  kinds     HIP events around every launch kind (`ops.OpTimer`), in a pass of its own: ms per frame
The expectation, until measured: one more neighbourhood walk beside the nine of a substep, so about a tenth more pass
time in the batch, and nothing visible in the single scene, which is bound by launches.

Each measurement runs in a child process of its own under `timeout`; this process never opens the GPU, and stops at the
first child that fails.

    python tools/vorticity_time.py [--frames 10 --warm 12 --batch 24] [--out profiles/vorticity.txt]
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

KINDS = ("pbf_predict", "pbf_grid", "pbf_lambda", "pbf_dp", "pbf_finish", "pbf_finish_ex", "pbf_vorticity")
WAYS = ("plain", "table", "vorticity", "both")
STEP_SECONDS = 420                     # limit of one child: 12 + 2 * 4 * 10 frames of up to 24 scenes, and the start-up


def worker(count, warm, frames):
    """One batch of `count` scenes measured the four ways -> a JSON line on stdout."""
    import numpy as np
    import torch

    import tpgan_amd  # noqa: F401
    from tpgan_amd import ops
    from tpgan_amd import simulate as S
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda", 0)
    scenes = [S.random_scene(s, viscosity="exponential") for s in range(1, count + 1)]
    counts = [len(s.particles()[0]) for s in scenes]
    plain, conf = ops.PbfParams(), ops.PbfParams(vorticity=ops.PBF_VORTICITY)
    x, v, lengths, lo, hi = S.pack(scenes, dev)
    tab = S.xsph_table(scenes, plain, dev)
    how = {"plain": (plain, {}), "table": (plain, {"xsph": tab}), "vorticity": (conf, {}), "both": (conf, {"xsph": tab})}
    dt = 1.0 / (S.FPS * S.SUBSTEPS)

    def frame(x, v, way):
        prm, extra = how[way]
        for _ in range(S.SUBSTEPS):
            x, v = ops.pbf_substep(x, v, lengths, lo, hi, dt, prm, **extra)
        return x, v
    for _ in range(warm):
        x, v = frame(x, v, "plain")
    torch.cuda.synchronize(dev)
    wall = {w: [] for w in WAYS}
    for _ in range(frames):
        for w in WAYS:
            t = time.perf_counter()
            frame(x, v, w)
            torch.cuda.synchronize(dev)
            wall[w].append((time.perf_counter() - t) * 1e3)
    timers = {w: ops.OpTimer() for w in WAYS}
    try:
        for _ in range(frames):
            for w in WAYS:
                ops.set_timer(timers[w])
                frame(x, v, w)
                torch.cuda.synchronize(dev)
    finally:
        ops.set_timer(None)
    kinds = {w: {k: r["total_ms"] / frames for k, r in timers[w].summary().items()} for w in WAYS}
    print(json.dumps({"device": torch.cuda.get_device_name(0), "scenes": count, "particles": int(np.sum(counts)),
                      "largest": int(max(counts)), "iters": plain.iters, "substeps": S.SUBSTEPS,
                      "wall": {w: statistics.median(wall[w]) for w in WAYS}, "kinds": kinds}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--warm", type=int, default=12)
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.warm, a.frames)
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True,
                                         stderr=subprocess.DEVNULL).strip()
    except Exception:
        commit = "working tree"
    results = []
    for count in (1, a.batch):
        cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--worker", str(count),
               "--frames", str(a.frames), "--warm", str(a.warm)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if done.returncode != 0:                             # nothing more is started on the GPU after a failure
            sys.exit(f"the measurement of {count} scene(s) ended with status {done.returncode}")
        results.append(json.loads([l for l in done.stdout.splitlines() if l.startswith("{")][-1]))
    r0 = results[0]
    lines = [f"# {r0['device']}; {commit}; substeps {r0['substeps']}, iters {r0['iters']}; {a.warm} plain frames of warm-up, "
             f"then the same frame {a.frames} times each way, alternating: wall = host clock + synchronise, median; kinds = "
             "HIP events in a pass of their own; viscosities: exponential law per body; confinement: the shipped strength"]
    for r in results:
        name = f"{r['scenes']} scene(s), {r['particles']} particles (largest {r['largest']})"
        lines.append(name)
        lines.append(f"{'ms per frame':28s}" + "".join(f"{w:>14s}" for w in WAYS))
        lines.append(f"{'wall':28s}" + "".join(f"{r['wall'][w]:14.3f}" for w in WAYS))
        lines.append(f"{'wall / plain':28s}" + "".join(f"{r['wall'][w] / r['wall']['plain']:14.3f}" for w in WAYS))
        for k in KINDS:
            lines.append(f"{k:28s}" + "".join(f"{r['kinds'][w].get(k, 0.0):14.3f}" for w in WAYS))
        total = {w: sum(r["kinds"][w].values()) for w in WAYS}
        lines.append(f"{'sum of the kinds':28s}" + "".join(f"{total[w]:14.3f}" for w in WAYS))
        lines.append(f"{'sum / plain':28s}" + "".join(f"{total[w] / total['plain']:14.3f}" for w in WAYS))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
