"""What the signed distance to a triangle mesh costs (`ops.mesh_sdf`, csrc/mesh_sdf.hip), and what mesh obstacles cost the
fluid simulator (`ops.pbf_substep(sdf_obstacles=...)`, pbf_collide_sdf_kernel of csrc/pbf.hip).  GPU box.

Part 1: `ops.mesh_sdf` for the 127^3 nodes of a lattice around the mesh against 2 304 (torus:0.5,0.2,48,24), 20 480
(icosphere:5) and 81 920 (icosphere:6) faces: one warm call, then the wall clock around three calls that each end in a
device synchronise (median; the call includes the op's host read of the mesh), and the kernel alone by HIP events
(`ops.OpTimer`) in a pass of its own.  Brute force: pairs = queries x faces.

Part 2: the protocol of tools/obstacle_time.py: scenes of the default size (`simulate.random_scene(seed)`, seeds 1..),
default substeps and iterations, WARM frames first, then the wall clock around one frame that ends in a device synchronise
(median of the timed frames) and, in a pass of their own, HIP events around every launch kind.  One scene and a batch of
24, in three columns each:
  0 obst         the scenes of tools/simulate_time.py: the untouched path
  2 mesh, off    the scenes of the same seeds drawn with 2 obstacles, each replaced by a mesh (an icosphere:3 or the
                 torus of part 1, alternating) of 0.8 times its largest extent at the same pose, simulated WITHOUT
                 their table: the baseline of the next column
  2 mesh         the same scenes with their table and fields: (1 + iters) collide_sdf launches per substep more; the
                 time to sample the fields (once per batch) is reported beside it

Every measurement runs in a child process of its own under a time limit, one after the other; the first that fails or
runs out of time ends the run.

    python tools/mesh_sdf_time.py [--frames 10 --warm 12 --batch 24] [--out profiles/mesh_sdf.txt]
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

KINDS = ("pbf_predict", "pbf_collide", "pbf_collide_sdf", "pbf_grid", "pbf_lambda", "pbf_dp", "pbf_finish")
MESHES = ("torus:0.5,0.2,48,24", "icosphere:5", "icosphere:6")
OBSTACLE_MESHES = ("icosphere:3", "torus:0.5,0.2,48,24")
LATTICE = 127
OBSTACLES = 2
STEP_SECONDS = 240


def measure_sdf(spec, calls=3):
    """-> dict(faces, queries, wall ms per call (median), kernel ms per call by events, inside fraction)."""
    import numpy as np
    import torch

    import tpgan_amd  # noqa: F401
    from tpgan_amd import mesh, ops
    dev = torch.device("cuda", 0)
    v, f = mesh.load_spec(spec)
    lo, hi = v.min(0) - 0.1, v.max(0) + 0.1
    axes = [torch.linspace(float(lo[a]), float(hi[a]), LATTICE, device=dev) for a in range(3)]
    q = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3).contiguous()
    V, F = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    d, _ = ops.mesh_sdf(q, V, F)
    torch.cuda.synchronize(dev)
    wall = []
    for _ in range(calls):
        t = time.perf_counter()
        d, _ = ops.mesh_sdf(q, V, F)
        torch.cuda.synchronize(dev)
        wall.append((time.perf_counter() - t) * 1e3)
    timer = ops.OpTimer()
    ops.set_timer(timer)
    try:
        for _ in range(calls):
            ops.mesh_sdf(q, V, F)
        torch.cuda.synchronize(dev)
    finally:
        ops.set_timer(None)
    assert bool(torch.isfinite(d).all())
    return dict(spec=spec, faces=int(f.shape[0]), queries=int(q.shape[0]), wall=statistics.median(wall),
                spread=[min(wall), max(wall)], kernel=timer.summary()["mesh_sdf"]["total_ms"] / calls,
                inside=float((d < 0).float().mean()), device=torch.cuda.get_device_name(0),
                closed=mesh.check_closed(v, f), unit=1.0 / ops.mesh_sdf_grid(np.asarray(v))[1])


def as_mesh(ob, k):
    import numpy as np
    largest = 2.0 * float(np.max(np.atleast_1d(ob["size"])))
    return {"shape": "mesh", "mesh": OBSTACLE_MESHES[k % len(OBSTACLE_MESHES)], "size": 0.8 * largest, "centre": ob["centre"],
            "rotation": ob["rotation"]}


def measure_frames(scenes, warm, frames, obstacles, apply):
    """-> dict(wall ms per frame (median), kinds {kind: event ms per frame}, particle counts, field sampling ms)."""
    import torch

    import tpgan_amd  # noqa: F401
    from tpgan_amd import ops
    from tpgan_amd import simulate as S
    dev = torch.device("cuda", 0)
    prm = ops.PbfParams()
    group = [S.random_scene(s, obstacles=obstacles) for s in range(1, scenes + 1)]
    for s in group:
        s.obstacles = [as_mesh(o, k) for k, o in enumerate(s.obstacles)]
    x, v, lengths, lo, hi = S.pack(group, dev)
    sdf, sampling, nodes = None, 0.0, 0
    if apply:
        S.sdf_obstacle_table(group[:1], dev)                                     # code objects, the meshes' host cache
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        sdf = S.sdf_obstacle_table(group, dev)
        torch.cuda.synchronize(dev)
        sampling, nodes = (time.perf_counter() - t) * 1e3, int(sdf[1].numel())
    extra = {} if sdf is None else {"sdf_obstacles": sdf}

    def frame(x, v):
        for _ in range(S.SUBSTEPS):
            x, v = ops.pbf_substep(x, v, lengths, lo, hi, 1.0 / (S.FPS * S.SUBSTEPS), prm, **extra)
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
                sampling=sampling, nodes=nodes, device=torch.cuda.get_device_name(0))


def child(args, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--frames", str(a.frames), "--warm", str(a.warm)] + args
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_SECONDS)              # raises when it runs out
    if done.returncode != 0:
        sys.stderr.write(done.stdout + done.stderr)
        return None
    line = [l for l in done.stdout.splitlines() if l.startswith("RESULT ")][-1]
    print("done: " + " ".join(args), file=sys.stderr, flush=True)
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--warm", type=int, default=12)
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sdf", type=str, default=None, help=argparse.SUPPRESS)              # the child of part 1: a SPEC
    ap.add_argument("--one", type=int, nargs=3, default=None, help=argparse.SUPPRESS)      # part 2: scenes, obstacles, table on
    a = ap.parse_args()
    if a.sdf:
        print("RESULT " + json.dumps(measure_sdf(a.sdf)), flush=True)
        return 0
    if a.one:
        print("RESULT " + json.dumps(measure_frames(a.one[0], a.warm, a.frames, a.one[1], bool(a.one[2]))), flush=True)
        return 0
    rows, columns = [], {}
    for spec in MESHES:
        r = child(["--sdf", spec], a)
        if r is None:
            return 1
        rows.append(r)
    for scenes in (1, a.batch):
        for obstacles, apply in ((0, 0), (OBSTACLES, 0), (OBSTACLES, 1)):
            r = child(["--one", str(scenes), str(obstacles), str(apply)], a)
            if r is None:
                return 1
            columns[f"{scenes} sc, {obstacles} mesh" + (", off" if obstacles and not apply else "")] = r
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True,
                                         stderr=subprocess.DEVNULL).strip()
    except Exception:
        commit = "working tree"
    lines = [f"# {rows[0]['device']}; {commit} plus mesh_sdf and mesh obstacles; every measurement in a process of its own",
             f"# part 1: ops.mesh_sdf, {LATTICE}^3 = {rows[0]['queries']} queries; one warm call, then 3 timed calls: wall = host "
             "clock + synchronise, median (min .. max); kernel = HIP events in a pass of their own",
             f"{'mesh':24s}{'faces':>8s}{'wall ms':>12s}{'min .. max':>22s}{'kernel ms':>12s}{'G pairs/s':>11s}{'inside':>8s}"]
    for r in rows:
        lines.append(f"{r['spec']:24s}{r['faces']:8d}{r['wall']:12.3f}{'%.3f .. %.3f' % tuple(r['spread']):>22s}{r['kernel']:12.3f}"
                     f"{r['queries'] * r['faces'] / r['kernel'] / 1e6:11.1f}{r['inside']:8.3f}")
    names = list(columns)
    lines += [f"# part 2: substeps 4, iters 4; {a.warm} frames of warm-up, then {a.frames} timed frames: wall = host clock + "
              "synchronise, median (min .. max below); kinds = HIP events in a pass of their own",
              f"scenes: seeds 1..{a.batch}; particles " + ", ".join(f"{n}: {sum(columns[n]['counts'])}" for n in names)]
    lines.append(f"{'ms per frame':28s}" + "".join(f"{n:>18s}" for n in names))
    lines.append(f"{'wall':28s}" + "".join(f"{columns[n]['wall']:18.3f}" for n in names))
    lines.append(f"{'wall, min .. max':28s}" + "".join(f"{'%.3f .. %.3f' % tuple(columns[n]['spread']):>18s}" for n in names))
    for k in KINDS:
        lines.append(f"{k:28s}" + "".join(f"{columns[n]['kinds'].get(k, 0.0):18.3f}" for n in names))
    lines.append(f"{'sum of the kinds':28s}" + "".join(f"{sum(columns[n]['kinds'].values()):18.3f}" for n in names))
    lines.append(f"{'collide_sdf launches/frame':28s}" +
                 "".join(f"{columns[n]['launches'].get('pbf_collide_sdf', 0.0):18.1f}" for n in names))
    lines.append(f"{'sampling the fields, ms':28s}" + "".join(f"{columns[n]['sampling']:18.3f}" for n in names))
    lines.append(f"{'field nodes':28s}" + "".join(f"{columns[n]['nodes']:18d}" for n in names))
    for scenes in (1, a.batch):
        base, with_ = columns[f"{scenes} sc, {OBSTACLES} mesh, off"], columns[f"{scenes} sc, {OBSTACLES} mesh"]
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
