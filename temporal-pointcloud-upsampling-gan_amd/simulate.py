"""Training data from a particle fluid simulator on the GPU.

    python -m tpgan_amd.simulate --out DATA --cases 20 --frames 200 --seed 1 [--test_out TEST --test_cases 4]
        [--particle_radius 0.0125 --substeps 4 --iters 4 --box 3 2.5 3 --body_size 0.68 --batch 8 --device cuda]

writes `DATA/case{c}/data_{s}.npz` (`pos`, `vel`: float32 (N,3)) for c = 1.., s = 0.., the layout `data.FluidSequences`
and `python -m tpgan_amd.train --train_dataset_path DATA` read, and `DATA/case{c}/scene.json` beside them.

The reference makes these directories with an external solver (fluid_data_generation/ drives SPlisHSPlasH's DFSPH on
scenes from create_physics_scenes.py, with models it does not ship).  Here the solver is the project's own: Position
Based Fluids with Jacobi iterations, `ops.pbf_substep` (csrc/pbf.hip; the rule in full: include/tpgan_ops.h), every scene
of a batch in the same launches and all frames kept on the device until they are written.  It is NOT a DFSPH
reimplementation: the look and the statistics of the sequences are this project's own.  The scene generator keeps the
reference's recipe: one to three bodies of fluid (box, ball, upright cylinder) sampled on a lattice of one particle
spacing, each scaled, rotated, placed without overlap in a box and thrown with its own start velocity, 40 frames per
second.  No particle is created or removed: every frame holds the same particles in the same order.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

from . import ops

FPS = 40                               # exported frames per second (the step's DT = 0.025)
SUBSTEPS = 4                           # dt = 1 / 160 s: a particle at 4 m/s moves one spacing per substep
DEFAULT_BOX = (3.0, 2.5, 3.0)          # with BODY_SIZE: roughly 20k-120k particles per scene, three bodies still fit
BODY_SIZE = 0.68                       # edge of the unscaled box body in metres (a ball / cylinder of about its volume)
COUNT_RANGE = (20000, 120000)
SHAPES = ("box", "ball", "cylinder")


class Scene:
    """A box and the fluid in it at t = 0.  `bodies`: dicts of shape, size (the scaled edge), rotation (3x3, row-major),
    centre and velocity, from which `particles()` rebuilds the same points; or explicit `pos` / `vel` (n,3)."""

    def __init__(self, box_lo, box_hi, bodies=(), seed=None, radius=ops.PBF_RADIUS, pos=None, vel=None):
        self.box_lo = [float(v) for v in box_lo]
        self.box_hi = [float(v) for v in box_hi]
        self.bodies, self.seed, self.radius = list(bodies), seed, float(radius)
        self._pos = None if pos is None else np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
        self._vel = None if vel is None else np.ascontiguousarray(vel, dtype=np.float32).reshape(-1, 3)

    def particles(self):
        """-> pos, vel (n,3) float32."""
        if self._pos is None:
            pos = [body_points(b, 2.0 * self.radius) for b in self.bodies]
            vel = [np.broadcast_to(np.asarray(b["velocity"], np.float64), p.shape) for b, p in zip(self.bodies, pos)]
            self._pos = np.concatenate(pos).astype(np.float32) if pos else np.zeros((0, 3), np.float32)
            self._vel = np.concatenate(vel).astype(np.float32) if vel else np.zeros((0, 3), np.float32)
        if self._vel is None:
            self._vel = np.zeros_like(self._pos)
        return self._pos, self._vel

    def to_json(self):
        return {"seed": self.seed, "box_lo": self.box_lo, "box_hi": self.box_hi, "particle_radius": self.radius,
                "bodies": self.bodies}

    @classmethod
    def from_json(cls, d):
        return cls(d["box_lo"], d["box_hi"], d["bodies"], d["seed"], d["particle_radius"])


def body_half_extent(shape, size):
    """Half extents of the body's own frame (x, y, z); ball and cylinder have about the box's volume."""
    if shape == "box":
        return np.array([size / 2, size / 2, size / 2])
    if shape == "ball":
        return np.full(3, 0.62 * size)
    return np.array([0.5 * size, 0.64 * size, 0.5 * size])     # cylinder: radius, half height, radius


def body_points(body, spacing):
    """The lattice points of spacing `spacing` inside the body, rotated and moved to its centre -> (n,3) float64."""
    half = body_half_extent(body["shape"], body["size"])
    axes = [np.arange(-np.floor(e / spacing), np.floor(e / spacing) + 1) * spacing for e in half]
    g = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    if body["shape"] == "ball":
        g = g[(g ** 2).sum(1) <= half[0] ** 2]
    elif body["shape"] == "cylinder":
        g = g[g[:, 0] ** 2 + g[:, 2] ** 2 <= half[0] ** 2]
    return g @ np.asarray(body["rotation"], np.float64).reshape(3, 3).T + np.asarray(body["centre"], np.float64)


def _random_rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def random_scene(seed, box=DEFAULT_BOX, radius=ops.PBF_RADIUS, body_size=BODY_SIZE, count_range=None, max_tries=1000):
    """The scene of `seed` (an int or a sequence of ints), everything drawn from numpy.random.default_rng(seed): one to
    three bodies, each a box, ball or upright cylinder of `body_size` scaled by U(0.5, 1.5) and rotated at random, placed
    by rejection so that the bodies' bounding spheres stay a particle spacing apart and inside the box, thrown with a
    start velocity of U(-2, 2) in x and z and U(-0.5, 0.5) in y.  The box is [0, box].  count_range (lo, hi): redraw
    (from the same generator) until the particle count lies in it; None: COUNT_RANGE for the default box and body size,
    no condition otherwise."""
    rng = np.random.default_rng(seed)
    box = np.asarray(box, np.float64).reshape(3)
    if count_range is None and tuple(box) == DEFAULT_BOX and body_size == BODY_SIZE and radius == ops.PBF_RADIUS:
        count_range = COUNT_RANGE
    spacing = 2.0 * radius
    for _ in range(max_tries):
        bodies, spheres = [], []
        for _ in range(int(rng.integers(1, 4))):
            shape = SHAPES[int(rng.integers(0, 3))]
            size = float(body_size * rng.uniform(0.5, 1.5))
            rot = _random_rotation(rng)
            bound = float(np.linalg.norm(body_half_extent(shape, size))) + spacing
            velocity = [float(rng.uniform(-2, 2)), float(rng.uniform(-0.5, 0.5)), float(rng.uniform(-2, 2))]
            for _ in range(100):
                if (2 * bound >= box).any():
                    break
                centre = rng.uniform(bound, box - bound)
                if all(np.linalg.norm(centre - c) >= bound + b for c, b in spheres):
                    spheres.append((centre, bound))
                    bodies.append({"shape": shape, "size": size, "rotation": rot.reshape(-1).tolist(),
                                   "centre": centre.tolist(), "velocity": velocity})
                    break
        seed_out = seed if isinstance(seed, (int, np.integer)) else [int(s) for s in seed]
        scene = Scene([0.0, 0.0, 0.0], box.tolist(), bodies, seed_out, radius)
        n = scene.particles()[0].shape[0]
        if bodies and (count_range is None or count_range[0] <= n <= count_range[1]):
            return scene
    raise RuntimeError(f"no scene of {count_range} particles in {max_tries} draws: box {box.tolist()}, body_size {body_size}")


def pack(scenes, device):
    """-> x, v (B,N,3) fp32 on `device` (rows beyond a scene's count are 0), lengths (B,) int64, box_lo, box_hi (B,3)."""
    parts = [s.particles() for s in scenes]
    B, N = len(scenes), max([p.shape[0] for p, _ in parts] + [0])
    x, v = np.zeros((B, N, 3), np.float32), np.zeros((B, N, 3), np.float32)
    for b, (p, u) in enumerate(parts):
        x[b, :p.shape[0]], v[b, :p.shape[0]] = p, u
    lengths = torch.tensor([p.shape[0] for p, _ in parts], dtype=torch.int64)
    lo = np.array([s.box_lo for s in scenes], np.float32).reshape(B, 3)
    hi = np.array([s.box_hi for s in scenes], np.float32).reshape(B, 3)
    return torch.from_numpy(x).to(device), torch.from_numpy(v).to(device), lengths.to(device), lo, hi


def simulate(scenes, frames, substeps=SUBSTEPS, iters=ops.PBF_ITERS, params=None, device="cuda"):
    """`frames` exported frames of every scene, frame 0 being the start state and each further one 1/40 s later, made of
    `substeps` substeps of dt = 1 / (40 * substeps).  All scenes advance in the same launches; the frames stay on the
    device.  params: an `ops.PbfParams` (its `iters` wins); None: the defaults with `iters`, at the first scene's radius.
    -> pos, vel (B, frames, N, 3) fp32, lengths (B,) int64 (rows beyond a scene's length are 0)."""
    if frames < 1 or substeps < 1:
        raise ValueError("frames and substeps must be >= 1")
    prm = params if params is not None else ops.PbfParams(radius=scenes[0].radius if scenes else ops.PBF_RADIUS, iters=iters)
    x, v, lengths, lo, hi = pack(scenes, torch.device(device))
    B, N, _ = x.shape
    pos, vel = x.new_zeros((B, frames, N, 3)), x.new_zeros((B, frames, N, 3))
    dt = 1.0 / (FPS * substeps)
    for f in range(frames):
        if f:
            for _ in range(substeps):
                x, v = ops.pbf_substep(x, v, lengths, lo, hi, dt, prm)
        pos[:, f], vel[:, f] = x, v
    return pos, vel, lengths


def write_cases(out, scenes, first_case, frames, substeps, prm, device, settings):
    """Simulate `scenes` as one batch and write case{first_case + b}; one JSON line per case on stdout."""
    t0 = time.time()
    pos, vel, lengths = simulate(scenes, frames, substeps, params=prm, device=device)
    pos, vel = pos.cpu().numpy(), vel.cpu().numpy()              # the copy waits for the launches
    seconds = time.time() - t0
    for b, scene in enumerate(scenes):
        case = os.path.join(out, f"case{first_case + b}")
        os.makedirs(case, exist_ok=True)
        n = int(lengths[b])
        for s in range(frames):
            np.savez(os.path.join(case, f"data_{s}.npz"), pos=pos[b, s, :n], vel=vel[b, s, :n])
        with open(os.path.join(case, "scene.json"), "w") as f:
            json.dump(dict(scene.to_json(), frames=frames, substeps=substeps, fps=FPS, params=prm.as_dict(), **settings), f)
        print(json.dumps({"case": first_case + b, "dir": case, "particles": n, "frames": frames,
                          "seconds": round(seconds / len(scenes), 3), "batch": len(scenes)}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m tpgan_amd.simulate",
                                 description="Simulate fluid scenes on the GPU and write training sequences.")
    ap.add_argument("--out", required=True, help="directory of the training cases (case1 ..)")
    ap.add_argument("--cases", type=int, default=20)
    ap.add_argument("--frames", type=int, default=200, help="frames per case at 40 per second (frame 0: the start state)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--test_out", type=str, default=None, help="directory of held-out cases (seeds disjoint from --out's)")
    ap.add_argument("--test_cases", type=int, default=4)
    ap.add_argument("--particle_radius", type=float, default=ops.PBF_RADIUS)
    ap.add_argument("--substeps", type=int, default=SUBSTEPS)
    ap.add_argument("--iters", type=int, default=ops.PBF_ITERS)
    ap.add_argument("--box", type=float, nargs=3, default=list(DEFAULT_BOX), help="the box is [0, box]")
    ap.add_argument("--body_size", type=float, default=BODY_SIZE, help="edge of the unscaled box body")
    ap.add_argument("--batch", type=int, default=8, help="scenes simulated together")
    ap.add_argument("--device", type=str, default="cuda")
    a = ap.parse_args(argv)
    if a.cases < 0 or a.test_cases < 0 or a.frames < 1 or a.batch < 1 or a.substeps < 1 or a.iters < 0:
        ap.error("--cases, --test_cases, --iters >= 0; --frames, --batch, --substeps >= 1")
    prm = ops.PbfParams(radius=a.particle_radius, iters=a.iters)
    settings = {"box": list(a.box), "body_size": a.body_size}
    # split 0: training, 1: held out -- the seed sequences (seed, split, case) can never coincide
    for split, (out, cases) in enumerate(((a.out, a.cases), (a.test_out, a.test_cases if a.test_out else 0))):
        for c0 in range(0, cases, a.batch):
            scenes = [random_scene([a.seed, split, c], tuple(a.box), a.particle_radius, a.body_size)
                      for c in range(c0, min(c0 + a.batch, cases))]
            write_cases(out, scenes, c0 + 1, a.frames, a.substeps, prm, a.device, settings)
    return 0


if __name__ == "__main__":
    sys.exit(main())
