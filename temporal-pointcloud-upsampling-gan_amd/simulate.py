"""Training data from a particle fluid simulator on the GPU.

    python -m tpgan_amd.simulate --out DATA --cases 20 --frames 200 --seed 1 [--test_out TEST --test_cases 4]
        [--particle_radius 0.0125 --substeps 4 --iters 4 --box 3 2.5 3 --body_size 0.68 --batch 8 --device cuda]
        [--obstacles 2 --obstacle_size 0.3 0.6]
        [--fluid_mesh SPEC ... --obstacle_mesh SPEC ...]          SPEC: a .obj / .ply path, icosphere:3, torus:0.5,0.2,48,24
        [--viscosity exponential|uniform|log10_uniform --vorticity [EPS]]

writes `DATA/case{c}/data_{s}.npz` (`pos`, `vel`: float32 (N,3)) for c = 1.., s = 0.., the layout `data.FluidSequences`
and `python -m tpgan_amd.train --train_dataset_path DATA` read, and `DATA/case{c}/scene.json` beside them.
--obstacles K puts K static solids (ball, box, cylinder; `ops.pbf_collide`, the rule: include/tpgan_ops.h, "solid
obstacles") into the lower half of every scene; `scene.json` records them and `DATA/case{c}/obstacles.ply` is their
surface (`obstacle_mesh`), to be loaded beside the fluid's meshes.  --fluid_mesh / --obstacle_mesh add closed triangle
meshes to the shapes the bodies / the obstacles are drawn from: a mesh body is filled with the lattice nodes at least a
particle radius inside it (`ops.mesh_sdf`), a mesh obstacle is its distance field sampled once per batch
(`ops.pbf_sdf_obstacles`, the rule: include/tpgan_ops.h, "mesh obstacles").  --viscosity LAW draws a viscosity per fluid
body as the reference's recipe does and turns it into an XSPH coefficient per particle (`ops.pbf_xsph`; a knob of this
solver, not a physical viscosity); --vorticity adds vorticity confinement (the rule: include/tpgan_ops.h, "vorticity
confinement and per-particle viscosity").  `scene.json` records the viscosities per body and the strength in `params`.

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
OBSTACLE_SIZE = (0.3, 0.6)             # range of an obstacle's largest extent (edge, diameter, height) in metres
MAX_RANDOM_OBSTACLES = 3
MIN_OBSTACLE_SPACINGS = 4.0            # no obstacle thinner than this many particle spacings (tunnelling: tpgan_ops.h)
MESH = "mesh"                          # the shape of a body or obstacle given by a triangle mesh (its "mesh": a SPEC)
_MESHES = {}                           # SPEC -> (vertices centred on their box, faces, extents): read and checked once


def mesh_geometry(spec, size):
    """The closed mesh of `spec` (`mesh.load_spec`) in its own frame: its bounding box centred on the origin and scaled so
    that the box's largest extent is `size` -> (vertices (V,3) float32, faces (F,3) int32, half extents (3,) float64).
    Raises on a mesh with boundary or non-manifold edges: the distance's sign needs a closed one."""
    from . import mesh
    if spec not in _MESHES:
        v, f = mesh.load_spec(spec)
        ops._need(v.shape[0] > 0 and f.shape[0] > 0, f"mesh {spec!r} is empty")
        report = mesh.check_closed(v, f)
        ops._need(report["boundary_edges"] == 0 and report["nonmanifold_edges"] == 0,
                  f"mesh {spec!r} is not closed: {report}")
        lo, hi = v.astype(np.float64).min(0), v.astype(np.float64).max(0)
        ops._need(float((hi - lo).max()) > 0.0, f"mesh {spec!r} has no extent")
        _MESHES[spec] = (v.astype(np.float64) - 0.5 * (lo + hi), f, hi - lo)
    v, f, extent = _MESHES[spec]
    scale = float(size) / float(extent.max())
    return (v * scale).astype(np.float32), f, 0.5 * extent * scale


def _scene_device(device=None):
    return torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))


def mesh_distance(spec, size, points, device=None):
    """`ops.mesh_sdf` of local points (n,3) against the mesh of `mesh_geometry(spec, size)` -> (n,) float32 tensor on
    `device` (default: the GPU when there is one; CPU tensors need a registered checker, as everywhere)."""
    dev = _scene_device(device)
    v, f, _ = mesh_geometry(spec, size)
    q = torch.as_tensor(points, dtype=torch.float32).to(dev).contiguous()
    return ops.mesh_sdf(q, torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev))[0]


class Scene:
    """A box and the fluid in it at t = 0.  `bodies`: dicts of shape, size (the scaled edge), rotation (3x3, row-major),
    centre and velocity, from which `particles()` rebuilds the same points, and optionally "viscosity" (`viscosity()`); or
    explicit `pos` / `vel` (n,3).
    `obstacles`: the static solids in the box, dicts as `ops.pbf_obstacles` takes them (shape, centre, rotation, size).
    A body or obstacle of shape "mesh" names its triangle mesh in "mesh" (a SPEC); its size is the largest extent."""

    def __init__(self, box_lo, box_hi, bodies=(), seed=None, radius=ops.PBF_RADIUS, pos=None, vel=None, obstacles=()):
        self.box_lo = [float(v) for v in box_lo]
        self.box_hi = [float(v) for v in box_hi]
        self.bodies, self.seed, self.radius = list(bodies), seed, float(radius)
        self.obstacles = list(obstacles)
        self._counts = None                                  # particles per body, once `particles()` has built them
        self._pos = None if pos is None else np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
        self._vel = None if vel is None else np.ascontiguousarray(vel, dtype=np.float32).reshape(-1, 3)

    def particles(self):
        """-> pos, vel (n,3) float32."""
        if self._pos is None:
            pos = [body_points(b, 2.0 * self.radius) for b in self.bodies]
            self._counts = [p.shape[0] for p in pos]
            vel = [np.broadcast_to(np.asarray(b["velocity"], np.float64), p.shape) for b, p in zip(self.bodies, pos)]
            self._pos = np.concatenate(pos).astype(np.float32) if pos else np.zeros((0, 3), np.float32)
            self._vel = np.concatenate(vel).astype(np.float32) if vel else np.zeros((0, 3), np.float32)
        if self._vel is None:
            self._vel = np.zeros_like(self._pos)
        return self._pos, self._vel

    def viscosity(self):
        """-> the viscosity of every particle (n,) float64, from the bodies' "viscosity" (`ops.PBF_VISCOSITY` for a body
        without one); None when no body has the key, or the scene was given as explicit particles."""
        if not any("viscosity" in b for b in self.bodies):
            return None
        self.particles()
        if self._counts is None:
            return None
        return np.concatenate([np.full(n, float(b.get("viscosity", ops.PBF_VISCOSITY)))
                               for b, n in zip(self.bodies, self._counts)])

    def to_json(self):
        d = {"seed": self.seed, "box_lo": self.box_lo, "box_hi": self.box_hi, "particle_radius": self.radius,
             "bodies": self.bodies}
        if self.obstacles:                                   # a scene without obstacles is written as it always was
            d["obstacles"] = self.obstacles
        return d

    @classmethod
    def from_json(cls, d):
        return cls(d["box_lo"], d["box_hi"], d["bodies"], d["seed"], d["particle_radius"], obstacles=d.get("obstacles", ()))


def body_half_extent(shape, size, spec=None):
    """Half extents of the body's own frame (x, y, z); ball and cylinder have about the box's volume; a mesh (spec: its
    SPEC) has its bounding box's."""
    if shape == MESH:
        return mesh_geometry(spec, size)[2]
    if shape == "box":
        return np.array([size / 2, size / 2, size / 2])
    if shape == "ball":
        return np.full(3, 0.62 * size)
    return np.array([0.5 * size, 0.64 * size, 0.5 * size])     # cylinder: radius, half height, radius


def body_points(body, spacing, device=None):
    """The lattice points of spacing `spacing` inside the body, rotated and moved to its centre -> (n,3) float64.  Of a
    mesh body: the nodes in the mesh's box whose signed distance (`ops.mesh_sdf`, on `device`) is <= -spacing / 2, so that
    every particle's sphere lies inside the mesh."""
    half = body_half_extent(body["shape"], body["size"], body.get("mesh"))
    axes = [np.arange(-np.floor(e / spacing), np.floor(e / spacing) + 1) * spacing for e in half]
    g = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    if body["shape"] == MESH:
        d = mesh_distance(body["mesh"], body["size"], g, device).cpu().numpy()
        g = g[d <= -np.float32(0.5 * spacing)]
    elif body["shape"] == "ball":
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


def obstacle_bound(ob):
    """The radius of an obstacle's bounding sphere about its centre (a mesh: of its bounding box)."""
    if ob["shape"] == MESH:
        return float(np.linalg.norm(mesh_geometry(ob["mesh"], ob["size"])[2]))
    size = np.atleast_1d(np.asarray(ob["size"], np.float64))
    return float(size[0]) if ob["shape"] == "ball" else float(np.linalg.norm(size))


def random_obstacles(rng, count, box, spacing, size_range=OBSTACLE_SIZE, max_tries=1000, meshes=(), mesh_rng=None):
    """`count` obstacle dicts drawn from `rng`: a ball, box or cylinder whose largest extent is U(size_range) metres (a
    ball's diameter; a box's longest edge, the others U(0.6, 1) of it; a cylinder's height, its diameter U(0.6, 1) of it),
    rotated at random, the centre in the lower half of the box [0, box] and at least a bounding radius from the walls, no
    two bounding spheres overlapping.  An obstacle thinner than MIN_OBSTACLE_SPACINGS particle spacings is never drawn.
    meshes: SPECs that join the three shapes; whether a draw becomes one of them is decided by `mesh_rng`, a generator of
    its own, AFTER the draw's values have been taken from `rng`: without meshes `rng` gives what it always gave."""
    out, spheres = [], []
    for _ in range(max_tries):
        if len(out) == count:
            return out
        shape = SHAPES[int(rng.integers(0, 3))]
        half = 0.5 * float(rng.uniform(*size_range))
        thin = [float(t) for t in rng.uniform(0.6, 1.0, 2)]
        rot = _random_rotation(rng)
        size = {"ball": half, "box": [half, half * thin[0], half * thin[1]], "cylinder": [half * thin[0], half]}[shape]
        ob = {"shape": shape, "size": size, "rotation": rot.reshape(-1).tolist()}
        thinnest = 2.0 * float(np.min(size))
        if meshes:
            k = int(mesh_rng.integers(0, len(SHAPES) + len(meshes)))
            if k >= len(SHAPES):
                ob = {"shape": MESH, "mesh": meshes[k - len(SHAPES)], "size": 2.0 * half, "rotation": rot.reshape(-1).tolist()}
                thinnest = 2.0 * float(mesh_geometry(ob["mesh"], ob["size"])[2].min())
        bound = obstacle_bound(ob)
        top = np.array([box[0] - bound, 0.5 * box[1], box[2] - bound])
        if thinnest < MIN_OBSTACLE_SPACINGS * spacing or (top < bound).any():
            continue
        centre = rng.uniform(bound, top)
        if all(np.linalg.norm(centre - c) >= bound + b for c, b in spheres):
            spheres.append((centre, bound))
            out.append(dict(ob, centre=centre.tolist()))
    if len(out) == count:
        return out
    raise RuntimeError(f"no room for {count} obstacles of {size_range} m in the lower half of the box {box.tolist()}")


VISCOSITY_LAWS = ("exponential", "uniform", "log10_uniform")


def draw_viscosity(rng, law):
    """One body's viscosity by the reference recipe's laws: exponential with scale 1/20 plus 0.01 (its default), U(0.01,
    0.3), or 0.01 * 10^U(0, 1.5).  A knob of this project's solver (`ops.pbf_xsph`), not SPlisHSPlasH's viscosity."""
    if law == "exponential":
        return float(rng.exponential(scale=1.0 / 20.0) + 0.01)
    if law == "uniform":
        return float(rng.uniform(0.01, 0.3))
    if law == "log10_uniform":
        return float(0.01 * 10.0 ** rng.uniform(0.0, 1.5))
    raise ValueError(f"viscosity must be None or one of {VISCOSITY_LAWS}")


def random_scene(seed, box=DEFAULT_BOX, radius=ops.PBF_RADIUS, body_size=BODY_SIZE, count_range=None, max_tries=1000,
                 obstacles=0, obstacle_size=OBSTACLE_SIZE, fluid_meshes=(), obstacle_meshes=(), viscosity=None):
    """The scene of `seed` (an int or a sequence of ints), everything drawn from numpy.random.default_rng(seed): one to
    three bodies, each a box, ball or upright cylinder of `body_size` scaled by U(0.5, 1.5) and rotated at random, placed
    by rejection so that the bodies' bounding spheres stay a particle spacing apart and inside the box, thrown with a
    start velocity of U(-2, 2) in x and z and U(-0.5, 0.5) in y.  The box is [0, box].  count_range (lo, hi): redraw
    (from the same generator) until the particle count lies in it; None: COUNT_RANGE for the default box and body size,
    no condition otherwise.  obstacles: 0 to 3 static solids (`random_obstacles`), drawn first and from a generator of
    their OWN (the seed's sequence with spawn key 1), so that the fluid's draws are those of the scene without obstacles;
    a body is then also rejected unless its bounding sphere stays a spacing clear of every obstacle's.
    fluid_meshes / obstacle_meshes: SPECs of closed triangle meshes that join the shapes bodies / obstacles are drawn from.
    Which draw becomes a mesh is decided by generators of their own (spawn keys 2 and 3) after the draw has taken its
    values, so that without these options every seed gives the scene it gave, draw for draw.
    viscosity: None, or one of VISCOSITY_LAWS: every accepted body gets a "viscosity" drawn by `draw_viscosity` from a
    generator of its own (spawn key 4), so that every other draw of the seed is what it was."""
    fluid_meshes, obstacle_meshes = [str(m) for m in fluid_meshes], [str(m) for m in obstacle_meshes]
    if viscosity is not None and viscosity not in VISCOSITY_LAWS:
        raise ValueError(f"viscosity must be None or one of {VISCOSITY_LAWS}")
    thick = np.random.default_rng(np.random.SeedSequence(seed, spawn_key=(4,))) if viscosity is not None else None
    if not 0 <= int(obstacles) <= MAX_RANDOM_OBSTACLES:
        raise ValueError(f"obstacles must be 0 .. {MAX_RANDOM_OBSTACLES}")
    rng = np.random.default_rng(seed)
    box = np.asarray(box, np.float64).reshape(3)
    if count_range is None and tuple(box) == DEFAULT_BOX and body_size == BODY_SIZE and radius == ops.PBF_RADIUS:
        count_range = COUNT_RANGE
    spacing = 2.0 * radius
    solids = []
    if obstacles:
        own = np.random.default_rng(np.random.SeedSequence(seed, spawn_key=(1,)))
        pick = np.random.default_rng(np.random.SeedSequence(seed, spawn_key=(3,))) if obstacle_meshes else None
        solids = random_obstacles(own, int(obstacles), box, spacing, obstacle_size, meshes=obstacle_meshes, mesh_rng=pick)
    keep_out = [(np.asarray(o["centre"]), obstacle_bound(o)) for o in solids]
    pick = np.random.default_rng(np.random.SeedSequence(seed, spawn_key=(2,))) if fluid_meshes else None
    for _ in range(max_tries):
        bodies, spheres = [], []
        for _ in range(int(rng.integers(1, 4))):
            shape = SHAPES[int(rng.integers(0, 3))]
            size = float(body_size * rng.uniform(0.5, 1.5))
            rot = _random_rotation(rng)
            spec = None
            if fluid_meshes:
                k = int(pick.integers(0, len(SHAPES) + len(fluid_meshes)))
                if k >= len(SHAPES):
                    shape, spec = MESH, fluid_meshes[k - len(SHAPES)]
            bound = float(np.linalg.norm(body_half_extent(shape, size, spec))) + spacing
            velocity = [float(rng.uniform(-2, 2)), float(rng.uniform(-0.5, 0.5)), float(rng.uniform(-2, 2))]
            for _ in range(100):
                if (2 * bound >= box).any():
                    break
                centre = rng.uniform(bound, box - bound)
                if all(np.linalg.norm(centre - c) >= bound + b for c, b in spheres + keep_out):
                    spheres.append((centre, bound))
                    bodies.append({"shape": shape, "size": size, "rotation": rot.reshape(-1).tolist(),
                                   "centre": centre.tolist(), "velocity": velocity})
                    if spec is not None:
                        bodies[-1]["mesh"] = spec
                    if thick is not None:
                        bodies[-1]["viscosity"] = draw_viscosity(thick, viscosity)
                    break
        seed_out = seed if isinstance(seed, (int, np.integer)) else [int(s) for s in seed]
        scene = Scene([0.0, 0.0, 0.0], box.tolist(), bodies, seed_out, radius, obstacles=solids)
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


def obstacle_table(scenes, device):
    """The batch's device table (B,M,16) of `ops.pbf_obstacles`, validated on the host; None when no scene has an
    obstacle (the substeps then launch nothing for them)."""
    analytic = [[o for o in s.obstacles if o["shape"] != MESH] for s in scenes]
    if not any(analytic):
        return None
    return ops.pbf_obstacles(analytic, len(scenes), device)


def sdf_obstacle_table(scenes, device, step=None):
    """The batch's mesh obstacles as the device pair (table (B,M,24), fields) of `ops.pbf_sdf_obstacles`; None when no
    scene has one.  Every distinct (mesh, size) is sampled ONCE, by `ops.mesh_sdf` at the nodes of a lattice of `step`
    (default: the particle radius) that reaches a radius and two steps beyond the mesh's box, and shared by every
    obstacle of the batch that uses it, at any pose."""
    if not any(o["shape"] == MESH for s in scenes for o in s.obstacles):
        return None
    dev = torch.device(device)
    fields, per_scene = {}, []
    for s in scenes:
        rows = []
        for o in s.obstacles:
            if o["shape"] != MESH:
                continue
            h = float(np.float32(s.radius if step is None else step))
            key = (o["mesh"], float(o["size"]), h, float(s.radius))
            if key not in fields:
                half = mesh_geometry(o["mesh"], o["size"])[2]
                reach = half + (s.radius + 2.0 * h)
                origin = (-reach).astype(np.float32)
                dims = tuple(int(n) for n in np.ceil((reach - origin.astype(np.float64)) / h).astype(np.int64) + 1)
                axes = [torch.from_numpy(origin[a] + np.arange(dims[a], dtype=np.float32) * np.float32(h)).to(dev)
                        for a in range(3)]
                nodes = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3).contiguous()
                fields[key] = (mesh_distance(o["mesh"], o["size"], nodes, dev).view(dims), origin, h)
            field, origin, h = fields[key]
            rows.append({"field": field, "origin": origin, "step": h, "centre": o["centre"],
                         "rotation": o.get("rotation", np.eye(3).reshape(-1).tolist())})
        per_scene.append(rows)
    return ops.pbf_sdf_obstacles(per_scene, len(scenes), dev)


def xsph_table(scenes, prm, device):
    """The batch's per-particle XSPH table (B,N) of `ops.pbf_xsph`, from the bodies' viscosities; a scene without any gets
    `ops.PBF_VISCOSITY`, rows beyond a scene's count 0.  None when no scene has a viscosity (the substeps then take
    params.c, in the launches of before)."""
    nus = [s.viscosity() for s in scenes]
    if all(nu is None for nu in nus):
        return None
    counts = [s.particles()[0].shape[0] for s in scenes]
    table = np.zeros((len(scenes), max(counts + [0])), np.float64)
    for b, (nu, n) in enumerate(zip(nus, counts)):
        table[b, :n] = ops.PBF_VISCOSITY if nu is None else nu
    return ops.pbf_xsph(table, prm, torch.device(device))


def simulate(scenes, frames, substeps=SUBSTEPS, iters=ops.PBF_ITERS, params=None, device="cuda"):
    """`frames` exported frames of every scene, frame 0 being the start state and each further one 1/40 s later, made of
    `substeps` substeps of dt = 1 / (40 * substeps).  All scenes advance in the same launches; the frames stay on the
    device.  params: an `ops.PbfParams` (its `iters` wins); None: the defaults with `iters`, at the first scene's radius.
    The scenes' obstacles go into one table, built once and passed to every substep; mesh obstacles into a table and a
    field buffer of their own (`sdf_obstacle_table`), also built once.  Bodies with a "viscosity" make a per-particle XSPH
    table (`xsph_table`), built once; params.vorticity > 0 adds vorticity confinement to every substep.
    -> pos, vel (B, frames, N, 3) fp32, lengths (B,) int64 (rows beyond a scene's length are 0)."""
    if frames < 1 or substeps < 1:
        raise ValueError("frames and substeps must be >= 1")
    prm = params if params is not None else ops.PbfParams(radius=scenes[0].radius if scenes else ops.PBF_RADIUS, iters=iters)
    x, v, lengths, lo, hi = pack(scenes, torch.device(device))
    table = obstacle_table(scenes, torch.device(device))
    sdf = sdf_obstacle_table(scenes, torch.device(device))
    extra = {} if sdf is None else {"sdf_obstacles": sdf}    # without mesh obstacles: the call of before
    xsph = xsph_table(scenes, prm, device)
    if xsph is not None:                                     # without viscosities: the call of before
        extra["xsph"] = xsph
    B, N, _ = x.shape
    pos, vel = x.new_zeros((B, frames, N, 3)), x.new_zeros((B, frames, N, 3))
    dt = 1.0 / (FPS * substeps)
    for f in range(frames):
        if f:
            for _ in range(substeps):
                x, v = ops.pbf_substep(x, v, lengths, lo, hi, dt, prm, table, **extra)
        pos[:, f], vel[:, f] = x, v
    return pos, vel, lengths


def obstacle_distance(obstacles, points):
    """The signed distance (negative inside) of points (n,3) to the union of the obstacle dicts, exact per shape, in
    the points' dtype on their device -> (n,).  A mesh obstacle's is `ops.mesh_sdf` of the points in its frame (fp32)."""
    best = torch.full(points.shape[:1], float("inf"), dtype=points.dtype, device=points.device)
    for ob in obstacles:
        t = lambda v: torch.tensor(v, dtype=points.dtype, device=points.device)  # noqa: E731
        R = t(ob.get("rotation", np.eye(3).reshape(-1).tolist())).view(3, 3)
        q = (points - t(ob["centre"])) @ R                                       # q_k = sum_i d_i R[i][k]
        if ob["shape"] == MESH:
            best = torch.minimum(best, mesh_distance(ob["mesh"], ob["size"], q.float(), points.device).to(points.dtype))
            continue
        size = t(ob["size"]).reshape(-1)
        if ob["shape"] == "ball":
            d = q.norm(dim=1) - size[0]
        else:
            if ob["shape"] == "box":
                e = q.abs() - size
            else:
                e = torch.stack([q[:, [0, 2]].norm(dim=1) - size[0], q[:, 1].abs() - size[1]], 1)
            d = e.clamp(min=0).norm(dim=1) + e.amax(dim=1).clamp(max=0)
        best = torch.minimum(best, d)
    return best


def obstacle_mesh(scene, step=None, device="cuda"):
    """The surface of a scene's obstacles as a `mesh.Mesh` wound outward, to be loaded beside the fluid's meshes: the
    union's signed distance, negated so that inside is positive, sampled on a lattice of `step` (default one particle
    spacing) around the obstacles and meshed at level 0 by `ops.iso_surface`.  Linear interpolation of a distance field
    puts the surface within one step of the true one; edges and corners are rounded at that scale."""
    from . import mesh
    ops._need(len(scene.obstacles) > 0, "the scene has no obstacles")
    step = float(np.float32(2.0 * scene.radius if step is None else step))
    ops._need(np.isfinite(step) and step > 0.0, "step must be positive and finite")
    centres = np.array([o["centre"] for o in scene.obstacles], np.float64)
    bounds = np.array([obstacle_bound(o) for o in scene.obstacles])[:, None]
    lo, hi = (centres - bounds).min(0) - 2.0 * step, (centres + bounds).max(0) + 2.0 * step
    shape = tuple(int(n) for n in np.ceil((hi - lo) / step).astype(np.int64) + 1)
    ops._need(shape[0] * shape[1] * shape[2] <= mesh.MAX_NODES, f"a lattice of {shape} nodes is too large: raise step")
    lattice = mesh.Lattice(lo.astype(np.float32), step, shape)
    dev = torch.device(device)
    axes = [torch.from_numpy(lattice.origin[a] + np.arange(shape[a], dtype=np.float32) * np.float32(step)).to(dev)
            for a in range(3)]
    nodes = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    field = (-obstacle_distance(scene.obstacles, nodes)).reshape(shape).contiguous()
    vertices, faces, nrm = ops.iso_surface(field, lattice.origin, step, 0.0, True)
    return mesh.Mesh(vertices, faces, nrm, lattice, 0.0)


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
        if scene.obstacles:
            from . import mesh
            mesh.write_ply(os.path.join(case, "obstacles.ply"), obstacle_mesh(scene, device=device))
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
    ap.add_argument("--obstacles", type=int, default=0, help="static solids per scene (0 .. 3), in the lower half of the box")
    ap.add_argument("--obstacle_size", type=float, nargs=2, default=list(OBSTACLE_SIZE),
                    help="range of an obstacle's largest extent in metres")
    ap.add_argument("--fluid_mesh", type=str, nargs="*", default=[], metavar="SPEC",
                    help="closed meshes that join the shapes bodies are drawn from: a .obj/.ply path, icosphere:N, torus:R,r,nu,nv")
    ap.add_argument("--obstacle_mesh", type=str, nargs="*", default=[], metavar="SPEC",
                    help="closed meshes that join the shapes obstacles are drawn from (needs --obstacles >= 1)")
    ap.add_argument("--viscosity", choices=("default",) + VISCOSITY_LAWS, default="default",
                    help="the law every fluid body's viscosity is drawn from (the reference recipe's); default: every "
                         "body is the liquid of viscosity 0.01, and nothing is recorded")
    ap.add_argument("--vorticity", type=float, nargs="?", const=ops.PBF_VORTICITY, default=0.0, metavar="EPS",
                    help=f"vorticity confinement of strength EPS m/s (the bare flag: {ops.PBF_VORTICITY}); absent: none")
    a = ap.parse_args(argv)
    if not (np.isfinite(a.vorticity) and a.vorticity >= 0.0):
        ap.error("--vorticity EPS >= 0")
    if a.obstacle_mesh and not a.obstacles:
        ap.error("--obstacle_mesh adds shapes to the obstacles' draw: give --obstacles 1 .. 3 as well")
    if a.cases < 0 or a.test_cases < 0 or a.frames < 1 or a.batch < 1 or a.substeps < 1 or a.iters < 0:
        ap.error("--cases, --test_cases, --iters >= 0; --frames, --batch, --substeps >= 1")
    if not 0 <= a.obstacles <= MAX_RANDOM_OBSTACLES or not 0 < a.obstacle_size[0] <= a.obstacle_size[1]:
        ap.error(f"--obstacles 0 .. {MAX_RANDOM_OBSTACLES}; --obstacle_size 0 < LO <= HI")
    prm = ops.PbfParams(radius=a.particle_radius, iters=a.iters, vorticity=a.vorticity)
    law = None if a.viscosity == "default" else a.viscosity
    settings = {"box": list(a.box), "body_size": a.body_size}
    if a.obstacles:                                          # without obstacles scene.json holds what it always held
        settings["obstacle_size"] = list(a.obstacle_size)
    if a.fluid_mesh:
        settings["fluid_mesh"] = list(a.fluid_mesh)
    if a.obstacle_mesh:
        settings["obstacle_mesh"] = list(a.obstacle_mesh)
    # split 0: training, 1: held out -- the seed sequences (seed, split, case) can never coincide
    for split, (out, cases) in enumerate(((a.out, a.cases), (a.test_out, a.test_cases if a.test_out else 0))):
        for c0 in range(0, cases, a.batch):
            scenes = [random_scene([a.seed, split, c], tuple(a.box), a.particle_radius, a.body_size, obstacles=a.obstacles,
                                   obstacle_size=tuple(a.obstacle_size), fluid_meshes=a.fluid_mesh,
                                   obstacle_meshes=a.obstacle_mesh, viscosity=law)
                      for c in range(c0, min(c0 + a.batch, cases))]
            write_cases(out, scenes, c0 + 1, a.frames, a.substeps, prm, a.device, settings)
    return 0


if __name__ == "__main__":
    sys.exit(main())
