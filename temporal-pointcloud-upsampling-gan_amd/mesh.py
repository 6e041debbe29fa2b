"""Triangle meshes of particle frames on the GPU: the fluid's surface as geometry, with OBJ / PLY export.

    python -m tpgan_amd.mesh --frames 'out/pcd_{i}.npy' --count 200 --out meshes [--format ply|obj --spacing 0.025
        --support 0.05 --step 0.0125 --iso 0.5 --stats stats.npz --kernel isotropic|anisotropic --cov_radius 0.1
        --smooth_lambda 0.9 --render PNGDIR (and the options of tpgan_amd.render)]

The reference ends its demo (train_fluid/demo.ipynb, cell 5) by writing every upsampled frame to a geometry file for an
external renderer that reconstructs the fluid's surface.  Here the surface is built on the device: the particles' cubic
kernel density (`ops.radius_reduce`, the reference's particle_dns2grid_dns) is sampled on a lattice around the frame and
its level set at a fraction of the density inside a full particle lattice is meshed by `ops.iso_surface` (marching
tetrahedra, csrc/isosurface.hip).  The mesher is this project's own: no parity with any external reconstruction tool is
claimed.  A mesh also gives the enclosed volume and the surface area of a frame, which `analysis` cannot.

--kernel anisotropic replaces the density of one ball per particle by that of one ellipsoid per particle, fitted to the
particle's neighbourhood (`ops.anisotropic_kernels` / `ops.anisotropic_field`, csrc/aniso.hip; Yu and Turk): irregular
particle spacing no longer shows as bumps on flat regions.  Its centre smoothing pulls the surface INWARDS by about one
particle spacing against the isotropic surface; --smooth_lambda and --iso are the knobs, nothing compensates
for it silently.
"""
import argparse
import collections
import json
import os

import numpy as np
import torch

from . import analysis, ops, render

MAX_NODES = ops.ISO_MAX_NODES
NODES_PER_CALL = 1 << 22               # lattice nodes per radius_reduce call: bounds the node positions held at once

Lattice = collections.namedtuple("Lattice", "origin step shape")             # origin (3,) fp32 host, step fp32, (nx,ny,nz)
Mesh = collections.namedtuple("Mesh", "vertices faces normals lattice iso")  # iso: the field value that was meshed


def _valid_rows(points, lengths=None):
    """(N,3) -> the rows that are points: finite, every |coordinate| < 900 (the 999 rows of hard masking are not), below
    `lengths` when given."""
    p = torch.as_tensor(points).detach().float()
    ops._need(p.dim() == 2 and p.shape[1] == 3, f"points must be (N,3), got {tuple(p.shape)}")
    valid = torch.isfinite(p).all(-1) & (p.abs() < render.PADDING).all(-1)
    if lengths is not None:
        n = int(torch.as_tensor(lengths).reshape(-1)[0])
        valid &= torch.arange(p.shape[0], device=p.device) < n
    return p[valid].contiguous()


def lattice_for(points, support, step, lengths=None, reach=None):
    """The lattice of spacing `step` around the valid rows of `points` (N,3): their bounding box padded by support +
    2 step on every side (`reach` + 2 step when given: the anisotropic field's kernels extend to s_max * support), so
    that the boundary nodes lie beyond every particle's support (field 0 there) and no active edge comes within one node
    of the boundary: the mesh is closed.  Raises, naming a step that fits, when the lattice would hold more than 2^27
    nodes."""
    support, step = float(support), float(np.float32(step))
    ops._need(np.isfinite(support) and support > 0.0, "support must be positive and finite")
    ops._need(np.isfinite(step) and step > 0.0, "step must be positive and finite")
    p = _valid_rows(points, lengths)
    ops._need(p.shape[0] > 0, "no valid point to build a lattice around")
    lo, hi = p.amin(0).double().cpu().numpy(), p.amax(0).double().cpu().numpy()
    pad = (support if reach is None else float(reach)) + 2.0 * step
    origin = (lo - pad).astype(np.float32)
    extent = (hi + pad) - origin.astype(np.float64)
    shape = tuple(int(np.ceil(e / step)) + 1 for e in extent)                 # origin + (n - 1) step >= hi + pad
    nodes = float(shape[0]) * shape[1] * shape[2]
    if nodes > MAX_NODES:
        fit = step * (nodes / MAX_NODES) ** (1.0 / 3.0) * 1.02
        raise RuntimeError(f"a lattice of {shape[0]} x {shape[1]} x {shape[2]} nodes at step {step:g} exceeds 2^27 nodes; "
                           f"a step of {fit:.4g} would fit")
    return Lattice(origin, step, shape)


def lattice_nodes(lattice, first, count, device):
    """The positions (count,3) fp32 of the nodes first .. first + count - 1: origin[a] + (float)index_a * step, the
    kernels' arithmetic."""
    nx, ny, nz = lattice.shape
    n = torch.arange(first, first + count, device=device)
    ij = torch.div(n, nz, rounding_mode="floor")
    idx = torch.stack([torch.div(ij, ny, rounding_mode="floor"), ij % ny, n % nz], 1)
    return torch.from_numpy(lattice.origin).to(device).view(1, 3) + idx.float() * lattice.step


def density_field(points, lattice, support, lengths=None):
    """(nx,ny,nz) fp32 on the points' device: at every node the sum of the cubic kernel of width `support` over the valid
    rows of `points` -- `ops.radius_reduce(nodes, points, support, "cubic")`, bit for bit, NODES_PER_CALL nodes per call.
    A backend without that op (the CPU checker) runs its torch statement."""
    p = _valid_rows(points, lengths)
    be = ops.backend_for(p)
    nx, ny, nz = lattice.shape
    G = nx * ny * nz
    field = torch.empty(G, dtype=torch.float32, device=p.device)
    with torch.no_grad():
        for first in range(0, G, NODES_PER_CALL):
            count = min(NODES_PER_CALL, G - first)
            nodes = lattice_nodes(lattice, first, count, p.device)
            if hasattr(be, "radius_reduce"):
                field[first:first + count] = ops.radius_reduce(nodes, p, support, "cubic")[1]
            else:
                field[first:first + count] = ops._radius_cubic_sums_torch(nodes, p, support)
    return field.view(nx, ny, nz)


def cubic_kernel(q):
    """analysis_helper.py:102-113 with coefficient 1, float64."""
    q = np.asarray(q, dtype=np.float64)
    return np.where(q <= 0.5, 6.0 * (q ** 3 - q ** 2) + 1.0, 2.0 * np.clip(1.0 - q, 0.0, None) ** 3)


def lattice_value(spacing, support):
    """The density at a particle of an infinite cubic lattice of `spacing`: the float64 sum of the cubic kernel of width
    `support` over the lattice points within it, the particle itself included (as `ops.pbf_lattice_sum` for its kernel)."""
    spacing, support = float(spacing), float(support)
    m = int(np.floor(support / spacing)) + 1
    r = np.arange(-m, m + 1, dtype=np.float64) * spacing
    d = np.sqrt((r[:, None, None] ** 2 + r[None, :, None] ** 2) + r[None, None, :] ** 2)
    return float(cubic_kernel(d[d <= support] / support).sum())


def lattice_covariance(spacing, cov_radius):
    """The per-axis weighted variance, in units of cov_radius^2, of an infinite cubic lattice of `spacing` seen from one
    of its points: sum w x^2 / sum w over the lattice points within cov_radius (the particle itself included) with the
    weights w = 1 - (d / cov_radius)^3 of the anisotropic kernels' stage A, float64.  Its reciprocal is the `ks` that
    makes the kernel of a particle inside a full lattice the isotropic one (0.150571... at 4 spacings)."""
    spacing, rc = float(spacing), float(cov_radius)
    ops._need(np.isfinite(spacing) and spacing > 0.0 and np.isfinite(rc) and rc > 0.0,
              "spacing and cov_radius must be positive and finite")
    m = int(np.floor(rc / spacing)) + 1
    r = np.arange(-m, m + 1, dtype=np.float64) * spacing
    x = np.broadcast_to(r[:, None, None], (r.shape[0],) * 3)
    d = np.sqrt((r[:, None, None] ** 2 + r[None, :, None] ** 2) + r[None, None, :] ** 2)
    inside = d <= rc
    w = 1.0 - (d[inside] / rc) ** 3
    return float((w * (x[inside] / rc) ** 2).sum() / w.sum())


ANISO_S_MAX = 2.0                       # the clamp on the extents: the anisotropic kernels reach s_max * support


def anisotropic_field(points, lattice, spacing, support, cov_radius=None, smooth_lambda=0.9, lengths=None):
    """(nx,ny,nz) fp32 on the points' device: the anisotropic kernels' density of the valid rows of `points` at every
    node -- `ops.anisotropic_kernels` at the defaults with cov_radius (default 2 support) and ks = 1 /
    `lattice_covariance(spacing, cov_radius)`, then `ops.anisotropic_field`, NODES_PER_CALL nodes per call.  Inside a
    full lattice of `spacing` it is the isotropic `density_field`."""
    p = _valid_rows(points, lengths)
    rc = 2.0 * float(support) if cov_radius is None else float(cov_radius)
    ks = 1.0 / lattice_covariance(spacing, rc)
    nx, ny, nz = lattice.shape
    G = nx * ny * nz
    field = torch.empty(G, dtype=torch.float32, device=p.device)
    with torch.no_grad():
        centres, mat, det, _ = ops.anisotropic_kernels(p, rc, ks, smooth_lambda, s_max=ANISO_S_MAX)
        for first in range(0, G, NODES_PER_CALL):
            count = min(NODES_PER_CALL, G - first)
            nodes = lattice_nodes(lattice, first, count, p.device)
            field[first:first + count] = ops.anisotropic_field(nodes, centres, mat, det, support, ANISO_S_MAX)
    return field.view(nx, ny, nz)


KERNELS = ("isotropic", "anisotropic")


def surface_mesh(points, spacing=analysis.BASE_RADIUS, support=None, step=None, iso=0.5, lengths=None, normals=True,
                 kernel="isotropic", cov_radius=None, smooth_lambda=0.9):
    """The surface of one frame of particles (N,3) as a `Mesh`: the cubic density of width `support` (default 2 spacings)
    on a lattice of `step` (default spacing / 2), meshed at `iso` x the density inside a full particle lattice
    (`lattice_value`; at support = 2 spacings the field inside a full lattice varies by under 0.3 %, so 0.5 leaves no
    cavities).  vertices (V,3) f32, faces (F,3) int32 wound outward, normals (V,3) f32 or None, on the points' device.
    kernel="anisotropic": the density of `anisotropic_field` (cov_radius, smooth_lambda) on a lattice padded by
    s_max * support + 2 step; the level keeps its meaning, since inside a full lattice the two fields agree.  The
    smoothed centres pull that surface inwards by about one spacing: smooth_lambda and iso are the knobs."""
    spacing = float(spacing)
    ops._need(np.isfinite(spacing) and spacing > 0.0, "spacing must be positive and finite")
    support = 2.0 * spacing if support is None else float(support)
    step = spacing / 2.0 if step is None else float(step)
    ops._need(np.isfinite(iso) and iso > 0.0, "iso must be a positive fraction of the lattice density")
    ops._need(kernel in KERNELS, f"kernel must be one of {KERNELS}")
    if kernel == "anisotropic":
        # the centres are convex combinations of the points: the points' bounding box bounds them too
        lattice = lattice_for(points, support, step, lengths, reach=ANISO_S_MAX * support)
        field = anisotropic_field(points, lattice, spacing, support, cov_radius, smooth_lambda, lengths)
    else:
        lattice = lattice_for(points, support, step, lengths)
        field = density_field(points, lattice, support, lengths)
    level = float(np.float32(float(iso) * lattice_value(spacing, support)))
    vertices, faces, nrm = ops.iso_surface(field, lattice.origin, lattice.step, level, normals)
    return Mesh(vertices, faces, nrm, lattice, level)


def _corners(mesh):
    v, f = mesh.vertices.double(), mesh.faces.long()
    return v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]


def volume(mesh):
    """The volume a closed mesh encloses (positive for outward winding): sum of a . (b x c) / 6 over the faces, float64."""
    a, b, c = _corners(mesh)
    return float((torch.linalg.cross(a, b) * c).sum() / 6.0)


def area(mesh):
    """The mesh's surface area: sum of |(b - a) x (c - a)| / 2 over the faces, float64."""
    a, b, c = _corners(mesh)
    return float(torch.linalg.cross(b - a, c - a).norm(dim=1).sum() / 2.0)


def _host(mesh):
    v = mesh.vertices.detach().cpu().numpy().astype("<f4")
    f = mesh.faces.detach().cpu().numpy().astype("<i4")
    n = None if mesh.normals is None else mesh.normals.detach().cpu().numpy().astype("<f4")
    return v, f, n


def write_ply(path, mesh, ascii=False):
    """Binary little-endian PLY: vertices x y z [nx ny nz] float, faces as `list uchar int`.  Standard library and numpy.
    ascii: the same file as text, nine significant digits, so that fp32 values read back unchanged."""
    v, f, n = _host(mesh)
    props = ["x", "y", "z"] + ([] if n is None else ["nx", "ny", "nz"])
    header = ["ply", "format %s 1.0" % ("ascii" if ascii else "binary_little_endian"), "comment tpgan_amd.mesh",
              f"element vertex {v.shape[0]}"]
    header += [f"property float {name}" for name in props]
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    rows = v if n is None else np.concatenate([v, n], axis=1)
    if ascii:
        with open(path, "w") as out:
            out.write("\n".join(header) + "\n")
            out.writelines(" ".join("%.9g" % x for x in row) + "\n" for row in rows.tolist())
            out.writelines("3 %d %d %d\n" % tuple(row) for row in f.tolist())
        return
    faces = np.empty(f.shape[0], dtype=[("count", "u1"), ("index", "<i4", (3,))])
    faces["count"] = 3
    faces["index"] = f
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(np.ascontiguousarray(rows, dtype="<f4").tobytes())
        out.write(faces.tobytes())


def write_obj(path, mesh):
    """Wavefront OBJ: `v`, `vn` (when the mesh has normals) and `f a//a b//b c//c`, indices from 1; nine significant
    digits, so that fp32 values read back unchanged."""
    v, f, n = _host(mesh)
    with open(path, "w") as out:
        out.write("# tpgan_amd.mesh\n")
        out.writelines("v %.9g %.9g %.9g\n" % tuple(row) for row in v.tolist())
        if n is not None:
            out.writelines("vn %.9g %.9g %.9g\n" % tuple(row) for row in n.tolist())
            out.writelines("f %d//%d %d//%d %d//%d\n" % (a, a, b, b, c, c) for a, b, c in (f + 1).tolist())
        else:
            out.writelines("f %d %d %d\n" % tuple(row) for row in (f + 1).tolist())


WRITERS = {"ply": write_ply, "obj": write_obj}


# ---- meshes in: readers, a closedness check and two generators (what `ops.mesh_sdf` and `simulate` take) ------------
def _obj_index(token, count):
    i = int(token.split("/")[0])                             # v, v/vt, v//vn, v/vt/vn
    return i - 1 if i > 0 else count + i                     # negative: relative to the vertices read so far


def read_obj(path):
    """Wavefront OBJ -> (vertices (V,3) float32, faces (F,3) int32): the `v` and `f` lines, everything else ignored.
    Polygons are fanned about their first corner; `v/vt/vn` forms and negative (relative) indices are accepted."""
    vertices, faces = [], []
    with open(path) as src:
        for line in src:
            parts = line.split()
            if not parts:
                continue
            if parts[0] == "v":
                vertices.append([float(x) for x in parts[1:4]])
            elif parts[0] == "f":
                idx = [_obj_index(t, len(vertices)) for t in parts[1:]]
                faces += [[idx[0], idx[k], idx[k + 1]] for k in range(1, len(idx) - 1)]
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ops._need(f.size == 0 or (int(f.min()) >= 0 and int(f.max()) < v.shape[0]), f"{path}: a face names a missing vertex")
    return v, f.astype(np.int32)


def read_ply(path):
    """The triangle PLY files `write_ply` writes, binary little-endian or ASCII -> (vertices (V,3) float32, faces (F,3)
    int32, normals (V,3) float32 or None): float vertex properties of which x y z [nx ny nz] are taken, faces as
    `list uchar int` of three indices each."""
    with open(path, "rb") as src:
        ops._need(src.readline().strip() == b"ply", f"{path}: not a PLY file")
        fmt, elements = None, []
        while True:
            line = src.readline()
            ops._need(len(line) > 0, f"{path}: no end_header")
            parts = line.decode("ascii").split()
            if not parts or parts[0] in ("comment", "obj_info"):
                continue
            if parts[0] == "format":
                fmt = parts[1]
            elif parts[0] == "element":
                elements.append((parts[1], int(parts[2]), []))
            elif parts[0] == "property":
                elements[-1][2].append(parts[1:])
            elif parts[0] == "end_header":
                break
        ops._need(fmt in ("ascii", "binary_little_endian"), f"{path}: format {fmt} is not read")
        ops._need([e[0] for e in elements] == ["vertex", "face"], f"{path}: expected the elements vertex, face")
        (_, V, vprops), (_, F, fprops) = elements
        ops._need(all(len(q) == 2 and q[0] in ("float", "float32") for q in vprops), f"{path}: vertex properties must be float")
        ops._need(len(fprops) == 1 and fprops[0][:3] in (["list", "uchar", "int"], ["list", "uint8", "int32"]),
                  f"{path}: faces must be `list uchar int`")
        names = [q[1] for q in vprops]
        if fmt == "ascii":
            tokens = src.read().split()
            rows = np.array(tokens[:V * len(names)], dtype=np.float64).astype(np.float32).reshape(V, len(names))
            rest = np.array(tokens[V * len(names):V * len(names) + 4 * F], dtype=np.int64).reshape(F, 4)
            counts, faces = rest[:, 0], rest[:, 1:]
        else:
            rows = np.frombuffer(src.read(4 * V * len(names)), dtype="<f4").reshape(V, len(names))
            rec = np.frombuffer(src.read(13 * F), dtype=[("count", "u1"), ("index", "<i4", (3,))])
            counts, faces = rec["count"], rec["index"]
        ops._need(bool((np.asarray(counts) == 3).all()), f"{path}: every face must be a triangle")
    col = lambda *want: np.ascontiguousarray(rows[:, [names.index(w) for w in want]], dtype=np.float32)  # noqa: E731
    normals = col("nx", "ny", "nz") if all(w in names for w in ("nx", "ny", "nz")) else None
    return col("x", "y", "z"), np.ascontiguousarray(faces, dtype=np.int32), normals


def check_closed(vertices, faces):
    """Counts that say whether `ops.mesh_sdf`'s sign means anything for a mesh -> dict:
        boundary_edges      undirected edges used by exactly one face          (the sign needs 0)
        nonmanifold_edges   undirected edges used by more than two faces       (the sign needs 0)
        zero_normal_faces   faces whose fp32 normal is exactly zero            (skipped by the op; reported)
        inconsistent_pairs  edges whose two faces run along them in the SAME direction (reported; parity does not care)"""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = np.minimum(e[:, 0], e[:, 1]) * (int(f.max(initial=0)) + 1) + np.maximum(e[:, 0], e[:, 1])
    forward = (e[:, 0] < e[:, 1]).astype(np.int64)
    uniq, inverse, counts = np.unique(key, return_inverse=True, return_counts=True)
    fwd = np.bincount(inverse.reshape(-1), weights=forward, minlength=len(uniq))
    u, w = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                  u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    return {"boundary_edges": int((counts == 1).sum()), "nonmanifold_edges": int((counts > 2).sum()),
            "zero_normal_faces": int((n == 0).all(1).sum()),
            "inconsistent_pairs": int(((counts == 2) & (fwd != 1)).sum())}


def make_icosphere(subdivisions=2, radius=1.0):
    """A closed sphere of 20 * 4^subdivisions triangles wound outward: the icosahedron, every triangle split in four and
    the new vertices pushed onto the sphere -> (vertices (V,3) float32, faces (F,3) int32)."""
    ops._need(0 <= int(subdivisions) <= 7, "subdivisions must be 0 .. 7")
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1),
         (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [tuple(np.asarray(p, np.float64) / np.linalg.norm(p)) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    for _ in range(int(subdivisions)):
        mid, out = {}, []

        def middle(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                m = np.asarray(v[a]) + np.asarray(v[b])
                v.append(tuple(m / np.linalg.norm(m)))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return (np.asarray(v, np.float64) * float(radius)).astype(np.float32), np.asarray(f, dtype=np.int32)


def make_torus(R=0.5, r=0.2, nu=48, nv=24):
    """A closed torus about the y axis, wound outward: centre circle of radius R in the xz plane, tube radius r, nu
    segments around the axis and nv around the tube, 2 nu nv triangles -> (vertices (nu*nv,3) float32, faces int32)."""
    ops._need(int(nu) >= 3 and int(nv) >= 3 and 0.0 < float(r) < float(R), "a torus needs nu, nv >= 3 and 0 < r < R")
    nu, nv = int(nu), int(nv)
    u = 2.0 * np.pi * np.arange(nu) / nu
    w = 2.0 * np.pi * np.arange(nv) / nv
    ring = R + r * np.cos(w)[None, :]
    v = np.stack([ring * np.cos(u)[:, None], np.broadcast_to(r * np.sin(w)[None, :], (nu, nv)), ring * np.sin(u)[:, None]],
                 -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a, b = i * nv + j, ((i + 1) % nu) * nv + j
    c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
    f = np.concatenate([np.stack([a, d, c], -1).reshape(-1, 3), np.stack([a, c, b], -1).reshape(-1, 3)])
    return v.astype(np.float32), f.astype(np.int32)


def load_spec(spec):
    """A mesh from a SPEC: a path to an .obj or .ply file, `icosphere:SUBDIVISIONS` or `torus:R,r,nu,nv` ->
    (vertices (V,3) float32, faces (F,3) int32)."""
    spec = str(spec)
    kind, _, args = spec.partition(":")
    if kind == "icosphere" and not os.path.exists(spec):
        return make_icosphere(int(args) if args else 2)
    if kind == "torus" and not os.path.exists(spec):
        a = [x for x in args.split(",") if x]
        ops._need(len(a) in (0, 4), "torus:R,r,nu,nv")
        return make_torus(*((float(a[0]), float(a[1]), int(a[2]), int(a[3])) if a else ()))
    ops._need(os.path.exists(spec), f"mesh spec {spec!r}: no such file, and not icosphere:N or torus:R,r,nu,nv")
    if spec.lower().endswith(".obj"):
        return read_obj(spec)
    v, f, _ = read_ply(spec)
    return v, f


class SequenceMesher:
    """Meshes of a sequence, `pcd_{i:04d}.ply` (or .obj) in `out_dir`.  `push(frames, first)`: frames = list of (n_t,3)
    clouds, first = index of the first one -> one record per frame (frame, points, vertices, faces, volume, area), also
    appended to `records`.  on_mesh(index, mesh): called with every mesh after its file is written."""

    def __init__(self, out_dir, fmt="ply", spacing=analysis.BASE_RADIUS, support=None, step=None, iso=0.5, device="cuda",
                 kernel="isotropic", cov_radius=None, smooth_lambda=0.9, on_mesh=None):
        if fmt not in WRITERS:
            raise ValueError(f"format must be one of {sorted(WRITERS)}")
        if kernel not in KERNELS:
            raise ValueError(f"kernel must be one of {KERNELS}")
        self.out_dir, self.fmt, self.device = out_dir, fmt, torch.device(device)
        self.spacing, self.support, self.step, self.iso = spacing, support, step, iso
        self.kernel, self.cov_radius, self.smooth_lambda = kernel, cov_radius, smooth_lambda
        self.records, self.on_mesh = [], on_mesh
        os.makedirs(out_dir, exist_ok=True)

    def push(self, frames, first):
        out = []
        for t, frame in enumerate(frames):
            p = torch.as_tensor(frame).detach().float().reshape(-1, 3).to(self.device)
            m = surface_mesh(p, self.spacing, self.support, self.step, self.iso, kernel=self.kernel,
                             cov_radius=self.cov_radius, smooth_lambda=self.smooth_lambda)
            WRITERS[self.fmt](os.path.join(self.out_dir, f"pcd_{first + t:04d}.{self.fmt}"), m)
            if self.on_mesh is not None:
                self.on_mesh(first + t, m)
            out.append(dict(frame=first + t, points=int(_valid_rows(p).shape[0]), vertices=int(m.vertices.shape[0]),
                            faces=int(m.faces.shape[0]), volume=volume(m), area=area(m)))
        self.records += out
        return out

    def stats(self):
        """Per-frame volume and area and their first differences (`analysis.first_difference`)."""
        vol = np.array([r["volume"] for r in self.records], dtype=np.float64)
        are = np.array([r["area"] for r in self.records], dtype=np.float64)
        return {"volume": vol, "area": are, "d_volume": analysis.first_difference(vol),
                "d_area": analysis.first_difference(are)}


def add_mesh_options(ap):
    ap.add_argument("--format", choices=sorted(WRITERS), default="ply", help="mesh files: binary PLY or OBJ")
    ap.add_argument("--spacing", type=float, default=analysis.BASE_RADIUS, help="the particles' spacing")
    ap.add_argument("--support", type=float, default=None, help="width of the density kernel (default 2 spacings)")
    ap.add_argument("--step", type=float, default=None, help="lattice step (default spacing / 2)")
    ap.add_argument("--iso", type=float, default=0.5, help="level, as a fraction of a full lattice's density")
    ap.add_argument("--kernel", choices=KERNELS, default="isotropic",
                    help="one ball per particle, or one ellipsoid fitted to its neighbourhood (smoother; sits further in)")
    ap.add_argument("--cov_radius", type=float, default=None,
                    help="anisotropic: neighbourhood radius of the fit (default 2 supports)")
    ap.add_argument("--smooth_lambda", type=float, default=0.9,
                    help="anisotropic: how far a kernel's centre moves toward its neighbours' weighted mean, 0..1")


def mesher_from(a, out_dir, device):
    return SequenceMesher(out_dir, a.format, a.spacing, a.support, a.step, a.iso, device, a.kernel, a.cov_radius,
                          a.smooth_lambda)


class MeshPictures:
    """`--render`: every mesh that was written, drawn with its vertex normals to `pcd_{i:04d}.png` in `out_dir` under one
    camera, fitted to the first mesh; `a` holds the options of `render.add_render_options` (its --solids are drawn too)."""

    def __init__(self, a, out_dir):
        self.a, self.out_dir, self.camera = a, out_dir, None
        self.solids = load_spec(a.solids) if a.solids else None
        os.makedirs(out_dir, exist_ok=True)

    def __call__(self, index, m):
        a = self.a
        if self.camera is None:
            ops._need(m.vertices.shape[0] > 0, "--render: the first frame has no surface to fit the camera to")
            self.camera = render.Camera.fit(m.vertices, direction=a.direction, mode=a.mode, width=a.width, height=a.height)
        image, depth = render.render_mesh(m, self.camera, return_depth=True)
        if self.solids is not None:
            image, _ = render._with_solids(image[None], depth[None], self.solids, a.solids_color, self.camera.row()[None],
                                           self.camera, 1, (255, 255, 255), ops.RENDER_KEY_BYTES)
            image = image[0]
        render.write_png(os.path.join(self.out_dir, f"pcd_{index:04d}.png"), image)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m tpgan_amd.mesh",
                                 description="Mesh the fluid surface of a sequence of frames to PLY / OBJ files.")
    ap.add_argument("--frames", required=True, help="frame files, '{i}' = frame index, e.g. 'out/pcd_{i}.npy'")
    ap.add_argument("--count", type=int, required=True, help="frames 0 .. count-1")
    ap.add_argument("--out", required=True, help="output directory for pcd_{i:04d}.ply")
    add_mesh_options(ap)
    ap.add_argument("--stats", default=None, metavar="FILE.npz", help="per-frame volume, area and their first differences")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--render", default=None, metavar="PNGDIR", help="also draw every mesh to PNGDIR/pcd_{i:04d}.png")
    render.add_render_options(ap)
    a = ap.parse_args(argv)
    if "{i}" not in a.frames:
        ap.error("--frames must contain '{i}'")
    if a.count < 1:
        ap.error("--count must be at least 1")
    if a.translucent:
        ap.error("--translucent goes with pictures of the particles (--style surface of tpgan_amd.render and "
                 "tpgan_amd.rollout): --render here draws the mesh, which is opaque")
    seq = mesher_from(a, a.out, a.device)
    if a.render:
        seq.on_mesh = MeshPictures(a, a.render)
    for i in range(a.count):
        for record in seq.push([render.load_frame(a.frames.format(i=i))], i):
            print(json.dumps(record), flush=True)
    if a.stats:
        np.savez(a.stats, **seq.stats())


if __name__ == "__main__":
    main()
