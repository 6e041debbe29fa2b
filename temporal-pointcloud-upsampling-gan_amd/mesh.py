"""Triangle meshes of particle frames on the GPU: the fluid's surface as geometry, with OBJ / PLY export.

    python -m tpgan_amd.mesh --frames 'out/pcd_{i}.npy' --count 200 --out meshes [--format ply|obj --spacing 0.025
        --support 0.05 --step 0.0125 --iso 0.5 --stats stats.npz --kernel isotropic|anisotropic --cov_radius 0.1
        --smooth_lambda 0.9]

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


def write_ply(path, mesh):
    """Binary little-endian PLY: vertices x y z [nx ny nz] float, faces as `list uchar int`.  Standard library and numpy."""
    v, f, n = _host(mesh)
    props = ["x", "y", "z"] + ([] if n is None else ["nx", "ny", "nz"])
    header = ["ply", "format binary_little_endian 1.0", "comment tpgan_amd.mesh", f"element vertex {v.shape[0]}"]
    header += [f"property float {name}" for name in props]
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    rows = v if n is None else np.concatenate([v, n], axis=1)
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


class SequenceMesher:
    """Meshes of a sequence, `pcd_{i:04d}.ply` (or .obj) in `out_dir`.  `push(frames, first)`: frames = list of (n_t,3)
    clouds, first = index of the first one -> one record per frame (frame, points, vertices, faces, volume, area), also
    appended to `records`."""

    def __init__(self, out_dir, fmt="ply", spacing=analysis.BASE_RADIUS, support=None, step=None, iso=0.5, device="cuda",
                 kernel="isotropic", cov_radius=None, smooth_lambda=0.9):
        if fmt not in WRITERS:
            raise ValueError(f"format must be one of {sorted(WRITERS)}")
        if kernel not in KERNELS:
            raise ValueError(f"kernel must be one of {KERNELS}")
        self.out_dir, self.fmt, self.device = out_dir, fmt, torch.device(device)
        self.spacing, self.support, self.step, self.iso = spacing, support, step, iso
        self.kernel, self.cov_radius, self.smooth_lambda = kernel, cov_radius, smooth_lambda
        self.records = []
        os.makedirs(out_dir, exist_ok=True)

    def push(self, frames, first):
        out = []
        for t, frame in enumerate(frames):
            p = torch.as_tensor(frame).detach().float().reshape(-1, 3).to(self.device)
            m = surface_mesh(p, self.spacing, self.support, self.step, self.iso, kernel=self.kernel,
                             cov_radius=self.cov_radius, smooth_lambda=self.smooth_lambda)
            WRITERS[self.fmt](os.path.join(self.out_dir, f"pcd_{first + t:04d}.{self.fmt}"), m)
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


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m tpgan_amd.mesh",
                                 description="Mesh the fluid surface of a sequence of frames to PLY / OBJ files.")
    ap.add_argument("--frames", required=True, help="frame files, '{i}' = frame index, e.g. 'out/pcd_{i}.npy'")
    ap.add_argument("--count", type=int, required=True, help="frames 0 .. count-1")
    ap.add_argument("--out", required=True, help="output directory for pcd_{i:04d}.ply")
    add_mesh_options(ap)
    ap.add_argument("--stats", default=None, metavar="FILE.npz", help="per-frame volume, area and their first differences")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    if "{i}" not in a.frames:
        ap.error("--frames must contain '{i}'")
    if a.count < 1:
        ap.error("--count must be at least 1")
    seq = mesher_from(a, a.out, a.device)
    for i in range(a.count):
        for record in seq.push([render.load_frame(a.frames.format(i=i))], i):
            print(json.dumps(record), flush=True)
    if a.stats:
        np.savez(a.stats, **seq.stats())


if __name__ == "__main__":
    main()
