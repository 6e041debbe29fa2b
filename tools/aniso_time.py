"""What the anisotropic surface kernels cost beside the isotropic field (`tpgan_amd.mesh`, csrc/aniso.hip).  GPU box.

The two frames of tools/mesh_time.py:
  scene    the simulator's default scene (`simulate.random_scene(1)`, 61 445 particles) after WARM frames, meshed at the
           defaults (spacing 0.025, support 0.05, step 0.0125, cov_radius 0.1)
  dense    a jittered lattice block of about 5 * 10^5 points at spacing 0.0125, meshed at --spacing 0.0125
Per frame, wall ms (host clock around a call that ends in a device synchronise, median of the repeats after a warm-up):
  iso field     `mesh.lattice_for` + `mesh.density_field`, the isotropic field, in the same run
  A walk        tpg_aniso_kernels_f32, stages = 1: the grid build over the particles and the ten neighbourhood sums
  A finish      stages = 2: the float64 finish, one lane per particle
  B build       tpg_aniso_field_f32 with ONE query: the second grid build (over the smoothed centres) and one wave
  aniso field   `mesh.lattice_for` (padded by s_max * support) + the field at every node with the kernels of stage A
                given (each call of NODES_PER_CALL nodes builds the grid again)
  count, emit   tpg_iso_count_f32 / tpg_iso_emit_f32 on the anisotropic field
and `mesh.surface_mesh` as one call, both ways, with the vertices, faces, `mesh.volume` and `mesh.area` of both meshes:
the shrinkage of the anisotropic surface as a number.

    python tools/aniso_time.py [--repeats 10 --warm 12] [--out profiles/aniso.txt]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import tpgan_amd  # noqa: F401
from mesh_time import dense_frame, median_ms, scene_frame
from tpgan_amd import mesh, ops


def measure(points, spacing, dev, repeats):
    support, step = 2.0 * spacing, spacing / 2.0
    rc, s_max = 2.0 * support, mesh.ANISO_S_MAX
    level = float(np.float32(0.5 * mesh.lattice_value(spacing, support)))
    be = ops.backend_for(points)
    prm = ops._aniso_params(rc, 1.0 / mesh.lattice_covariance(spacing, rc), 0.9, 4.0, 0.125, s_max, 0.5, 25)
    batch = points.unsqueeze(0)

    def iso_field():
        lattice = mesh.lattice_for(points, support, step)
        return lattice, mesh.density_field(points, lattice, support)
    t_iso, (iso_lattice, iso) = median_ms(iso_field, dev, repeats)
    out = be.aniso_kernels(batch, None, prm, True)
    t_walk, _ = median_ms(lambda: be.aniso_kernels(batch, None, prm, True, stages=1, out=out), dev, repeats)
    t_finish, _ = median_ms(lambda: be.aniso_kernels(batch, None, prm, True, stages=2, out=out), dev, repeats)
    whole = be.aniso_kernels(batch, None, prm, True)
    assert all(torch.equal(a, b) for a, b in zip(out, whole)), "the two stages one by one and in one call disagree"
    centres, G, det, count = (t[0] for t in out)
    reach = float(np.float32(s_max) * np.float32(support))
    one = points[:1].unsqueeze(0).contiguous()
    t_build, _ = median_ms(lambda: be.aniso_field(one, out[0], out[1], out[2], None, None, float(np.float32(support)), reach, True),
                           dev, repeats)

    def aniso_field():
        lattice = mesh.lattice_for(points, support, step, reach=s_max * support)
        nx, ny, nz = lattice.shape
        field = torch.empty(nx * ny * nz, dtype=torch.float32, device=dev)
        for first in range(0, field.shape[0], mesh.NODES_PER_CALL):
            n = min(mesh.NODES_PER_CALL, field.shape[0] - first)
            nodes = mesh.lattice_nodes(lattice, first, n, dev)
            field[first:first + n] = ops.anisotropic_field(nodes, centres, G, det, support, s_max)
        return lattice, field.view(nx, ny, nz)
    t_field, (lattice, field) = median_ms(aniso_field, dev, repeats)
    t_count, (ws, V, F) = median_ms(lambda: be.iso_count(field, level), dev, repeats)

    def emit():
        v = torch.empty((V, 3), dtype=torch.float32, device=dev)
        n = torch.empty((V, 3), dtype=torch.float32, device=dev)
        f = torch.empty((F, 3), dtype=torch.int32, device=dev)
        be.iso_emit(field, lattice.origin, lattice.step, level, ws, V, F, v, n, f)
        return mesh.Mesh(v, f, n, lattice, level)
    t_emit, m_aniso = median_ms(emit, dev, repeats)
    t_all_iso, m_iso = median_ms(lambda: mesh.surface_mesh(points, spacing), dev, repeats)
    t_all, m_all = median_ms(lambda: mesh.surface_mesh(points, spacing, kernel="anisotropic"), dev, repeats)
    assert torch.equal(m_all.vertices, m_aniso.vertices) and torch.equal(m_all.faces, m_aniso.faces)

    def nodes_of(lat):
        return lat.shape[0] * lat.shape[1] * lat.shape[2]
    few = int((count <= 25).sum())
    lines = [f"  points {points.shape[0]}; neighbours within cov_radius {rc:g}: median {int(count.median())}, max {int(count.max())}, "
             f"{few} particles at or below n_eps",
             f"  isotropic    lattice {' x '.join(map(str, iso_lattice.shape))} = {nodes_of(iso_lattice)} nodes, "
             f"vertices {m_iso.vertices.shape[0]}, faces {m_iso.faces.shape[0]}, volume {mesh.volume(m_iso):.5f}, area {mesh.area(m_iso):.4f}",
             f"  anisotropic  lattice {' x '.join(map(str, lattice.shape))} = {nodes_of(lattice)} nodes, "
             f"vertices {V}, faces {F}, volume {mesh.volume(m_aniso):.5f}, area {mesh.area(m_aniso):.4f}",
             f"  iso field    {t_iso:9.3f}",
             f"  A walk       {t_walk:9.3f}", f"  A finish     {t_finish:9.3f}", f"  B build      {t_build:9.3f}",
             f"  aniso field  {t_field:9.3f}   ({t_field / t_iso:.1f} x the isotropic field)",
             f"  count        {t_count:9.3f}", f"  emit         {t_emit:9.3f}",
             f"  mesh.surface_mesh, one call, isotropic   {t_all_iso:9.3f}",
             f"  mesh.surface_mesh, one call, anisotropic {t_all:9.3f}"]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warm", type=int, default=12, help="simulated frames before the scene's frame is taken")
    ap.add_argument("--commit", default=None, help="the commit the times are taken on (default: git's HEAD)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda", 0)
    commit = a.commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                        text=True).stdout.strip()
    lines = [f"# {torch.cuda.get_device_name(0)}; commit {commit or 'unknown'}; wall ms per frame = host clock + synchronise, "
             f"median of {a.repeats} after a warm-up"]
    lines.append("scene: the simulator's default scene, spacing 0.025")
    lines += measure(scene_frame(dev, a.warm), 0.025, dev, a.repeats)
    lines.append("dense: a jittered lattice block, spacing 0.0125")
    lines += measure(dense_frame(dev, 0.0125), 0.0125, dev, a.repeats)
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
