"""What a surface mesh of a frame costs (`tpgan_amd.mesh`, `ops.iso_surface`, csrc/isosurface.hip).  GPU box.

Two frames:
  scene    the simulator's default scene (`simulate.random_scene(1)`, 61 445 particles, the scene of profiles/simulate.txt)
           after WARM frames, meshed at the defaults (spacing 0.025, support 0.05, step 0.0125)
  dense    a jittered lattice block of about 5 * 10^5 points at spacing 0.0125, the size of an 8x upsampled frame, meshed
           at --spacing 0.0125 (support 0.025, step 0.00625)
Per frame, wall ms (host clock around a call that ends in a device synchronise, median of the repeats after a warm-up):
  field      `mesh.lattice_for` + `mesh.density_field` (the dense evaluation of `ops.radius_reduce` at every node)
  count      tpg_iso_count_f32 and the host read of the two totals
  emit       tpg_iso_emit_f32 into fresh buffers
  download   vertices, normals and faces to the host
  write      `mesh.write_ply` of the downloaded mesh to a temporary directory
beside `render.render_surface` of the same frame (768 x 768, on the device, and with the download and `write_png`), and
for the scene the numpy statement of the rule (tests/iso_rule.py) on the host, on as many x-layers of the same field as
hold at most 4 * 10^6 nodes, which must EQUAL the device's mesh of those layers or the tool fails.

    python tools/mesh_time.py [--repeats 10 --warm 12] [--out profiles/mesh.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import tpgan_amd  # noqa: F401
from tpgan_amd import mesh, ops, render
from tpgan_amd import simulate as S

EXTENT = 768


def wall_ms(fn, dev):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) * 1e3, out


def median_ms(fn, dev, repeats):
    fn()                                                             # warm-up: code objects, workspaces
    runs = [wall_ms(fn, dev) for _ in range(repeats)]
    return statistics.median(r[0] for r in runs), runs[-1][1]


def scene_frame(dev, warm):
    state = S.pack([S.random_scene(1)], dev)
    for _ in range(warm):
        x, v, lengths, lo, hi = state
        for _ in range(S.SUBSTEPS):
            x, v = ops.pbf_substep(x, v, lengths, lo, hi, 1.0 / (S.FPS * S.SUBSTEPS))
        state = (x, v, lengths, lo, hi)
    n = int(state[2][0]) if state[2] is not None else state[0].shape[1]
    return state[0][0, :n].contiguous()


def dense_frame(dev, spacing):
    rng = np.random.default_rng(7)
    ax = [np.arange(n) * spacing for n in (100, 50, 100)]
    p = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    p = p + rng.uniform(-0.2, 0.2, size=p.shape) * spacing
    return torch.from_numpy(p.astype(np.float32)).to(dev)


def measure(points, spacing, dev, repeats, tmp):
    support, step = 2.0 * spacing, spacing / 2.0
    level = float(np.float32(0.5 * mesh.lattice_value(spacing, support)))
    be = ops.backend_for(points)

    def field_():
        lattice = mesh.lattice_for(points, support, step)
        return lattice, mesh.density_field(points, lattice, support)
    t_field, (lattice, field) = median_ms(field_, dev, repeats)
    t_count, (ws, V, F) = median_ms(lambda: be.iso_count(field, level), dev, repeats)

    def emit_():
        v = torch.empty((V, 3), dtype=torch.float32, device=dev)
        n = torch.empty((V, 3), dtype=torch.float32, device=dev)
        f = torch.empty((F, 3), dtype=torch.int32, device=dev)
        be.iso_emit(field, lattice.origin, lattice.step, level, ws, V, F, v, n, f)
        return mesh.Mesh(v, f, n, lattice, level)
    t_emit, m = median_ms(emit_, dev, repeats)
    t_down, host = median_ms(lambda: m._replace(vertices=m.vertices.cpu(), faces=m.faces.cpu(), normals=m.normals.cpu()),
                             dev, repeats)
    t_write, _ = median_ms(lambda: mesh.write_ply(os.path.join(tmp, "frame.ply"), host), dev, repeats)
    t_all, _ = median_ms(lambda: mesh.surface_mesh(points, spacing), dev, repeats)
    size = os.path.getsize(os.path.join(tmp, "frame.ply"))

    camera = render.Camera.fit(points, width=EXTENT, height=EXTENT)
    batch = points.unsqueeze(0)
    t_pic, image = median_ms(lambda: render.render_surface(batch, camera, spacing), dev, repeats)
    t_png, _ = median_ms(lambda: render.write_png(os.path.join(tmp, "frame.png"),
                                                  render.render_surface(batch, camera, spacing)[0].cpu()), dev, repeats)
    nodes = lattice.shape[0] * lattice.shape[1] * lattice.shape[2]
    lines = [f"  points {points.shape[0]}, lattice {lattice.shape[0]} x {lattice.shape[1]} x {lattice.shape[2]} = {nodes} nodes "
             f"at step {lattice.step:g}, vertices {V}, faces {F}, volume {mesh.volume(m):.5f}, area {mesh.area(m):.4f}, "
             f"PLY {size / 1e6:.1f} MB",
             f"  field    {t_field:9.3f}", f"  count    {t_count:9.3f}", f"  emit     {t_emit:9.3f}",
             f"  download {t_down:9.3f}", f"  write    {t_write:9.3f}",
             f"  sum      {t_field + t_count + t_emit + t_down + t_write:9.3f}   (field: "
             f"{t_field / (t_field + t_count + t_emit + t_down + t_write):.2f} of it)",
             f"  mesh.surface_mesh, one call, on the device {t_all:9.3f}",
             f"  render_surface {EXTENT} x {EXTENT}, on the device   {t_pic:9.3f}",
             f"  render_surface + download + write_png        {t_png:9.3f}"]
    return lines, field, lattice, level, host


HOST_NODES = 4_000_000


def host_rule_line(field, lattice, level):
    """The numpy statement on the first x-layers of the field that hold at most HOST_NODES nodes (a lattice small enough
    to finish), against the device's mesh of the same layers."""
    import iso_rule as R
    nx, ny, nz = lattice.shape
    layers = max(2, min(nx, HOST_NODES // (ny * nz)))
    part = field[:layers].contiguous()
    dv, df, dn = (t.cpu().numpy() for t in ops.iso_surface(part, lattice.origin, lattice.step, level))
    f = part.cpu().numpy()
    t = time.perf_counter()
    v, faces, n = R.iso_surface(f, lattice.origin, lattice.step, level)
    ms = (time.perf_counter() - t) * 1e3
    same = (np.array_equal(v.view(np.int32), dv.view(np.int32)) and np.array_equal(n.view(np.int32), dn.view(np.int32))
            and np.array_equal(R.rotate_smallest_first(faces), R.rotate_smallest_first(df)))
    assert same and faces.shape[0] > 0, "the numpy statement and the device disagree"
    return (f"  numpy statement of the rule on the host, {layers} x {ny} x {nz} = {layers * ny * nz} nodes of the same field, "
            f"{faces.shape[0]} faces: {ms:.0f} ms (one run), equal to the device's mesh bit for bit")


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
    with tempfile.TemporaryDirectory() as tmp:
        lines.append("scene: the simulator's default scene, spacing 0.025")
        got, field, lattice, level, host = measure(scene_frame(dev, a.warm), 0.025, dev, a.repeats, tmp)
        lines += got + [host_rule_line(field, lattice, level)]
        del field, host
        lines.append("dense: a jittered lattice block, spacing 0.0125")
        lines += measure(dense_frame(dev, 0.0125), 0.0125, dev, a.repeats, tmp)[0]
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
