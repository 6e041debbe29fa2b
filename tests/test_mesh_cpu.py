"""Surface meshing without a GPU: known answers, topology and geometry of the numpy statement of the isosurface rule
(tests/iso_rule.py), `ops._iso_surface_torch` against it bit for bit, the three C entries' argument checks, and the host
layers of tpgan_amd.mesh (lattice, density field, measurements, PLY / OBJ files, the CLI, rollout's --mesh) against the
oracle backend."""
import ctypes as C
import functools
import json
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iso_cases as K  # noqa: E402
import iso_rule as R  # noqa: E402

F32 = np.float32


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def coordinates(shape, origin, step=1.0):
    ax = [F32(origin[a]) + np.arange(shape[a], dtype=F32) * F32(step) for a in range(3)]
    return np.meshgrid(*ax, indexing="ij")


@functools.lru_cache(maxsize=None)
def sphere(radius):
    """R^2 - |x|^2 on an off-centre lattice of step 1 -> (vertices, faces, normals), computed once."""
    n = 2 * radius + 8
    origin = np.array([-n / 2 + 0.3, -n / 2 + 0.2, -n / 2 + 0.1], dtype=F32)
    X, Y, Z = coordinates((n, n, n), origin)
    field = (F32(radius * radius) - (X * X + Y * Y + Z * Z)).astype(F32)
    return R.iso_surface(field, origin, 1.0, 0.0)


# ---- the rule: known answers and topology -------------------------------------------------------------------------------
def test_one_inside_node_is_an_octahedron_like_cell_of_half_a_cube():
    f = np.zeros((5, 5, 5), F32)
    f[2, 2, 2] = 1.0
    for step in (1.0, 0.25):
        v, faces, n = R.iso_surface(f, (0.5, -1.0, 2.0), step, 0.5)
        assert v.shape == (14, 3) and faces.shape == (24, 3) and n.shape == (14, 3)
        assert abs(R.volume(v, faces) - 0.5 * step ** 3) < 1e-6 * step ** 3
        assert R.is_closed_oriented(faces, 14) and R.euler_characteristic(faces, 14) == 2
        centre = np.array([0.5, -1.0, 2.0]) + 2 * step
        out = v.astype(np.float64) - centre
        # the six vertices on the axes have unit normals pointing away from the node; on the eight diagonal edges both
        # ends' central differences vanish (the neighbours two nodes apart are all 0): len == 0 gives (0,0,0)
        length = np.linalg.norm(n.astype(np.float64), axis=1)
        axis = (np.abs(out) > 1e-9).sum(1) == 1
        assert axis.sum() == 6 and np.array_equal(length[axis], np.ones(6)) and np.array_equal(length[~axis], np.zeros(8))
        assert (np.einsum("ij,ij->i", n.astype(np.float64), out)[axis] > 0).all()
        assert not np.signbit(n[~axis]).any()


def test_the_three_winding_tables_agree():
    from tpgan_amd import ops
    _, flips = R.winding_table()
    assert np.array_equal(np.array(ops.iso_winding_table(), dtype=bool), flips)
    assert [list(map(tuple, p)) for p in R.tet_paths().tolist()] == [list(p) for p in ops.iso_tetrahedra()]
    # all six tetrahedra share the main diagonal, and every edge is one of the seven directions
    for path in R.tet_paths():
        assert tuple(path[0]) == (0, 0, 0) and tuple(path[3]) == (1, 1, 1)
        for a in range(4):
            for b in range(a + 1, 4):
                assert (R.D == path[b] - path[a]).all(1).any()


def test_a_random_interior_is_closed_and_consistently_oriented():
    rng = np.random.default_rng(5)
    f = np.full((12, 9, 11), -1.0, F32)
    f[1:-1, 1:-1, 1:-1] = rng.uniform(-1, 1, size=(10, 7, 9)).astype(F32)
    v, faces, _ = R.iso_surface(f, (0, 0, 0), 1.0, 0.0)
    assert faces.shape[0] > 1000 and R.is_closed_oriented(faces, v.shape[0])
    assert R.volume(v, faces) > 0.0
    assert np.unique(faces).shape[0] == v.shape[0]                               # every vertex is used


def test_euler_characteristics():
    v, faces, _ = sphere(8)
    assert R.euler_characteristic(faces, v.shape[0]) == 2 and R.is_closed_oriented(faces, v.shape[0])
    origin = np.array([-15.7, -7.8, -8.1], F32)
    X, Y, Z = coordinates((32, 16, 16), origin)
    two = np.maximum(25.0 - ((X + 7.5) ** 2 + Y * Y + Z * Z), 25.0 - ((X - 7.5) ** 2 + Y * Y + Z * Z)).astype(F32)
    v, faces, _ = R.iso_surface(two, origin, 1.0, 0.0)
    assert R.euler_characteristic(faces, v.shape[0]) == 4 and R.is_closed_oriented(faces, v.shape[0])
    origin = np.array([-11.6, -11.7, -5.8], F32)
    X, Y, Z = coordinates((24, 24, 12), origin)
    torus = (9.0 - ((np.sqrt(X * X + Y * Y) - 7.0) ** 2 + Z * Z)).astype(F32)       # major radius 7, minor radius 3
    v, faces, _ = R.iso_surface(torus, origin, 1.0, 0.0)
    assert R.euler_characteristic(faces, v.shape[0]) == 0 and R.is_closed_oriented(faces, v.shape[0])


# ---- the rule: sphere geometry --------------------------------------------------------------------------------------------
def sphere_bounds(radius, step=1.0):
    """Linear interpolation of a quadratic along an edge of at most sqrt(3) s moves the root radially by L^2 / (8 R) to
    first order: delta_1 = 3 s^2 / (8 R); the factor 2 covers the dropped higher-order terms."""
    d1 = 3.0 * step * step / (8.0 * radius)
    d = 2.0 * d1
    return d1, d, 4.0 * np.pi * (radius + d) ** 2 * d


@pytest.mark.parametrize("radius", [8, 16])
def test_sphere_vertices_and_volume(radius):
    v, faces, n = sphere(radius)
    d1, d, vol_bound = sphere_bounds(radius)
    r = np.linalg.norm(v.astype(np.float64), axis=1)
    print(f"R = {radius}: max |r - R| = {np.abs(r - radius).max() / d1:.4f} delta_1")
    assert np.abs(r - radius).max() <= d
    err = R.volume(v, faces) - 4.0 * np.pi * radius ** 3 / 3.0
    print(f"R = {radius}: volume error {err:.3f} ({100 * err / (4 * np.pi * radius ** 3 / 3):.3f} %), bound {vol_bound:.3f}")
    assert abs(err) <= vol_bound
    radial = v.astype(np.float64) / r[:, None]
    assert np.einsum("ij,ij->i", n.astype(np.float64), radial).min() > 0.999       # the field's gradient is radial


def test_sphere_volume_error_is_second_order():
    err = []
    for radius in (8, 16):
        v, faces, _ = sphere(radius)
        exact = 4.0 * np.pi * radius ** 3 / 3.0
        err.append(abs(R.volume(v, faces) - exact) / exact)
    print("relative volume errors at R = 8 s, 16 s:", err)
    assert err[1] * 3.0 <= err[0]


# ---- the rule: edge cases -------------------------------------------------------------------------------------------------
def test_values_equal_to_iso_give_t_zero_and_zero_area_faces_on_a_closed_surface():
    rng = np.random.default_rng(11)
    f = np.full((8, 8, 8), -1.0, F32)
    f[2:6, 2:6, 2:6] = rng.uniform(0.5, 1.0, size=(4, 4, 4)).astype(F32)
    f[3, 3, 1] = 0.25                                                            # exactly iso, its neighbours outside
    f[6, 4, 4] = 0.25                                                            # exactly iso beside the block
    v, faces, n = R.iso_surface(f, (0, 0, 0), 1.0, 0.25)
    assert R.is_closed_oriented(faces, v.shape[0])
    at_node = (v == np.array([3, 3, 1], F32)).all(1)
    assert at_node.sum() >= 7                                                     # t == 0: the vertices sit ON the node
    a, b, c = (v[faces[:, k]].astype(np.float64) for k in range(3))
    areas = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    assert (areas == 0).sum() > 0 and (areas > 0).sum() > 0
    assert np.isfinite(v).all()


def test_nan_nodes_are_outside_and_no_index_leaves_the_range():
    rng = np.random.default_rng(12)
    f = rng.uniform(-1, 1, size=(7, 6, 5)).astype(F32)
    holes = rng.random(f.shape) < 0.1
    g = f.copy()
    g[holes] = np.nan
    g[1, 1, 1] = np.inf
    v, faces, n = R.iso_surface(g, (0, 0, 0), 1.0, 0.0)
    assert faces.shape[0] > 0 and faces.min() >= 0 and faces.max() < v.shape[0]
    below = np.where(holes, F32(-1.0), f)
    below[1, 1, 1] = 1.0
    v2, faces2, _ = R.iso_surface(below, (0, 0, 0), 1.0, 0.0)                     # the same inside flags: the same indices
    assert np.array_equal(faces, faces2) and v.shape == v2.shape


def test_a_dimension_of_one_gives_an_empty_mesh():
    for shape in ((1, 5, 5), (5, 1, 5), (5, 5, 1), (0, 3, 3)):
        v, faces, n = R.iso_surface(np.ones(shape, F32), (0, 0, 0), 1.0, 0.5)
        assert v.shape == (0, 3) and faces.shape == (0, 3) and n.shape == (0, 3)


# ---- the torch statement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", K.FIELDS)
@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_torch_statement_equals_the_rule(shape, kind):
    from tpgan_amd import ops
    f = K.field(shape, kind)
    rv, rf, rn = R.iso_surface(f, K.ORIGIN, K.STEP, K.ISO)
    v, faces, n = ops._iso_surface_torch(torch.from_numpy(f), K.ORIGIN, float(K.STEP), float(K.ISO), True)
    if K.is_empty(shape, kind):
        assert rf.shape[0] == 0 and rv.shape[0] == 0
    else:
        assert rf.shape[0] > 0
    assert tuple(v.shape) == rv.shape and tuple(faces.shape) == rf.shape and faces.dtype == torch.int32
    assert np.array_equal(bits(v), bits(rv)) and np.array_equal(bits(n), bits(rn))
    assert np.array_equal(R.rotate_smallest_first(faces.numpy()), R.rotate_smallest_first(rf))


def test_iso_surface_dispatch_and_validation(oracle_cpu):
    from tpgan_amd import ops
    f = torch.from_numpy(K.field((9, 7, 5), "random"))
    v, faces, n = ops.iso_surface(f, K.ORIGIN, K.STEP, K.ISO)
    rv, rf, rn = R.iso_surface(f.numpy(), K.ORIGIN, K.STEP, K.ISO)
    assert np.array_equal(bits(v), bits(rv)) and np.array_equal(bits(n), bits(rn)) and faces.shape[0] == rf.shape[0] > 0
    assert ops.iso_surface(f, K.ORIGIN, K.STEP, K.ISO, normals=False)[2] is None
    v, faces, n = ops.iso_surface(torch.ones(4, 1, 4), K.ORIGIN, K.STEP, K.ISO)
    assert v.shape == (0, 3) and faces.shape == (0, 3) and faces.dtype == torch.int32 and n.shape == (0, 3)
    for match, kw in [("step", dict(step=0.0)), ("step", dict(step=float("nan"))), ("iso", dict(iso=float("inf"))),
                      ("origin", dict(origin=(0.0, 1.0))), ("origin", dict(origin=(0.0, float("nan"), 0.0))),
                      ("float tensor", dict(field=f.double())), ("3 dims", dict(field=f[0]))]:
        args = dict(field=f, origin=K.ORIGIN, step=K.STEP, iso=K.ISO)
        args.update(kw)
        with pytest.raises(RuntimeError, match=match):
            ops.iso_surface(**args)
    with pytest.raises(RuntimeError, match="2\\^27"):                          # 2^27 + 1 nodes; a meta tensor holds no memory
        ops.iso_surface(torch.empty((9, 9, 1657009), device="meta"), K.ORIGIN, K.STEP, K.ISO)


def test_cpu_tensors_are_refused_without_a_checker():
    from tpgan_amd import mesh, ops
    ops.unregister_backend("cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.iso_surface(torch.zeros(4, 4, 4), (0, 0, 0), 1.0, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.iso_surface(torch.zeros(4, 1, 4), (0, 0, 0), 1.0, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.surface_mesh(torch.zeros(8, 3))


# ---- the C entries' argument checks: no device is touched ---------------------------------------------------------------
def test_iso_entries_reject_bad_arguments_before_any_launch(hip_lib):
    buf = (C.c_float * 256)()
    base = C.addressof(buf)
    p = C.c_void_p((base + 255) & ~255)                                           # 256-byte aligned, 512 bytes behind it
    odd = C.c_void_p(p.value + 64)
    origin = np.zeros(3, np.float32)
    nan, inf = float("nan"), float("inf")
    big = (9, 9, 1657009)                                                         # 2^27 + 1 nodes
    assert 9 * 9 * 1657009 == (1 << 27) + 1
    assert hip_lib.tpg_iso_workspace_bytes(*big) == 0 and hip_lib.tpg_iso_workspace_bytes(4, 1, 4) == 0
    assert hip_lib.tpg_iso_workspace_bytes(512, 512, 512) >= 10 * (1 << 27)
    nodes = 70 * 33 * 35
    assert 10 * nodes <= hip_lib.tpg_iso_workspace_bytes(70, 33, 35) <= 10 * (nodes + 2048) + 8 * 64

    def count(field=p, shape=(4, 4, 4), iso=0.5, ws=p, counts=p):
        return hip_lib.tpg_iso_count_f32(field, *shape, iso, ws, counts, None)
    assert count(counts=None) == -1 and count(iso=nan) == -1 and count(iso=inf) == -1
    assert count(shape=(-1, 4, 4)) == -1 and count(shape=(4, 4, -2)) == -1
    assert count(ws=None) == -1 and count(ws=odd) == -1
    assert count(shape=big) == -3 and count(shape=big, ws=None) == -1              # the argument errors come first
    assert count(field=None) == -1

    def emit(field=p, shape=(4, 4, 4), org=origin, step=0.1, iso=0.5, ws=p, V_cap=8, F_cap=8, vertices=p, normals=p, faces=p):
        return hip_lib.tpg_iso_emit_f32(field, *shape, None if org is None else org.ctypes.data, step, iso, ws, V_cap, F_cap,
                                        vertices, normals, faces, None)
    assert emit(org=None) == -1 and emit(org=np.array([0, nan, 0], np.float32)) == -1
    assert emit(step=0.0) == -1 and emit(step=-1.0) == -1 and emit(step=nan) == -1 and emit(step=inf) == -1
    assert emit(iso=nan) == -1 and emit(iso=-inf) == -1
    assert emit(V_cap=-1) == -1 and emit(F_cap=-1) == -1 and emit(shape=(4, -1, 4)) == -1
    assert emit(vertices=None) == -1 and emit(faces=None) == -1
    assert emit(ws=None) == -1 and emit(ws=odd) == -1
    assert emit(shape=(4, 1, 4)) == 0 and emit(shape=(4, 1, 4), ws=None, field=None) == 0       # no cells: nothing to do
    assert emit(shape=big) == -3 and emit(field=None) == -1
    assert emit(V_cap=0, F_cap=0, vertices=None, faces=None, normals=None) == 0                 # nothing wanted


# ---- tpgan_amd.mesh: the host layers, on CPU tensors under the oracle backend ----------------------------------------------
SPACING = 0.025


def test_lattice_for_drops_dummies_pads_and_refuses_huge_lattices(oracle_cpu):
    from tpgan_amd import mesh
    rng = np.random.default_rng(3)
    pts = rng.uniform(-0.2, 0.3, size=(50, 3)).astype(F32)
    rows = np.concatenate([pts, np.full((4, 3), 999.0, F32), [[np.nan, 0, 0]], [[0, np.inf, 0]], [[0.0, 0.0, -950.0]]]).astype(F32)
    support, step = 0.05, 0.0125
    lat = mesh.lattice_for(torch.from_numpy(rows), support, step)
    clean = mesh.lattice_for(torch.from_numpy(pts), support, step)
    assert np.array_equal(lat.origin, clean.origin) and lat.shape == clean.shape and lat.step == clean.step
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    pad = support + 2 * step
    last = lat.origin.astype(np.float64) + (np.array(lat.shape) - 1) * float(lat.step)
    assert lat.origin.dtype == np.float32 and lat.step == float(F32(step))
    assert (np.abs(lat.origin - (lo - pad)) <= 1e-6).all() and (last >= hi + pad - 1e-6).all()
    assert (last - (hi + pad) < step + 1e-6).all()                                 # and no wider than needed
    lengths = mesh.lattice_for(torch.from_numpy(rows), support, step, lengths=20)
    assert lengths.shape != lat.shape or not np.array_equal(lengths.origin, lat.origin)
    first = mesh.lattice_for(torch.from_numpy(pts[:20]), support, step)
    assert lengths.shape == first.shape and np.array_equal(lengths.origin, first.origin)
    # the field vanishes on the boundary layer, and on the layer inside it
    field = mesh.density_field(torch.from_numpy(rows), lat, support)
    assert tuple(field.shape) == lat.shape and field.dtype == torch.float32 and float(field.max()) >= 1.0
    inner = field[2:-2, 2:-2, 2:-2]
    outer = field.clone()
    outer[2:-2, 2:-2, 2:-2] = 0.0
    assert float(outer.abs().max()) == 0.0 and float(inner.max()) > 0.0
    wide = torch.tensor([[0.0, 0.0, 0.0], [10.0, 10.0, 10.0]])
    with pytest.raises(RuntimeError, match="would fit") as info:
        mesh.lattice_for(wide, support, step)
    fit = float(str(info.value).split("a step of ")[1].split(" ")[0])
    ok = mesh.lattice_for(wide, support, fit)
    assert step < fit < 0.05 and np.prod(np.array(ok.shape, dtype=np.float64)) <= (1 << 27)
    with pytest.raises(RuntimeError, match="no valid point"):
        mesh.lattice_for(torch.full((3, 3), 999.0), support, step)


def test_lattice_value_is_the_full_lattice_sum():
    from tpgan_amd import mesh
    r = np.arange(-3, 4) * SPACING
    d = np.sqrt(r[:, None, None] ** 2 + r[None, :, None] ** 2 + r[None, None, :] ** 2) / (2 * SPACING)
    w = np.where(d <= 0.5, 6 * (d ** 3 - d ** 2) + 1, 2 * np.clip(1 - d, 0, None) ** 3)
    assert abs(mesh.lattice_value(SPACING, 2 * SPACING) - w.sum()) < 1e-12
    assert 3.0 < mesh.lattice_value(SPACING, 2 * SPACING) < 6.0
    assert mesh.lattice_value(SPACING, 0.5 * SPACING) == 1.0                      # only the particle itself


def half_space_offset(spacing, support, level):
    """Where, beyond the face of a half space filled with one particle per spacing^3, the cubic density of width
    `support` falls to `level`: the root x of M(x) / spacing^3 = level, M(x) = the kernel's mass beyond a plane at
    distance x from its centre = int_x^h 2 pi (int_z^h w(r / h) r dr) dz, in float64 by the midpoint rule + bisection."""
    h, n = support, 4000
    r = (np.arange(n) + 0.5) * h / n
    q = r / h
    w = np.where(q <= 0.5, 6 * (q ** 3 - q ** 2) + 1, 2 * (1 - q) ** 3)
    ring = 2 * np.pi * w * r * (h / n)
    disc = np.cumsum(ring[::-1])[::-1] - 0.5 * ring                               # A(z) at the midpoints
    cap = np.cumsum((disc * (h / n))[::-1])[::-1] - 0.5 * disc * (h / n)           # M(z) at the midpoints

    def mass(x):                                                                  # M(-x) = total - M(x)
        total = 2 * np.interp(0.0, r, cap)
        m = np.interp(abs(x), r, cap, right=0.0)
        return m if x >= 0 else total - m
    lo, hi = -h, h
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if mass(mid) / spacing ** 3 > level else (lo, mid)
    return 0.5 * (lo + hi)


@functools.lru_cache(maxsize=None)
def ball_mesh():
    from oracle import torch_backend
    from tpgan_amd import mesh
    torch_backend.install()
    try:
        ball = K.lattice_ball(6.2, SPACING)
        rows = np.concatenate([ball, np.full((3, 3), 999.0, F32)])
        return ball, mesh.surface_mesh(torch.from_numpy(rows), SPACING)
    finally:
        torch_backend.uninstall()


def test_a_ball_of_lattice_particles_meshes_to_a_closed_sphere_like_surface():
    from tpgan_amd import mesh
    ball, m = ball_mesh()
    V = m.vertices.shape[0]
    faces = m.faces.numpy()
    assert ball.shape[0] > 900 and faces.shape[0] > 1000
    assert R.is_closed_oriented(faces, V) and R.euler_characteristic(faces, V) == 2
    assert m.lattice.step == float(F32(SPACING / 2)) and m.iso == float(F32(0.5 * mesh.lattice_value(SPACING, 2 * SPACING)))
    assert abs(mesh.volume(m) - R.volume(m.vertices.numpy(), faces)) < 1e-12
    assert abs(mesh.area(m) - R.area(m.vertices.numpy(), faces)) < 1e-12
    centre = ball.astype(np.float64).mean(0)
    out = m.vertices.numpy().astype(np.float64) - centre
    assert np.einsum("ij,ij->i", m.normals.numpy().astype(np.float64), out).min() > 0.0


def test_the_balls_volume_is_that_of_its_sphere():
    """The sphere's radius: the particles' own extent (the furthest particle centre from their centroid) plus the
    level set's analytic offset: where, measured from the face of a continuum of one particle per spacing^3, the cubic
    density falls to the meshed level (`half_space_offset`, derived from `lattice_value`; about -0.0005 spacings,
    since the level is half of a full lattice's density and the kernel is symmetric).  The bound is the sphere bound of
    the rule's tests at the lattice step.  The ball (|z| <= 6.2 spacings, 1 021 particles) was chosen before any run;
    measured: extent 6.1644 s, volume 1.554498e-02 against the sphere's 1.532790e-02, error 2.17e-04 of a bound of
    2.29e-04 -- the staircase of a lattice ball is most of that, the mesher's own error (second order) very little."""
    from tpgan_amd import mesh
    ball, m = ball_mesh()
    centre = ball.astype(np.float64).mean(0)
    extent = np.linalg.norm(ball.astype(np.float64) - centre, axis=1).max()
    offset = half_space_offset(SPACING, 2 * SPACING, 0.5 * mesh.lattice_value(SPACING, 2 * SPACING))
    radius = extent + offset
    _, _, bound = sphere_bounds(radius, m.lattice.step)
    vol, exact = mesh.volume(m), 4.0 * np.pi * radius ** 3 / 3.0
    print(f"extent {extent / SPACING:.4f} s, offset {offset / SPACING:.4f} s, volume {vol:.6e}, sphere {exact:.6e}, "
          f"error {vol - exact:.3e}, bound {bound:.3e}, particles x s^3 {ball.shape[0] * SPACING ** 3:.6e}")
    assert abs(vol - exact) <= bound


# ---- files ----------------------------------------------------------------------------------------------------------------
def read_ply(path):
    """This test's own reader of the binary little-endian PLY files `write_ply` writes."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    counts, props, current = {}, {}, None
    for line in lines[2:]:
        w = line.split()
        if w[:1] == ["element"]:
            current = w[1]
            counts[current] = int(w[2])
            props[current] = []
        elif w[:1] == ["property"]:
            props[current].append(w[1:])
    names = [p[1] for p in props["vertex"]]
    assert all(p[0] == "float" for p in props["vertex"]) and props["face"] == [["list", "uchar", "int", "vertex_indices"]]
    nv, nf = counts["vertex"], counts["face"]
    rows = np.frombuffer(data, dtype="<f4", count=nv * len(names), offset=end).reshape(nv, len(names))
    at = end + 4 * nv * len(names)
    faces = np.zeros((nf, 3), np.int32)
    for i in range(nf):
        n, a, b, c = struct.unpack_from("<Biii", data, at)
        assert n == 3
        faces[i] = (a, b, c)
        at += 13
    assert at == len(data)
    return names, rows, faces


def read_obj(path):
    v, n, faces = [], [], []
    for line in open(path):
        w = line.split()
        if w[:1] == ["v"]:
            v.append([float(x) for x in w[1:]])
        elif w[:1] == ["vn"]:
            n.append([float(x) for x in w[1:]])
        elif w[:1] == ["f"]:
            cols = [x.split("//") for x in w[1:]]
            assert all(len(c) == 1 or c[0] == c[1] for c in cols)
            faces.append([int(c[0]) - 1 for c in cols])
    return np.array(v, F32).reshape(-1, 3), np.array(n, F32).reshape(-1, 3), np.array(faces, np.int32).reshape(-1, 3)


def test_ply_and_obj_files_read_back_to_the_same_arrays(tmp_path):
    from tpgan_amd import mesh
    _, m = ball_mesh()
    mesh.write_ply(str(tmp_path / "a.ply"), m)
    names, rows, faces = read_ply(str(tmp_path / "a.ply"))
    assert names == ["x", "y", "z", "nx", "ny", "nz"]
    assert np.array_equal(bits(rows[:, :3]), bits(m.vertices)) and np.array_equal(bits(rows[:, 3:]), bits(m.normals))
    assert np.array_equal(faces, m.faces.numpy())
    mesh.write_obj(str(tmp_path / "a.obj"), m)
    v, n, f = read_obj(str(tmp_path / "a.obj"))
    assert np.array_equal(bits(v), bits(m.vertices)) and np.array_equal(bits(n), bits(m.normals))
    assert np.array_equal(f, m.faces.numpy())
    bare = m._replace(normals=None)
    mesh.write_ply(str(tmp_path / "b.ply"), bare)
    names, rows, faces = read_ply(str(tmp_path / "b.ply"))
    assert names == ["x", "y", "z"] and np.array_equal(bits(rows), bits(m.vertices)) and np.array_equal(faces, m.faces.numpy())
    mesh.write_obj(str(tmp_path / "b.obj"), bare)
    v, n, f = read_obj(str(tmp_path / "b.obj"))
    assert n.shape[0] == 0 and np.array_equal(bits(v), bits(m.vertices)) and np.array_equal(f, m.faces.numpy())


def test_cli_writes_the_files_and_one_json_line_per_frame(tmp_path, capsys, oracle_cpu):
    from tpgan_amd import analysis, mesh
    small = K.lattice_ball(3.3, SPACING)
    np.save(tmp_path / "pcd_0.npy", small)
    np.save(tmp_path / "pcd_1.npy", np.concatenate([small * F32(1.1), np.full((2, 3), 999.0, F32)]))
    out = tmp_path / "meshes"
    mesh.main(["--frames", str(tmp_path / "pcd_{i}.npy"), "--count", "2", "--out", str(out), "--device", "cpu",
               "--stats", str(tmp_path / "stats.npz")])
    lines = [json.loads(line) for line in capsys.readouterr().out.strip().split("\n")]
    assert [r["frame"] for r in lines] == [0, 1] and all(set(r) == {"frame", "points", "vertices", "faces", "volume", "area"} for r in lines)
    for i, r in enumerate(lines):
        names, rows, faces = read_ply(str(out / f"pcd_{i:04d}.ply"))
        assert r["points"] == small.shape[0] and r["vertices"] == rows.shape[0] > 0 and r["faces"] == faces.shape[0] > 0
        assert abs(r["volume"] - R.volume(rows[:, :3], faces)) < 1e-9 and abs(r["area"] - R.area(rows[:, :3], faces)) < 1e-9
        assert r["volume"] > 0
    assert lines[1]["volume"] > lines[0]["volume"]
    stats = np.load(tmp_path / "stats.npz")
    assert np.allclose(stats["volume"], [r["volume"] for r in lines]) and np.allclose(stats["area"], [r["area"] for r in lines])
    assert np.array_equal(stats["d_volume"], analysis.first_difference(stats["volume"]))
    assert np.array_equal(stats["d_area"], analysis.first_difference(stats["area"]))
    mesh.main(["--frames", str(tmp_path / "pcd_{i}.npy"), "--count", "1", "--out", str(out), "--device", "cpu", "--format", "obj"])
    v, n, f = read_obj(str(out / "pcd_0000.obj"))
    assert v.shape[0] == lines[0]["vertices"] and f.shape[0] == lines[0]["faces"]
    with pytest.raises(SystemExit):
        mesh.main(["--frames", "nothing.npy", "--count", "1", "--out", str(out)])


class _EchoUpsampler:
    """Stands in for the network: every frame comes back as it went in."""

    def __init__(self, net, chunk=None):
        pass

    def push(self, features, positions):
        return [positions[t:t + 1] for t in range(positions.shape[0])]


def _run_rollout(tmp_path, monkeypatch, extra):
    from tpgan_amd import rollout
    monkeypatch.setattr(rollout, "load_generator", lambda checkpoint, in_feats, device: None)
    monkeypatch.setattr(rollout, "SequenceUpsampler", _EchoUpsampler)
    small = K.lattice_ball(3.3, SPACING)
    for i in range(3):
        np.savez(tmp_path / f"data_{i}.npz", pos=small + F32(0.01 * i))
    out = tmp_path / "out"
    rollout.main(["--checkpoint", "none", "--frames", str(tmp_path / "data_{i}.npz"), "--count", "3", "--chunk", "2",
                  "--out", str(out), "--device", "cpu"] + extra)
    return small, out


def test_rollout_without_mesh_is_unchanged(tmp_path, monkeypatch):
    from tpgan_amd import mesh
    called = []
    monkeypatch.setattr(mesh, "mesher_from", lambda *a: called.append(a))
    small, out = _run_rollout(tmp_path, monkeypatch, [])
    assert not called and sorted(os.listdir(out)) == ["pcd_0.npy", "pcd_1.npy", "pcd_2.npy"]
    assert sorted(os.listdir(tmp_path)) == ["data_0.npz", "data_1.npz", "data_2.npz", "out"]
    for i in range(3):
        assert np.abs(np.load(out / f"pcd_{i}.npy") - (small + F32(0.01 * i))).max() < 1e-6


def test_rollout_with_mesh_writes_one_mesh_per_frame(tmp_path, monkeypatch, oracle_cpu):
    small, out = _run_rollout(tmp_path, monkeypatch, ["--mesh", str(tmp_path / "meshes"), "--iso", "0.4"])
    assert sorted(os.listdir(tmp_path / "meshes")) == ["pcd_0000.ply", "pcd_0001.ply", "pcd_0002.ply"]
    names, rows, faces = read_ply(str(tmp_path / "meshes" / "pcd_0002.ply"))
    assert faces.shape[0] > 0 and R.is_closed_oriented(faces, rows.shape[0])
    centre = rows[:, :3].astype(np.float64).mean(0)
    assert np.abs(centre - (small.astype(np.float64).mean(0) + 0.02)).max() < 0.01   # the frame's own coordinates
    assert len(os.listdir(out)) == 3
