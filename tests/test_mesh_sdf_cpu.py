"""The signed distance to a triangle mesh without a GPU: the torch statement against the numpy rule (tests/mesh_sdf_rule.py)
bit for bit on the cases of tests/mesh_sdf_cases.py, planted defects that each case must see, the sign against two
independent yardsticks (an analytic torus, an analytic box), the magnitude against the analytic box, the C entry's
argument checks, and the host layer of tpgan_amd.mesh: readers, the closedness check, the generators."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_sdf_cases as K  # noqa: E402
import mesh_sdf_rule as R  # noqa: E402

F32 = np.float32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.int32)


def _torch(case):
    from tpgan_amd import ops
    box, inv_unit = ops.mesh_sdf_grid(case["vertices"])
    d, f = ops._mesh_sdf_torch(_t(case["query"]), _t(case["vertices"]), _t(case["faces"]), box, inv_unit)
    return d.numpy(), f.numpy()


@pytest.fixture(scope="module")
def tiling():
    return K.tiling_cases()


# ---- the statement against the rule -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.CASES))
def test_torch_statement_equals_the_rule_bit_for_bit(name):
    case = K.CASES[name]()
    wd, wf = R.mesh_sdf_rule(**case)
    d, f = _torch(case)
    assert d.dtype == F32 and f.dtype == np.int32
    assert np.array_equal(_bits(d), _bits(wd)) and np.array_equal(f, wf), name


@pytest.mark.parametrize("key", [(1, 257), (256, 256), (257, 1000), (773, 1000)])
def test_torch_statement_equals_the_rule_on_the_tiling_meshes(tiling, key):
    from tpgan_amd import ops
    case = tiling[key]
    wd, wf = R.mesh_sdf_rule(**case)
    d, f = _torch(case)
    assert np.array_equal(_bits(d), _bits(wd)) and np.array_equal(f, wf)
    box, inv_unit = ops.mesh_sdf_grid(case["vertices"])
    d, f = ops._mesh_sdf_torch(_t(case["query"]), _t(case["vertices"]), _t(case["faces"]), box, inv_unit, pairs_per_chunk=7000)
    assert np.array_equal(_bits(d.numpy()), _bits(wd)) and np.array_equal(f.numpy(), wf)      # another split of the faces


def test_the_snap_grid_of_the_op_is_the_rules():
    from tpgan_amd import ops
    rng = np.random.default_rng(3)
    for scale in (1.0, 3.0, 2.0 ** -16, 65536.0, 0.7, 1e-3, 123.456):
        v = (rng.uniform(-1, 1, (20, 3)) * scale + rng.uniform(-5, 5, 3)).astype(F32)
        (box, inv_unit), (wbox, winv) = ops.mesh_sdf_grid(v), R.grid_of(v)
        assert np.array_equal(box, wbox) and inv_unit == winv
        ext = float((box[3:].astype(np.float64) - box[:3]).max())
        assert 1.0 / inv_unit >= ext / 65536 > 0.5 / inv_unit                     # the smallest such power of two
    v = np.array([[0, 0, 0], [2, 1, 0.5]], F32)                                   # an extent that IS 2^16 units of 2^-15
    assert ops.mesh_sdf_grid(v)[1] == 2.0 ** 15 == R.grid_of(v)[1]
    assert ops.mesh_sdf_grid(np.ones((3, 3), F32))[1] == 1.0 == R.grid_of(np.ones((3, 3), F32))[1]


# ---- planted defects: each case sees the defect it is for -----------------------------------------------------------------
DEFECTS = {                                                                      # name -> (function of the rule, defect, case)
    "closed_edge_rule": ("_owns", lambda dy, dz: np.bool_(True), "ray_vertex"),
    "closed_edge_rule_on_cubes": ("_owns", lambda dy, dz: np.bool_(True), "ray_edge"),
    "ahead_not_strict": ("_ahead", lambda det: det <= 0, "surface_box"),
    "ties_to_the_highest_face": ("_better", lambda dd, best: dd <= best, "tie"),
    "zero_normal_faces_not_skipped": ("_skip", lambda zero: False, "zero_normal"),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_each_case_sees_the_defect_it_was_built_for(monkeypatch, defect):
    what, wrong, name = DEFECTS[defect]
    case = K.CASES[name]()
    want = R.mesh_sdf_rule(**case)
    monkeypatch.setattr(R, what, wrong)
    got = R.mesh_sdf_rule(**case)
    assert not (np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1])), defect


# ---- the sign against independent yardsticks --------------------------------------------------------------------------------
def test_sign_on_a_torus_equals_the_analytic_torus_beyond_the_sagitta():
    """make_torus(0.5, 0.2, 24, 12) against the float64 torus (hypot(hypot(x, z) - R, y) - r).  The polyhedron's vertices
    lie on the torus; between them it deviates by at most the two sagittas (R + r)(1 - cos(pi/nu)) + r (1 - cos(pi/nv)),
    plus a snap unit per axis.  Every query is built farther from the analytic surface than that, none is dropped: in
    torus coordinates at tube distances outside the band, and on rays through the mesh's own vertices and edge midpoints
    (the rays that meet vertices and edges) at the x of a fixed ladder that the band admits."""
    from tpgan_amd.mesh import make_torus
    Rr, r, nu, nv = 0.5, 0.2, 24, 12
    v, f = make_torus(Rr, r, nu, nv)
    band = (Rr + r) * (1 - np.cos(np.pi / nu)) + r * (1 - np.cos(np.pi / nv)) + 3 * 2.0 ** -15
    assert 0.012 < band < 0.0135

    def analytic(q):
        q = np.asarray(q, np.float64)
        return np.hypot(np.hypot(q[:, 0], q[:, 2]) - Rr, q[:, 1]) - r
    rng = np.random.default_rng(11)
    n = 4000
    rho = np.where(rng.random(n) < 0.5, rng.uniform(0, r - 1.05 * band, n), rng.uniform(r + 1.05 * band, 0.3, n))
    u, w = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    ring = Rr + rho * np.cos(w)
    q = [np.stack([ring * np.cos(u), rho * np.sin(w), ring * np.sin(u)], 1)]
    mids = 0.5 * (v[f[:, 0]].astype(np.float64) + v[f[:, 1]])
    for yz in (v.astype(np.float64), mids):
        for x in np.linspace(-0.69, 0.69, 24):
            cand = np.stack([np.full(len(yz), x), yz[:, 1], yz[:, 2]], 1)
            q.append(cand[np.abs(analytic(cand.astype(F32))) > 1.05 * band])
    q = np.concatenate(q).astype(F32)
    want = analytic(q)
    assert len(q) > 10000 and (np.abs(want) > band).all()
    d, _ = R.mesh_sdf_rule(q, v, f)
    assert np.array_equal(d < 0, want < 0), np.nonzero((d < 0) != (want < 0))[0][:10]
    assert (want < 0).sum() > 2000 and (want > 0).sum() > 2000
    assert (np.abs(d - want) <= band).all()                                       # and the magnitude is the polyhedron's


def _box_distance(q, lo, hi):
    """float64 signed distance to the box [lo, hi]^3."""
    q = np.asarray(q, np.float64)
    e = np.abs(q - 0.5 * (lo + hi)) - 0.5 * (hi - lo)
    return np.linalg.norm(np.maximum(e, 0), axis=1) + np.minimum(e.max(1), 0)


def _cube_queries():
    """Points of the lattice (1/8) Z^3 in [-0.25, 1.25]^3 (rays through the cube's corners, along its edges, through its
    face diagonals, in the planes of its faces) and random points on the lattice 2^-12 Z^3 (which the snap grid of the
    unit cube, 2^-16, holds exactly, so that no query sits within a unit of the surface without being on it)."""
    k = np.arange(-2, 11) / 8.0
    lattice = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(12)
    rand = rng.integers(-1024, 5120, (3000, 3)) / 4096.0
    return np.concatenate([lattice, rand]).astype(F32)


def test_sign_and_magnitude_on_a_cube_equal_the_analytic_box():
    """The sign: for EVERY query off the surface (analytic distance != 0).  The magnitude: the numpy rule's largest
    deviation from the float64 box distance over these queries, measured here, is 1.4855e-08 (the rounding of a square
    root below 0.5); the bound is four times that, 5.942e-08, fp32 rounding being the only source."""
    v, f = K.cube(0, 1)
    q = _cube_queries()
    want = _box_distance(q, 0.0, 1.0)
    off = want != 0
    assert off.sum() > 4500 and (~off).sum() > 300
    d, face = R.mesh_sdf_rule(q, v, f)
    assert np.array_equal((d < 0)[off], (want < 0)[off])
    assert (d[~off] == 0).all()
    dev = np.abs(d.astype(np.float64) - want).max()
    print("cube: largest deviation of the rule from the analytic distance", dev)
    assert dev <= 4 * 1.4855e-8
    td, tf = _torch(K.case(q, (v, f)))
    assert np.array_equal(_bits(td), _bits(d)) and np.array_equal(tf, face)


# ---- the C entry's argument checks ------------------------------------------------------------------------------------------
def test_mesh_sdf_entry_rejects_bad_arguments_before_any_launch(hip_lib):
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    box = np.array([0, 0, 0, 1, 1, 1], F32)

    def sdf(query=p, vertices=p, faces=p, Q=4, V=3, F=1, box=box, inv_unit=65536.0, dist=p, face=p):
        return hip_lib.tpg_mesh_sdf_f32(query, vertices, faces, Q, V, F, None if box is None else box.ctypes.data, inv_unit,
                                        dist, face, None)
    for name in ("query", "vertices", "faces", "box", "dist", "face"):
        assert sdf(**{name: None}) == -1, name
        assert sdf(**{name: None}, Q=0) == -1, name                               # a NULL pointer before the empty case
    assert sdf(Q=-1) == -1 and sdf(V=-1) == -1 and sdf(F=-1) == -1
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert sdf(inv_unit=bad) == -1
    assert sdf(box=np.array([0, 0, 0, 1, np.nan, 1], F32)) == -1 and sdf(box=np.array([0, 2, 0, 1, 1, 1], F32)) == -1
    assert sdf(box=np.array([0, 0, 0, np.inf, 1, 1], F32)) == -1
    assert sdf(Q=0) == 0 and sdf(Q=0, F=0, V=0) == 0                               # nothing to do is decided first
    assert sdf(F=0) == -3 and sdf(V=0) == -3
    assert sdf(Q=(1 << 30) + 1) == -3 and sdf(V=(1 << 30) + 1) == -3 and sdf(F=(1 << 30) + 1) == -3


def test_the_op_validates_on_the_host(oracle_cpu):
    from tpgan_amd import ops
    v, f = K.cube(0, 1)
    q = torch.zeros(2, 3)
    d, face = ops.mesh_sdf(q + 0.5, _t(v), _t(f))                                 # the checker runs the torch statement
    assert d.tolist() == [-0.5, -0.5] and face.dtype == torch.int32
    e = ops.mesh_sdf(torch.zeros(0, 3), _t(v), _t(f))
    assert e[0].shape == (0,) and e[1].shape == (0,)
    bad_f = f.copy()
    bad_f[5, 1] = 8
    nan_v = v.copy()
    nan_v[3, 2] = np.nan
    for args in ((q, _t(v), _t(bad_f)), (q, _t(nan_v), _t(f)), (q, _t(v), _t(f).long()), (q.double(), _t(v), _t(f)),
                 (q, _t(v), _t(f)[:0]), (q, _t(v)[:0], _t(f)), (torch.zeros(2, 4), _t(v), _t(f))):
        with pytest.raises(RuntimeError):
            ops.mesh_sdf(*args)
    ops.unregister_backend("cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mesh_sdf(q, _t(v), _t(f))


# ---- tpgan_amd.mesh: meshes in ------------------------------------------------------------------------------------------------
def test_check_closed_counts_what_the_sign_needs():
    from tpgan_amd import mesh
    clean = {"boundary_edges": 0, "nonmanifold_edges": 0, "zero_normal_faces": 0, "inconsistent_pairs": 0}
    for v, f in (mesh.make_icosphere(0), mesh.make_icosphere(2, 0.3), mesh.make_torus(0.5, 0.2, 7, 5), K.cube(0, 1), K.octahedron()):
        assert mesh.check_closed(v, f) == clean
        a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
        assert (np.cross(a, b) * c).sum() > 0                                     # wound outward: a positive volume
    v, f = mesh.make_icosphere(1)
    assert f.shape == (80, 3) and v.shape == (42, 3) and np.allclose(np.linalg.norm(v, axis=1), 1, atol=1e-6)
    assert mesh.check_closed(v, f[1:]) == dict(clean, boundary_edges=3)          # one face removed
    assert mesh.check_closed(v, np.concatenate([f, f[:1]])) == dict(clean, nonmanifold_edges=3)      # one face doubled
    flipped = f.copy()
    flipped[0] = flipped[0, ::-1]
    assert mesh.check_closed(v, flipped) == dict(clean, inconsistent_pairs=3)
    flat = np.concatenate([f, [[0, 0, 1]]])
    assert mesh.check_closed(v, flat)["zero_normal_faces"] == 1
    tv, tf = mesh.make_torus(0.5, 0.2, 48, 24)
    assert tf.shape == (2304, 3) and np.allclose(np.hypot(np.hypot(tv[:, 0], tv[:, 2]) - 0.5, tv[:, 1]), 0.2, atol=1e-6)


def test_readers_round_trip_the_writers_files(tmp_path):
    from tpgan_amd import mesh
    v, f = mesh.make_torus(0.37, 0.11, 9, 5)
    n = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    for normals in (None, _t(n)):
        m = mesh.Mesh(_t(v), _t(f), normals, None, 0.0)
        mesh.write_ply(str(tmp_path / "b.ply"), m)
        mesh.write_ply(str(tmp_path / "a.ply"), m, ascii=True)
        mesh.write_obj(str(tmp_path / "m.obj"), m)
        assert open(tmp_path / "a.ply", "rb").read(20).startswith(b"ply\nformat ascii 1.0")
        for name in ("b.ply", "a.ply"):
            rv, rf, rn = mesh.read_ply(str(tmp_path / name))
            assert np.array_equal(_bits(rv), _bits(v)) and np.array_equal(rf, f) and rf.dtype == np.int32
            assert (rn is None) if normals is None else np.array_equal(_bits(rn), _bits(n))
        rv, rf = mesh.read_obj(str(tmp_path / "m.obj"))
        assert np.array_equal(_bits(rv), _bits(v)) and np.array_equal(rf, f)
        for spec in ("b.ply", "m.obj"):
            lv, lf = mesh.load_spec(str(tmp_path / spec))
            assert np.array_equal(lv, v) and np.array_equal(lf, f)
    # polygons are fanned; relative and v/vt/vn indices are accepted
    (tmp_path / "quad.obj").write_text("# a unit square\nv 0 0 0\nv 1 0 0\nvt 0 0\nv 1 1 0\nv 0 1 0\nvn 0 0 1\n"
                                       "f 1/1/1 2/1/1 3/1/1 4/1/1\nf -4//1 -3//1 -1//1\ng rest\nf 1 2 3 4 1\n")
    qv, qf = mesh.read_obj(str(tmp_path / "quad.obj"))
    assert qv.shape == (4, 3) and qf.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 2, 3], [0, 3, 0]]
    (tmp_path / "bad.obj").write_text("v 0 0 0\nf 1 2 3\n")
    with pytest.raises(RuntimeError, match="missing vertex"):
        mesh.read_obj(str(tmp_path / "bad.obj"))
    sv, sf = mesh.load_spec("icosphere:1")
    assert sf.shape == (80, 3) and mesh.load_spec("torus:0.5,0.2,8,6")[1].shape == (96, 3)
    with pytest.raises(RuntimeError, match="no such file"):
        mesh.load_spec(str(tmp_path / "nothing.ply"))
