"""The meshes and queries the signed-distance tests share (tests/test_mesh_sdf_cpu.py, tests/test_mesh_sdf_gpu.py).  A case
is a dict of query (Q,3), vertices (V,3) float32 and faces (F,3) int32.  Every builder asserts through the numpy rule
(tests/mesh_sdf_rule.py), by equality tests on the rule's intermediates, that its queries sit on the edge they are for."""
import numpy as np

import mesh_sdf_rule as R

F32 = np.float32
CUBE_FACES = np.array([[0, 3, 2], [0, 1, 3], [4, 7, 5], [4, 6, 7], [0, 5, 1], [0, 4, 5], [2, 7, 6], [2, 3, 7],
                       [0, 6, 4], [0, 2, 6], [1, 7, 3], [1, 5, 7]], np.int32)        # vertex = 4 x + 2 y + z, outward


def cube(lo, hi):
    lo, hi = np.broadcast_to(np.asarray(lo, np.float64), 3), np.broadcast_to(np.asarray(hi, np.float64), 3)
    v = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    return v.astype(F32), CUBE_FACES.copy()


def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, f


def join(*meshes):
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + base)
        base += len(v)
    return np.concatenate(vs).astype(F32), np.concatenate(fs).astype(np.int32)


def case(query, mesh):
    return dict(query=np.ascontiguousarray(query, F32).reshape(-1, 3), vertices=np.ascontiguousarray(mesh[0], F32),
                faces=np.ascontiguousarray(mesh[1], np.int32))


def run(c, **kw):
    """The rule on a case -> (dist, face, trace)."""
    trace = {}
    d, f = R.mesh_sdf_rule(c["query"], c["vertices"], c["faces"], trace=trace, **kw)
    return d, f, trace


def _closed(mesh):
    from tpgan_amd.mesh import check_closed
    s = check_closed(*mesh)
    return s["boundary_edges"] == 0 and s["nonmanifold_edges"] == 0


# ---- the closest feature -----------------------------------------------------------------------------------------------
def regions_case():
    """One triangle (0,0,0), (4,0,0), (0,4,0) and a query in each of the seven regions, above the plane and in it; then a
    query on the face, on an edge and on a vertex: d == 0."""
    tri = (np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], F32), np.array([[0, 1, 2]], np.int32))
    q = np.array([[-1, -1, 1], [6, -1, 1], [2, -1, 1], [-1, 6, 1], [-1, 2, 1], [3, 3, 1], [1, 1, 1],       # a b ab c ac bc face
                  [-1, -1, 0], [6, -1, 0], [2, -1, 0], [-1, 6, 0], [-1, 2, 0], [3, 3, 0],
                  [1, 1, 0], [2, 0, 0], [2, 2, 0], [0, 1, 0], [4, 0, 0], [0, 0, 0], [0, 4, 0]], F32)
    c = case(q, tri)
    d, f, t = run(c)
    assert t["region"][:, 0].tolist() == [0, 1, 2, 3, 4, 5, 6, 0, 1, 2, 3, 4, 5] + [6, 2, 5, 4, 1, 0, 3]
    assert (d[13:] == 0).all() and (d[:13] > 0).all() and (f == 0).all()
    assert d[6] == 1 and d[2] == F32(np.sqrt(F32(2))) and d[5] == F32(np.sqrt(F32(3)))
    return c


def tie_case():
    """Faces 0 and 1 share the edge (0,0,0)-(0,4,0) and fold away from the query, which is nearest to that edge at the
    same dd for both: face 0.  Faces 2 and 3 share only the vertex (10,0,0); query 1 is nearest to it: face 2."""
    v = np.array([[0, 0, 0], [0, 4, 0], [-3, 2, -3], [3, 2, -3], [10, 0, 0], [12, -1, -2], [12, 1, -2], [8, -1, -2], [8, 1, -2]],
                 F32)
    f = np.array([[0, 1, 2], [1, 0, 3], [4, 5, 6], [4, 8, 7]], np.int32)
    c = case([[0, 2, 2], [10, 0, 1]], (v, f))
    d, face, t = run(c)
    assert t["dd"][0, 0] == t["dd"][0, 1] == 4 and t["region"][0, :2].tolist() == [2, 2] and face[0] == 0
    assert t["dd"][1, 2] == t["dd"][1, 3] == 1 and t["region"][1, 2:].tolist() == [0, 0] and face[1] == 2
    assert (t["dd"][0, 2:] > 4).all() and (t["dd"][1, :2] > 1).all()
    return c


def zero_normal_case():
    """Face 0 has collinear corners, face 1 coincident ones, face 2 is a proper triangle further away.  Each query sits
    next to a skipped face and still answers face 2."""
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [5, 5, 5], [0, 0, -4], [4, 0, -4], [0, 4, -4]], F32)
    f = np.array([[0, 1, 2], [3, 3, 3], [4, 5, 6]], np.int32)
    c = case([[1, 0, 0.5], [5, 5, 5.25], [1, 1, -3]], (v, f))
    d, face, t = run(c)
    assert (t["region"][:, :2] == -1).all() and (face == 2).all() and np.isfinite(d).all()
    assert d[0] == 4.5 and d[2] == 1
    return c


def all_zero_normal_case():
    """Nothing but zero-normal faces: +inf and -1, in the box and outside it."""
    v = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3]], F32)
    f = np.array([[0, 1, 2], [1, 1, 3], [3, 2, 0]], np.int32)
    c = case([[1, 1, 1], [0.5, 2, 1], [9, 9, 9]], (v, f))
    d, face, t = run(c)
    assert t["inbox"].tolist() == [True, True, False] and np.isposinf(d).all() and (face == -1).all()
    return c


# ---- the sign ------------------------------------------------------------------------------------------------------------
def ray_vertex_case():
    """The octahedron |x| + |y| + |z| <= 1.  Query 0 inside, its ray through the vertex (1,0,0) where four faces meet (and,
    in projection, the four at (-1,0,0)): every one has two edge functions that are 0, and exactly one counts.  Query 1
    inside with the ray through the edge (1,0,0)-(0,1,0) (one zero each on the four faces at (0,1,0)).  Query 2 OUTSIDE,
    its ray grazing the silhouette edge (0,1,0)-(0,0,1): the two faces on it project to the same side and count both or
    neither.  Query 3 inside, behind that edge."""
    c = case([[-0.5, 0, 0], [-0.25, 0.5, 0], [-0.25, 0.5, 0.5], [0, 0.25, 0.25]], octahedron())
    d, f, t = run(c)
    assert t["inbox"].all()
    assert (t["on_edge"][0] == 2).sum() == 8 and t["counted"][0].sum() == 1 and d[0] < 0
    assert (t["on_edge"][1] == 1).sum() == 4 and t["counted"][1].sum() == 1 and d[1] < 0
    grazed = np.nonzero(t["on_edge"][2] >= 1)[0]
    assert sorted(grazed.tolist()) == [0, 1] and t["counted"][2, 0] == t["counted"][2, 1] and t["ahead"][2, 0]
    assert t["counted"][2].sum() % 2 == 0 and d[2] > 0
    assert t["counted"][3].sum() == 1 and d[3] < 0
    return c


def ray_edge_case():
    """Two disjoint cubes, [0,1]^3 and [2,3] x [0.25,0.75]^2.  Query 0 between them, its ray running ALONG the edge
    y = z = 0.25 of the second (it touches four of its faces): outside.  Query 1 inside the first cube on the same ray: one
    crossing there, an even number further on.  Query 2 between them with the ray IN THE PLANE of the face y = 0.25 (whose
    projection has no area) through the edges of the faces x = 2 and x = 3.  Query 3 inside the second cube, the ray
    through the diagonal of its face x = 3."""
    mesh = join(cube(0, 1), cube([2, 0.25, 0.25], [3, 0.75, 0.75]))
    assert _closed(mesh)
    c = case([[1.5, 0.25, 0.25], [0.5, 0.25, 0.25], [1.5, 0.25, 0.5], [2.5, 0.5, 0.5]], mesh)
    d, f, t = run(c)
    assert t["inbox"].all()
    assert (t["on_edge"][0, 12:] >= 1).sum() >= 4 and t["counted"][0].sum() % 2 == 0 and d[0] == 0.5
    assert t["counted"][1, :12].sum() == 1 and t["counted"][1, 12:].sum() % 2 == 0 and d[1] == -0.25
    assert (t["on_edge"][2, 12:] >= 1).sum() >= 2 and t["counted"][2].sum() % 2 == 0 and d[2] == 0.5
    assert (t["on_edge"][3, 12:] == 1).sum() == 4 and t["counted"][3].sum() == 1 and d[3] == -0.25
    return c


def surface_box_case():
    """The cube [0,1]^3: queries exactly on the surface (face centres, an edge midpoint, a corner: d == 0 with whatever
    sign the rule gives), one an ulp inside the face x = 1 (it snaps ONTO the face: the rule calls it outside, the caveat of
    the snap grid), queries outside the box (never inside, a NaN among them) and inside."""
    on = [[0.5, 0.5, 0], [0.5, 0.5, 1], [0, 0.5, 0.5], [1, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 1, 0.5], [0.5, 0, 0], [1, 1, 1]]
    near = [[np.nextafter(F32(1), F32(0)), 0.5, 0.5]]
    out = [[1.5, 0.5, 0.5], [-0.25, 0.5, 0.5], [0.5, 0.5, np.nextafter(F32(1), F32(2))], [0.5, -2.0 ** -20, 0.5], [2, 2, 2],
           [np.nan, 0.5, 0.5]]
    inside = [[0.5, 0.5, 0.5], [1 - 2.0 ** -10, 0.5, 0.5], [0.25, 0.75, 0.125], [2.0 ** -12, 2.0 ** -12, 2.0 ** -12]]
    c = case(on + near + out + inside, cube(0, 1))
    d, f, t = run(c)
    assert t["inbox"].tolist() == [True] * 9 + [False] * 6 + [True] * 4
    assert (np.abs(d[:8]) == 0).all() and t["det0"][[2, 3, 7]].any(1).all()
    assert t["qi"][8, 0] == 65536 and t["det0"][8].any() and d[8] == F32(2.0 ** -24)
    assert (d[9:14] > 0).all() and np.isposinf(d[14]) and f[14] == -1 and (d[15:] < 0).all()
    return c


def cavity_case():
    """A sphere of radius 1 with a spherical cavity of radius 0.5 (its faces turned inward): the cavity is outside, the
    shell inside."""
    from tpgan_amd.mesh import make_icosphere
    outer, (vi, fi) = make_icosphere(1), make_icosphere(1, 0.5)
    mesh = join(outer, (vi, fi[:, ::-1]))
    assert _closed(mesh)
    c = case([[0, 0, 0], [0.1, -0.2, 0.05], [0.7, 0.1, 0.1], [-0.1, 0.72, 0], [0.95, 0.95, 0.95], [0, 0, 0.3]], mesh)
    d, f, t = run(c)
    assert t["inbox"].all() and (d[[0, 1, 5]] > 0).all() and (f[[0, 1, 5]] >= 80).all()
    assert (d[[2, 3]] < 0).all() and d[4] > 0 and t["counted"][0].sum() == 2
    return c


def inward_case():
    """The octahedron and the two cubes wound INWARD: parity does not care; every sign is the outward mesh's."""
    out = []
    for build in (ray_vertex_case, ray_edge_case):
        c = build()
        flipped = dict(c, faces=np.ascontiguousarray(c["faces"][:, ::-1]))
        d0, d1 = run(c)[0], run(flipped)[0]
        assert np.array_equal(np.signbit(d0), np.signbit(d1)) and np.allclose(d0, d1, rtol=1e-6, atol=0)   # corners reordered
        out.append(flipped)
    return out[0], out[1]


def units_case():
    """The cavity mesh scaled by 3 and moved: the snap unit is another power of two, and the signs at the moved queries are
    the same."""
    c = cavity_case()
    shift = np.array([10.5, -3.25, 0.125], F32)
    moved = case(c["query"] * F32(3) + shift, (c["vertices"] * F32(3) + shift, c["faces"]))
    (d0, _, t0), (d1, _, t1) = run(c), run(moved)
    assert t0["unit"] == 2.0 ** -15 and t1["unit"] == 2.0 ** -13
    assert np.array_equal(d0 < 0, d1 < 0) and (d0 < 0).sum() == 2
    return moved


# ---- the tiling ----------------------------------------------------------------------------------------------------------
def _stray(n, rng):
    """n small triangles far from the torus, each the nearest face of the query beside it."""
    base = np.array([2.0, 0.0, 0.0]) + np.arange(n)[:, None] * np.array([0.0, 0.5, 0.0])
    v = (base[:, None, :] + np.array([[0, 0, 0], [0.1, 0, 0], [0, 0, 0.1]])).reshape(-1, 3)
    return (v.astype(F32), np.arange(3 * n, dtype=np.int32).reshape(n, 3)), (base + [0.02, 0.05, 0.02]).astype(F32)


def tiling_cases():
    """F = 1, 256 (one tile), 257 and 3 * 256 + 5, each with Q = 1, 255, 256, 257 and 1000 of the same stream of queries.
    From 257 on the faces beyond the torus are stray triangles, each the nearest face of one query: the last tile's last
    face is an answer."""
    from tpgan_amd.mesh import make_torus
    rng = np.random.default_rng(5)
    pool = rng.uniform([-0.8, -0.3, -0.8], [0.8, 0.3, 0.8], (1000, 3)).astype(F32)
    out = {}
    for F, torus, extra in ((1, None, 1), (256, (16, 8), 0), (257, (16, 8), 1), (773, (24, 16), 5)):
        none = ((np.zeros((0, 3), F32), np.zeros((0, 3), np.int32)), np.zeros((0, 3), F32))
        stray, beside = _stray(extra, rng) if extra else none
        mesh = join(make_torus(0.5, 0.2, *torus), stray) if torus else stray
        assert len(mesh[1]) == F
        q = np.concatenate([beside, pool])[:1000]
        d, f, _ = run(case(q, mesh))
        if extra:
            assert f[:extra].tolist() == list(range(F - extra, F))
        if torus:
            assert (d < 0).sum() > 50 and (d > 0).sum() > 50 and len(np.unique(f)) > 100
        for Q in (1, 255, 256, 257, 1000):
            out[(F, Q)] = case(q[:Q], mesh)
    return out


CASES = {"regions": regions_case, "tie": tie_case, "zero_normal": zero_normal_case, "all_zero_normal": all_zero_normal_case,
         "ray_vertex": ray_vertex_case, "ray_edge": ray_edge_case, "surface_box": surface_box_case, "cavity": cavity_case,
         "inward_octahedron": lambda: inward_case()[0], "inward_cubes": lambda: inward_case()[1], "units": units_case}
