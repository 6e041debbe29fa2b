"""The simulator's mesh obstacles and mesh bodies without a GPU: the torch statement against the numpy rule
(tests/pbf_sdf_rule.py) bit for bit on the cases of tests/pbf_sdf_cases.py, planted defects that each case must see, the
host validation, the C entry's argument checks, the untouched path without mesh obstacles, mesh bodies, the scene
generator, a block of fluid dropped onto a torus, and the CLI through the CPU checker."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_sdf_cases as MK  # noqa: E402
import pbf_obstacle_cases as OK  # noqa: E402
import pbf_rule as P  # noqa: E402
import pbf_sdf_cases as K  # noqa: E402
import pbf_sdf_rule as S  # noqa: E402

F32 = np.float32
DT = float(F32(1.0 / 160.0))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.int32)


def _equal(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def cases():
    """name -> (case, [(p, hit) per scene by the rule]); built once, never modified."""
    out = {}
    for name, build in K.CASES.items():
        case = build()
        out[name] = (case, K.expected(case))
    return out


# ---- the statement against the rule -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.CASES))
def test_torch_collide_sdf_equals_the_rule_bit_for_bit(cases, name):
    from tpgan_amd import ops
    case, want = cases[name]
    prm = ops.PbfParams()
    for b, (wp, wh) in enumerate(want):
        n = int(case["lengths"][b])
        hit = torch.zeros(n, dtype=torch.int32)
        args = (_t(case["p"][b, :n]), _t(case["lo"][b]), _t(case["hi"][b]), _t(case["table"][b]), _t(case["fields"]), prm)
        got = ops._pbf_collide_sdf_torch(*args, hit)
        assert _equal(got.numpy(), wp) and np.array_equal(hit.numpy(), wh), (name, b)
        assert torch.equal(ops._pbf_collide_sdf_torch(*args), got)               # without hit: the same positions


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_torch_substep_with_mesh_obstacles_equals_the_rule_bit_for_bit(cases, name):
    """Every case as a fluid at rest (v = 0) for one substep: collide_sdf after predict and after every dp."""
    from tpgan_amd import ops
    case, _ = cases[name]
    prm = ops.PbfParams(iters=2)
    x, lengths = case["p"], case["lengths"]
    if name == "batch":                                                          # every chunk's ends are enough here
        keep = [0, 5, 63, 64, 70, 128, 129]
        case = {k: (v if k == "fields" else v[keep]) for k, v in case.items()}
        x, lengths = case["p"], case["lengths"]
    v = np.where(np.isnan(x), F32(np.nan), F32(0))
    B = len(lengths)
    xt, vt = ops._pbf_substep_torch(_t(x), _t(v), _t(lengths), ops.pbf_box(case["lo"], case["hi"], B), DT, prm,
                                    sdf_obstacles=(_t(case["table"]), _t(case["fields"])))
    for b, n in enumerate(lengths.tolist()):
        xr, vr = S.substep_rule(x[b, :n], v[b, :n], case["lo"][b], case["hi"][b], DT, prm, case["table"][b], case["fields"])
        assert _equal(xt[b, :n].numpy(), xr) and _equal(vt[b, :n].numpy(), vr), (name, b)
        assert np.isnan(xt[b, n:].numpy()).all() and np.isnan(vt[b, n:].numpy()).all()


def test_torch_substep_equals_the_rule_on_a_moving_fluid_behind_an_analytic_obstacle():
    from tpgan_amd import ops
    case, v = K.drop_case()
    box = ops.pbf_box(case["lo"], case["hi"], 1)
    sdf = (_t(case["table"]), _t(case["fields"]))
    ball = np.stack([OK.row(1, (0.25, 0.12, 0.2), size=0.05)])[None]
    for prm in (ops.PbfParams(), ops.PbfParams(iters=0)):
        for analytic in (None, ball):
            xt, vt = ops._pbf_substep_torch(_t(case["p"]), _t(v), _t(case["lengths"]), box, DT, prm, sdf_obstacles=sdf,
                                            obstacles=None if analytic is None else _t(analytic))
            xr, vr = S.substep_rule(case["p"][0], v[0], case["lo"][0], case["hi"][0], DT, prm, case["table"][0], case["fields"],
                                    analytic=None if analytic is None else analytic[0])
            assert _equal(xt[0].numpy(), xr) and _equal(vt[0].numpy(), vr), (prm.iters, analytic is None)


# ---- planted defects: each case sees the defect it is for -----------------------------------------------------------------
DEFECTS = {                                                                      # name -> (function of the rule, defect, case)
    "non_strict_phi_below_a": ("_lt", lambda phi, a: phi <= a, "skin"),
    "writes_back_what_did_not_move": ("_written", lambda moved: np.ones_like(moved), "rotation"),
    "no_final_clamp": ("_final_clamp", lambda p, lo, hi, prm: p, "wall"),
    "reversed_order": ("_order", lambda M: range(M - 1, -1, -1), "order"),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_each_case_sees_the_defect_it_was_built_for(cases, monkeypatch, defect):
    what, wrong, name = DEFECTS[defect]
    case, want = cases[name]
    assert all(_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) for g, w in zip(K.expected(case), want))
    monkeypatch.setattr(S, what, wrong)
    got = K.expected(case)
    assert any(not _equal(g[0], w[0]) for g, w in zip(got, want)), defect        # the POSITIONS differ, not only hit


# ---- host validation ----------------------------------------------------------------------------------------------------------
def test_pbf_sdf_obstacles_builds_the_pair_and_validates_on_the_host(cases):
    from tpgan_amd import ops
    field, origin, step = K.sphere_field(0.1, 0.15)
    other = np.full((3, 4, 5), 0.5, F32)
    R90 = OK.rotation((0, 0, 1), 90)
    a = {"field": field, "origin": origin, "step": step, "centre": [0.1, 0.2, 0.3]}
    b = {"field": field, "origin": origin, "step": step, "centre": [0, 0, 0], "rotation": R90.reshape(-1).tolist()}
    c = {"field": _t(other), "origin": [0, 0, 0], "step": 0.5, "centre": [1, 1, 1]}
    table, fields = ops.pbf_sdf_obstacles([a, b, c], B=3, device="cpu")
    assert table.shape == (3, 3, 24) and table.dtype == torch.float32 and fields.shape == (field.size + 60,)
    assert torch.equal(table[0], table[2]) and np.array_equal(fields[:field.size].numpy(), field.reshape(-1))
    rows = table[0].numpy()
    assert np.array_equal(_bits(rows[0]), _bits(K.row((field.shape, 0), a["centre"], OK.EYE, origin, step)))
    assert np.array_equal(_bits(rows[1]), _bits(K.row((field.shape, 0), (0, 0, 0), R90, origin, step)))      # ONE copy, two poses
    assert np.array_equal(_bits(rows[2]), _bits(K.row(((3, 4, 5), field.size), (1, 1, 1), OK.EYE, (0, 0, 0), 0.5)))
    assert not any(S.skipped(r, fields.numel()) for r in rows)
    ragged, rf = ops.pbf_sdf_obstacles([[c], None, [a, c]], device="cpu")
    assert ragged.shape == (3, 2, 24) and ragged[:, :, 0].tolist() == [[4, 0], [0, 0], [4, 4]] and rf.numel() == 60 + field.size
    empty = ops.pbf_sdf_obstacles(None, B=2, device="cpu")
    assert empty[0].shape == (2, 0, 24) and empty[1].shape == (0,)
    sheared = np.eye(3)
    sheared[0, 1] = 1e-3
    nan_field = field.copy()
    nan_field[2, 2, 2] = np.nan
    for bad in ([a] * 5, [dict(a, step=0.0)], [dict(a, step=-1.0)], [dict(a, centre=[0, np.nan, 0])], [dict(a, origin=[np.inf, 0, 0])],
                [dict(a, rotation=sheared.reshape(-1).tolist())], [dict(a, field=nan_field)], [dict(a, field=field[:1])],
                [dict(a, field=field.astype(np.float64))], [dict(a, field=field[0])], [{"field": field, "centre": [0, 0, 0]}]):
        with pytest.raises(RuntimeError):
            ops.pbf_sdf_obstacles(bad, device="cpu")
    # the ops refuse a pair of the wrong shape before any backend is asked
    ops.unregister_backend("cpu")
    p = torch.zeros(2, 4, 3)
    f0 = torch.zeros(8)
    for pair in ((torch.zeros(1, 1, 24), f0), (torch.zeros(2, 1, 16), f0), (torch.zeros(2, 5, 24), f0),
                 (torch.zeros(2, 1, 24, dtype=torch.float64), f0), (torch.zeros(2, 1, 24), torch.zeros(2, 4))):
        with pytest.raises(RuntimeError, match="table|fields|mesh obstacles"):
            ops.pbf_collide_sdf(p, None, [0, 0, 0], [1, 1, 1], *pair)
        with pytest.raises(RuntimeError, match="table|fields|mesh obstacles"):
            ops.pbf_substep(p, p, None, [0, 0, 0], [1, 1, 1], 0.01, sdf_obstacles=pair)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pbf_collide_sdf(p, None, [0, 0, 0], [1, 1, 1], torch.zeros(2, 1, 24), f0)


def test_collide_sdf_entry_rejects_bad_arguments_before_any_launch(hip_lib):
    buf = (C.c_float * 256)()
    p = C.cast(buf, C.c_void_p)
    box = np.array([[0, 0, 0, 1, 1, 1]], F32)
    flat = np.array([[0, 0, 0, 1, 0, 1]], F32)
    nan = float("nan")

    def collide(p_=p, box=box, table=p, fields=p, L=64, B=1, N=4, M=2, a=0.0125, p_out=p, hit=p):
        return hip_lib.tpg_pbf_collide_sdf_f32(p_, None, None if box is None else box.ctypes.data, table, fields, L, B, N, M, a,
                                               p_out, hit, None)
    assert collide(B=-1) == -1 and collide(N=-1) == -1 and collide(M=-1) == -1 and collide(L=-1) == -1
    assert collide(a=0.0) == -1 and collide(a=-1.0) == -1 and collide(a=nan) == -1 and collide(a=float("inf")) == -1
    assert collide(p_out=None) == -1 and collide(p_out=None, B=0) == -1 and collide(M=-1, N=0) == -1
    assert collide(B=0) == 0 and collide(N=0) == 0 and collide(B=0, p_=None, box=None, table=None, fields=None) == 0
    assert collide(N=0, M=5) == 0                                               # empty work is decided first
    assert collide(B=65536) == -3 and collide(N=(1 << 22) + 1) == -3 and collide(M=5) == -3
    assert collide(M=5, p_=None) == -3                                          # the limits before the other pointers
    assert collide(p_=None) == -1 and collide(box=None) == -1 and collide(box=flat) == -1
    assert collide(table=None) == -1 and collide(fields=None) == -1 and collide(fields=None, L=1 << 40) == -1


# ---- without mesh obstacles nothing changes --------------------------------------------------------------------------------
def test_substep_without_mesh_obstacles_is_the_old_path(oracle_cpu, monkeypatch):
    import pbf_cases
    from tpgan_amd import ops

    def never(*a, **k):
        raise AssertionError("collide_sdf was reached without mesh obstacles")
    monkeypatch.setattr(ops, "_pbf_collide_sdf_torch", never)
    x, v, lengths, lo, hi = pbf_cases.small_case()
    ball = _t(np.stack([OK.row(1, (0.2, 0.1, 0.2), size=0.05)])[None].repeat(2, 0))
    for kw in ({}, {"sdf_obstacles": None}, {"obstacles": ball}, {"obstacles": ball, "sdf_obstacles": None}):
        xs, vs = ops.pbf_substep(_t(x), _t(v), _t(lengths), lo, hi, DT, **kw)
        for b, n in enumerate(lengths.tolist()):
            if "obstacles" in kw:
                import pbf_obstacle_rule as O
                xr, vr = O.substep_rule(x[b, :n], v[b, :n], lo[b], hi[b], DT, ops.PbfParams(), ball[b].numpy())
            else:
                xr, vr = P.substep_rule(x[b, :n], v[b, :n], lo[b], hi[b], DT, ops.PbfParams())
            assert _equal(xs[b, :n].numpy(), xr) and _equal(vs[b, :n].numpy(), vr)
    with pytest.raises(AssertionError, match="collide_sdf was reached"):
        ops.pbf_substep(_t(x), _t(v), _t(lengths), lo, hi, DT, sdf_obstacles=(torch.zeros(2, 1, 24), torch.zeros(0)))


def test_collide_sdf_and_substep_through_the_checker_equal_the_rule(oracle_cpu, cases):
    from tpgan_amd import ops
    ragged, want = cases["batch"]
    got, hit = ops.pbf_collide_sdf(_t(ragged["p"]), _t(ragged["lengths"]), ragged["lo"], ragged["hi"], _t(ragged["table"]),
                                   _t(ragged["fields"]), return_hit=True)
    alone = ops.pbf_collide_sdf(_t(ragged["p"]), _t(ragged["lengths"]), ragged["lo"], ragged["hi"], _t(ragged["table"]),
                                _t(ragged["fields"]))
    for b, (wp, wh) in enumerate(want):
        n = len(wp)
        assert _equal(got[b, :n].numpy(), wp) and np.array_equal(hit[b, :n].numpy(), wh) and _equal(alone[b, :n].numpy(), wp)
        assert np.isnan(got[b, n:].numpy()).all() and not hit[b, n:].any()
    drop, v = K.drop_case()
    xs, vs = ops.pbf_substep(_t(drop["p"]), _t(v), _t(drop["lengths"]), drop["lo"], drop["hi"], DT,
                             sdf_obstacles=(_t(drop["table"]), _t(drop["fields"])))
    xr, vr = S.substep_rule(drop["p"][0], v[0], drop["lo"][0], drop["hi"][0], DT, ops.PbfParams(), drop["table"][0], drop["fields"])
    assert _equal(xs[0].numpy(), xr) and _equal(vs[0].numpy(), vr)


# ---- mesh bodies and scenes -----------------------------------------------------------------------------------------------------
def _write_cube(path):
    from tpgan_amd import mesh
    v, f = MK.cube(-1, 1)
    mesh.write_obj(path, mesh.Mesh(_t(v), _t(f), None, None, 0.0))
    return path


def test_body_points_of_a_cube_mesh_on_the_lattice_is_the_analytic_count(oracle_cpu, tmp_path):
    """A cube of edge 0.2 at spacing 0.025: the nodes k * 0.025 with |k * 0.025| <= 0.1 - 0.0125 on every axis, k = -3 .. 3,
    7^3 of them (no node lies at the radius itself), the same after a quarter turn; and they are the box body's nodes that
    keep a radius from the faces."""
    from tpgan_amd import simulate as sim
    spec = _write_cube(str(tmp_path / "cube.obj"))
    body = {"shape": "mesh", "mesh": spec, "size": 0.2, "rotation": np.eye(3).reshape(-1).tolist(), "centre": [0.5, 0.5, 0.5]}
    pts = sim.body_points(body, 0.025, device="cpu")
    assert pts.shape == (343, 3) and np.allclose(pts.min(0), 0.425) and np.allclose(pts.max(0), 0.575)
    box = sim.body_points(dict(body, shape="box"), 0.025)
    inner = box[(np.abs(box - 0.5) <= 0.0875 + 1e-9).all(1)]
    assert np.array_equal(np.sort(pts.round(9), 0), np.sort(inner.round(9), 0))
    turned = sim.body_points(dict(body, rotation=OK.rotation((0, 0, 1), 90).reshape(-1).tolist()), 0.025, device="cpu")
    assert turned.shape == (343, 3)
    assert np.array_equal(sim.body_half_extent("mesh", 0.2, spec), [0.1, 0.1, 0.1])
    assert sim.obstacle_bound(body) == pytest.approx(0.1 * 3 ** 0.5)
    # an open mesh is refused: the sign needs a closed one
    from tpgan_amd import mesh
    v, f = MK.cube(-1, 1)
    mesh.write_obj(str(tmp_path / "open.obj"), mesh.Mesh(_t(v), _t(f[1:]), None, None, 0.0))
    with pytest.raises(RuntimeError, match="not closed"):
        sim.body_points(dict(body, mesh=str(tmp_path / "open.obj")), 0.025, device="cpu")


@pytest.mark.parametrize("seed", range(6))
def test_random_scene_without_the_mesh_options_is_the_scene_it_was(seed):
    """The fluid's and the obstacles' draws do not depend on the mesh options: with them, the bodies and obstacles that stay
    analytic shapes, and every draw's size, rotation and velocity, are those of the scene without."""
    from tpgan_amd import simulate as sim
    kw = dict(box=(1.2, 1.0, 1.2), body_size=0.2, count_range=(1, 10 ** 9))
    plain = sim.random_scene(seed, obstacles=2, obstacle_size=(0.15, 0.3), **kw)
    again = sim.random_scene(seed, obstacles=2, obstacle_size=(0.15, 0.3), fluid_meshes=(), obstacle_meshes=(), **kw)
    assert plain.to_json() == again.to_json()
    assert all(o["shape"] in sim.SHAPES for o in plain.obstacles) and all(b["shape"] in sim.SHAPES for b in plain.bodies)


def test_random_scene_with_meshes(oracle_cpu):
    from tpgan_amd import ops
    from tpgan_amd import simulate as sim
    kw = dict(box=(1.2, 1.0, 1.2), body_size=0.2, count_range=(1, 10 ** 9), obstacles=2, obstacle_size=(0.32, 0.4))
    found_body = found_ob = False
    for seed in range(8):
        a = sim.random_scene(seed, fluid_meshes=["icosphere:1"], obstacle_meshes=["torus:0.5,0.25,12,8"], **kw)
        b = sim.random_scene(seed, fluid_meshes=["icosphere:1"], obstacle_meshes=["torus:0.5,0.25,12,8"], **kw)
        assert a.to_json() == b.to_json()
        again = sim.Scene.from_json(json.loads(json.dumps(a.to_json())))
        assert again.obstacles == a.obstacles and again.bodies == a.bodies
        for o in a.obstacles:
            if o["shape"] == "mesh":
                found_ob = True
                assert o["mesh"] == "torus:0.5,0.25,12,8" and 0.32 <= o["size"] <= 0.4
                half = sim.mesh_geometry(o["mesh"], o["size"])[2]
                assert 2 * half.min() >= sim.MIN_OBSTACLE_SPACINGS * 2 * a.radius and 2 * half.max() == pytest.approx(o["size"])
        for body in a.bodies:
            if body["shape"] == "mesh" and not found_body:
                found_body = True
                pts = sim.body_points(body, 2 * a.radius, device="cpu")
                local = (pts - body["centre"]) @ np.asarray(body["rotation"]).reshape(3, 3)
                # the icosphere's box is at least 0.85 of its diameter wide: its radius is below 0.5 size / 0.85
                assert len(pts) > 10 and (np.linalg.norm(local, axis=1) <= 0.5 * body["size"] / 0.85 - a.radius).all()
        if found_body and found_ob:
            break
    assert found_body and found_ob
    mixed = sim.Scene([0, 0, 0], [1, 1, 1], obstacles=[{"shape": "ball", "centre": [0.2, 0.2, 0.2], "size": 0.1},
                                                      {"shape": "mesh", "mesh": "icosphere:1", "size": 0.2, "centre": [0.6, 0.2, 0.6]}])
    assert sim.obstacle_table([mixed], "cpu").shape == (1, 1, 16)                # the analytic ones only
    table, fields = sim.sdf_obstacle_table([mixed, mixed], "cpu")
    assert table.shape == (2, 1, 24) and torch.equal(table[0], table[1])
    fl, dims, off = S.decode(table[0, 0].numpy())
    assert off == 0 and fields.numel() == dims[0] * dims[1] * dims[2] and fl[16] == F32(mixed.radius)
    assert sim.sdf_obstacle_table([sim.Scene([0, 0, 0], [1, 1, 1], obstacles=mixed.obstacles[:1])], "cpu") is None
    # the lattice reaches a radius and a cell beyond the mesh on every side
    assert (fl[13:16] <= -0.1 - mixed.radius - fl[16]).all()
    assert ((fl[13:16] + (np.array(dims) - 1) * fl[16]) >= 0.1 + mixed.radius + fl[16]).all()
    # the union's distance: the ball's exact one and the mesh's
    q = torch.tensor([[0.2, 0.2, 0.2], [0.6, 0.2, 0.6], [0.6, 0.5, 0.6]], dtype=torch.float64)
    d = sim.obstacle_distance(mixed.obstacles, q)
    assert d.dtype == torch.float64 and d[0] == pytest.approx(-0.1) and -0.1 <= d[1] < -0.07 and d[2] == pytest.approx(0.2, abs=1e-3)
    assert ops.PBF_MAX_SDF_OBSTACLES == 4


# ---- a block of fluid dropped onto a torus ------------------------------------------------------------------------------------
def test_a_block_dropped_onto_a_torus_rests_higher_and_stays_out_of_it(oracle_cpu):
    """10 x 5 x 10 particles dropped onto a torus (outer diameter 0.3, lying flat, its hole smaller than the block) on the
    floor of a box of 0.4 x 0.5 x 0.4, 40 frames through the CPU checker, against the same fluid without the torus.  No
    particle ends deeper inside the mesh than the field's step (the exact `ops.mesh_sdf` of the final positions), and the
    fluid's centre of mass rests measurably higher.  "Measurably": both runs are deterministic and a mean of fp32 heights
    below 0.5 m carries less than 1e-7 m of rounding, so any length the simulation resolves is measurable; the smallest it
    resolves is the particle radius (12.5 mm, also the field's step), and the test asks for a tenth of it, 1.25 mm."""
    from tpgan_amd import ops
    from tpgan_amd import simulate as sim
    torus = {"shape": "mesh", "mesh": "torus:0.5,0.25,16,8", "size": 0.3, "centre": [0.2, 0.0625, 0.2]}
    g = np.stack(np.meshgrid(np.arange(10), np.arange(5), np.arange(10), indexing="ij"), -1).reshape(-1, 3)
    pos = (np.array([0.0875, 0.16, 0.0875]) + g * 0.025).astype(F32)
    with_, without = (sim.Scene([0, 0, 0], [0.4, 0.5, 0.4], pos=pos, obstacles=obs) for obs in ([torus], []))
    prm = ops.PbfParams(iters=2)
    (pa, _, _), (pb, _, _) = (sim.simulate([s], 41, substeps=2, params=prm, device="cpu") for s in (with_, without))
    assert bool(torch.isfinite(pa).all()) and bool(torch.isfinite(pb).all())
    step = with_.radius
    for frame in (10, 20, 40):
        depth = sim.obstacle_distance([torus], pa[0, frame])
        assert float(depth.min()) >= -step, (frame, float(depth.min()))
    rest_with, rest_without = float(pa[0, 40, :, 1].double().mean()), float(pb[0, 40, :, 1].double().mean())
    print("drop onto a torus: mean height with", rest_with, "without", rest_without,
          "deepest", float(sim.obstacle_distance([torus], pa[0, 40]).min()))
    assert rest_with > rest_without + 0.1 * with_.radius
    assert not torch.equal(pa[0, 40], pb[0, 40])


# ---- the CLI through the CPU checker --------------------------------------------------------------------------------------------
def test_cli_with_mesh_options_writes_frames_scene_and_obstacles(oracle_cpu, tmp_path, capsys):
    from tpgan_amd import mesh
    from tpgan_amd import simulate as sim
    out = str(tmp_path / "train")
    found = None
    for seed in range(1, 40):                                                    # a seed whose scene has both kinds of mesh
        sc = sim.random_scene([seed, 0, 0], (0.6, 0.6, 0.6), body_size=0.11, obstacles=1, obstacle_size=(0.22, 0.26),
                              fluid_meshes=["icosphere:2"], obstacle_meshes=["torus:0.5,0.45,12,8"])
        if any(b["shape"] == "mesh" for b in sc.bodies) and sc.obstacles[0]["shape"] == "mesh":
            found = seed
            break
    assert found is not None
    argv = ["--out", out, "--cases", "1", "--frames", "3", "--seed", str(found), "--box", "0.6", "0.6", "0.6", "--body_size",
            "0.11", "--substeps", "2", "--iters", "2", "--device", "cpu", "--obstacles", "1", "--obstacle_size", "0.22", "0.26",
            "--fluid_mesh", "icosphere:2", "--obstacle_mesh", "torus:0.5,0.45,12,8"]
    assert sim.main(argv) == 0
    capsys.readouterr()
    case = os.path.join(out, "case1")
    meta = json.load(open(os.path.join(case, "scene.json")))
    scene = sim.Scene.from_json(meta)
    assert meta["fluid_mesh"] == ["icosphere:2"] and meta["obstacle_mesh"] == ["torus:0.5,0.45,12,8"]
    assert scene.obstacles == sc.obstacles and scene.bodies == sc.bodies and meta["obstacles"][0]["mesh"] == "torus:0.5,0.45,12,8"
    v, f, n = mesh.read_ply(os.path.join(case, "obstacles.ply"))
    report = mesh.check_closed(v, f)
    assert len(f) > 100 and report["boundary_edges"] == 0 and report["nonmanifold_edges"] == 0 and n is not None
    assert np.abs(v.mean(0) - scene.obstacles[0]["centre"]).max() < 0.05
    pos, vel, _ = sim.simulate([scene], 3, substeps=2, iters=2, device="cpu")
    with np.load(os.path.join(case, "data_2.npz")) as z:
        assert np.array_equal(z["pos"], pos[0, 2].numpy()) and np.array_equal(z["vel"], vel[0, 2].numpy())
    with pytest.raises(SystemExit):
        sim.main(["--out", out, "--cases", "1", "--obstacle_mesh", "icosphere:1"])    # no --obstacles
    capsys.readouterr()
    # a scene file without the keys loads as it always did
    for key in ("fluid_mesh", "obstacle_mesh", "obstacles"):
        del meta[key]
    meta["bodies"] = [b for b in meta["bodies"] if b["shape"] != "mesh"]
    assert sim.Scene.from_json(meta).obstacles == []


@pytest.mark.parametrize("seed", range(4))
def test_a_seed_without_the_options_gives_the_scene_of_before(seed):
    """The scene of a seed as the generator drew it before the mesh options existed, restated here draw for draw from
    numpy's generator (the recipe of `random_scene`'s docstring), against `random_scene(seed)` with a small box."""
    from tpgan_amd import simulate as sim
    box, body_size, radius = np.array([1.2, 1.0, 1.2]), 0.2, 0.0125
    scene = sim.random_scene(seed, tuple(box), radius, body_size, count_range=(1, 10 ** 9))
    rng = np.random.default_rng(seed)
    spacing = 2 * radius
    bodies, spheres = [], []
    for _ in range(int(rng.integers(1, 4))):
        shape = sim.SHAPES[int(rng.integers(0, 3))]
        size = float(body_size * rng.uniform(0.5, 1.5))
        rot = sim._random_rotation(rng)
        bound = float(np.linalg.norm(sim.body_half_extent(shape, size))) + spacing
        velocity = [float(rng.uniform(-2, 2)), float(rng.uniform(-0.5, 0.5)), float(rng.uniform(-2, 2))]
        for _ in range(100):
            if (2 * bound >= box).any():
                break
            centre = rng.uniform(bound, box - bound)
            if all(np.linalg.norm(centre - c) >= bound + b for c, b in spheres):
                spheres.append((centre, bound))
                bodies.append({"shape": shape, "size": size, "rotation": rot.reshape(-1).tolist(), "centre": centre.tolist(),
                               "velocity": velocity})
                break
    assert bodies and scene.bodies == bodies and scene.obstacles == []
