"""The simulator's solid obstacles without a GPU: the torch statement against the numpy rule (tests/pbf_obstacle_rule.py)
bit for bit on the cases of tests/pbf_obstacle_cases.py, planted defects that each case must see, the host validation,
the C entry's argument checks, the untouched path without obstacles, the scene generator, a block of fluid dropped onto
a ball, the obstacles' mesh, and the CLI through the CPU checker."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pbf_obstacle_cases as K  # noqa: E402
import pbf_obstacle_rule as O  # noqa: E402
import pbf_rule as P  # noqa: E402

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
def test_torch_collide_equals_the_rule_bit_for_bit(cases, name):
    from tpgan_amd import ops
    case, want = cases[name]
    prm = ops.PbfParams()
    for b, (wp, wh) in enumerate(want):
        n = int(case["lengths"][b])
        hit = torch.zeros(n, dtype=torch.int32)
        got = ops._pbf_collide_torch(_t(case["p"][b, :n]), _t(case["lo"][b]), _t(case["hi"][b]), _t(case["table"][b]), prm, hit)
        assert _equal(got.numpy(), wp) and np.array_equal(hit.numpy(), wh), (name, b)
        again = ops._pbf_collide_torch(_t(case["p"][b, :n]), _t(case["lo"][b]), _t(case["hi"][b]), _t(case["table"][b]), prm)
        assert torch.equal(again, got)                                           # without hit: the same positions


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_torch_substep_with_obstacles_equals_the_rule_bit_for_bit(cases, name):
    """Every case as a fluid at rest (v = 0) for one substep: collide after predict and after every dp."""
    from tpgan_amd import ops
    case, _ = cases[name]
    prm = ops.PbfParams(iters=2)
    x, lengths = case["p"], case["lengths"]
    v = np.where(np.isnan(x), F32(np.nan), F32(0))
    B = len(lengths)
    xt, vt = ops._pbf_substep_torch(_t(x), _t(v), _t(lengths), ops.pbf_box(case["lo"], case["hi"], B), DT, prm,
                                    obstacles=_t(case["table"]))
    for b, n in enumerate(lengths.tolist()):
        xr, vr = O.substep_rule(x[b, :n], v[b, :n], case["lo"][b], case["hi"][b], DT, prm, case["table"][b])
        assert _equal(xt[b, :n].numpy(), xr) and _equal(vt[b, :n].numpy(), vr), (name, b)
        assert np.isnan(xt[b, n:].numpy()).all() and np.isnan(vt[b, n:].numpy()).all()


def test_torch_substep_equals_the_rule_on_a_moving_fluid():
    from tpgan_amd import ops
    case, v = K.drop_case()
    box = ops.pbf_box(case["lo"], case["hi"], 2)
    for prm in (ops.PbfParams(), ops.PbfParams(iters=0)):
        xt, vt = ops._pbf_substep_torch(_t(case["p"]), _t(v), _t(case["lengths"]), box, DT, prm, obstacles=_t(case["table"]))
        for b, n in enumerate(case["lengths"].tolist()):
            xr, vr = O.substep_rule(case["p"][b, :n], v[b, :n], case["lo"][b], case["hi"][b], DT, prm, case["table"][b])
            assert _equal(xt[b, :n].numpy(), xr) and _equal(vt[b, :n].numpy(), vr), (prm.iters, b)


# ---- planted defects: each case sees the defect it is for -----------------------------------------------------------------
def _highest_axis(pen):
    k1 = pen[1] <= pen[0]
    k2 = pen[2] <= np.where(k1, pen[1], pen[0])
    return np.where(k2, 2, np.where(k1, 1, 0))


DEFECTS = {                                                                      # name -> (function of the rule, defect, case)
    "non_strict_inside": ("_lt", lambda a, b: a <= b, "ball"),
    "writes_back_what_was_not_inside": ("_written", lambda inside: np.ones_like(inside), "rotation"),
    "no_final_clamp": ("_final_clamp", lambda p, lo, hi, prm: p, "wall"),
    "reversed_order": ("_order", lambda M: range(M - 1, -1, -1), "order"),
    "ties_to_the_highest_axis": ("_box_axis", _highest_axis, "box"),
    "cap_tie_goes_radial": ("_cap_first", lambda pen_h, pen_r: pen_h < pen_r, "cylinder"),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_each_case_sees_the_defect_it_was_built_for(cases, monkeypatch, defect):
    what, wrong, name = DEFECTS[defect]
    case, want = cases[name]
    assert all(_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) for g, w in zip(K.expected(case), want))
    monkeypatch.setattr(O, what, wrong)
    got = K.expected(case)
    assert any(not _equal(g[0], w[0]) for g, w in zip(got, want)), defect        # the POSITIONS differ, not only hit


# ---- host validation ----------------------------------------------------------------------------------------------------------
def test_pbf_obstacles_builds_the_table_and_validates_on_the_host():
    from tpgan_amd import ops
    ball = {"shape": "ball", "centre": [0.1, 0.2, 0.3], "size": 0.25}
    box = {"shape": "box", "centre": [0, 0, 0], "size": [0.1, 0.2, 0.3], "rotation": K.rotation((0, 0, 1), 90).reshape(-1).tolist()}
    cyl = {"shape": "cylinder", "centre": [1, 1, 1], "size": [0.1, 0.4]}
    shared = ops.pbf_obstacles([ball, box], B=3, device="cpu")
    assert shared.shape == (3, 2, 16) and shared.dtype == torch.float32 and torch.equal(shared[0], shared[2])
    assert np.array_equal(shared[0].numpy(), np.stack([K.row(1, ball["centre"], size=0.25),
                                                       K.row(2, (0, 0, 0), K.rotation((0, 0, 1), 90), (0.1, 0.2, 0.3))]))
    ragged = ops.pbf_obstacles([[ball], None, [cyl, box, ball]], device="cpu")
    assert ragged.shape == (3, 3, 16) and ragged[:, :, 0].tolist() == [[1, 0, 0], [0, 0, 0], [3, 2, 1]]
    assert np.array_equal(ragged[2, 0].numpy(), K.row(3, (1, 1, 1), size=(0.1, 0.4)))
    assert ops.pbf_obstacles(None, B=2, device="cpu").shape == (2, 0, 16)
    sheared = np.eye(3)
    sheared[0, 1] = 1e-3
    for bad in ([ball] * 9, [dict(ball, size=-0.1)], [dict(box, size=[0.1, 0.0, 0.1])], [dict(box, rotation=sheared.reshape(-1).tolist())],
                [dict(box, rotation=(2 * np.eye(3)).reshape(-1).tolist())], [dict(ball, centre=[0.0, float("nan"), 0.0])],
                [dict(cyl, centre=[float("inf"), 0, 0])], [dict(cyl, size=[0.1, float("inf")])], [dict(ball, shape="cone")],
                [dict(ball, size=[0.1, 0.2])], [{"shape": "ball", "size": 0.1}]):
        with pytest.raises(RuntimeError):
            ops.pbf_obstacles(bad, device="cpu")
    nearly = K.rotation((1, 2, 3), 20.0) + 4e-6                                  # within 1e-5 of orthonormal
    assert ops.pbf_obstacles([dict(box, rotation=nearly.reshape(-1).tolist())], device="cpu").shape == (1, 1, 16)
    # the ops refuse a table of the wrong shape before any backend is asked
    ops.unregister_backend("cpu")
    p = torch.zeros(2, 4, 3)
    for table in (torch.zeros(1, 1, 16), torch.zeros(2, 1, 15), torch.zeros(2, 9, 16), torch.zeros(2, 1, 16, dtype=torch.float64)):
        with pytest.raises(RuntimeError, match="obstacles"):
            ops.pbf_collide(p, None, [0, 0, 0], [1, 1, 1], table)
        with pytest.raises(RuntimeError, match="obstacles"):
            ops.pbf_substep(p, p, None, [0, 0, 0], [1, 1, 1], 0.01, obstacles=table)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pbf_collide(p, None, [0, 0, 0], [1, 1, 1], torch.zeros(2, 1, 16))


def test_collide_entry_rejects_bad_arguments_before_any_launch(hip_lib):
    buf = (C.c_float * 256)()
    p = C.cast(buf, C.c_void_p)
    box = np.array([[0, 0, 0, 1, 1, 1]], F32)
    flat = np.array([[0, 0, 0, 1, 0, 1]], F32)
    nan_box = np.array([[0, 0, 0, 1, np.nan, 1]], F32)
    nan = float("nan")

    def collide(p_=p, box=box, obstacles=p, B=1, N=4, M=2, a=0.0125, p_out=p, hit=p):
        return hip_lib.tpg_pbf_collide_f32(p_, None, None if box is None else box.ctypes.data, obstacles, B, N, M, a, p_out,
                                           hit, None)
    assert collide(B=-1) == -1 and collide(N=-1) == -1 and collide(M=-1) == -1
    assert collide(a=0.0) == -1 and collide(a=-1.0) == -1 and collide(a=nan) == -1 and collide(a=float("inf")) == -1
    assert collide(p_out=None) == -1 and collide(p_out=None, B=0) == -1 and collide(M=-1, N=0) == -1
    assert collide(B=0) == 0 and collide(N=0) == 0 and collide(B=0, p_=None, box=None, obstacles=None) == 0
    assert collide(N=0, M=9) == 0                                               # empty work is decided first
    assert collide(B=65536) == -3 and collide(N=(1 << 22) + 1) == -3 and collide(M=9) == -3
    assert collide(M=9, p_=None) == -3                                          # the limits before the other pointers
    assert collide(p_=None) == -1 and collide(box=None) == -1 and collide(box=flat) == -1 and collide(box=nan_box) == -1
    assert collide(obstacles=None) == -1 and collide(obstacles=None, M=1) == -1


# ---- without obstacles nothing changes -------------------------------------------------------------------------------------
def test_substep_without_obstacles_is_the_old_path(oracle_cpu, monkeypatch):
    import pbf_cases
    from tpgan_amd import ops

    def never(*a, **k):
        raise AssertionError("collide was reached without obstacles")
    monkeypatch.setattr(ops, "_pbf_collide_torch", never)
    monkeypatch.setattr(ops.backend_for(torch.zeros(1)), "pbf_collide", never, raising=False)
    x, v, lengths, lo, hi = pbf_cases.small_case()
    for kw in ({}, {"obstacles": None}):
        xs, vs = ops.pbf_substep(_t(x), _t(v), _t(lengths), lo, hi, DT, **kw)
        for b, n in enumerate(lengths.tolist()):
            xr, vr = P.substep_rule(x[b, :n], v[b, :n], lo[b], hi[b], DT, ops.PbfParams())
            assert _equal(xs[b, :n].numpy(), xr) and _equal(vs[b, :n].numpy(), vr)
    with pytest.raises(AssertionError, match="collide was reached"):
        ops.pbf_substep(_t(x), _t(v), _t(lengths), lo, hi, DT, obstacles=torch.zeros(2, 1, 16))


def test_collide_and_substep_through_the_checker_equal_the_rule(oracle_cpu, cases):
    from tpgan_amd import ops
    case, want = cases["rotation"]
    got, hit = ops.pbf_collide(_t(case["p"]), _t(case["lengths"]), case["lo"], case["hi"], _t(case["table"]), return_hit=True)
    alone = ops.pbf_collide(_t(case["p"]), _t(case["lengths"]), case["lo"], case["hi"], _t(case["table"]))
    assert torch.equal(alone, got) and hit.dtype == torch.int32
    for b, (wp, wh) in enumerate(want):
        assert _equal(got[b].numpy(), wp) and np.array_equal(hit[b].numpy(), wh)
    ragged, _ = cases["batch"]
    got, hit = ops.pbf_collide(_t(ragged["p"]), _t(ragged["lengths"]), ragged["lo"], ragged["hi"], _t(ragged["table"]),
                               return_hit=True)
    for b, (wp, wh) in enumerate(cases["batch"][1]):
        n = len(wp)
        assert _equal(got[b, :n].numpy(), wp) and np.array_equal(hit[b, :n].numpy(), wh)
        assert np.isnan(got[b, n:].numpy()).all() and not hit[b, n:].any()
    drop, v = K.drop_case()
    xs, vs = ops.pbf_substep(_t(drop["p"]), _t(v), _t(drop["lengths"]), drop["lo"], drop["hi"], DT, obstacles=_t(drop["table"]))
    xr, vr = O.substep_rule(drop["p"][1, :320], v[1, :320], drop["lo"][1], drop["hi"][1], DT, ops.PbfParams(), drop["table"][1])
    assert _equal(xs[1, :320].numpy(), xr) and _equal(vs[1, :320].numpy(), vr)


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def _signed_distance(obstacles, points, grow=0.0):
    """float64 signed distance of points (n,3) to the union of the obstacles grown by `grow` (exact for the ball; for
    the box and the cylinder the distance to the shape minus grow, which is the rounded expansion: a lower bound of the
    distance to the rule's sharp-edged one)."""
    from tpgan_amd import simulate as S
    return S.obstacle_distance(obstacles, torch.from_numpy(np.asarray(points, np.float64))).numpy() - grow


@pytest.mark.parametrize("seed", range(10))
def test_random_scene_without_obstacles_is_the_scene_it_was(seed):
    from tpgan_amd import simulate as S
    kw = dict(box=(1.2, 1.0, 1.2), body_size=0.2)
    a, b = S.random_scene(seed, **kw), S.random_scene(seed, obstacles=0, **kw)
    assert a.to_json() == b.to_json() and "obstacles" not in a.to_json() and a.obstacles == []
    assert all(np.array_equal(u, w) for u, w in zip(a.particles(), b.particles()))


@pytest.mark.parametrize("seed", [1, 2, (7, 1, 3)])
def test_random_scene_with_obstacles(seed):
    from tpgan_amd import ops
    from tpgan_amd import simulate as S
    kw = dict(box=(1.2, 1.0, 1.2), body_size=0.2, obstacles=2, obstacle_size=(0.15, 0.3))
    a, b = S.random_scene(seed, **kw), S.random_scene(seed, **kw)
    assert a.to_json() == b.to_json() and len(a.obstacles) == 2 and len(a.bodies) >= 1
    again = S.Scene.from_json(json.loads(json.dumps(a.to_json())))
    assert again.obstacles == a.obstacles and np.array_equal(again.particles()[0], a.particles()[0])
    assert ops.pbf_obstacles(a.obstacles, device="cpu").shape == (1, 2, 16)      # they pass the host validation
    spacing = 2 * a.radius
    for o in a.obstacles:
        c, bound = np.array(o["centre"]), S.obstacle_bound(o)
        assert o["shape"] in S.SHAPES and 2 * np.min(o["size"]) >= 4 * spacing and 2 * np.max(o["size"]) <= 0.3
        assert (c >= bound).all() and c[0] <= 1.2 - bound and c[2] <= 1.2 - bound and c[1] <= 0.5    # the lower half
    (c0, c1), (b0, b1) = [np.array(o["centre"]) for o in a.obstacles], [S.obstacle_bound(o) for o in a.obstacles]
    assert np.linalg.norm(c0 - c1) >= b0 + b1
    pos = a.particles()[0]
    assert len(pos) > 50 and (_signed_distance(a.obstacles, pos, a.radius) > 0).all()
    for body in a.bodies:                                                        # a spacing clear of every obstacle's sphere
        reach = np.linalg.norm(S.body_half_extent(body["shape"], body["size"])) + spacing
        assert all(np.linalg.norm(np.array(body["centre"]) - c) >= reach + bb for c, bb in ((c0, b0), (c1, b1)))
    with pytest.raises(ValueError):
        S.random_scene(1, obstacles=4)
    with pytest.raises(RuntimeError, match="no room"):
        S.random_scene(1, box=(0.3, 0.3, 0.3), body_size=0.05, obstacles=1)


# ---- a block of fluid dropped onto a ball ------------------------------------------------------------------------------------
def test_a_block_dropped_onto_a_ball_flows_round_it(monkeypatch):
    """12 x 12 x 6 particles dropped onto a ball of radius 0.1 in a corner of the box, 40 frames by the host statement.
    The expanded ball stays clear of the clamp planes (it hangs 5 mm above the floor's), so no wedge pins a particle.  After every frame each particle's float64 signed distance to the expanded ball is >= -1e-5 m: about ten
    fp32 roundings of values below 4 m come to at most 2.4e-6 m, and this allows four times that."""
    from tpgan_amd import ops
    from tpgan_amd import simulate as S
    ball = {"shape": "ball", "centre": [0.15, 0.13, 0.15], "size": 0.1}
    g = np.stack(np.meshgrid(np.arange(12), np.arange(6), np.arange(12), indexing="ij"), -1).reshape(-1, 3)
    pos = (np.array([0.04, 0.24, 0.04]) + g * 0.025).astype(F32)
    scene = S.Scene([0, 0, 0], [0.7, 0.6, 0.34], pos=pos, obstacles=[ball])
    ever = torch.zeros(len(pos), dtype=torch.int32)
    collide = ops._pbf_collide_torch

    def counting(p, lo, hi, table, prm, hit=None):
        mine = torch.zeros(p.shape[0], dtype=torch.int32)
        out = collide(p, lo, hi, table, prm, mine)
        ever.bitwise_or_(mine)
        return out
    monkeypatch.setattr(ops, "_pbf_collide_torch", counting)
    x, v, _, lo, hi = S.pack([scene], "cpu")
    table = S.obstacle_table([scene], "cpu")
    box, dt, prm = ops.pbf_box(lo, hi, 1), float(F32(1.0 / (S.FPS * S.SUBSTEPS))), ops.PbfParams()
    for frame in range(40):
        for _ in range(S.SUBSTEPS):
            x, v = ops._pbf_substep_torch(x, v, None, box, dt, prm, obstacles=table)
        sd = _signed_distance([ball], x[0].numpy(), float(F32(0.1) + F32(prm.radius)) - 0.1)
        assert bool(torch.isfinite(x).all()) and sd.min() >= -1e-5, (frame, sd.min())
    com = x[0].double().mean(0).numpy()
    print("drop onto a ball: centre of mass", com, "ever hit", int((ever > 0).sum()), "of", len(pos))
    assert _signed_distance([ball], com[None], 0.0125)[0] > 0                    # beside the ball: not inside it,
    assert com[1] < 0.13 and com[0] > 0.15 + 0.1125                               # nor above it, but on the open side
    assert 0 < int((ever > 0).sum()) < len(pos)


# ---- the obstacles' mesh --------------------------------------------------------------------------------------------------------
def _closed(faces):
    f = faces.numpy().astype(np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    return len(f) > 0 and bool((counts == 2).all())


def test_obstacle_mesh_is_closed_and_has_the_shapes_volume(oracle_cpu):
    from tpgan_amd import mesh
    from tpgan_amd import simulate as S
    h = 0.025
    r = 0.2
    ball = S.Scene([0, 0, 0], [1, 1, 1], obstacles=[{"shape": "ball", "centre": [0.5, 0.3, 0.5], "size": r}])
    m = S.obstacle_mesh(ball, device="cpu")
    assert m.lattice.step == float(F32(h)) and _closed(m.faces) and m.normals.shape == m.vertices.shape
    assert 4 / 3 * math.pi * (r - h) ** 3 <= mesh.volume(m) <= 4 / 3 * math.pi * (r + h) ** 3
    e = np.array([0.2, 0.12, 0.15])
    rot = K.rotation((0.3, -1.0, 0.55), 37.0).reshape(-1).tolist()
    box = S.Scene([0, 0, 0], [1, 1, 1], obstacles=[{"shape": "box", "centre": [0.5, 0.3, 0.5], "size": e.tolist(), "rotation": rot}])
    m = S.obstacle_mesh(box, step=h, device="cpu")
    edges = 2 * e
    dilated = edges.prod() + 2 * (edges[0] * edges[1] + edges[1] * edges[2] + edges[2] * edges[0]) * h \
        + math.pi * edges.sum() * h ** 2 + 4 / 3 * math.pi * h ** 3              # Steiner's formula for a box
    assert _closed(m.faces) and (2 * (e - h)).prod() <= mesh.volume(m) <= dilated
    c = m.vertices.double().numpy().mean(0)
    assert np.abs(c - [0.5, 0.3, 0.5]).max() < h
    with pytest.raises(RuntimeError, match="no obstacles"):
        S.obstacle_mesh(S.Scene([0, 0, 0], [1, 1, 1]), device="cpu")


# ---- the CLI through the CPU checker --------------------------------------------------------------------------------------------
def test_cli_writes_the_obstacles_beside_the_frames(oracle_cpu, tmp_path, capsys):
    from tpgan_amd import simulate as S
    from tpgan_amd.data import FluidSequences
    out = str(tmp_path / "train")
    argv = ["--out", out, "--cases", "1", "--frames", "3", "--seed", "4", "--box", "0.6", "0.6", "0.6", "--body_size", "0.11",
            "--substeps", "2", "--iters", "2", "--device", "cpu", "--obstacles", "1", "--obstacle_size", "0.12", "0.2"]
    assert S.main(argv) == 0
    capsys.readouterr()
    case = os.path.join(out, "case1")
    meta = json.load(open(os.path.join(case, "scene.json")))
    scene = S.Scene.from_json(meta)
    assert len(meta["obstacles"]) == 1 and scene.obstacles == meta["obstacles"] and meta["obstacle_size"] == [0.12, 0.2]
    assert scene.obstacles == S.random_scene([4, 0, 0], (0.6, 0.6, 0.6), body_size=0.11, obstacles=1,
                                             obstacle_size=(0.12, 0.2)).obstacles
    with open(os.path.join(case, "obstacles.ply"), "rb") as f:
        head = f.read(200)
    assert head.startswith(b"ply\nformat binary_little_endian") and b"element vertex" in head
    seq = FluidSequences(out, 1, 3, device="cpu")
    assert len(seq) == 1 and seq.pos.shape[0] == 3 * int(seq.count.sum())
    # the frames are the statement's with the scene's table
    pos, vel, _ = S.simulate([scene], 3, substeps=2, iters=2, device="cpu")
    with np.load(os.path.join(case, "data_2.npz")) as f:
        assert np.array_equal(f["pos"], pos[0, 2].numpy()) and np.array_equal(f["vel"], vel[0, 2].numpy())
    # a scene file without the key loads as it always did
    del meta["obstacles"]
    assert S.Scene.from_json(meta).obstacles == []
