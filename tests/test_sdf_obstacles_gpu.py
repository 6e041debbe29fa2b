"""The simulator's collide_sdf kernel (csrc/pbf.hip) against the numpy statement of its rule (tests/pbf_sdf_rule.py), bit
for bit, positions and hit bits, on the cases of tests/pbf_sdf_cases.py; then whole substeps and frames with mesh
obstacles, batch positions across the chunked launches, and the untouched path without them."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pbf_cases  # noqa: E402
import pbf_obstacle_cases as OK  # noqa: E402
import pbf_rule as P  # noqa: E402
import pbf_sdf_cases as K  # noqa: E402
import pbf_sdf_rule as S  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
DT = float(F32(1.0 / 160.0))
FRAMES, SUBSTEPS, ITERS = 5, 2, 2          # frame 0 and four simulated ones


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cases():
    """name -> (case, [(p, hit) per scene by the rule]); built once, never modified."""
    out = {}
    for name, build in K.CASES.items():
        case = build()
        out[name] = (case, K.expected(case))
    return out


@pytest.fixture(scope="module")
def drop():
    """The falling fluid of pbf_sdf_cases.drop_case and the rule's substep for the shipped parameters."""
    from tpgan_amd import ops
    case, v = K.drop_case()
    want = S.substep_rule(case["p"][0], v[0], case["lo"][0], case["hi"][0], DT, ops.PbfParams(), case["table"][0], case["fields"])
    return case, v, want


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, F32)
    return np.ascontiguousarray(a).view(np.int32)


def _equal(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _collide(dev, case, **kw):
    from tpgan_amd import ops
    return ops.pbf_collide_sdf(_up(case["p"], dev), _up(case["lengths"], dev), case["lo"], case["hi"], _up(case["table"], dev),
                               _up(case["fields"], dev), **kw)


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_collide_sdf_equals_the_rule_positions_and_hit_bits(dev, cases, name):
    from tpgan_amd import ops
    case, want = cases[name]
    got, hit = _collide(dev, case, return_hit=True)
    alone = _collide(dev, case)                                                  # hit_out == NULL
    be = ops.backend_for(torch.zeros(1, device=dev))
    B = len(case["lengths"])
    inplace = _up(case["p"], dev)                                                # p_out is p itself
    be.pbf_collide_sdf(inplace, _up(case["lengths"], dev), ops.pbf_box(case["lo"], case["hi"], B), _up(case["table"], dev),
                       _up(case["fields"], dev), ops.PbfParams(), inplace)
    assert hit.dtype == torch.int32 and hit.shape == got.shape[:2]
    for b, (wp, wh) in enumerate(want):
        n = len(wp)
        assert _equal(got[b, :n], wp), (name, b)
        assert np.array_equal(hit[b, :n].cpu().numpy(), wh), (name, b)
        assert _equal(alone[b, :n], wp) and _equal(inplace[b, :n], wp), (name, b)
        # rows beyond the length: never read (NaN there), never written
        assert all(bool(torch.isnan(t[b, n:]).all()) for t in (got, alone, inplace)) and not bool(hit[b, n:].any()), (name, b)


def test_substep_with_mesh_obstacles_equals_the_rule(dev, drop, cases):
    from tpgan_amd import ops
    case, v, (xr, vr) = drop
    X, V, L = _up(case["p"], dev), _up(v, dev), _up(case["lengths"], dev)
    sdf = (_up(case["table"], dev), _up(case["fields"], dev))
    xs, vs = ops.pbf_substep(X, V, L, case["lo"], case["hi"], DT, sdf_obstacles=sdf)
    assert _equal(xs[0], xr) and _equal(vs[0], vr)
    bare = P.substep_rule(case["p"][0], v[0], case["lo"][0], case["hi"][0], DT, ops.PbfParams())
    assert not _equal(bare[0], xr)                                               # the fields reach the result
    # behind an analytic obstacle: collide, then collide_sdf
    ball = np.stack([OK.row(1, (0.25, 0.12, 0.2), size=0.05)])[None]
    xs, vs = ops.pbf_substep(X, V, L, case["lo"], case["hi"], DT, obstacles=_up(ball, dev), sdf_obstacles=sdf)
    xb, vb = S.substep_rule(case["p"][0], v[0], case["lo"][0], case["hi"][0], DT, ops.PbfParams(), case["table"][0],
                            case["fields"], analytic=ball[0])
    assert _equal(xs[0], xb) and _equal(vs[0], vb) and not _equal(xb, xr)
    # the edge cases as a fluid at rest: lattice faces, skipped rows and four rows inside a whole substep
    few = ops.PbfParams(iters=ITERS)
    for name in ("faces", "skin", "skipped", "m4"):
        c, _ = cases[name]
        x = c["p"]
        z = np.where(np.isnan(x), F32(np.nan), F32(0))
        xs, vs = ops.pbf_substep(_up(x, dev), _up(z, dev), _up(c["lengths"], dev), c["lo"], c["hi"], DT, few,
                                 sdf_obstacles=(_up(c["table"], dev), _up(c["fields"], dev)))
        for b, n in enumerate(c["lengths"].tolist()):
            xw, vw = S.substep_rule(x[b, :n], z[b, :n], c["lo"][b], c["hi"][b], DT, few, c["table"][b], c["fields"])
            assert _equal(xs[b, :n], xw) and _equal(vs[b, :n], vw), (name, b)


def test_whole_frames_onto_an_icosphere_and_a_torus_equal_the_rules_trajectory_twice(dev, drop):
    """Four frames of the 500 particles that fall onto an icosphere field and a rotated torus field."""
    from tpgan_amd import ops
    case, v, _ = drop
    few = ops.PbfParams(iters=ITERS)
    sdf = (_up(case["table"], dev), _up(case["fields"], dev))

    def frames():
        x, vel, L = _up(case["p"], dev), _up(v, dev), _up(case["lengths"], dev)
        pos, vels = [], []
        for _ in range(FRAMES - 1):
            for _ in range(SUBSTEPS):
                x, vel = ops.pbf_substep(x, vel, L, case["lo"], case["hi"], float(F32(1.0 / (40.0 * SUBSTEPS))), few,
                                         sdf_obstacles=sdf)
            pos.append(x[0])
            vels.append(vel[0])
        return torch.stack(pos), torch.stack(vels)
    pos, vel = frames()
    again = frames()
    assert torch.equal(pos, again[0]) and torch.equal(vel, again[1])             # the same calls, the same bits
    wp, wv = S.frames_rule(case["p"][0], v[0], case["lo"][0], case["hi"][0], FRAMES - 1, SUBSTEPS, few, case["table"][0],
                           case["fields"])
    assert _equal(pos, wp) and _equal(vel, wv)
    bare, _ = P.frames_rule(case["p"][0], v[0], case["lo"][0], case["hi"][0], FRAMES - 1, SUBSTEPS, few)
    moved = (bare[-1] != wp[-1]).any(1).sum()
    assert moved > 100, moved                                                    # the fluid has run into the solids


def test_a_scene_gives_the_same_bits_at_every_batch_position_and_in_every_chunk(dev, drop, cases):
    """The drop scene alone, first and last of a batch of two, and at positions 0, 64 and 129 of the 130-scene batch
    (padded to N = 500): one row in each of the three launches of the chunked kernels.  The 130 scenes' fields and the
    drop's two share one buffer, the drop's rows re-based onto their place in it."""
    from tpgan_amd import ops
    case, v, (xr, vr) = drop
    big, _ = cases["batch"]
    fields = np.concatenate([big["fields"], case["fields"]])
    t0 = case["table"][0].copy()
    for r in t0:
        fl, dims, off = S.decode(r)
        r[:] = S.make_row(fl[0], fl[1:4], fl[4:13], fl[13:16], fl[16], dims, off + len(big["fields"]))
    x0, v0, lo0, hi0 = case["p"][0], v[0], case["lo"][0], case["hi"][0]

    def substep(x, vel, lengths, lo, hi, table):
        return ops.pbf_substep(_up(x, dev), _up(vel, dev), _up(np.asarray(lengths, np.int64), dev), lo, hi, DT,
                               sdf_obstacles=(_up(table, dev), _up(fields, dev)))
    alone = substep(x0[None], v0[None], [500], lo0[None], hi0[None], t0[None])
    assert _equal(alone[0][0], xr) and _equal(alone[1][0], vr)
    B, N, at = 130, 500, (0, 64, 129)
    x, vel = np.full((B, N, 3), np.nan, F32), np.full((B, N, 3), np.nan, F32)
    x[:, :48] = big["p"]
    vel[:, :48] = np.where(np.isnan(big["p"]), F32(np.nan), F32(0))
    lengths, lo, hi, table = big["lengths"].copy(), big["lo"].copy(), big["hi"].copy(), big["table"].copy()
    for order in ((0, 1), (1, 0)):
        i = [0 if o == 0 else 7 for o in order]                                  # scene 7 of the batch as the companion
        xx, vv, ll, llo, hhi, tt = x[i].copy(), vel[i].copy(), lengths[i].copy(), lo[i].copy(), hi[i].copy(), table[i].copy()
        k = order.index(0)
        xx[k], vv[k], ll[k], llo[k], hhi[k], tt[k] = x0, v0, 500, lo0, hi0, t0
        xs, vs = substep(xx, vv, ll, llo, hhi, tt)
        assert torch.equal(xs[k], alone[0][0]) and torch.equal(vs[k], alone[1][0]), order
    for b in at:
        x[b], vel[b], lengths[b], lo[b], hi[b], table[b] = x0, v0, 500, lo0, hi0, t0
    xs, vs = substep(x, vel, lengths, lo, hi, table)
    prm = ops.PbfParams()
    for b in range(B):
        n = int(lengths[b])
        if b in at:
            assert torch.equal(xs[b], alone[0][0]) and torch.equal(vs[b], alone[1][0]), b
        else:
            wx, wv = S.substep_rule(x[b, :n], vel[b, :n], lo[b], hi[b], DT, prm, table[b], fields)
            assert _equal(xs[b, :n], wx) and _equal(vs[b, :n], wv), b
            assert bool(torch.isnan(xs[b, n:]).all()) and bool(torch.isnan(vs[b, n:]).all())


def test_no_mesh_obstacles_and_a_table_of_skipped_rows_are_the_substep_without(dev, cases):
    from tpgan_amd import ops
    x, v, lengths, lo, hi = pbf_cases.small_case()
    X, V, L = _up(x, dev), _up(v, dev), _up(lengths, dev)
    old = ops.pbf_substep(X, V, L, lo, hi, DT)
    none = ops.pbf_substep(X, V, L, lo, hi, DT, sdf_obstacles=None)
    skipped, _ = cases["skipped"]
    rows = np.ascontiguousarray(np.broadcast_to(skipped["table"][0], (2, 4, 24)))          # scene 0: four skipped rows
    pads = (torch.zeros(2, 3, 24, device=dev), torch.zeros(0, device=dev))
    bad = (_up(rows, dev), _up(skipped["fields"], dev))
    empty = ops.pbf_sdf_obstacles(None, B=2, device=dev)
    for b, n in enumerate(lengths.tolist()):
        xr, vr = P.substep_rule(x[b, :n], v[b, :n], lo[b], hi[b], DT, ops.PbfParams())
        for xs, vs in (old, none, ops.pbf_substep(X, V, L, lo, hi, DT, sdf_obstacles=pads),
                       ops.pbf_substep(X, V, L, lo, hi, DT, sdf_obstacles=bad),
                       ops.pbf_substep(X, V, L, lo, hi, DT, sdf_obstacles=empty)):
            assert _equal(xs[b, :n], xr) and _equal(vs[b, :n], vr), b
    # None launches nothing new; a table does, once after predict and once after every dp
    for sdf, launches in ((None, 0), (pads, 1 + ops.PBF_ITERS)):
        timer = ops.OpTimer()
        ops.set_timer(timer)
        try:
            ops.pbf_substep(X, V, L, lo, hi, DT, sdf_obstacles=sdf)
            torch.cuda.synchronize()
        finally:
            ops.set_timer(None)
        assert len(timer.pending.get("pbf_collide_sdf", [])) == launches and "pbf_collide" not in timer.pending
        assert len(timer.pending["pbf_dp"]) == ops.PBF_ITERS


def test_the_fields_of_the_op_on_the_device_drive_the_same_collide(dev):
    """mesh out -> mesh in on the device: `ops.mesh_sdf` at the nodes of a lattice gives the field the rule's own
    (numpy) distances give, so `pbf_sdf_obstacles` built from it moves the drop's particles to the same bits."""
    from tpgan_amd import ops
    from tpgan_amd.mesh import make_icosphere
    sv, sf = make_icosphere(1, 0.07)
    field, origin, step = K.mesh_field(sv, sf, float(K.A), 0.04)
    dims = field.shape
    pos = (origin + np.stack(np.meshgrid(*[np.arange(n, dtype=F32) for n in dims], indexing="ij"), -1) * step).astype(F32)
    d, _ = ops.mesh_sdf(_up(pos.reshape(-1, 3), dev), _up(sv, dev), _up(sf, dev))
    assert _equal(d.view(dims), field)
    ob = {"field": d.view(dims), "origin": origin, "step": step, "centre": (0.16, 0.1, 0.2)}
    table, fields = ops.pbf_sdf_obstacles([ob, dict(ob, centre=(0.3, 0.1, 0.2))], device=dev)
    assert table.shape == (1, 2, 24) and fields.numel() == field.size                # one copy of the shared field
    case, _ = K.drop_case()
    got = ops.pbf_collide_sdf(_up(case["p"], dev), None, case["lo"], case["hi"], table, fields)
    want = S.collide_sdf_rule(case["p"][0], case["lo"][0], case["hi"][0], table[0].cpu().numpy(), field.reshape(-1),
                              ops.PbfParams())
    assert _equal(got[0], want) and not _equal(want, case["p"][0])


def test_simulate_with_a_mesh_body_and_a_mesh_obstacle_equals_the_rules_trajectory(dev):
    """simulate() end to end on the device: an icosphere of fluid (`body_points` through `ops.mesh_sdf`) falls onto a torus
    obstacle whose field `sdf_obstacle_table` samples; the frames are the rule's with that table and those fields."""
    from tpgan_amd import ops
    from tpgan_amd import simulate as sim
    body = {"shape": "mesh", "mesh": "icosphere:2", "size": 0.2, "rotation": np.eye(3).reshape(-1).tolist(),
            "centre": [0.25, 0.3, 0.25], "velocity": [0.0, -1.0, 0.0]}
    torus = {"shape": "mesh", "mesh": "torus:0.5,0.25,16,8", "size": 0.3, "centre": [0.25, 0.0625, 0.25]}
    scene = sim.Scene([0, 0, 0], [0.5, 0.5, 0.5], [body], obstacles=[torus])
    pts = sim.body_points(body, 0.025, device=dev)
    d, _ = ops.mesh_sdf(_up((pts - body["centre"]).astype(F32), dev), *(_up(a, dev) for a in sim.mesh_geometry("icosphere:2", 0.2)[:2]))
    assert 100 < len(pts) < 600 and float(d.max()) <= -0.0125                    # every particle's sphere inside the mesh
    few = ops.PbfParams(iters=ITERS)
    pos, vel, lengths = sim.simulate([scene], 4, SUBSTEPS, params=few, device=dev)
    table, fields = sim.sdf_obstacle_table([scene], dev)
    x0, v0 = scene.particles()
    wp, wv = S.frames_rule(x0, v0, np.zeros(3, F32), np.full(3, 0.5, F32), 3, SUBSTEPS, few, table[0].cpu().numpy(),
                           fields.cpu().numpy())
    assert lengths.tolist() == [len(pts)] and _equal(pos[0, 0], x0)
    assert _equal(pos[0, 1:], wp) and _equal(vel[0, 1:], wv)
    assert float(sim.obstacle_distance([torus], pos[0, 3]).min()) >= -0.0125
