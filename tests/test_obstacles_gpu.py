"""The simulator's collide kernel (csrc/pbf.hip) against the numpy statement of its rule (tests/pbf_obstacle_rule.py), bit
for bit, positions and hit bits, on the cases of tests/pbf_obstacle_cases.py; then whole substeps and frames with
obstacles, batch positions across the chunked launches, the untouched path without obstacles, and the table across
batch shapes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pbf_cases  # noqa: E402
import pbf_obstacle_cases as K  # noqa: E402
import pbf_obstacle_rule as O  # noqa: E402
import pbf_rule as P  # noqa: E402

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
    """The moving fluid of pbf_obstacle_cases.drop_case and the rule's substep per scene for the shipped parameters."""
    from tpgan_amd import ops
    case, v = K.drop_case()
    want = [O.substep_rule(case["p"][b, :n], v[b, :n], case["lo"][b], case["hi"][b], DT, ops.PbfParams(), case["table"][b])
            for b, n in enumerate(case["lengths"].tolist())]
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
    return ops.pbf_collide(_up(case["p"], dev), _up(case["lengths"], dev), case["lo"], case["hi"], _up(case["table"], dev), **kw)


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_collide_equals_the_rule_positions_and_hit_bits(dev, cases, name):
    from tpgan_amd import ops
    case, want = cases[name]
    got, hit = _collide(dev, case, return_hit=True)
    alone = _collide(dev, case)                                                  # hit_out == NULL
    # p_out is p itself
    be = ops.backend_for(torch.zeros(1, device=dev))
    B = len(case["lengths"])
    inplace = _up(case["p"], dev)
    be.pbf_collide(inplace, _up(case["lengths"], dev), ops.pbf_box(case["lo"], case["hi"], B), _up(case["table"], dev),
                   ops.PbfParams(), inplace)
    assert hit.dtype == torch.int32 and hit.shape == got.shape[:2]
    for b, (wp, wh) in enumerate(want):
        n = len(wp)
        assert _equal(got[b, :n], wp), (name, b)
        assert np.array_equal(hit[b, :n].cpu().numpy(), wh), (name, b)
        assert _equal(alone[b, :n], wp) and _equal(inplace[b, :n], wp), (name, b)
        # rows beyond the length: never read (NaN there), never written
        assert all(bool(torch.isnan(t[b, n:]).all()) for t in (got, alone, inplace)) and not bool(hit[b, n:].any()), (name, b)


def test_substep_with_obstacles_equals_the_rule(dev, drop, cases):
    from tpgan_amd import ops
    case, v, want = drop
    X, V, L, T = _up(case["p"], dev), _up(v, dev), _up(case["lengths"], dev), _up(case["table"], dev)
    xs, vs = ops.pbf_substep(X, V, L, case["lo"], case["hi"], DT, obstacles=T)
    for b, (xr, vr) in enumerate(want):
        n = len(xr)
        assert _equal(xs[b, :n], xr) and _equal(vs[b, :n], vr), b
        assert bool(torch.isnan(xs[b, n:]).all()) and bool(torch.isnan(vs[b, n:]).all())
        bare = P.substep_rule(case["p"][b, :n], v[b, :n], case["lo"][b], case["hi"][b], DT, ops.PbfParams())
        assert not _equal(bare[0], xr)                                           # the obstacles reach the result
    none = ops.PbfParams(iters=0)                                                # predict | collide | grid | finish
    xs, vs = ops.pbf_substep(X, V, L, case["lo"], case["hi"], DT, none, obstacles=T)
    for b, n in enumerate(case["lengths"].tolist()):
        xr, vr = O.substep_rule(case["p"][b, :n], v[b, :n], case["lo"][b], case["hi"][b], DT, none, case["table"][b])
        assert _equal(xs[b, :n], xr) and _equal(vs[b, :n], vr), b
    # the edge cases as a fluid at rest: ties, skipped rows and eight obstacles inside a whole substep
    few = ops.PbfParams(iters=ITERS)
    for name in ("box", "cylinder", "skipped", "m8"):
        c, _ = cases[name]
        x = c["p"]
        z = np.where(np.isnan(x), F32(np.nan), F32(0))
        xs, vs = ops.pbf_substep(_up(x, dev), _up(z, dev), _up(c["lengths"], dev), c["lo"], c["hi"], DT, few,
                                 obstacles=_up(c["table"], dev))
        for b, n in enumerate(c["lengths"].tolist()):
            xr, vr = O.substep_rule(x[b, :n], z[b, :n], c["lo"][b], c["hi"][b], DT, few, c["table"][b])
            assert _equal(xs[b, :n], xr) and _equal(vs[b, :n], vr), (name, b)


def test_whole_frames_with_obstacles_equal_the_rules_trajectory_twice(dev, drop):
    """Four frames of the 500 particles that fall onto a ball and a rotated box, through simulate() and its table."""
    from tpgan_amd import ops
    from tpgan_amd import simulate as S
    case, v, _ = drop
    scene = S.Scene(case["lo"][0], case["hi"][0], pos=case["p"][0, :500], vel=v[0, :500], obstacles=K.as_dicts(case["table"][0]))
    assert np.array_equal(S.obstacle_table([scene], "cpu")[0].numpy(), case["table"][0])
    few = ops.PbfParams(iters=ITERS)
    pos, vel, lengths = S.simulate([scene], FRAMES, SUBSTEPS, ITERS, device=dev)
    again = S.simulate([scene], FRAMES, SUBSTEPS, ITERS, device=dev)
    assert torch.equal(pos, again[0]) and torch.equal(vel, again[1])             # the same call, the same bits
    wp, wv = O.frames_rule(case["p"][0, :500], v[0, :500], case["lo"][0], case["hi"][0], FRAMES - 1, SUBSTEPS, few, case["table"][0])
    assert lengths.tolist() == [500] and _equal(pos[0, 0], case["p"][0, :500])
    assert _equal(pos[0, 1:], wp) and _equal(vel[0, 1:], wv)
    bare, _ = P.frames_rule(case["p"][0, :500], v[0, :500], case["lo"][0], case["hi"][0], FRAMES - 1, SUBSTEPS, few)
    moved = (bare[-1] != wp[-1]).any(1).sum()
    assert moved > 100, moved                                                    # the fluid has run into the obstacles


def test_a_scene_gives_the_same_bits_at_every_batch_position_and_in_every_chunk(dev, drop, cases):
    """The drop's first scene alone, first and last of a batch of two, and at positions 0, 64 and 129 of the 130-scene
    batch (padded to N = 500, M = 3): one row in each of the three launches of the chunked kernels."""
    from tpgan_amd import ops
    case, v, want = drop
    x0, v0, lo0, hi0, t0 = case["p"][0], v[0], case["lo"][0], case["hi"][0], case["table"][0]
    xr, vr = want[0]

    def substep(x, vel, lengths, lo, hi, table):
        return ops.pbf_substep(_up(x, dev), _up(vel, dev), _up(np.asarray(lengths, np.int64), dev), lo, hi, DT,
                               obstacles=_up(table, dev))
    alone = substep(x0[None], v0[None], [500], lo0[None], hi0[None], t0[None])
    assert _equal(alone[0][0], xr) and _equal(alone[1][0], vr)
    for order in ((0, 1), (1, 0)):
        i = list(order)
        xs, vs = substep(case["p"][i], v[i], case["lengths"][i], case["lo"][i], case["hi"][i], case["table"][i])
        at = order.index(0)
        assert torch.equal(xs[at], alone[0][0]) and torch.equal(vs[at], alone[1][0]), order
        assert _equal(xs[1 - at, :320], want[1][0]) and _equal(vs[1 - at, :320], want[1][1]), order
    big, _ = cases["batch"]
    B, N, at = 130, 500, (0, 64, 129)
    x, vel = np.full((B, N, 3), np.nan, F32), np.full((B, N, 3), np.nan, F32)
    x[:, :48] = big["p"]
    vel[:, :48] = np.where(np.isnan(big["p"]), F32(np.nan), F32(0))
    lengths, lo, hi, table = big["lengths"].copy(), big["lo"].copy(), big["hi"].copy(), big["table"].copy()
    for b in at:
        x[b], vel[b], lengths[b], lo[b], hi[b] = x0, v0, 500, lo0, hi0
        table[b] = 0
        table[b, :2] = t0
    xs, vs = substep(x, vel, lengths, lo, hi, table)
    prm = ops.PbfParams()
    for b in range(B):
        n = int(lengths[b])
        if b in at:
            assert torch.equal(xs[b], alone[0][0]) and torch.equal(vs[b], alone[1][0]), b
        else:
            wx, wv = O.substep_rule(x[b, :n], vel[b, :n], lo[b], hi[b], DT, prm, table[b])
            assert _equal(xs[b, :n], wx) and _equal(vs[b, :n], wv), b
            assert bool(torch.isnan(xs[b, n:]).all()) and bool(torch.isnan(vs[b, n:]).all())


def test_no_obstacles_and_a_table_of_padding_rows_are_the_substep_without(dev):
    from tpgan_amd import ops
    x, v, lengths, lo, hi = pbf_cases.small_case()
    X, V, L = _up(x, dev), _up(v, dev), _up(lengths, dev)
    old = ops.pbf_substep(X, V, L, lo, hi, DT)
    none = ops.pbf_substep(X, V, L, lo, hi, DT, obstacles=None)
    padding = ops.pbf_substep(X, V, L, lo, hi, DT, obstacles=torch.zeros(2, 3, 16, device=dev))
    empty = ops.pbf_substep(X, V, L, lo, hi, DT, obstacles=ops.pbf_obstacles(None, B=2, device=dev))
    for b, n in enumerate(lengths.tolist()):
        xr, vr = P.substep_rule(x[b, :n], v[b, :n], lo[b], hi[b], DT, ops.PbfParams())
        for xs, vs in (old, none, padding, empty):
            assert _equal(xs[b, :n], xr) and _equal(vs[b, :n], vr), b
    # None launches nothing for the obstacles; a table does, once after predict and once after every dp
    for table, launches in ((None, 0), (torch.zeros(2, 3, 16, device=dev), 1 + ops.PBF_ITERS)):
        timer = ops.OpTimer()
        ops.set_timer(timer)
        try:
            ops.pbf_substep(X, V, L, lo, hi, DT, obstacles=table)
            torch.cuda.synchronize()
        finally:
            ops.set_timer(None)
        assert len(timer.pending.get("pbf_collide", [])) == launches and len(timer.pending["pbf_dp"]) == ops.PBF_ITERS


def test_a_small_batch_after_a_large_one_with_another_M_sees_only_its_own_table(dev, cases):
    """batch (130 x 48, M = 3), m8 (1 x 38, M = 8), rotation (3 x 120, M = 2), m0 (M = 0) and m8 again, back to back on
    one stream, each equal to its reference."""
    names = ("batch", "m8", "rotation", "m0", "m8")
    runs = [_collide(dev, cases[name][0], return_hit=True) for name in names]
    torch.cuda.synchronize()
    for name, (got, hit) in zip(names, runs):
        for b, (wp, wh) in enumerate(cases[name][1]):
            n = len(wp)
            assert _equal(got[b, :n], wp) and np.array_equal(hit[b, :n].cpu().numpy(), wh), (name, b)
