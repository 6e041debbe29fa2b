"""The fluid simulator without a GPU: the torch statement of its rule against the numpy one (tests/pbf_rule.py) bit for
bit, the lattice constant, the scene generator, the C entries' argument checks, the CLI through the CPU checker, and the
behaviour of the statement itself with the shipped parameters."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pbf_cases  # noqa: E402
import pbf_rule as P  # noqa: E402

F32 = np.float32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- the rule ---------------------------------------------------------------------------------------------------------
def test_lattice_sum_and_a_lattice_at_rest():
    from tpgan_amd import ops
    brute = sum(max(1.0 - (x * x + y * y + z * z) / 4.0, 0.0) ** 3
                for x in range(-3, 4) for y in range(-3, 4) for z in range(-3, 4))
    assert ops.pbf_lattice_sum() == P.lattice_sum() == brute == 5.15625         # 1 + 6 (3/4)^3 + 12 (1/2)^3 + 8 (1/4)^3
    prm = ops.PbfParams()
    assert prm.S0 == 5.15625 and prm.h == float(F32(0.05)) and prm.radius == float(F32(0.0125))
    assert prm.dp_scale == float(F32(-7.0 * 0.05 * 5.15625 / 64.0)) and prm.cs == float(F32(ops.PBF_XSPH / 5.15625))
    assert prm.wq == float(F32(0.96 ** 3)) and prm.iters == ops.PBF_ITERS and prm.gravity[1] == float(F32(-9.81))
    # a = 2^-6: every coordinate, distance and weight of the lattice is exact in fp32, so C is exactly 0 inside it
    exact = ops.PbfParams(radius=2.0 ** -6)
    g = np.stack(np.meshgrid(*[np.arange(7)] * 3, indexing="ij"), -1).reshape(-1, 3)
    p = (g * 2.0 ** -5).astype(F32)
    lam, Cn = P.lambda_rule(p, exact)
    inside = ((g >= 2) & (g <= 4)).all(1)
    assert inside.sum() == 27 and (Cn[inside] == 0).all() and (lam[inside] == 0).all()
    assert (Cn == 0).all()                                                       # the rim is below the rest density
    lam_t, C_t, _ = ops._pbf_lambda_torch(_t(p), exact)
    assert np.array_equal(C_t.numpy(), Cn) and np.array_equal(lam_t.numpy(), lam)
    # squeezed by 10 %: the inside is above it
    _, squeezed = P.lambda_rule((p * F32(0.9)).astype(F32), exact)
    assert (squeezed[inside] > 0.1).all()


def test_torch_statement_equals_the_numpy_rule_bit_for_bit():
    from tpgan_amd import ops
    prm = ops.PbfParams()
    dt = float(F32(1.0 / 160.0))
    for case in (pbf_cases.small_case(), pbf_cases.tiny_case()):
        x, v, lengths, lo, hi = case
        box = ops.pbf_box(lo, hi, 2)
        xt, vt = ops._pbf_substep_torch(_t(x), _t(v), _t(lengths), box, dt, prm)
        for b in range(2):
            n = int(lengths[b])
            xr, vr = P.substep_rule(x[b, :n], v[b, :n], lo[b], hi[b], dt, prm)
            assert np.array_equal(xt[b, :n].numpy(), xr) and np.array_equal(vt[b, :n].numpy(), vr)
            assert np.isnan(xt[b, n:].numpy()).all() and np.isnan(vt[b, n:].numpy()).all()
            assert np.isfinite(xr).all() and np.isfinite(vr).all()
            if n > 1:
                assert not np.array_equal(xr, x[b, :n])
    # the pieces, on the first cloud's predicted positions
    x, v, lengths, lo, hi = pbf_cases.small_case()
    p, _ = P.predict_rule(x[0], v[0], lo[0], hi[0], dt, prm)
    assert (p[:, 0] == lo[0, 0] + pbf_cases.A).any() and (p[:, 0] == hi[0, 0] - pbf_cases.A).any()     # walls are touched
    lam, Cn = P.lambda_rule(p, prm)
    lam_t, C_t, pr = ops._pbf_lambda_torch(_t(p), prm)
    assert np.array_equal(lam_t.numpy(), lam) and np.array_equal(C_t.numpy(), Cn) and (Cn > 0).sum() > 100
    assert int(torch.bincount(pr.i).max()) > 64                                  # several trips of the candidate loop
    pn, dp = P.dp_rule(p, lam, lo[0], hi[0], prm)
    pn_t, dp_t = ops._pbf_dp_torch(_t(p), lam_t, pr, _t(lo[0]), _t(hi[0]), prm)
    assert np.array_equal(pn_t.numpy(), pn) and np.array_equal(dp_t.numpy(), dp) and np.abs(dp).max() > 1e-3
    dup = np.all(p[-20:, None, :] == p[None, :-20, :], -1).any(1)
    assert dup.sum() >= 10                                                       # duplicates that no wall separated


NEW_CASES = ("chunk", "wide", "flat", "clamp")


@pytest.fixture(scope="module")
def cases():
    """name -> (the batch, its parameters, its dt, the rule's substep per scene); built once, never modified."""
    out = {}
    for name in NEW_CASES + ("small",):
        batch, prm, dt = pbf_cases.CASES[name][0](), pbf_cases.params(name), pbf_cases.CASES[name][2]
        out[name] = (batch, prm, dt, _rule_substeps(batch, dt, prm))
    return out


def _rule_substeps(batch, dt, prm, box_row=lambda b: b):
    x, v, lengths, lo, hi = batch
    return [P.substep_rule(x[b, :n], v[b, :n], lo[box_row(b)], hi[box_row(b)], dt, prm)
            for b, n in enumerate(lengths.tolist())]


def _statement_equals(batch, dt, prm, want, lengths="own"):
    from tpgan_amd import ops
    x, v, own, lo, hi = batch
    L = None if lengths is None else _t(own)
    xt, vt = ops._pbf_substep_torch(_t(x), _t(v), L, ops.pbf_box(lo, hi, x.shape[0]), dt, prm)
    for b, (xr, vr) in enumerate(want):
        n = len(xr)
        assert np.array_equal(xt[b, :n].numpy(), xr) and np.array_equal(vt[b, :n].numpy(), vr), b
        for got, given in ((xt, x), (vt, v)):                                   # rows beyond the length come back as given
            assert np.array_equal(got[b, n:].numpy(), given[b, n:], equal_nan=True)
        assert np.isfinite(xr).all() and np.isfinite(vr).all()


@pytest.mark.parametrize("name", NEW_CASES)
def test_torch_statement_equals_the_rule_at_the_batch_grid_and_clamp_edges(cases, name):
    batch, prm, dt, want = cases[name]
    _statement_equals(batch, dt, prm, want)


@pytest.mark.parametrize("variant", sorted(pbf_cases.VARIANTS))
def test_torch_statement_equals_the_rule_with_other_parameters(cases, variant):
    from tpgan_amd import ops
    batch, _, dt, shipped = cases["small"]
    prm = ops.PbfParams(**pbf_cases.VARIANTS[variant])
    want = _rule_substeps(batch, dt, prm)
    assert not np.array_equal(want[0][1], shipped[0][1])                        # the parameter reaches the result
    _statement_equals(batch, dt, prm, want)


def test_torch_statement_without_lengths_and_with_lengths_outside_0_N(cases):
    """lengths = None is N; a length is clamped into [0, N] as the 64-bit value it is: N + 7 and 2^32 + 5 are N, -3 is 0."""
    from tpgan_amd import ops
    _, prm, dt, _ = cases["small"]
    full = pbf_cases.full_small()
    x, v, _, lo, hi = full
    want = _rule_substeps(full, dt, prm)
    _statement_equals(full, dt, prm, want, lengths=None)
    for given, means in pbf_cases.odd_lengths(700):
        xt, vt = ops._pbf_substep_torch(_t(x), _t(v), torch.tensor(given), ops.pbf_box(lo, hi, 2), dt, prm)
        for b, n in enumerate(means):
            assert np.array_equal(xt[b].numpy(), want[b][0] if n else x[b]), (given, b)
            assert np.array_equal(vt[b].numpy(), want[b][1] if n else v[b]), (given, b)


# ---- planted defects: each case sees the defect it is for ------------------------------------------------------------
def _differs(got, want):
    return not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))


def test_chunk_case_sees_another_chunks_box_row(cases):
    batch, prm, dt, want = cases["chunk"]
    wrong = _rule_substeps(batch, dt, prm, box_row=lambda b: b % 64)            # box.c[blockIdx.y] without b0, in one launch
    lengths = batch[2]
    assert all(not _differs(wrong[b], want[b]) for b in range(64))
    assert all(_differs(wrong[b], want[b]) for b in range(64, 130) if lengths[b] > 0)
    assert (lengths[64:] > 0).sum() >= 60 and lengths[128] > 0 and lengths[129] > 0


@pytest.mark.parametrize("defect", ["none", "after_conversion"])
def test_clamp_case_sees_a_missing_and_a_late_term_clamp(cases, monkeypatch, defect):
    batch, prm, dt, want = cases["clamp"]
    bound = np.int64(1024) << 30

    def fix30(term, mask, count=None):
        with np.errstate(all="ignore"):
            q = (np.where(mask, term, F32(0)) * P.U30).astype(np.int64)
            if defect == "after_conversion":                                    # clamps what the conversion left of the term
                q = np.clip(q, -bound, bound)
        return q.sum(1, dtype=np.int64).astype(F32) * P.INV_U30
    monkeypatch.setattr(P, "_fix30", fix30)
    wrong = _rule_substeps(batch, dt, prm)
    if defect == "none":
        assert all(_differs(wrong[b], want[b]) for b in range(2))
    else:
        assert _differs(wrong[1], want[1])                                      # scene 1 has the terms beyond 2^33


def _walk_pairs(keep):
    """pbf_rule.Pairs restricted to the candidates `keep(grid)` lists per particle."""
    class Walked(P.Pairs):
        def __init__(self, p, prm):
            super().__init__(p, prm)
            seen = np.zeros(self.near.shape, bool)
            for i, cand in enumerate(keep(pbf_cases.Grid(p, prm.h))):
                seen[i, cand] = True
            self.near, self.grad = self.near & seen, self.grad & seen
    return Walked


@pytest.mark.parametrize("name", ["wide", "flat"])
def test_the_grid_walk_stated_in_numpy_reaches_every_neighbour(cases, monkeypatch, name):
    """The walk of tests/pbf_cases.py is what the planted defects below alter: unaltered, it changes nothing."""
    batch, prm, dt, want = cases[name]
    monkeypatch.setattr(P, "Pairs", _walk_pairs(lambda g: g.walks()))
    assert not any(_differs(a, b) for a, b in zip(_rule_substeps(batch, dt, prm), want))


def test_wide_case_sees_a_walk_that_stops_after_64_candidates(cases, monkeypatch):
    batch, prm, dt, want = cases["wide"]
    monkeypatch.setattr(P, "Pairs", _walk_pairs(lambda g: [w[:64] for w in g.walks()]))
    wrong = _rule_substeps(batch, dt, prm)
    assert all(_differs(wrong[b], want[b]) for b in range(2))


def test_flat_case_sees_a_wrong_bound_on_an_axis_of_one_cell(cases, monkeypatch):
    batch, prm, dt, want = cases["flat"]
    monkeypatch.setattr(P, "Pairs", _walk_pairs(lambda g: g.walks(lower_strict=True)))      # yy > 0 for yy >= 0
    wrong = _rule_substeps(batch, dt, prm)
    assert all(_differs(wrong[b], want[b]) for b in range(2))


def test_substep_validates_and_refuses_cpu_tensors_without_a_checker():
    from tpgan_amd import ops
    ops.unregister_backend("cpu")
    x = torch.zeros(1, 4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pbf_substep(x, x, None, [0, 0, 0], [1, 1, 1], 0.01)
    for bad in (dict(dt=0.0), dict(dt=float("nan")), dict(hi=[1, 0, 1]), dict(v=torch.zeros(1, 5, 3)),
                dict(x=torch.zeros(1, 4, 3, dtype=torch.float64))):
        kw = dict(x=x, v=x, dt=0.01, hi=[1, 1, 1])
        kw.update(bad)
        with pytest.raises(RuntimeError):
            ops.pbf_substep(kw["x"], kw["v"], None, [0, 0, 0], kw["hi"], kw["dt"])
    with pytest.raises(RuntimeError):
        ops.PbfParams(eps=-1.0)


def test_substep_through_the_checker_equals_the_statement(oracle_cpu):
    from tpgan_amd import ops
    x, v, lengths, lo, hi = pbf_cases.tiny_case()
    got = ops.pbf_substep(_t(x), _t(v), _t(lengths), lo, hi, 1.0 / 160.0)
    want = ops._pbf_substep_torch(_t(x), _t(v), _t(lengths), ops.pbf_box(lo, hi, 2), float(F32(1.0 / 160.0)), ops.PbfParams())
    assert all(np.array_equal(g.numpy(), w.numpy(), equal_nan=True) for g, w in zip(got, want))
    # one particle in free fall: v = v0 + dt g, x = x0 + dt v, clamped at the floor
    assert got[0][0, 0, 1] == F32(0.0125) and got[0][0, 0, 0] > 0.05            # the floor caught it; x moved on


# ---- scenes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, (7, 1, 3)])
def test_random_scene_is_reproducible_inside_the_box_and_without_overlap(seed):
    from scipy.spatial import cKDTree
    from tpgan_amd import simulate as S
    kw = dict(box=(1.2, 1.0, 1.2), body_size=0.2)
    a, b = S.random_scene(seed, **kw), S.random_scene(seed, **kw)
    assert a.to_json() == b.to_json() and 1 <= len(a.bodies) <= 3
    pa, va = a.particles()
    pb, vb = b.particles()
    assert np.array_equal(pa, pb) and np.array_equal(va, vb) and pa.dtype == F32 and len(pa) > 50
    assert (pa >= a.radius).all() and (pa <= np.array(a.box_hi) - a.radius).all()
    again = S.Scene.from_json(json.loads(json.dumps(a.to_json()))).particles()
    assert np.array_equal(again[0], pa) and np.array_equal(again[1], va)
    other = S.random_scene(12345, **kw)
    assert other.to_json() != a.to_json()
    parts = [S.body_points(body, 2 * a.radius) for body in a.bodies]
    for body, pts in zip(a.bodies, parts):
        assert body["shape"] in S.SHAPES and 0.1 <= body["size"] <= 0.3
        vx, vy, vz = body["velocity"]
        assert abs(vx) <= 2 and abs(vz) <= 2 and abs(vy) <= 0.5
        d, _ = cKDTree(pts).query(pts, k=2)
        assert d[:, 1].min() > 2 * a.radius * 0.999                              # a lattice of one spacing
    for i in range(len(parts)):
        for j in range(i + 1, len(parts)):
            d, _ = cKDTree(parts[i]).query(parts[j])
            assert d.min() >= 2 * a.radius                                       # bodies do not overlap


def test_default_scene_size():
    from tpgan_amd import simulate as S
    n = [len(S.random_scene(s).particles()[0]) for s in (1, 2, 3)]
    assert all(S.COUNT_RANGE[0] <= k <= S.COUNT_RANGE[1] for k in n), n


# ---- the C entries' argument checks: no device is touched ---------------------------------------------------------------
def test_pbf_entries_reject_bad_arguments_before_any_launch(hip_lib):
    buf = (C.c_float * 256)()
    p = C.cast(buf, C.c_void_p)
    aligned = C.c_void_p((p.value + 255) & ~255)
    odd = C.c_void_p(aligned.value + 4)
    box = np.array([[0, 0, 0, 1, 1, 1]], F32)
    flat = np.array([[0, 0, 0, 1, 0, 1]], F32)
    nan_box = np.array([[0, 0, 0, 1, np.nan, 1]], F32)
    g = np.array([0, -9.81, 0], F32)
    nan = float("nan")
    assert hip_lib.tpg_pbf_workspace_bytes(0, 8) == 0 and hip_lib.tpg_pbf_workspace_bytes(2, 700) > 2 * 700 * 20

    def predict(x=p, v=p, box=box, B=1, N=4, dt=0.01, a=0.0125, gravity=g, p_out=p, v_out=p):
        return hip_lib.tpg_pbf_predict_f32(x, v, None, None if box is None else box.ctypes.data, B, N, dt, a,
                                           None if gravity is None else gravity.ctypes.data, p_out, v_out, None)
    assert predict(dt=0.0) == -1 and predict(dt=-1.0) == -1 and predict(dt=nan) == -1 and predict(a=0.0) == -1
    assert predict(p_out=None) == -1 and predict(v_out=None) == -1 and predict(B=-1) == -1 and predict(N=-1) == -1
    assert predict(B=0) == 0 and predict(N=0) == 0 and predict(B=0, x=None, v=None, box=None) == 0
    assert predict(x=None) == -1 and predict(v=None) == -1 and predict(box=None) == -1 and predict(gravity=None) == -1
    assert predict(box=flat) == -1 and predict(box=nan_box) == -1
    assert predict(B=65536) == -3 and predict(N=(1 << 22) + 1) == -3

    def grid(p_=p, B=1, N=4, h=0.05, ws=aligned):
        return hip_lib.tpg_pbf_grid_f32(p_, None, B, N, h, ws, None)
    assert grid(h=0.0) == -1 and grid(h=nan) == -1 and grid(ws=None) == -1 and grid(ws=odd) == -1 and grid(p_=None) == -1
    assert grid(B=0) == 0 and grid(N=0, ws=None) == 0 and grid(B=65536) == -3

    def lam(p_=p, B=1, N=4, h=0.05, S0=5.0, eps=0.1, ws=aligned, out=p):
        return hip_lib.tpg_pbf_lambda_f32(p_, None, B, N, h, S0, eps, ws, out, None, None)
    assert lam(h=-1.0) == -1 and lam(S0=0.0) == -1 and lam(S0=nan) == -1 and lam(eps=-0.1) == -1 and lam(out=None) == -1
    assert lam(ws=None) == -1 and lam(ws=odd) == -1 and lam(p_=None) == -1 and lam(B=0) == 0 and lam(N=0) == 0
    assert lam(B=65536) == -3

    def dp(p_=p, lam_=p, box=box, B=1, N=4, h=0.05, a=0.0125, wq=0.88, k=0.1, scale=-0.03, ws=aligned, out=p):
        return hip_lib.tpg_pbf_dp_f32(p_, lam_, None, None if box is None else box.ctypes.data, B, N, h, a, wq, k, scale,
                                      ws, out, None, None)
    assert dp(h=0.0) == -1 and dp(a=0.0) == -1 and dp(wq=0.0) == -1 and dp(k=-1.0) == -1 and dp(scale=nan) == -1
    assert dp(out=None) == -1 and dp(ws=None) == -1 and dp(ws=odd) == -1 and dp(p_=None) == -1 and dp(lam_=None) == -1
    assert dp(box=None) == -1 and dp(box=flat) == -1 and dp(B=0) == 0 and dp(N=0) == 0 and dp(B=65536) == -3

    q = C.c_void_p(p.value + 512)

    def finish(p_=p, x=p, B=1, N=4, h=0.05, dt=0.01, cs=0.01, ws=aligned, x_out=q, v_out=q):
        return hip_lib.tpg_pbf_finish_f32(p_, x, None, B, N, h, dt, cs, ws, x_out, v_out, None)
    assert finish(h=0.0) == -1 and finish(dt=0.0) == -1 and finish(cs=-1.0) == -1 and finish(x_out=None) == -1
    assert finish(v_out=None) == -1 and finish(x_out=p) == -1 and finish(ws=None) == -1 and finish(ws=odd) == -1
    assert finish(p_=None) == -1 and finish(B=0) == 0 and finish(N=0) == 0 and finish(B=65536) == -3


# ---- the CLI through the CPU checker --------------------------------------------------------------------------------------
def test_cli_writes_what_fluid_sequences_reads(oracle_cpu, tmp_path, capsys):
    from tpgan_amd import simulate as S
    from tpgan_amd.data import FluidSequences
    out, test_out = str(tmp_path / "train"), str(tmp_path / "test")
    argv = ["--out", out, "--cases", "2", "--frames", "3", "--seed", "4", "--test_out", test_out, "--test_cases", "1",
            "--box", "0.5", "0.5", "0.5", "--body_size", "0.11", "--substeps", "2", "--iters", "2", "--device", "cpu"]
    assert S.main(argv) == 0
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["case"] for l in lines] == [1, 2, 1] and all(l["frames"] == 3 and l["seconds"] >= 0 for l in lines)
    seeds = []
    for root, cases in ((out, 2), (test_out, 1)):
        for c in range(1, cases + 1):
            meta = json.load(open(os.path.join(root, f"case{c}", "scene.json")))
            scene = S.Scene.from_json(meta)
            pos0, vel0 = scene.particles()
            n = len(pos0)
            assert 20 <= n <= 2000 and lines[len(seeds)]["particles"] == n
            seeds.append(tuple(meta["seed"]))
            assert meta["frames"] == 3 and meta["substeps"] == 2 and meta["params"]["iters"] == 2 and meta["fps"] == 40
            assert meta["params"]["eps"] == float(F32(0.25)) and meta["box"] == [0.5, 0.5, 0.5]
            for s in range(3):
                with np.load(os.path.join(root, f"case{c}", f"data_{s}.npz")) as f:
                    assert sorted(f.files) == ["pos", "vel"]
                    pos, vel = f["pos"], f["vel"]
                assert pos.dtype == F32 and vel.dtype == F32 and pos.shape == (n, 3) and vel.shape == (n, 3)
                assert np.isfinite(pos).all() and np.isfinite(vel).all()
                if s == 0:
                    assert np.array_equal(pos, pos0) and np.array_equal(vel, vel0)   # scene.json reproduces the scene
                else:
                    assert not np.array_equal(pos, pos0)
            assert not os.path.exists(os.path.join(root, f"case{c}", "data_3.npz"))
    assert len(set(seeds)) == 3 and seeds[2][1] == 1 and seeds[0][1] == 0          # held-out seeds are their own split
    seq = FluidSequences(out, 2, 3, device="cpu")
    assert len(seq) == 2 and seq.pos.shape == seq.vel.shape and seq.pos.shape[0] == 3 * int(seq.count.sum())
    # frame 1 is the statement's: the same scene advanced by hand
    scene = S.Scene.from_json(json.load(open(os.path.join(out, "case2", "scene.json"))))
    pos, vel, lengths = S.simulate([scene], 2, substeps=2, iters=2, device="cpu")
    with np.load(os.path.join(out, "case2", "data_1.npz")) as f:
        assert np.array_equal(f["pos"], pos[0, 1].numpy()) and np.array_equal(f["vel"], vel[0, 1].numpy())


# ---- behaviour of the statement with the shipped parameters -------------------------------------------------------------
def _drop(iters):
    """One rotated box of 1331 particles dropped from rest into a box of 0.6 m for 40 frames (1 s), by the host statement
    -> (pos (40,n,3), final mean C over the particles with at least 20 neighbours, smallest pair distance of any frame / s)."""
    from scipy.spatial import cKDTree
    from tpgan_amd import ops
    from tpgan_amd import simulate as S
    rot = S._random_rotation(np.random.default_rng(5)).reshape(-1).tolist()
    body = {"shape": "box", "size": 0.29, "rotation": rot, "centre": [0.3, 0.35, 0.3], "velocity": [0.0, 0.0, 0.0]}
    scene = S.Scene([0, 0, 0], [0.6, 0.6, 0.6], [body])
    prm = ops.PbfParams(iters=iters)
    x, v, _, lo, hi = S.pack([scene], "cpu")
    box, dt = ops.pbf_box(lo, hi, 1), float(F32(1.0 / (S.FPS * S.SUBSTEPS)))
    frames, nearest = [], np.inf
    for _ in range(40):
        for _ in range(S.SUBSTEPS):
            x, v = ops._pbf_substep_torch(x, v, None, box, dt, prm)
        frames.append(x[0].numpy().copy())
        d, _ = cKDTree(frames[-1].astype(np.float64)).query(frames[-1].astype(np.float64), k=2)
        nearest = min(nearest, float(d[:, 1].min()))
    _, Cn, pr = ops._pbf_lambda_torch(x[0], prm)
    crowded = torch.bincount(pr.i, minlength=x.shape[1]) >= 21                   # 20 neighbours and itself
    return np.stack(frames), float(Cn[crowded].mean()), nearest / (2 * prm.radius), v[0].numpy()


def test_a_dropped_body_stays_a_fluid():
    pos, mean_c, nearest, vel = _drop(4)
    lo, hi = F32(0.0) + F32(0.0125), F32(0.6) - F32(0.0125)
    assert pos.shape == (40, 1331, 3)                                            # the particle count is constant
    assert np.isfinite(pos).all() and np.isfinite(vel).all()
    assert (pos >= lo).all() and (pos <= hi).all()                               # no particle leaves the box
    assert pos[-1, :, 1].mean() < 0.1 < pos[0, :, 1].mean()                      # it fell
    # the solver at work: the same run with iters = 0 piles everything on the floor.  Observed (this scene, 40 frames):
    #   mean C over particles with >= 20 neighbours     iters = 0: 5.03       shipped: 0.000003
    #   smallest pair distance of any frame, in s       iters = 0: 0.047      shipped: 0.398
    # the bounds are halfway between the two
    print("drop, shipped parameters: mean C", mean_c, "nearest pair / s", nearest)
    assert mean_c < 2.52
    assert nearest > 0.223


def test_the_bounds_of_the_drop_test_separate_the_solver_from_none():
    _, mean_c, nearest, _ = _drop(0)
    print("drop, iters = 0: mean C", mean_c, "nearest pair / s", nearest)
    assert mean_c > 2.52 and nearest < 0.223
