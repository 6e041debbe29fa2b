"""Vorticity confinement and per-particle viscosity without a GPU: the torch statement against the numpy rule
(tests/pbf_vort_rule.py) bit for bit on the cases of tests/pbf_vort_cases.py, the curl's normalisation, momentum under a
table, planted defects, "no options, no change", the scene generator's viscosities, the C entries' argument checks, the CLI
through the CPU checker, and the behaviour of the statement at the shipped strength."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pbf_cases  # noqa: E402
import pbf_obstacle_cases  # noqa: E402
import pbf_obstacle_rule as O  # noqa: E402
import pbf_rule as P  # noqa: E402
import pbf_vort_cases as K  # noqa: E402
import pbf_vort_rule as V  # noqa: E402

F32 = np.float32
NAMES = tuple(K.CASES)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _prm(name, **over):
    from tpgan_amd import ops
    return ops.PbfParams(**dict(K.case(name)["kw"], **over))


def _rule(c, prm, tab, lengths=None):
    """The rule's substep per scene -> [(x, v)]; an empty scene gives empty arrays."""
    lengths = c["lengths"] if lengths is None else lengths
    out = []
    for b, n in enumerate(lengths):
        n = int(n)
        if n == 0:
            out.append((np.zeros((0, 3), F32), np.zeros((0, 3), F32)))
            continue
        out.append(V.substep_ex_rule(c["x"][b, :n], c["v"][b, :n], c["lo"][b], c["hi"][b], c["dt"], prm,
                                     None if tab is None else tab[b, :n]))
    return out


def _statement(c, prm, tab, lengths="own"):
    from tpgan_amd import ops
    L = _t(c["lengths"]) if isinstance(lengths, str) else (None if lengths is None else torch.tensor(lengths))
    return ops._pbf_substep_torch(_t(c["x"]), _t(c["v"]), L, ops.pbf_box(c["lo"], c["hi"], c["x"].shape[0]), c["dt"], prm,
                                  xsph=None if tab is None else _t(tab))


def _equal(got, want, c):
    for b, (xr, vr) in enumerate(want):
        n = len(xr)
        assert np.array_equal(got[0][b, :n].numpy(), xr) and np.array_equal(got[1][b, :n].numpy(), vr), b
        assert np.array_equal(got[0][b, n:].numpy(), c["x"][b, n:], equal_nan=True)       # rows beyond: as given
        assert np.array_equal(got[1][b, n:].numpy(), c["v"][b, n:], equal_nan=True)
        assert np.isfinite(vr).all()


# ---- 1. the torch statement equals the numpy rule -----------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("options", ["table", "curl", "both"])
def test_torch_statement_equals_the_rule_bit_for_bit(name, options):
    c = K.case(name)
    prm = _prm(name) if options != "table" else _prm(name, vorticity=0.0)
    tab = None if options == "curl" else c["tab"]
    _equal(_statement(c, prm, tab), _rule(c, prm, tab), c)


@pytest.mark.parametrize("name", NAMES)
def test_the_pieces_equal_the_rule_bit_for_bit(name):
    from tpgan_amd import ops
    c, prm = K.case(name), _prm(name)
    for b, n in enumerate(c["lengths"].tolist()):
        if n == 0:
            continue
        p, x, tab = K.final_p(c, b, prm), c["x"][b, :n], c["tab"][b, :n]
        vr, wr = V.finish_ex_rule(p, x, c["dt"], prm, tab, True)
        vt, wt = ops._pbf_finish_torch(_t(p), _t(x), c["dt"], prm, cs_tab=_t(tab), curl=True)
        assert np.array_equal(vt.numpy(), vr) and np.array_equal(wt.numpy(), wr), (name, b)
        assert np.array_equal(ops._pbf_vorticity_torch(_t(p), wt, vt, c["dt"], prm).numpy(),
                              V.vorticity_rule(p, wr, vr, c["dt"], prm)), (name, b)
        plain = ops._pbf_finish_torch(_t(p), _t(x), c["dt"], prm)
        assert np.array_equal(plain.numpy(), P.finish_rule(p, x, c["dt"], prm))
        assert np.array_equal(V.finish_ex_rule(p, x, c["dt"], prm), plain.numpy())


def test_torch_statement_without_lengths_and_with_lengths_outside_0_N():
    c, prm = K.case("ragged"), _prm("ragged")
    for given, means in K.ragged_lengths():
        _equal(_statement(c, prm, c["tab"], given), _rule(c, prm, c["tab"], means), dict(c, x=c["x"], v=c["v"]))


def test_whole_substeps_with_obstacles_present():
    from tpgan_amd import ops
    case, v = pbf_obstacle_cases.drop_case()
    prm = ops.PbfParams(vorticity=K.EPS)
    lengths, x = case["lengths"], case["p"]
    tab = np.random.default_rng(5).uniform(0, 2 * prm.cs, x.shape[:2]).astype(F32)
    got = ops._pbf_substep_torch(_t(x), _t(v), _t(lengths), ops.pbf_box(case["lo"], case["hi"], 2), K.DT, prm,
                                 obstacles=_t(case["table"]), xsph=_t(tab))
    for b, n in enumerate(lengths.tolist()):
        solids = lambda p, b=b: O.collide_rule(p, case["lo"][b], case["hi"][b], case["table"][b], prm)   # noqa: E731
        xr, vr = V.substep_ex_rule(x[b, :n], v[b, :n], case["lo"][b], case["hi"][b], K.DT, prm, tab[b, :n], solids)
        free, _ = V.substep_ex_rule(x[b, :n], v[b, :n], case["lo"][b], case["hi"][b], K.DT, prm, tab[b, :n])
        assert np.array_equal(got[0][b, :n].numpy(), xr) and np.array_equal(got[1][b, :n].numpy(), vr), b
        assert not np.array_equal(free, xr)                                       # the obstacles reach the result


def test_fix30_of_this_rule_is_the_simulators():
    rng = np.random.default_rng(0)
    term = (rng.normal(0, 400, (40, 40)) * rng.choice([1, 1, 10], (40, 40))).astype(F32)
    mask = rng.random((40, 40)) < 0.7
    assert (np.abs(term[mask]) > 1024).any()
    assert np.array_equal(V.fix30(term, mask)[0], P._fix30(term, mask))


# ---- 2. the normalisation ---------------------------------------------------------------------------------------------------
def test_lattice_curl_constant_and_a_rotating_lattice():
    from tpgan_amd import ops
    R0 = ops.pbf_lattice_curl()
    assert abs(R0 - 1.06818514) < 1e-8 and abs(R0 - V.lattice_curl()) <= 1e-12
    exact = (6 * 0.25 + 12 * ((2 - 2 ** 0.5) / 2) ** 2 * 2 ** 0.5 + 8 * ((2 - 3 ** 0.5) / 2) ** 2 * 3 ** 0.5) / 3
    assert abs(R0 - exact) <= 1e-12
    prm = ops.PbfParams(vorticity=K.EPS)
    assert prm.vs == float(F32(K.EPS / (0.025 * R0))) and prm.delta == ops.PBF_VORT_DELTA and prm.vorticity == K.EPS
    for rate in (K.OMEGA, -1.0):
        p, x, dt = K.rotation_state(rate)
        _, omega = V.finish_ex_rule(p, x, dt, prm, None, True)
        got = omega[len(p) // 2, :3].astype(np.float64) / (2.0 * prm.radius * R0)
        print("rotation", rate, "centre curl / (s R0)", got)
        assert np.abs(got - [0.0, 2.0 * rate, 0.0]).max() <= 1e-4 * 2.0 * abs(rate)
        wt = ops._pbf_finish_torch(_t(p), _t(x), dt, prm, curl=True)[1]
        assert np.array_equal(wt.numpy(), omega)


def test_delta_is_the_smallest_power_of_two_that_silences_the_interior():
    from tpgan_amd import ops
    p, x, dt = K.rotation_state()
    inside = K.interior()

    def worst(delta):
        prm = ops.PbfParams(vorticity=K.EPS)
        prm.delta = float(F32(delta))
        _, omega = V.finish_ex_rule(p, x, dt, prm, None, True)
        out = {}
        V.vorticity_rule(p, omega, np.zeros_like(p), dt, prm, out)
        return float(np.abs(out["N"][inside]).max()), float(np.abs(out["eta_f"][inside]).max())
    at, noise = worst(ops.PBF_VORT_DELTA)
    half, _ = worst(ops.PBF_VORT_DELTA / 2)
    print("interior |eta| <=", noise, "|N| at delta:", at, "at delta / 2:", half)
    assert at < 2.0 ** -10 <= half and np.log2(ops.PBF_VORT_DELTA) == round(np.log2(ops.PBF_VORT_DELTA))


# ---- 3. a table moves momentum, it makes none ---------------------------------------------------------------------------
def test_table_pairs_cancel_exactly():
    c, prm = K.case("tables"), _prm("tables")
    for b in range(3):
        out = {}
        p = K.final_p(c, b, prm)
        V.finish_ex_rule(p, c["x"][b], c["dt"], prm, c["tab"][b], False, out)
        assert out["xsph"].dtype == np.int64 and (out["xsph"] != 0).any()
        assert (out["xsph"].sum(0) == 0).all(), b


# ---- 4. planted defects -------------------------------------------------------------------------------------------------------
def _late_clamp(term, mask):
    bound = np.int64(1024) << 30
    with np.errstate(all="ignore"):
        return np.clip((np.where(mask, term, F32(0)) * P.U30).astype(np.int64), -bound, bound)


def _negated(u, G):
    with np.errstate(all="ignore"):
        return [u[2] * G[1] - u[1] * G[2], u[0] * G[2] - u[2] * G[0], u[1] * G[0] - u[0] * G[1]]


DEFECTS = {
    "the curl's sign": ("lattice_rotation", "curl_terms", _negated),
    "d2 == 0 not skipped": ("pair", "gradient_pairs", lambda pr: pr.near),
    "eta without the m_i term": ("lattice_rotation", "eta_coefficient", lambda m: np.broadcast_to(-m[None, :], (len(m),) * 2)),
    "cs_i instead of the pair mean": ("tables", "pair_cs", lambda tab: np.broadcast_to(tab[:, None], (len(tab),) * 2)),
    "curl taken after XSPH": ("tables", "curl_velocity", lambda before, after: after),
    "the clamp applied after conversion": ("clamp", "terms30", _late_clamp),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_a_planted_defect_changes_the_bits_of_its_case(monkeypatch, defect):
    name, attr, wrong = DEFECTS[defect]
    c, prm = K.case(name), _prm(name)
    seen = ("vb", "omega", "vo", "force")

    def tails():
        with np.errstate(all="ignore"):
            return [K.pieces(c, b, prm) for b in range(len(c["lengths"]))]
    want = tails()
    monkeypatch.setattr(V, attr, wrong)
    got = tails()
    differs = [any(not np.array_equal(g[k], w[k], equal_nan=True) for k in seen) for g, w in zip(got, want)]
    assert all(np.array_equal(g["p"], w["p"]) for g, w in zip(got, want))        # positions are not the tail's business
    if defect == "the clamp applied after conversion":
        assert differs[1]                                                         # scene 1 has the terms beyond 2^33
    elif defect == "cs_i instead of the pair mean":
        assert differs[:2] == [True, True] and not differs[2]                     # a uniform table cannot see it
    else:
        assert all(differs), differs


# ---- 5. no options, no change ----------------------------------------------------------------------------------------------
def test_default_parameters_and_no_table_are_the_substep_of_before():
    from tpgan_amd import ops
    x, v, lengths, lo, hi = pbf_cases.small_case()
    prm = ops.PbfParams()
    assert prm.vorticity == 0.0 and prm.vs == 0.0 and "vorticity" not in prm.as_dict()
    assert ops.PbfParams(vorticity=0.25).as_dict()["vorticity"] == 0.25
    got = ops._pbf_substep_torch(_t(x), _t(v), _t(lengths), ops.pbf_box(lo, hi, 2), pbf_cases.DT, prm, xsph=None)
    for b, n in enumerate(lengths.tolist()):
        xr, vr = P.substep_rule(x[b, :n], v[b, :n], lo[b], hi[b], pbf_cases.DT, prm)
        assert np.array_equal(got[0][b, :n].numpy(), xr) and np.array_equal(got[1][b, :n].numpy(), vr)
        xe, ve = V.substep_ex_rule(x[b, :n], v[b, :n], lo[b], hi[b], pbf_cases.DT, prm)
        assert np.array_equal(xe, xr) and np.array_equal(ve, vr)
    with pytest.raises(RuntimeError):
        ops.PbfParams(vorticity=-0.1)
    with pytest.raises(RuntimeError):
        ops.PbfParams(vorticity=float("nan"))


def test_xsph_table_from_viscosities():
    from tpgan_amd import ops
    prm = ops.PbfParams()
    nu = np.array([[0.0, 0.01, 0.05, 0.1, 0.3, 1e6]])
    tab = ops.pbf_xsph(nu, prm, "cpu")
    assert tab.dtype == torch.float32 and tab.shape == (1, 6)
    want = np.minimum(ops.PBF_XSPH * nu / 0.01, ops.PBF_XSPH_MAX) / 5.15625
    assert np.array_equal(tab.numpy(), want.astype(F32)) and ops.PBF_XSPH_MAX == 0.5
    assert tab[0, 1].item() == prm.cs and tab[0, 3].item() == tab[0, 4].item() == float(F32(0.5 / 5.15625))     # the cap
    assert torch.equal(ops.pbf_xsph(torch.from_numpy(nu), prm), tab)
    for bad in ([[-0.01]], [[float("nan")]], [[float("inf")]], [0.01]):
        with pytest.raises(RuntimeError):
            ops.pbf_xsph(np.array(bad), prm, "cpu")


LAWS = {"exponential": (0.01, np.inf), "uniform": (0.01, 0.3), "log10_uniform": (0.01, 0.01 * 10 ** 1.5)}


@pytest.mark.parametrize("seed", [1, 2, (7, 1, 3)])
def test_viscosity_draws_leave_every_other_draw_of_a_seed_alone(seed):
    from tpgan_amd import simulate as S
    kw = dict(box=(1.2, 1.0, 1.2), body_size=0.2)
    plain = S.random_scene(seed, **kw)
    assert plain.viscosity() is None and all("viscosity" not in b for b in plain.bodies)
    seen = []
    for law, (lo, hi) in LAWS.items():
        scene = S.random_scene(seed, viscosity=law, **kw)
        nus = [b["viscosity"] for b in scene.bodies]
        assert all(lo <= nu <= hi for nu in nus), (law, nus)
        stripped = json.loads(json.dumps(scene.to_json()))
        for b in stripped["bodies"]:
            del b["viscosity"]
        assert stripped == plain.to_json()
        assert np.array_equal(scene.particles()[0], plain.particles()[0])
        again = S.Scene.from_json(json.loads(json.dumps(scene.to_json())))
        assert [b["viscosity"] for b in again.bodies] == nus
        per = scene.viscosity()
        counts = [len(S.body_points(b, 2 * scene.radius)) for b in scene.bodies]
        assert per.shape == (len(scene.particles()[0]),) and np.array_equal(per, np.repeat(nus, counts))
        assert np.array_equal(again.viscosity(), per)
        assert S.random_scene(seed, viscosity=law, **kw).to_json() == scene.to_json()
        seen.append(tuple(nus))
    assert len(set(seen)) == 3
    with pytest.raises(ValueError):
        S.random_scene(seed, viscosity="thick", **kw)


def test_a_batch_with_one_viscous_scene_gets_a_table_for_all():
    from tpgan_amd import ops
    from tpgan_amd import simulate as S
    kw = dict(box=(0.5, 0.5, 0.5), body_size=0.11)
    plain, thick = S.random_scene(3, **kw), S.random_scene(4, viscosity="uniform", **kw)
    prm = ops.PbfParams()
    assert S.xsph_table([plain, plain], prm, "cpu") is None
    tab = S.xsph_table([plain, thick], prm, "cpu")
    n0, n1 = len(plain.particles()[0]), len(thick.particles()[0])
    assert tab.shape == (2, max(n0, n1)) and (tab[0, :n0] == prm.cs).all() and (tab[0, n0:] == 0).all()
    assert torch.equal(tab[1, :n1], ops.pbf_xsph(thick.viscosity()[None], prm, "cpu")[0])


# ---- 6. behaviour of the statement ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spin():
    """The spinning block (tests/pbf_vort_cases.py), by the host statement, run once per setting."""
    from tpgan_amd import ops
    return {"none": K.spin_history(ops.PbfParams()), "shipped": K.spin_history(ops.PbfParams(vorticity=ops.PBF_VORTICITY)),
            "thin": K.spin_history(ops.PbfParams(), 6, xsph=0.01), "thick": K.spin_history(ops.PbfParams(), 6, xsph=0.1)}


# Observed (729 particles, 12 frames, angular momentum about the axis at the end, unit masses; it starts at 48.6):
#   no confinement 24.78      shipped strength 35.76      the bound is halfway
SPIN_BOUND = 30.27
# Observed (kinetic energy at frame 6; 194.4 at the start, the block collapses under gravity meanwhile):
#   viscosity 0.01: 426.7     viscosity 0.1 (c = 0.5): 306.2     the bound is halfway
VISCOUS_BOUND = 366.4


def test_confinement_keeps_a_spinning_block_spinning(spin):
    L = spin["shipped"][:, 0]
    print("angular momentum, shipped strength:", L.tolist(), "total energy:", spin["shipped"][:, 2].tolist())
    assert abs(L[0] - 48.6) < 1e-3 and L[-1] > SPIN_BOUND and np.isfinite(spin["shipped"]).all()


def test_the_spin_bound_separates_confinement_from_none(spin):
    L = spin["none"][:, 0]
    print("angular momentum, no confinement:", L.tolist())
    assert L[-1] < SPIN_BOUND


def test_a_viscous_block_loses_its_kinetic_energy_sooner(spin):
    print("kinetic energy, viscosity 0.1:", spin["thick"][:, 1].tolist())
    assert spin["thick"][6, 1] < VISCOUS_BOUND and np.isfinite(spin["thick"]).all()


def test_the_viscosity_bound_separates_thick_from_thin(spin):
    print("kinetic energy, viscosity 0.01:", spin["thin"][:, 1].tolist())
    assert spin["thin"][6, 1] > VISCOUS_BOUND
    # the table of viscosity 0.01 holds params.cs: the same liquid as without a table, up to where the factor is applied
    assert abs(spin["thin"][6, 1] - spin["none"][6, 1]) < 0.01 * spin["none"][6, 1]


def _drop80(vorticity):
    """The drop scene of tests/test_simulate_cpu.py continued to 80 frames -> (mean C, nearest pair / s, final rms speed)."""
    from scipy.spatial import cKDTree
    from tpgan_amd import ops
    from tpgan_amd import simulate as S
    rot = S._random_rotation(np.random.default_rng(5)).reshape(-1).tolist()
    body = {"shape": "box", "size": 0.29, "rotation": rot, "centre": [0.3, 0.35, 0.3], "velocity": [0.0, 0.0, 0.0]}
    prm = ops.PbfParams(iters=4, vorticity=vorticity)
    x, v, _, lo, hi = S.pack([S.Scene([0, 0, 0], [0.6, 0.6, 0.6], [body])], "cpu")
    box, dt = ops.pbf_box(lo, hi, 1), float(F32(1.0 / (S.FPS * S.SUBSTEPS)))
    nearest = np.inf
    for _ in range(80):
        for _ in range(S.SUBSTEPS):
            x, v = ops._pbf_substep_torch(x, v, None, box, dt, prm)
        q = x[0].numpy().astype(np.float64)
        nearest = min(nearest, float(cKDTree(q).query(q, k=2)[0][:, 1].min()))
    _, Cn, pr = ops._pbf_lambda_torch(x[0], prm)
    crowded = torch.bincount(pr.i, minlength=x.shape[1]) >= 21
    return float(Cn[crowded].mean()), nearest / (2 * prm.radius), float(np.sqrt((v[0].double().numpy() ** 2).sum(1).mean()))


def test_a_dropped_body_comes_to_rest_at_the_shipped_strength():
    """The two conditions the shipped strength was chosen by: the bounds of
    tests/test_simulate_cpu.py hold, and after 2 s the pool's rms speed is at most 1.5 times that without confinement
    (observed: 0.0238 against 0.0235 m/s; the same run with one start coordinate moved by an ulp: 0.0244)."""
    from tpgan_amd import ops
    mean_c, nearest, rms = _drop80(ops.PBF_VORTICITY)
    _, _, rms0 = _drop80(0.0)
    print("drop, 80 frames, shipped strength: mean C", mean_c, "nearest pair / s", nearest, "rms", rms, "without:", rms0)
    assert mean_c < 2.52 and nearest > 0.223
    assert rms <= 1.5 * rms0


# ---- 7. the C entries' argument checks: no device is touched -------------------------------------------------------------
def test_new_pbf_entries_reject_bad_arguments_before_any_launch(hip_lib):
    buf = (C.c_float * 512)()
    p = C.cast(buf, C.c_void_p)
    aligned = C.c_void_p((p.value + 255) & ~255)
    odd = C.c_void_p(aligned.value + 4)
    q = C.c_void_p(p.value + 1024)
    nan = float("nan")

    def finish(p_=p, x=p, B=1, N=4, h=0.05, dt=0.01, cs=0.01, tab=p, ws=aligned, x_out=q, v_out=q, om=q):
        return hip_lib.tpg_pbf_finish_ex_f32(p_, x, None, B, N, h, dt, cs, tab, ws, x_out, v_out, om, None)
    assert finish(h=0.0) == -1 and finish(h=nan) == -1 and finish(dt=0.0) == -1 and finish(dt=nan) == -1
    assert finish(cs=-1.0) == -1 and finish(cs=nan) == -1 and finish(x_out=None) == -1 and finish(v_out=None) == -1
    assert finish(x_out=p) == -1 and finish(ws=None) == -1 and finish(ws=odd) == -1
    assert finish(B=-1) == -1 and finish(N=-1) == -1
    assert finish(B=0) == 0 and finish(N=0) == 0 and finish(B=0, p_=None, x=None, tab=None, om=None, ws=None) == 0
    assert finish(B=65536) == -3 and finish(N=(1 << 22) + 1) == -3
    assert finish(p_=None) == -1 and finish(x=None) == -1
    assert finish(p_=None, tab=None, om=None) == -1

    def vort(p_=p, om=p, v=p, B=1, N=4, h=0.05, dt=0.01, vs=10.0, delta=2.0 ** -13, ws=aligned, v_out=q):
        return hip_lib.tpg_pbf_vorticity_f32(p_, om, v, None, B, N, h, dt, vs, delta, ws, v_out, None)
    assert vort(h=0.0) == -1 and vort(dt=0.0) == -1 and vort(dt=nan) == -1 and vort(vs=-1.0) == -1 and vort(vs=nan) == -1
    assert vort(delta=0.0) == -1 and vort(delta=nan) == -1 and vort(v_out=None) == -1
    assert vort(ws=None) == -1 and vort(ws=odd) == -1 and vort(B=-1) == -1 and vort(N=-1) == -1
    assert vort(B=0) == 0 and vort(N=0) == 0 and vort(N=0, p_=None, om=None, v=None, ws=None) == 0
    assert vort(B=65536) == -3 and vort(N=(1 << 22) + 1) == -3
    assert vort(p_=None) == -1 and vort(om=None) == -1 and vort(v=None) == -1


# ---- 8. the CLI through the CPU checker --------------------------------------------------------------------------------------
def test_cli_records_viscosities_and_strength(oracle_cpu, tmp_path, capsys):
    from tpgan_amd import ops
    from tpgan_amd import simulate as S
    from tpgan_amd.data import FluidSequences
    base = ["--cases", "2", "--frames", "3", "--seed", "4", "--box", "0.5", "0.5", "0.5", "--body_size", "0.11",
            "--substeps", "2", "--iters", "2", "--device", "cpu"]
    with_out, without = str(tmp_path / "with"), str(tmp_path / "without")
    assert S.main(["--out", with_out, "--viscosity", "uniform", "--vorticity"] + base) == 0
    assert S.main(["--out", without] + base) == 0
    capsys.readouterr()
    moved = False
    for c in (1, 2):
        meta = json.load(open(os.path.join(with_out, f"case{c}", "scene.json")))
        old = json.load(open(os.path.join(without, f"case{c}", "scene.json")))
        assert meta["params"]["vorticity"] == ops.PBF_VORTICITY and "vorticity" not in old["params"]
        assert all(0.01 <= b["viscosity"] <= 0.3 for b in meta["bodies"]) and all("viscosity" not in b for b in old["bodies"])
        assert "viscosity" not in json.dumps(old) and "vorticity" not in json.dumps(old)
        for s in range(3):
            with np.load(os.path.join(with_out, f"case{c}", f"data_{s}.npz")) as f, \
                    np.load(os.path.join(without, f"case{c}", f"data_{s}.npz")) as g:
                assert sorted(f.files) == ["pos", "vel"] and f["pos"].dtype == F32 and np.isfinite(f["vel"]).all()
                if s == 0:
                    assert np.array_equal(f["pos"], g["pos"]) and np.array_equal(f["vel"], g["vel"])   # the same scene
                else:
                    moved = moved or not np.array_equal(f["vel"], g["vel"])
    assert moved                                                                 # the options reach the frames
    seq = FluidSequences(with_out, 2, 3, device="cpu")
    assert len(seq) == 2 and seq.pos.shape[0] == 3 * int(seq.count.sum())
    # frame 1 is the statement's: the scene of scene.json advanced by hand with its table and its strength
    meta = json.load(open(os.path.join(with_out, "case2", "scene.json")))
    scene = S.Scene.from_json(meta)
    prm = ops.PbfParams(iters=2, vorticity=meta["params"]["vorticity"])
    x, v, lengths, lo, hi = S.pack([scene], "cpu")
    tab = ops.pbf_xsph(scene.viscosity()[None], prm, "cpu")
    for _ in range(2):
        x, v = ops._pbf_substep_torch(x, v, lengths, ops.pbf_box(lo, hi, 1), float(F32(1.0 / 80.0)), prm, xsph=tab)
    with np.load(os.path.join(with_out, "case2", "data_1.npz")) as f:
        assert np.array_equal(f["pos"], x[0].numpy()) and np.array_equal(f["vel"], v[0].numpy())
    # one value given: that strength
    assert S.main(["--out", str(tmp_path / "eps"), "--vorticity", "0.05"] + base[:1] + ["1"] + base[2:]) == 0
    assert json.load(open(os.path.join(str(tmp_path / "eps"), "case1", "scene.json")))["params"]["vorticity"] == 0.05
