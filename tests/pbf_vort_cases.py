"""The small batches the tests of vorticity confinement and per-particle viscosity share (tests/test_vorticity_cpu.py,
tests/test_vorticity_gpu.py): shapes at which finish_ex and vorticity of csrc/pbf.hip can still go wrong, small enough for
the O(N^2) numpy rule (tests/pbf_vort_rule.py).  Every case is the input of one substep,
    dict(x, v (B,N,3), lengths (B,), lo, hi (B,3), tab (B,N) fp32 XSPH table, kw (PbfParams arguments), dt)
and asserts through the rule, at the positions the tail of that substep sees, that it reaches the edge it is for."""
import numpy as np

import pbf_cases
import pbf_rule as P
import pbf_vort_rule as V

F32 = np.float32
A = pbf_cases.A
EPS = 0.4                               # confinement strength of the cases: large, so that the force is far above rounding
OMEGA = 3.0                             # rad/s of the rotating lattice
DT = pbf_cases.DT
_CACHE = {}


def params(name):
    from tpgan_amd import ops
    return ops.PbfParams(**case(name)["kw"])


def case(name):
    """Built once per process, never modified."""
    if name not in _CACHE:
        _CACHE[name] = CASES[name]()
    return _CACHE[name]


def _prm(**kw):
    from tpgan_amd import ops
    return ops.PbfParams(**kw)


def _table(rng, shape, prm):
    """A per-particle table of cs values in [0, 2 cs]: every pair has cs_i != cs_j."""
    return (rng.uniform(0.0, 2.0 * prm.cs, shape)).astype(F32)


def final_p(c, b, prm=None):
    """The positions the tail of the substep of scene b walks: predict and the iterations, by the rule."""
    prm = prm or _prm(**c["kw"])
    n = int(min(max(int(c["lengths"][b]), 0), c["x"].shape[1]))
    p, _ = P.predict_rule(c["x"][b, :n], c["v"][b, :n], c["lo"][b], c["hi"][b], c["dt"], prm)
    for _ in range(prm.iters):
        lam, _ = P.lambda_rule(p, prm)
        p, _ = P.dp_rule(p, lam, c["lo"][b], c["hi"][b], prm)
    return p


def _tail(c, b, prm):
    """finish_ex with table and curl, then vorticity, on scene b -> (p, v after finish, omega, v, what the rule met)."""
    n = int(c["lengths"][b])
    p, out = final_p(c, b, prm), {}
    vf, omega = V.finish_ex_rule(p, c["x"][b, :n], c["dt"], prm, c["tab"][b, :n], True, out)
    return p, vf, omega, V.vorticity_rule(p, omega, vf, c["dt"], prm, out), out


def pieces(c, b, prm, lengths=None):
    """What every launch kind of the tail must give for scene b, by the rule: the final positions p, finish_ex's v in
    its three flag combinations (vt: table, vc: curl, vb: both), omega, vorticity's output on (omega, vb), and `force`:
    its output on zero velocities, where a force far below an ulp of v still shows."""
    n = int(c["lengths"][b] if lengths is None else lengths[b])
    if n == 0:
        return dict(n=0)
    cc = c if lengths is None else dict(c, lengths=np.asarray(lengths, np.int64))
    p, x, tab, dt = final_p(cc, b, prm), c["x"][b, :n], c["tab"][b, :n], c["dt"]
    vt = V.finish_ex_rule(p, x, dt, prm, tab, False)
    vc, omega_c = V.finish_ex_rule(p, x, dt, prm, None, True)
    vb, omega = V.finish_ex_rule(p, x, dt, prm, tab, True)
    assert np.array_equal(vb, vt)                                                # the curl does not reach the velocities
    return dict(n=n, p=p, vt=vt, vc=vc, vb=vb, omega=omega, omega_c=omega_c, vo=V.vorticity_rule(p, omega, vb, dt, prm),
                force=V.vorticity_rule(p, omega, np.zeros_like(p), dt, prm), v0=P.finish_rule(p, x, dt, prm))


def rotation_state(omega=OMEGA, n=7, dt=2.0 ** -7):
    """A lattice of n^3 particles at spacing 0.025 centred on the origin, rotating rigidly about +y: the final positions p
    and the previous ones x = p - dt (Omega x r), so that finish sees v = Omega x r -> p, x (n^3,3) fp32, dt."""
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)
    p = ((g - (n - 1) / 2) * 0.025).astype(F32)
    v = np.stack([F32(omega) * p[:, 2], np.zeros(len(p), F32), -(F32(omega) * p[:, 0])], 1)
    return p, (p - F32(dt) * v).astype(F32), float(dt)


def interior(n=7):
    """The particles of the n^3 lattice all of whose neighbours (|z| < 2: one layer) have all of theirs: in exact
    arithmetic every m their eta reads is the same, so eta is 0 there."""
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return ((g >= 2) & (g <= n - 3)).all(1)


def lattice_rotation_case():
    """7^3 particles at spacing 0.025 with v = Omega x r about +y, no gravity, no iterations: the tail of the substep sees
    the lattice turned by dt Omega.  Asserted on the exact state (`rotation_state`): the centre particle's curl over s R0
    is (0, 2 Omega, 0) within 1e-4, and the eta of the 27 interior particles is rounding noise: |N| < 2^-10."""
    kw = dict(iters=0, gravity=(0.0, 0.0, 0.0), vorticity=EPS)
    prm = _prm(**kw)
    p, x, dt = rotation_state()
    _, omega = V.finish_ex_rule(p, x, dt, prm, None, True)
    centre = len(p) // 2
    assert (p[centre] == 0).all()
    got = omega[centre, :3].astype(np.float64) / (2.0 * prm.radius * V.lattice_curl())
    assert np.abs(got - [0.0, 2.0 * OMEGA, 0.0]).max() <= 1e-4 * 2.0 * OMEGA, got
    out = {}
    V.vorticity_rule(p, omega, np.zeros_like(p), dt, prm, out)
    inside = interior()
    assert inside.sum() == 27 and np.abs(out["N"][inside]).max() < 2.0 ** -10, np.abs(out["N"][inside]).max()
    v = np.stack([F32(OMEGA) * p[:, 2], np.zeros(len(p), F32), -(F32(OMEGA) * p[:, 0])], 1)
    rng = np.random.default_rng(7)
    return dict(x=p[None].copy(), v=v[None].copy(), lengths=np.array([len(p)], np.int64), lo=np.full((1, 3), -0.3, F32),
                hi=np.full((1, 3), 0.3, F32), tab=_table(rng, (1, len(p)), prm), kw=kw, dt=DT)


def pair_case():
    """Five particles, no gravity, no iterations: a pair 0.03 apart whose velocities differ (omega_0 == omega_1 != 0, so
    m_0 - m_1 == 0, eta == 0 and the force is EXACTLY 0), a coincident pair (d2 == 0: a pair of the XSPH sum that has no
    gradient, so its omega is 0) and an isolated particle.  Asserted: all of that, and that vorticity returns its input."""
    kw = dict(iters=0, gravity=(0.0, 0.0, 0.0), vorticity=EPS)
    prm = _prm(**kw)
    x = np.array([[[0.1, 0.1, 0.1], [0.13, 0.1, 0.1], [0.3, 0.3, 0.3], [0.3, 0.3, 0.3], [0.5, 0.1, 0.4]]], F32)
    v = np.array([[[0.0, 0.0, 0.0], [0.0, 1.0, 0.5], [0.4, 0.0, 0.1], [0.4, 0.0, 0.1], [0.2, 0.0, 0.0]]], F32)
    c = dict(x=x, v=v, lengths=np.array([5], np.int64), lo=np.zeros((1, 3), F32), hi=np.full((1, 3), 0.6, F32),
             tab=np.array([[0.0, 0.02, 0.01, 0.03, 0.01]], F32), kw=kw, dt=DT)
    p, vf, omega, vout, out = _tail(c, 0, prm)
    assert np.array_equal(p[2], p[3]) and not np.array_equal(p[0], p[1])
    assert np.array_equal(omega[0], omega[1]) and omega[0, 3] > 0 and (omega[2:] == 0).all()
    assert (out["eta"] == 0).all() and np.array_equal(vout, vf)
    return c


def wide_case():
    """pbf_cases.wide_case (a 4 m scene: coarse cells) without iterations: the first dp pass already spreads the cluster
    below 128 candidates per walk.  Asserted on the final positions: some walk has more than 128 candidates (three trips),
    the cells are coarse, and the force is not zero."""
    x, v, lengths, lo, hi = pbf_cases.wide_case()
    kw = dict(iters=0, vorticity=EPS)
    prm = _prm(**kw)
    c = dict(x=x, v=v, lengths=lengths, lo=lo, hi=hi, tab=_table(np.random.default_rng(3), x.shape[:2], prm), kw=kw, dt=DT)
    for b in range(2):
        p, vf, omega, vout, _ = _tail(c, b, prm)
        g = pbf_cases.Grid(p, prm.h)
        assert max(len(w) for w in g.walks()) > 128 and g.edge > F32(prm.h) * F32(1.2), b
        assert (vout != vf).any()
    return c


def flat_case():
    """pbf_cases.flat_case: a sheet (dim == 1 along y) and a row (dim == 1 along y and z).  Asserted on the final
    positions: the grids are flat; the sheet's curl is along y alone and its force in the plane; the row's curl is 0."""
    x, v, lengths, lo, hi = pbf_cases.flat_case()
    kw = dict(vorticity=EPS)
    prm = _prm(**kw)
    c = dict(x=x, v=v, lengths=lengths, lo=lo, hi=hi, tab=_table(np.random.default_rng(4), x.shape[:2], prm), kw=kw, dt=DT)
    for b, flat in ((0, [1]), (1, [1, 2])):
        p, vf, omega, vout, _ = _tail(c, b, prm)
        assert (pbf_cases.Grid(p, prm.h).dim[flat] == 1).all(), b
        if b == 0:
            assert (omega[:, [0, 2]] == 0).all() and (omega[:, 1] != 0).any()
            assert np.array_equal(vout[:, 1], vf[:, 1]) and (vout != vf).any()
        else:
            assert (omega == 0).all() and np.array_equal(vout, vf)
    return c


def ragged_case():
    """B = 3, N = 150: an empty scene, a full one and one of 77 particles (not a multiple of the 4 waves of a workgroup).
    Every row holds a particle, so that the same arrays serve lengths = None and lengths beyond N; `ragged_lengths`
    lists the lengths to run with and what they stand for."""
    rng = np.random.default_rng(21)
    kw = dict(vorticity=EPS)
    prm = _prm(**kw)
    B, N = 3, 150
    x = np.stack([pbf_cases._lattice([0.05, 0.05, 0.05], (6, 5, 5)) + rng.uniform(0, 0.004, (N, 3)).astype(F32)
                  for _ in range(B)])
    v = rng.normal(0, 0.8, (B, N, 3)).astype(F32)
    lo, hi = np.zeros((B, 3), F32), np.full((B, 3), 0.4, F32)
    return dict(x=x, v=v, lengths=np.array([0, N, 77], np.int64), lo=lo, hi=hi, tab=_table(rng, (B, N), prm), kw=kw, dt=DT)


def ragged_lengths(N=150):
    """(lengths or None, what they stand for) for the three scenes of ragged_case."""
    return [([0, N, 77], [0, N, 77]), (None, [N, N, N]), ([2 ** 32 + 5, -3, 77], [N, 0, 77])]


def clamp_case():
    """The term clamp, with dt = 2^-37, no gravity, no iterations: 14 particles within 0.02 m of a point.  Scene 0: speeds
    of 1e5 m/s.  Scene 1: speeds of 2e10 m/s, whose curl terms lie beyond 2^33, where a clamp applied after the conversion
    to integer has already overflowed.  Asserted on the final positions of both: terms of the table's XSPH sum, of the
    curl and of eta lie beyond the term clamp, none is NaN, and the results are finite."""
    rng = np.random.default_rng(8)
    kw = dict(iters=0, gravity=(0.0, 0.0, 0.0), vorticity=EPS)
    prm = _prm(**kw)
    dt = float(2.0 ** -37)
    xs, vs = [], []
    for speed in (1e5, 2e10):
        p = (np.array([0.3, 0.3, 0.3]) + rng.uniform(-0.012, 0.012, (14, 3))).astype(F32)
        v = (rng.choice([-1.0, 1.0], (14, 3)) * rng.uniform(0.5 * speed, speed, (14, 3))).astype(F32)
        xs.append((p - F32(dt) * v).astype(F32))
        vs.append(v)
    c = dict(x=np.stack(xs), v=np.stack(vs), lengths=np.array([14, 14], np.int64), lo=np.zeros((2, 3), F32),
             hi=np.full((2, 3), 0.6, F32), tab=np.full((2, 14), prm.cs, F32) * rng.uniform(0.5, 2.0, (2, 14)).astype(F32),
             kw=kw, dt=dt)
    for b in range(2):
        pf, vf, omega, vout, out = _tail(c, b, prm)
        assert out["xsph_over"] > 20 and out["curl_over"] > 20 and out["eta_over"] > 20, (b, out)
        assert out["xsph_nan"] == 0 and out["curl_nan"] == 0 and out["eta_nan"] == 0
        assert b == 0 or out["curl_max"] > 2.0 ** 33
        assert np.isfinite(vf).all() and np.isfinite(omega).all() and np.isfinite(vout).all()
    return c


def tables_case():
    """One geometry three times (two lattice bodies of 5^3 thrown at each other) with three tables: zeros for body 0 and a
    value for body 1; the values of viscosity 0.01 and 0.1 per body (pairs with cs_i != cs_j where the bodies meet); one
    value everywhere.  Asserted: bodies touch at the final positions, and the three tables give three results."""
    from tpgan_amd import ops
    kw = dict(vorticity=EPS)
    prm = _prm(**kw)
    a = pbf_cases._lattice([0.05, 0.05, 0.05], (5, 5, 5))
    b = pbf_cases._lattice([0.18, 0.055, 0.06], (5, 5, 5))
    x0 = np.concatenate([a, b])
    v0 = np.concatenate([np.tile(np.array([[3.0, 0.0, 0.2]], F32), (125, 1)), np.tile(np.array([[-3.0, 0.5, 0.0]], F32), (125, 1))])
    v0 = v0 + np.random.default_rng(2).normal(0, 0.2, v0.shape).astype(F32)
    cs = (ops.pbf_xsph_coefficient([0.01, 0.1]) / prm.S0).astype(F32)
    tab = np.zeros((3, 250), F32)
    tab[0, 125:] = cs[0]
    tab[1, :125], tab[1, 125:] = cs[0], cs[1]
    tab[2] = cs[1]
    c = dict(x=np.stack([x0] * 3), v=np.stack([v0] * 3), lengths=np.array([250] * 3, np.int64), lo=np.zeros((3, 3), F32),
             hi=np.full((3, 3), 0.4, F32), tab=tab, kw=kw, dt=DT)
    res = [_tail(c, s, prm) for s in range(3)]
    near = P.Pairs(res[0][0], prm).near
    assert near[:125, 125:].sum() > 50                                           # pairs across the two bodies
    assert not np.array_equal(res[0][1], res[1][1]) and not np.array_equal(res[1][1], res[2][1])
    return c


# ---- behaviour: a spinning block, run by the host statement -------------------------------------------------------------
SPIN_BOX, SPIN_RATE = 0.45, 8.0


def spinning_block():
    """9^3 particles at spacing 0.025 standing on the floor in the middle of a box of 0.45 m, spinning at 8 rad/s about
    the vertical through the box's centre -> x, v (1,729,3) fp32, lo, hi (1,3)."""
    g = np.stack(np.meshgrid(*[np.arange(9)] * 3, indexing="ij"), -1).reshape(-1, 3)
    r = (g - 4) * 0.025
    x = r + [SPIN_BOX / 2, 4 * 0.025 + float(A), SPIN_BOX / 2]
    v = np.stack([SPIN_RATE * r[:, 2], np.zeros(len(r)), -SPIN_RATE * r[:, 0]], 1)
    return x[None].astype(F32), v[None].astype(F32), np.zeros((1, 3), F32), np.full((1, 3), SPIN_BOX, F32)


def spin_history(prm, frames=12, xsph=None, substeps=4):
    """The block advanced by `ops._pbf_substep_torch` -> per frame (frame 0: the start state), in float64 and for unit
    masses: angular momentum about the axis, kinetic energy, total energy (kinetic + g y)."""
    import torch
    from tpgan_amd import ops
    x, v, lo, hi = spinning_block()
    x, v = torch.from_numpy(x), torch.from_numpy(v)
    box, dt = ops.pbf_box(lo, hi, 1), float(F32(1.0 / (40 * substeps)))
    tab = None if xsph is None else ops.pbf_xsph(np.full((1, 729), xsph), prm, "cpu")
    rows = []
    for f in range(frames + 1):
        if f:
            for _ in range(substeps):
                x, v = ops._pbf_substep_torch(x, v, None, box, dt, prm, xsph=tab)
        X, U = x[0].double().numpy(), v[0].double().numpy()
        rx, rz = X[:, 0] - SPIN_BOX / 2, X[:, 2] - SPIN_BOX / 2
        ke = 0.5 * (U ** 2).sum()
        rows.append((float((rz * U[:, 0] - rx * U[:, 2]).sum()), float(ke), float(ke + 9.81 * X[:, 1].sum())))
    return np.array(rows)


CASES = {"lattice_rotation": lattice_rotation_case, "pair": pair_case, "wide": wide_case, "flat": flat_case,
         "ragged": ragged_case, "clamp": clamp_case, "tables": tables_case}
