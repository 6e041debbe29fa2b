"""finish_ex and vorticity of csrc/pbf.hip against the numpy statement of their rule (tests/pbf_vort_rule.py), bit for bit
and launch kind by launch kind, on the batches of tests/pbf_vort_cases.py; then whole substeps and a short trajectory,
batch positions, the workspaces across batch shapes, the launch sequence with and without the options, and `simulate`
with viscosities per body against the torch statement."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pbf_vort_cases as K  # noqa: E402
import pbf_vort_rule as V  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL = 7.0
NAMES = tuple(K.CASES)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _substeps(c, prm, tab, lengths=None):
    out = []
    for b, n in enumerate(c["lengths"] if lengths is None else lengths):
        n = int(n)
        out.append(V.substep_ex_rule(c["x"][b, :n], c["v"][b, :n], c["lo"][b], c["hi"][b], c["dt"], prm,
                                     None if tab is None else tab[b, :n]) if n else None)
    return out


@pytest.fixture(scope="module")
def reference():
    """name -> (case, params, per scene the pieces of the tail, per scene one whole substep with both options), by the
    numpy rule; computed once, never modified."""
    out = {}
    for name in NAMES:
        c, prm = K.case(name), K.params(name)
        out[name] = (c, prm, [K.pieces(c, b, prm) for b in range(len(c["lengths"]))], _substeps(c, prm, c["tab"]))
    return out


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _packed(pcs, key, N, width=3):
    """The scenes' rows of `key` as (B,N,width) with NaN beyond the lengths: a read there would poison a sum."""
    out = np.full((len(pcs), N, width), np.nan, F32)
    for b, c in enumerate(pcs):
        if c["n"]:
            out[b, :c["n"]] = c[key]
    return out


def _tail_launches(dev, c, prm, pcs, L):
    """One launch of every kind of the tail on fresh SENTINEL-filled outputs -> the outputs by name."""
    from tpgan_amd import ops
    be = ops.backend_for(torch.zeros(1, device=dev))
    B, N, _ = c["x"].shape
    P_, X, T = _up(_packed(pcs, "p", N), dev), _up(c["x"], dev), _up(c["tab"], dev)
    dt = c["dt"]

    def fresh(*shape):
        return torch.full(shape, SENTINEL, dtype=torch.float32, device=dev)
    ws = be.pbf_ws(P_, B, N)
    be.pbf_grid(P_, L, prm, ws)
    o = {k: fresh(B, N, 3) for k in ("x0", "v0", "xn", "vn", "xt", "vt", "xc", "vc", "xb", "vb", "vo", "force")}
    o["wc"], o["wb"] = fresh(B, N, 4), fresh(B, N, 4)
    be.pbf_finish(P_, X, L, dt, prm, ws, o["x0"], o["v0"])
    be.pbf_finish_ex(P_, X, L, dt, prm, ws, o["xn"], o["vn"])
    be.pbf_finish_ex(P_, X, L, dt, prm, ws, o["xt"], o["vt"], cs_tab=T)
    be.pbf_finish_ex(P_, X, L, dt, prm, ws, o["xc"], o["vc"], omega_out=o["wc"])
    be.pbf_finish_ex(P_, X, L, dt, prm, ws, o["xb"], o["vb"], cs_tab=T, omega_out=o["wb"])
    be.pbf_vorticity(P_, o["wb"], o["vb"], L, dt, prm, ws, o["vo"])
    o["vi"] = o["vb"].clone()
    be.pbf_vorticity(P_, o["wb"], o["vi"], L, dt, prm, ws, o["vi"])                 # in place
    zero = torch.zeros(B, N, 3, device=dev)
    be.pbf_vorticity(P_, o["wb"], zero, L, dt, prm, ws, o["force"])
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in o.items()}


KINDS = (("x0", "p", "finish x"), ("v0", "v0", "finish v"), ("xn", "p", "finish_ex x, no option"),
         ("vn", "v0", "finish_ex v, no option"), ("xt", "p", "table x"), ("vt", "vt", "table v"), ("xc", "p", "curl x"),
         ("vc", "vc", "curl v"), ("wc", "omega_c", "curl omega"), ("xb", "p", "both x"), ("vb", "vb", "both v"),
         ("wb", "omega", "both omega"), ("vo", "vo", "vorticity"), ("vi", "vo", "vorticity in place"),
         ("force", "force", "vorticity on zero velocities"))


def _check_launches(o, pcs, what):
    assert torch.equal(o["xn"], o["x0"]) and torch.equal(o["vn"], o["v0"]), what    # neither option: finish itself
    for b, c in enumerate(pcs):
        n = c["n"]
        for got, want, kind in KINDS:
            if n:
                assert np.array_equal(o[got][b, :n].numpy(), c[want]), (what, b, kind)
            assert bool((o[got][b, n:] == SENTINEL).all()), (what, b, kind, "rows beyond the length")


@pytest.mark.parametrize("name", NAMES)
def test_every_launch_kind_equals_the_rule(dev, reference, name):
    c, prm, pcs, _ = reference[name]
    o = _tail_launches(dev, c, prm, pcs, _up(c["lengths"], dev))
    _check_launches(o, pcs, name)
    if name == "pair":
        assert torch.equal(o["vo"], o["vb"]) and (o["force"][0, :5] == 0).all()     # eta == 0: the force is exactly 0


def test_lengths_none_and_lengths_outside_0_N(dev, reference):
    c, prm, _, _ = reference["ragged"]
    for given, means in K.ragged_lengths()[1:]:
        pcs = [K.pieces(c, b, prm, means) for b in range(3)]
        L = None if given is None else torch.tensor(given, dtype=torch.int64, device=dev)
        _check_launches(_tail_launches(dev, c, prm, pcs, L), pcs, given)


# ---- whole substeps -----------------------------------------------------------------------------------------------------------
def _substep(dev, c, prm, tab, lengths="own"):
    from tpgan_amd import ops
    L = _up(c["lengths"], dev) if isinstance(lengths, str) else lengths
    xs, vs = ops.pbf_substep(_up(c["x"], dev), _up(c["v"], dev), L, c["lo"], c["hi"], c["dt"], prm,
                             xsph=None if tab is None else _up(tab, dev))
    return xs.cpu(), vs.cpu()


def _check_substep(got, want, c, what):
    for b, w in enumerate(want):
        n = 0 if w is None else len(w[0])
        if n:
            assert np.array_equal(got[0][b, :n].numpy(), w[0]) and np.array_equal(got[1][b, :n].numpy(), w[1]), (what, b)
        assert np.array_equal(got[0][b, n:].numpy(), c["x"][b, n:], equal_nan=True), (what, b)
        assert np.array_equal(got[1][b, n:].numpy(), c["v"][b, n:], equal_nan=True), (what, b)


@pytest.mark.parametrize("name", NAMES)
def test_whole_substeps_equal_the_rule_and_repeat(dev, reference, name):
    from tpgan_amd import ops
    c, prm, _, want = reference[name]
    got = _substep(dev, c, prm, c["tab"])
    _check_substep(got, want, c, name)
    again = _substep(dev, c, prm, c["tab"])
    assert all(np.array_equal(a.numpy(), g.numpy(), equal_nan=True) for a, g in zip(again, got))
    if name in ("tables", "flat"):                                                # each option on its own
        plain = ops.PbfParams(**dict(c["kw"], vorticity=0.0))
        _check_substep(_substep(dev, c, plain, c["tab"]), _substeps(c, plain, c["tab"]), c, (name, "table"))
        _check_substep(_substep(dev, c, prm, None), _substeps(c, prm, None), c, (name, "curl"))


def test_a_two_frame_trajectory_equals_the_rules_twice(dev, reference):
    from tpgan_amd import ops
    c, prm, _, _ = reference["tables"]
    runs = []
    for _ in range(2):
        X, U, T = _up(c["x"], dev), _up(c["v"], dev), _up(c["tab"], dev)
        for _ in range(4):                                                        # two frames of two substeps
            X, U = ops.pbf_substep(X, U, None, c["lo"], c["hi"], c["dt"], prm, xsph=T)
        runs.append((X.cpu(), U.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for b in range(3):
        x, v = c["x"][b], c["v"][b]
        for _ in range(4):
            x, v = V.substep_ex_rule(x, v, c["lo"][b], c["hi"][b], c["dt"], prm, c["tab"][b])
        assert np.array_equal(runs[0][0][b].numpy(), x) and np.array_equal(runs[0][1][b].numpy(), v), b


def test_a_scene_gives_the_same_bits_alone_and_at_either_batch_position(dev, reference):
    c, prm, _, want = reference["tables"]

    def run(rows):
        sub = dict(c, x=c["x"][rows], v=c["v"][rows], lengths=c["lengths"][rows], lo=c["lo"][rows], hi=c["hi"][rows])
        return _substep(dev, sub, prm, c["tab"][rows])
    both, swapped = run([0, 1]), run([1, 0])
    for scene, first, second in ((0, 0, 1), (1, 1, 0)):
        alone = run([scene])
        for k in (0, 1):
            assert torch.equal(alone[k][0], both[k][first]) and torch.equal(alone[k][0], swapped[k][second])
            assert np.array_equal(alone[k][0].numpy(), want[scene][k])


def test_a_small_batch_after_a_large_one_sees_only_its_own_grid_and_omega(dev, reference):
    """The grid's workspace and omega are growing buffers per stream: tables (3 x 250), pair (1 x 5), ragged (3 x 150)
    and tables again, back to back on one stream, each equal to its reference."""
    order = ("tables", "pair", "ragged", "tables")
    runs = []
    for name in order:
        c, prm, _, _ = reference[name]
        runs.append(_substep(dev, c, prm, c["tab"]))
    for name, got in zip(order, runs):
        c, _, _, want = reference[name]
        _check_substep(got, want, c, name)


# ---- the launches ---------------------------------------------------------------------------------------------------------------
def test_the_launch_sequence_changes_only_in_its_tail(dev, reference, monkeypatch):
    from tpgan_amd import ops
    c, prm, _, _ = reference["tables"]
    be = ops.backend_for(torch.zeros(1, device=dev))
    seen, call = [], be._call

    def spy(symbol, *a, **kw):
        seen.append(symbol)
        return call(symbol, *a, **kw)
    monkeypatch.setattr(be, "_call", spy)
    X, U, T = _up(c["x"], dev), _up(c["v"], dev), _up(c["tab"], dev)

    def run(p, **kw):
        seen.clear()
        ops.pbf_substep(X, U, None, c["lo"], c["hi"], c["dt"], p, **kw)
        return list(seen)
    plain = ops.PbfParams()
    before = ["tpg_pbf_predict_f32"] + ["tpg_pbf_grid_f32", "tpg_pbf_lambda_f32", "tpg_pbf_dp_f32"] * plain.iters + \
             ["tpg_pbf_grid_f32", "tpg_pbf_finish_f32"]
    assert run(plain) == before and run(plain, xsph=None) == before
    assert run(plain, xsph=T) == before[:-1] + ["tpg_pbf_finish_ex_f32"]
    assert run(prm) == before[:-1] + ["tpg_pbf_finish_ex_f32", "tpg_pbf_vorticity_f32"]
    assert run(prm, xsph=T) == before[:-1] + ["tpg_pbf_finish_ex_f32", "tpg_pbf_vorticity_f32"]


# ---- simulate ---------------------------------------------------------------------------------------------------------------------
def test_simulate_with_viscosities_per_body_equals_the_torch_statement(dev):
    from tpgan_amd import ops
    from tpgan_amd import simulate as S
    eye = np.eye(3).reshape(-1).tolist()

    def body(centre, velocity, nu=None):
        b = {"shape": "box", "size": 0.1, "rotation": eye, "centre": centre, "velocity": velocity}
        return b if nu is None else dict(b, viscosity=nu)
    scenes = [S.Scene([0, 0, 0], [0.5, 0.4, 0.5], [body([0.15, 0.1, 0.2], [2.0, 0.0, 0.3], 0.02),
                                                  body([0.32, 0.11, 0.21], [-2.0, 0.2, 0.0], 0.25)]),
              S.Scene([0, 0, 0], [0.4, 0.5, 0.4], [body([0.2, 0.12, 0.2], [0.5, -1.0, 0.5], 0.08),
                                                  body([0.2, 0.27, 0.21], [0.0, -2.0, 0.0])])]
    prm = ops.PbfParams(iters=2, vorticity=ops.PBF_VORTICITY)
    pos, vel, lengths = S.simulate(scenes, 3, 2, params=prm, device=dev)
    x, v, L, lo, hi = S.pack(scenes, "cpu")
    tab = S.xsph_table(scenes, prm, "cpu")
    assert tab is not None and len(torch.unique(tab[0, :int(L[0])])) == 2 and len(torch.unique(tab[1, :int(L[1])])) == 2
    assert lengths.tolist() == L.tolist() and min(L.tolist()) > 100
    box, dt = ops.pbf_box(lo, hi, 2), float(F32(1.0 / 80.0))
    for f in range(3):
        if f:
            for _ in range(2):
                x, v = ops._pbf_substep_torch(x, v, L, box, dt, prm, xsph=tab)
        assert torch.equal(pos[:, f].cpu(), x) and torch.equal(vel[:, f].cpu(), v), f
    plain = S.simulate(scenes, 3, 2, params=ops.PbfParams(iters=2), device=dev)
    assert not torch.equal(plain[1][:, 2], vel[:, 2])
