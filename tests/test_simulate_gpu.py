"""The fluid simulator's kernels (csrc/pbf.hip) against the numpy statement of the rule (tests/pbf_rule.py), bit for bit
and launch kind by launch kind, on the batches of tests/pbf_cases.py (two everyday ones; 130 scenes in three launches of
the kernels that carry boxes; a coarse grid; flat grids; the term clamp); then batch positions across those launches,
other parameters, lengths None and outside [0, N], the workspace across batch shapes, whole frames, repeatability, and
the data it writes through the loader, the sampler, the analysis and one training step."""
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pbf_cases  # noqa: E402
import pbf_rule as P  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
DT = float(F32(1.0 / 160.0))
SENTINEL = 7.0
FRAMES, SUBSTEPS, ITERS = 6, 2, 2          # frame 0 and five simulated ones, for the whole-frame checks


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


NAMES = ("small", "tiny", "chunk", "wide", "flat", "clamp")


def _pieces(x, v, lo, hi, dt, prm):
    """What every launch kind of the first iteration and one whole substep must give for one scene, by the numpy rule."""
    p, vp = P.predict_rule(x, v, lo, hi, dt, prm)
    lam, Cn = P.lambda_rule(p, prm)
    pn, dp = P.dp_rule(p, lam, lo, hi, prm)
    vf = P.finish_rule(pn, x, dt, prm)
    xs, vs = P.substep_rule(x, v, lo, hi, dt, prm)
    return dict(n=len(x), p=p, vp=vp, lam=lam, C=Cn, pn=pn, dp=dp, vf=vf, xs=xs, vs=vs)


@pytest.fixture(scope="module")
def reference():
    """Per batch of tests/pbf_cases.py and cloud: what every launch kind of the first iteration and one whole substep with
    the batch's parameters must give and, for small and tiny, FRAMES frames at SUBSTEPS / ITERS -- computed once by the
    numpy rule, never modified."""
    from tpgan_amd import ops
    few = ops.PbfParams(iters=ITERS)
    out = {}
    for name in NAMES:
        case, prm, dt = pbf_cases.CASES[name][0](), pbf_cases.params(name), pbf_cases.CASES[name][2]
        x, v, lengths, lo, hi = case
        clouds = []
        for b in range(len(lengths)):
            n = int(lengths[b])
            xb, vb = x[b, :n], v[b, :n]
            c = _pieces(xb, vb, lo[b], hi[b], dt, prm)
            if name in ("small", "tiny"):
                c["pos"], c["vel"] = P.frames_rule(xb, vb, lo[b], hi[b], FRAMES - 1, SUBSTEPS, few)
            clouds.append(c)
        out[name] = (case, clouds)
    return out


@pytest.fixture(scope="module")
def full_reference():
    """small_case with every row in use (pbf_cases.full_small) and its pieces per scene."""
    from tpgan_amd import ops
    case = pbf_cases.full_small()
    x, v, _, lo, hi = case
    return case, [_pieces(x[b], v[b], lo[b], hi[b], DT, ops.PbfParams()) for b in range(2)]


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rows(t, b, n):
    return t[b, :n].cpu().numpy()


def _untouched(t, b, n):
    return bool((t[b, n:] == SENTINEL).all())


KINDS = (("p", "p", "predict p"), ("vp", "vp", "predict v"), ("lam", "lam", "lambda"), ("C", "C", "C"), ("dp", "dp", "dp"),
         ("pn", "pn", "p + dp"), ("pi", "pn", "p + dp in place"), ("vo", "vf", "finish v"), ("xo", "pn", "finish x"))


def _launch_kinds(dev, X, V, L, box, dt, prm):
    """One launch of every kind on fresh SENTINEL-filled outputs: predict | grid | lambda | dp with dp_out | dp in place
    with dp_out == NULL, the form pbf_substep uses | grid | finish -> the outputs by name."""
    from tpgan_amd import ops
    be = ops.backend_for(torch.zeros(1, device=dev))
    B, N, _ = X.shape

    def fresh(*shape):
        return torch.full(shape, SENTINEL, dtype=torch.float32, device=dev)
    ws = be.pbf_ws(X, B, N)
    o = dict(p=fresh(B, N, 3), vp=fresh(B, N, 3), lam=fresh(B, N), C=fresh(B, N), pn=fresh(B, N, 3), dp=fresh(B, N, 3),
             xo=fresh(B, N, 3), vo=fresh(B, N, 3))
    be.pbf_predict(X, V, L, box, dt, prm, o["p"], o["vp"])
    be.pbf_grid(o["p"], L, prm, ws)
    be.pbf_lambda(o["p"], L, prm, ws, o["lam"], o["C"])
    be.pbf_dp(o["p"], o["lam"], L, box, prm, ws, o["pn"], o["dp"])
    o["pi"] = o["p"].clone()
    be.pbf_dp(o["pi"], o["lam"], L, box, prm, ws, o["pi"])
    be.pbf_grid(o["pn"], L, prm, ws)
    be.pbf_finish(o["pn"], X, L, dt, prm, ws, o["xo"], o["vo"])
    return o


@pytest.mark.parametrize("name", NAMES)
def test_every_launch_kind_equals_the_rule(dev, reference, name):
    from tpgan_amd import ops
    (x, v, lengths, lo, hi), clouds = reference[name]
    prm, dt = pbf_cases.params(name), pbf_cases.CASES[name][2]
    X, V, L, box = _up(x, dev), _up(v, dev), _up(lengths, dev), ops.pbf_box(lo, hi, len(lengths))
    o = _launch_kinds(dev, X, V, L, box, dt, prm)
    xs, vs = ops.pbf_substep(X, V, L, lo, hi, dt, prm)
    torch.cuda.synchronize()
    o = {k: t.cpu() for k, t in o.items()}
    xs, vs = xs.cpu(), vs.cpu()
    for b, c in enumerate(clouds):
        n = c["n"]
        for got, want, what in [(o[g], c[w], what) for g, w, what in KINDS] + [(xs, c["xs"], "substep x"),
                                                                               (vs, c["vs"], "substep v")]:
            assert np.array_equal(got[b, :n].numpy(), want), (name, b, what)
        # lengths: rows beyond were never read (they are NaN: a read would have poisoned a sum) and never written
        assert all(_untouched(t, b, n) for t in o.values()), (name, b)
        assert torch.isnan(xs[b, n:]).all() and torch.isnan(vs[b, n:]).all()
        assert np.isfinite(c["xs"]).all() and np.isfinite(c["vs"]).all()


def test_a_scene_gives_the_same_bits_in_every_chunk_of_a_large_batch(dev, reference):
    """small_case's first scene at batch positions 0, 63, 64 and 129 of chunk_case's 130 scenes (padded to N = 700): the
    ends of the first two launches of the kernels that carry their boxes, and the last row of the third."""
    from tpgan_amd import ops
    (sx, sv, sl, slo, shi), small = reference["small"]
    (cx, cv, cl, clo, chi), chunk = reference["chunk"]
    at = (0, 63, 64, 129)
    B, N = 130, 700
    x, v = np.full((B, N, 3), np.nan, F32), np.full((B, N, 3), np.nan, F32)
    x[:, :48], v[:, :48] = cx, cv
    lengths, lo, hi = cl.copy(), clo.copy(), chi.copy()
    for b in at:
        x[b], v[b], lengths[b], lo[b], hi[b] = sx[0], sv[0], sl[0], slo[0], shi[0]
    xs, vs = ops.pbf_substep(_up(x, dev), _up(v, dev), _up(lengths, dev), lo, hi, DT)
    alone = ops.pbf_substep(_up(sx[:1], dev), _up(sv[:1], dev), _up(sl[:1], dev), slo[:1], shi[:1], DT)
    xs, vs = xs.cpu(), vs.cpu()
    for b in range(B):
        c = small[0] if b in at else chunk[b]
        n = c["n"]
        assert np.array_equal(xs[b, :n].numpy(), c["xs"]) and np.array_equal(vs[b, :n].numpy(), c["vs"]), b
        assert torch.isnan(xs[b, n:]).all() and torch.isnan(vs[b, n:]).all()
    for b in at:
        assert torch.equal(xs[b], alone[0][0].cpu()) and torch.equal(vs[b], alone[1][0].cpu())


@pytest.mark.parametrize("variant", sorted(pbf_cases.VARIANTS))
def test_substep_equals_the_rule_with_other_parameters(dev, reference, variant):
    from tpgan_amd import ops
    (x, v, lengths, lo, hi), shipped = reference["small"]
    prm = ops.PbfParams(**pbf_cases.VARIANTS[variant])
    xs, vs = ops.pbf_substep(_up(x, dev), _up(v, dev), _up(lengths, dev), lo, hi, DT, prm)
    for b, n in enumerate(lengths.tolist()):
        xr, vr = P.substep_rule(x[b, :n], v[b, :n], lo[b], hi[b], DT, prm)
        assert not np.array_equal(vr, shipped[b]["vs"])                          # the parameter reaches the result
        assert np.array_equal(_rows(xs, b, n), xr) and np.array_equal(_rows(vs, b, n), vr), (variant, b)
        assert torch.isnan(xs[b, n:]).all() and torch.isnan(vs[b, n:]).all()


def test_lengths_none_and_lengths_outside_0_N_are_clamped_as_64_bit_values(dev, full_reference):
    """include/tpgan_ops.h: lengths[b] stands for min(max(lengths[b], 0), N) taken in 64 bits, in every launch kind and in
    the grid build alike -- N + 7, 2^32 + 5 (5 after a narrowing to int) and 2^63 - 1 are N, -3 and -2^63 are 0 -- and
    NULL is N.  Through pbf_substep, through the launch kinds, and equal to the torch statement."""
    from tpgan_amd import ops
    (x, v, _, lo, hi), clouds = full_reference
    prm, box = ops.PbfParams(), ops.pbf_box(lo, hi, 2)
    X, V = _up(x, dev), _up(v, dev)
    for given, means in [(None, [700, 700])] + pbf_cases.odd_lengths(700):
        L = None if given is None else torch.tensor(given, dtype=torch.int64, device=dev)
        xs, vs = ops.pbf_substep(X, V, L, lo, hi, DT, prm)
        xt, vt = ops._pbf_substep_torch(_up(x, "cpu"), _up(v, "cpu"), None if L is None else L.cpu(), box, DT, prm)
        assert np.array_equal(xs.cpu().numpy(), xt.numpy()) and np.array_equal(vs.cpu().numpy(), vt.numpy()), given
        o = {k: t.cpu() for k, t in _launch_kinds(dev, X, V, L, box, DT, prm).items()}
        for b, (c, n) in enumerate(zip(clouds, means)):
            assert np.array_equal(xs[b].cpu().numpy(), c["xs"] if n else x[b]), (given, b)
            assert np.array_equal(vs[b].cpu().numpy(), c["vs"] if n else v[b]), (given, b)
            for g, w, what in KINDS:
                assert np.array_equal(o[g][b, :n].numpy(), c[w][:n]), (given, b, what)
                assert _untouched(o[g], b, n), (given, b, what)


def test_a_small_batch_after_a_large_one_sees_only_its_own_grid(dev, reference):
    """The workspace is one growing buffer per stream whose layout depends on (B, N): chunk (130 x 48), small (2 x 700),
    tiny (2 x 3) and small again, back to back on one stream, each equal to its reference."""
    from tpgan_amd import ops
    runs = []
    for name in ("chunk", "small", "tiny", "small"):
        (x, v, lengths, lo, hi), _ = reference[name]
        runs.append(ops.pbf_substep(_up(x, dev), _up(v, dev), _up(lengths, dev), lo, hi, DT))
    torch.cuda.synchronize()
    for name, (xs, vs) in zip(("chunk", "small", "tiny", "small"), runs):
        for b, c in enumerate(reference[name][1]):
            assert np.array_equal(_rows(xs, b, c["n"]), c["xs"]) and np.array_equal(_rows(vs, b, c["n"]), c["vs"]), (name, b)
    for k in (0, 1):                                                             # the rows beyond the lengths are NaN
        assert np.array_equal(runs[1][k].cpu().numpy(), runs[3][k].cpu().numpy(), equal_nan=True)


def _scenes(case):
    from tpgan_amd import simulate as S
    x, v, lengths, lo, hi = case
    return [S.Scene(lo[b], hi[b], pos=x[b, :int(lengths[b])], vel=v[b, :int(lengths[b])]) for b in range(2)]


def test_whole_frames_equal_the_rules_trajectory_twice(dev, reference):
    from tpgan_amd import simulate as S
    for name in ("small", "tiny"):
        case, clouds = reference[name]
        scenes = _scenes(case)
        pos, vel, lengths = S.simulate(scenes, FRAMES, SUBSTEPS, ITERS, device=dev)
        again = S.simulate(scenes, FRAMES, SUBSTEPS, ITERS, device=dev)
        assert torch.equal(pos, again[0]) and torch.equal(vel, again[1])           # the same call, the same bits
        assert lengths.tolist() == [c["n"] for c in clouds] and pos.shape[:2] == (2, FRAMES)
        for b, c in enumerate(clouds):
            n = c["n"]
            assert np.array_equal(pos[b, 0, :n].cpu().numpy(), case[0][b, :n])      # frame 0 is the start state
            assert np.array_equal(pos[b, 1:, :n].cpu().numpy(), c["pos"]), (name, b)
            assert np.array_equal(vel[b, 1:, :n].cpu().numpy(), c["vel"]), (name, b)
            assert (pos[b, :, n:] == 0).all()


def test_a_scene_gives_the_same_bits_alone_and_at_either_batch_position(dev, reference):
    from tpgan_amd import simulate as S
    case, clouds = reference["small"]
    a, b = _scenes(case)
    both, swapped = S.simulate([a, b], 3, SUBSTEPS, ITERS, device=dev), S.simulate([b, a], 3, SUBSTEPS, ITERS, device=dev)
    for scene, first, second in ((a, 0, 1), (b, 1, 0)):
        alone = S.simulate([scene], 3, SUBSTEPS, ITERS, device=dev)
        n = int(alone[2][0])
        for k in (0, 1):
            assert torch.equal(alone[k][0, :, :n], both[k][first, :, :n])
            assert torch.equal(alone[k][0, :, :n], swapped[k][second, :, :n])
        assert np.array_equal(alone[0][0, 1:, :n].cpu().numpy(), clouds[first]["pos"][:2])


def test_simulated_data_feeds_the_loader_the_sampler_the_analysis_and_a_training_step(dev, tmp_path):
    from tpgan_amd import analysis
    from tpgan_amd import simulate as S
    from tpgan_amd.data import ClipSampler, FluidSequences
    from tpgan_amd.gan_step import tempo_gan_step
    from tpgan_amd.set_abstraction import FluidSpatialDis, FluidTempoDis
    from tpgan_amd.srnet import SRNet
    from tpgan_amd.synthetic import force_all_keep
    scenes = [S.random_scene([3, 0, c], box=(0.8, 0.8, 0.8), body_size=0.27, count_range=(1200, 2000)) for c in range(2)]
    prm = S.ops.PbfParams()
    S.write_cases(str(tmp_path), scenes, 1, 6, S.SUBSTEPS, prm, dev, {})
    seq = FluidSequences(str(tmp_path), 2, 6, device=dev)
    counts = [len(s.particles()[0]) for s in scenes]
    assert seq.count.tolist() == counts and all(1200 <= n <= 2000 for n in counts)
    assert torch.isfinite(seq.pos).all() and torch.isfinite(seq.vel).all()
    first = seq.pos[:counts[0]].cpu().numpy()
    assert np.array_equal(first, scenes[0].particles()[0])
    last = seq.pos[int(seq.frame_first[0, 5]):][:counts[0]]
    assert float((last.cpu() - torch.from_numpy(first)).abs().max()) > 0.01        # it moved
    box = torch.tensor([0.0125, 0.8 - 0.0125], device=dev)
    assert (seq.pos >= box[0]).all() and (seq.pos <= box[1]).all()
    # the smallest patch the sampler accepts from scenes of this size: any sample_num below their particle count
    sampler = ClipSampler(seq, 2, 1024, generator=torch.Generator().manual_seed(5))
    batch = sampler.sample()
    assert len(batch) == 13 and batch[0].shape == (2, 1024, 3) and batch[6].shape == (2, 128, 3)
    assert all(torch.isfinite(t).all() for t in batch[:12])
    density = analysis.particle_density_batch(last.unsqueeze(0), 0.05)
    assert density.shape == (1, counts[0]) and torch.isfinite(density).all() and float(density.min()) >= 1.0
    torch.manual_seed(0)
    np.random.seed(0)
    G = force_all_keep(SRNet(3, 128)).to(dev)
    Ds, Dt = FluidSpatialDis().to(dev), FluidTempoDis(3).to(dev)
    og, ot, os_ = (torch.optim.Adam(m.parameters(), 1e-4) for m in (G, Dt, Ds))
    opt = Namespace(use_vel=False, in_node_feats=3, cutoff=0.025, R=0.10, w=0.5)
    losses = tempo_gan_step(G, Ds, Dt, list(batch[6:9]), None, list(batch[0:3]), None, 1.0, opt, 12, og, ot, os_)
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in losses.values()), losses
