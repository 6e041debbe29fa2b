"""The fluid simulator's kernels (csrc/pbf.hip) against the numpy statement of the rule (tests/pbf_rule.py), bit for bit
and launch kind by launch kind, on the batches of tests/pbf_cases.py; then whole frames, repeatability, batch positions,
ragged lengths, and the data it writes through the loader, the sampler, the analysis and one training step."""
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


@pytest.fixture(scope="module")
def reference():
    """Per batch (small, tiny) and cloud: what every launch kind of the first iteration, one whole substep with the shipped
    parameters and FRAMES frames at SUBSTEPS / ITERS must give -- computed once by the numpy rule, never modified."""
    from tpgan_amd import ops
    prm, few = ops.PbfParams(), ops.PbfParams(iters=ITERS)
    out = {}
    for name, case in (("small", pbf_cases.small_case()), ("tiny", pbf_cases.tiny_case())):
        x, v, lengths, lo, hi = case
        clouds = []
        for b in range(2):
            n = int(lengths[b])
            xb, vb = x[b, :n], v[b, :n]
            p, vp = P.predict_rule(xb, vb, lo[b], hi[b], DT, prm)
            lam, Cn = P.lambda_rule(p, prm)
            pn, dp = P.dp_rule(p, lam, lo[b], hi[b], prm)
            vf = P.finish_rule(pn, xb, DT, prm)
            xs, vs = P.substep_rule(xb, vb, lo[b], hi[b], DT, prm)
            pos, vel = P.frames_rule(xb, vb, lo[b], hi[b], FRAMES - 1, SUBSTEPS, few)
            clouds.append(dict(n=n, p=p, vp=vp, lam=lam, C=Cn, pn=pn, dp=dp, vf=vf, xs=xs, vs=vs, pos=pos, vel=vel))
        out[name] = (case, clouds)
    return out


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rows(t, b, n):
    return t[b, :n].cpu().numpy()


def _untouched(t, b, n):
    return bool((t[b, n:] == SENTINEL).all())


@pytest.mark.parametrize("name", ["small", "tiny"])
def test_every_launch_kind_equals_the_rule(dev, reference, name):
    from tpgan_amd import ops
    (x, v, lengths, lo, hi), clouds = reference[name]
    prm, be = ops.PbfParams(), ops.backend_for(torch.zeros(1, device=dev))
    X, V, L, box = _up(x, dev), _up(v, dev), _up(lengths, dev), ops.pbf_box(lo, hi, 2)
    B, N, _ = X.shape

    def fresh(*shape):
        return torch.full(shape, SENTINEL, dtype=torch.float32, device=dev)
    ws = be.pbf_ws(X, B, N)
    p, vp, lam, Cn, pn, dp, xo, vo = (fresh(B, N, 3), fresh(B, N, 3), fresh(B, N), fresh(B, N), fresh(B, N, 3),
                                      fresh(B, N, 3), fresh(B, N, 3), fresh(B, N, 3))
    be.pbf_predict(X, V, L, box, DT, prm, p, vp)
    be.pbf_grid(p, L, prm, ws)
    be.pbf_lambda(p, L, prm, ws, lam, Cn)
    be.pbf_dp(p, lam, L, box, prm, ws, pn, dp)
    be.pbf_grid(pn, L, prm, ws)
    be.pbf_finish(pn, X, L, DT, prm, ws, xo, vo)
    xs, vs = ops.pbf_substep(X, V, L, lo, hi, DT, prm)
    torch.cuda.synchronize()
    for b, c in enumerate(clouds):
        n = c["n"]
        for got, want, what in ((p, c["p"], "predict p"), (vp, c["vp"], "predict v"), (lam, c["lam"], "lambda"),
                                (Cn, c["C"], "C"), (dp, c["dp"], "dp"), (pn, c["pn"], "p + dp"), (vo, c["vf"], "finish v"),
                                (xo, c["pn"], "finish x"), (xs, c["xs"], "substep x"), (vs, c["vs"], "substep v")):
            assert np.array_equal(_rows(got, b, n), want), (name, b, what)
        # lengths: rows beyond were never read (they are NaN: a read would have poisoned a sum) and never written
        assert all(_untouched(t, b, n) for t in (p, vp, lam, Cn, pn, dp, xo, vo)), (name, b)
        assert torch.isnan(xs[b, n:]).all() and torch.isnan(vs[b, n:]).all()
        assert np.isfinite(c["xs"]).all() and np.isfinite(c["vs"]).all()


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
