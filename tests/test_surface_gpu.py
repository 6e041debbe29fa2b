"""The surface renderer on the GPU: tpg_render_spheres_f32, tpg_surface_smooth_f32 and tpg_surface_shade_f32 through
`ops.render_surface` against the numpy statement of their rule (tests/surface_rule.py).  Sphere fronts, winner map,
smoothed depth and picture must be EQUAL to it bit for bit, with no cap on differing pixels; then repeatability, batch
position, chunking, and the layers above."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_rule as R  # noqa: E402
import surface_rule as S  # noqa: E402
from test_render_cpu import read_png  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
MODES = {"ortho": R.ORTHO, "pinhole": R.PINHOLE}
SIZES = {"37x23": (37, 23), "70x50": (70, 50)}      # smaller than and no multiple of the 32 x 8 tile; several tiles


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def shade_table():
    from tpgan_amd import ops
    return ops.surface_shade()


@functools.lru_cache(maxsize=None)
def random_case(mode, size):
    """F = 2, 300 points, ragged, 30 exact duplicates, ten rows that must be dropped, one camera per frame; rad gives discs
    of 3-6 pixels radius.  -> (arguments, raw fronts, winner) with the statement's fronts computed once."""
    W, H = SIZES[size]
    rng = np.random.default_rng(100 * MODES[mode] + W)
    pts = R.random_cloud(rng, 2, 300, spread=0.2)
    pts[0, 7] = [0.28, -0.18, 0.73]                  # 0.8 units towards the cameras: in front of the cloud
    pts[0, 100:130] = pts[0, 7]
    pts[1, 50:60] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [999, 999, 999], [np.nan] * 3, [0, 0, np.nan],
                     [np.inf] * 3, [999, 0, 0], [0, -999, 0], [-np.inf, np.inf, 0]]
    px = 0.45 * min(W, H)                            # pixels per unit length at the cameras' target
    cams = np.stack([R.tilted_cam(W, H, MODES[mode], scale=px),
                     R.tilted_cam(W, H, MODES[mode], eye=(-2.0, 0.4, 1.5), scale=px)])
    args = dict(points=pts, cams=cams, W=W, H=H, rad=4.2 / px, lengths=[300, 211])
    for f in range(2):                               # the discs ARE of 3-6 pixels radius
        _, _, zv, t = R.project(pts[f, :args["lengths"][f]], cams[f])
        rp = S.pixel_radius(zv, cams[f], args["rad"])[np.isfinite(zv) & (np.abs(pts[f, :len(zv)]) < 900).all(-1)]
        assert rp.min() >= 3.0 and rp.max() <= 6.0, (rp.min(), rp.max())
    depth, winner = S.spheres_rule(**args)
    assert np.isfinite(depth).mean() >= 0.10, "the case is vacuous"
    depth.setflags(write=False)
    winner.setflags(write=False)
    scalar = rng.normal(size=(2, 300)).astype(F32)
    scalar[1, 3] = np.nan
    return args, depth, winner, scalar


@functools.lru_cache(maxsize=None)
def smoothed(mode, size, k, iters):
    args, depth, _, _ = random_case(mode, size)
    if iters == 0:
        return depth
    out = S.smooth_rule(smoothed(mode, size, k, iters - 1), k, F32(2.0) * F32(args["rad"]))
    out.setflags(write=False)
    return out


def run(dev, points, cams, W, H, rad, lengths=None, scalar=None, **kw):
    from tpgan_amd import ops
    image, depth, winner = ops.render_surface(
        torch.from_numpy(np.ascontiguousarray(points)).to(dev), cams, W, H, torch.from_numpy(R.code_lut()), rad,
        lengths=lengths, scalar=None if scalar is None else torch.from_numpy(scalar).to(dev), background=R.BG, **kw)
    assert image.dtype == torch.uint8 and depth.dtype == torch.float32 and winner.dtype == torch.int32
    return image.cpu().numpy(), depth.cpu().numpy(), winner.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def compare(got, want, what):
    image, depth, winner = got
    want_image, want_depth, want_winner = want
    diff = (int((winner != want_winner).sum()), int((depth.view(np.uint32) != want_depth.view(np.uint32)).sum()),
            int((image != want_image).any(-1).sum()))
    print(f"{what}: pixels whose winner / depth bits / colour differ from the rule: {diff[0]} / {diff[1]} / {diff[2]} of "
          f"{winner.size}; surface {int(np.isfinite(want_depth).sum())}")
    assert np.array_equal(winner, want_winner), what
    assert same_bits(depth, want_depth), what
    assert np.array_equal(image, want_image), what


# ---- random clouds against the rule ----------------------------------------------------------------------------------
@pytest.mark.parametrize("size", sorted(SIZES))
@pytest.mark.parametrize("mode", sorted(MODES))
def test_sphere_fronts_equal_the_rule(dev, mode, size):
    args, depth, winner, _ = random_case(mode, size)
    assert np.isfinite(depth).mean() >= 0.10 and np.isinf(depth).any()
    assert not np.isin(winner[0], np.arange(100, 130)).any() and (winner[0] == 7).any()    # duplicates: the lowest index
    assert winner[1].max() < 211 and not np.isin(winner[1], np.arange(50, 60)).any()
    want = S.shade_rule(depth, winner, args["cams"], R.code_lut(), R.BG, shade_table()), depth, winner
    compare(run(dev, **args, iters=0), want, "raw fronts")


@pytest.mark.parametrize("half_width", [1, 4])
@pytest.mark.parametrize("size", sorted(SIZES))
@pytest.mark.parametrize("mode", sorted(MODES))
def test_smoothed_and_shaded_surface_equals_the_rule(dev, mode, size, half_width):
    args, _, winner, scalar = random_case(mode, size)
    for iters in (1, 3):
        depth = smoothed(mode, size, half_width, iters)
        for colour in (dict(), dict(scalar=scalar, lo=-1.0, hi=1.5)):
            want = S.shade_rule(depth, winner, args["cams"], R.code_lut(), R.BG, shade_table(), **colour), depth, winner
            compare(run(dev, **args, half_width=half_width, iters=iters, **colour), want,
                    f"k = {half_width}, {iters} passes, {'scalar' if colour else 'depth'} colour")


def test_other_lights_and_exponents_equal_the_rule(dev):
    from tpgan_amd import ops
    args, _, winner, scalar = random_case("pinhole", "70x50")
    depth = smoothed("pinhole", "70x50", 1, 1)
    for shade in (ops.surface_shade((0.7, 0.2, -0.3), 0.1, 0.9, 0.8, 0.6, 0), ops.surface_shade((0.0, -1.0, -0.2), p=8)):
        want = S.shade_rule(depth, winner, args["cams"], R.code_lut(), R.BG, shade, scalar, -1.0, 1.5), depth, winner
        compare(run(dev, **args, half_width=1, iters=1, scalar=scalar, lo=-1.0, hi=1.5, shade=shade), want, "light")


def whole(points, cams, W, H, rad, **kw):
    image, depth, winner = S.surface_rule(points, cams, W, H, rad, R.code_lut(), R.BG, shade_table(), **kw)
    return image, depth, winner


def test_a_disc_at_the_64_pixel_cap(dev):
    """rp = 100 -> 64: the large-disc path, a 129 x 129 box that is clipped on every side of a 150 x 150 picture or not."""
    cam = R.cam_row(scale=100.0, cx=75.0, cy=75.0, far=100.0)
    for centre, pixels in (((0.0, 0.0), (12800, 12900)), ((-0.7, 0.6), (4000, 9000))):     # pi 64^2 = 12868
        args = dict(points=np.array([[[centre[0], centre[1], 5.0]]], F32), cams=cam, W=150, H=150, rad=1.0)
        want = whole(**args, iters=1, half_width=2)
        assert pixels[0] < np.isfinite(want[1]).sum() < pixels[1]
        compare(run(dev, **args, iters=1, half_width=2), want, f"cap at {centre}")


def test_discs_of_every_width_class(dev):
    """Pinhole, one radius in the world, depths 1 .. 20: discs of 2 .. 40 pixels radius in one wave, boxes of every
    power-of-two class of the kernel's lane layout, nearer ones over farther ones."""
    rng = np.random.default_rng(9)
    W, H, n = 70, 50, 40
    z = np.geomspace(1.0, 20.0, n)
    pts = np.stack([rng.uniform(-0.8, 0.8, n) * z, rng.uniform(-0.5, 0.5, n) * z, z], 1).astype(F32)[None]
    cam = R.cam_row(scale=40.0, cx=W / 2, cy=H / 2, near=0.5, far=30.0, mode=R.PINHOLE)
    rp = S.pixel_radius(pts[0, :, 2], cam, 1.0)
    assert rp.min() <= 2.0 and rp.max() >= 40.0
    args = dict(points=pts, cams=cam, W=W, H=H, rad=1.0)
    compare(run(dev, **args, iters=1, half_width=2), whole(**args, iters=1, half_width=2), "mixed radii")


def test_discs_smaller_than_a_pixel(dev):
    """Eight points with rp = 0.3: a disc covers the pixel centre it lies next to, or nothing."""
    xy = [[3.5, 3.5], [7.0, 7.0], [9.45, 2.6], [12.5, 12.29], [12.5, 8.81], [0.4, 15.6], [5.5, 9.5], [5.75, 9.5]]
    pts = np.array([[x, y, 2.0 + 0.1 * i] for i, (x, y) in enumerate(xy)], F32)[None]
    args = dict(points=pts, cams=R.cam_row(), W=16, H=16, rad=0.3)
    want = whole(**args, iters=1, half_width=1)
    assert sorted(set(want[2].ravel())) == [-1, 0, 2, 3, 5, 6]                 # 1, 4 cover no centre; 7 is behind 6
    compare(run(dev, **args, iters=1, half_width=1), want, "sub-pixel discs")


# ---- repeatability, batch position, chunking -------------------------------------------------------------------------
def test_repeatability_batch_position_and_chunking(dev):
    args, _, _, scalar = random_case("pinhole", "70x50")
    W, H = args["W"], args["H"]
    pts = np.concatenate([args["points"][1:], args["points"]])                 # frames 1, 0, 1
    cams = np.stack([args["cams"][1], args["cams"][0], args["cams"][1]])
    kw = dict(points=pts, cams=cams, W=W, H=H, rad=args["rad"], lengths=[211, 300, 211],
              scalar=np.concatenate([scalar[1:], scalar]), lo=-1.0, hi=1.5, half_width=2, iters=3)
    first, again = run(dev, **kw), run(dev, **kw)
    for a, b in zip(first, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))             # the same bits on every run
    alone = run(dev, **{**kw, "points": pts[1:2], "cams": cams[1], "lengths": [300], "scalar": kw["scalar"][1:2]})
    for a, b in zip(alone, first):
        assert np.array_equal(a[0].view(np.uint8), b[1].view(np.uint8))       # alone = at position 1 of 3
    for cap in (8 * W * H, 2 * 8 * W * H + 3):                                # 1 and 2 frames per call
        part = run(dev, **kw, max_key_bytes=cap)
        for a, b in zip(part, first):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), cap
    shared = run(dev, **{**kw, "cams": cams[1]}, max_key_bytes=8 * W * H)      # one camera for all frames
    for a, b in zip(shared, alone):
        assert np.array_equal(a[1].view(np.uint8), b[0].view(np.uint8))


# ---- the layers above ------------------------------------------------------------------------------------------------
def test_render_layer_and_sequence_renderer(dev, tmp_path):
    from tpgan_amd import ops, render
    rng = np.random.default_rng(31)
    clouds = [(rng.normal(size=(n, 3)) * 0.2).astype(F32) for n in (500, 420, 380)]
    batch, lengths = render.pad_frames(clouds, dev)
    cam = render.Camera.fit(clouds, width=72, height=56)
    image, depth, winner = ops.render_surface(batch, cam.row(), 72, 56, render.default_lut(), 0.03, lengths=lengths)
    assert 0.1 < float(torch.isfinite(depth).float().mean()) < 1.0
    got = render.render_surface(batch, cam, 0.03, lengths=lengths, return_depth=True, return_winner=True)
    assert all(torch.equal(a, b) for a, b in zip(got, (image, depth, winner)))
    one = render.render_surface(torch.from_numpy(clouds[1]).to(dev), cam, 0.03)                  # (N,3) -> (H,W,3)
    assert one.shape == (56, 72, 3) and torch.equal(one, image[1])
    raw = render.render_surface(batch, cam, 0.03, lengths=lengths, iters=0, half_width=1, light=(0.5, -0.5, -0.5))
    want = ops.render_surface(batch, cam.row(), 72, 56, render.default_lut(), 0.03, lengths=lengths, iters=0, half_width=1,
                              shade=ops.surface_shade((0.5, -0.5, -0.5)))[0]
    assert torch.equal(raw, want) and not torch.equal(raw, image)
    speed = torch.from_numpy(rng.uniform(size=(3, 500)).astype(F32)).to(dev)
    tinted = render.render_surface(batch, cam, 0.03, speed, lengths=lengths, lo=0.0, hi=1.0)
    assert torch.equal(tinted, ops.render_surface(batch, cam.row(), 72, 56, render.default_lut(), 0.03, lengths=lengths,
                                                  scalar=speed, lo=0.0, hi=1.0)[0])

    seq = render.SequenceRenderer(str(tmp_path / "surface"), width=72, height=56, camera=cam, device=dev,
                                  style="surface", particle_radius=0.03, smooth_iters=3, half_width=2)
    seq.push(clouds, 4)
    for t in range(3):
        assert np.array_equal(read_png(str(tmp_path / "surface" / f"pcd_{4 + t:04d}.png"))[0], image[t].cpu().numpy())

    # style="points" is today's object: the bytes `render.render` and `write_png` give
    render.SequenceRenderer(str(tmp_path / "points"), 2, 72, 56, camera=cam, device=dev).push(clouds, 0)
    render.SequenceRenderer(str(tmp_path / "styled"), 2, 72, 56, camera=cam, device=dev, style="points").push(clouds, 0)
    plain = render.render(batch, cam, "depth", 2, lengths).cpu().numpy()
    for t in range(3):
        render.write_png(str(tmp_path / "want.png"), plain[t])
        want_bytes = open(tmp_path / "want.png", "rb").read()
        for d in ("points", "styled"):
            assert open(tmp_path / d / f"pcd_{t:04d}.png", "rb").read() == want_bytes
