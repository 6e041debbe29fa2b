"""The surface renderer without a GPU: known answers of the numpy statement of its rule (tests/surface_rule.py), the three
C entries' argument checks, `ops.render_surface`'s validation, `ops.surface_shade` and the CLI's new options."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_rule as R  # noqa: E402
import surface_rule as S  # noqa: E402

F32 = np.float32
W16 = H16 = 16


def spheres(points, rad, cams=None, W=W16, H=H16, lengths=None):
    pts = np.asarray(points, dtype=F32)
    return S.spheres_rule(pts[None] if pts.ndim == 2 else pts, R.cam_row(far=100.0) if cams is None else cams, W, H, rad,
                          lengths)


# ---- (a) sphere fronts ------------------------------------------------------------------------------------------------
def test_one_sphere_of_four_pixels_radius_on_a_pixel_corner():
    depth, winner = spheres([[8.0, 8.0, 6.0]], 4.0)                  # identity camera: rp = rad = 4, t = z
    covered = winner[0] == 0
    assert np.array_equal(covered, covered[::-1]) and np.array_equal(covered, covered[:, ::-1])
    # pixel centres sit at half-integer offsets (i + 1/2, j + 1/2) from the corner: inside iff (2i+1)^2 + (2j+1)^2 < 64
    brute = sum((2 * i + 1) ** 2 + (2 * j + 1) ** 2 < 64 for i in range(-8, 8) for j in range(-8, 8))
    assert covered.sum() == brute == 52
    assert np.isinf(depth[0][~covered]).all() and (winner[0][~covered] == -1).all()
    front = F32(6.0) - F32(4.0) * np.sqrt(F32(1.0) - F32(2 * 0.125 ** 2))
    centre = depth[0, 7:9, 7:9]
    assert (centre == front).all() and depth[0][covered].min() == front
    assert (np.sort(depth[0][covered])[4:] > front).all()             # nearest at the four centre pixels only


def test_the_nearer_front_wins_pixel_by_pixel():
    a, b = [6.0, 8.0, 6.0], [10.0, 8.0, 6.5]                          # a is the nearer SPHERE
    depth, winner = spheres([a, b], 4.0)
    da, _ = spheres([a], 4.0)
    db, _ = spheres([b], 4.0)
    assert np.array_equal(depth, np.minimum(da, db))
    both = np.isfinite(da[0]) & np.isfinite(db[0])
    assert np.array_equal(winner[0][both], np.where(db[0][both] < da[0][both], 1, 0))
    assert (winner[0][both] == 1).any() and (winner[0][both] == 0).any()
    assert winner[0, 8, 10] == 1 and db[0, 8, 10] < da[0, 8, 10]      # b's centre shows b although a's sphere is nearer


def test_exact_duplicates_show_the_lower_index():
    depth, winner = spheres([[9.0, 9.0, 7.0], [5.2, 6.1, 5.0], [5.2, 6.1, 5.0], [5.2, 6.1, 5.0]], 2.0)
    only, _ = spheres([[5.2, 6.1, 5.0]], 2.0)
    disc = np.isfinite(only[0])
    assert disc.sum() > 4 and set(winner[0][disc]) == {1}


def test_dropped_rows_draw_nothing():
    nan, inf = np.nan, np.inf
    just_below = np.nextafter(F32(0.5), F32(0))                       # t = zv - near just below 0 with near = 0.5
    just_above = np.nextafter(F32(10), F32(20))                       # zv just above far = 10
    rows = [[6.5, 6.5, just_below], [6.5, 6.5, just_above], [6.5, 6.5, nan], [6.5, 6.5, 5.0], [nan, 6.5, 1.0],
            [6.5, inf, 1.0], [-inf, 6.5, 1.0], [6.5, 6.5, inf], [6.5, 6.5, -inf], [999.0, 999.0, 999.0], [6.5, nan, 0.6],
            [6.5, 6.5, 3.0], [6.5, 6.5, 2.0]]                         # rows 11, 12 are nearer but lie beyond lengths
    depth, winner = spheres(rows, 2.0, cams=R.cam_row(near=0.5), lengths=[11])
    want_depth, want_winner = spheres([[6.5, 6.5, 5.0]], 2.0, cams=R.cam_row(near=0.5))
    assert np.array_equal(depth, want_depth) and np.array_equal(winner >= 0, want_winner >= 0)
    assert set(winner[0][winner[0] >= 0]) == {3}
    # off the picture by more than the radius; rad's sign is the caller's to get right, rp <= 0 draws nothing
    _, none = spheres([[-2.5, 8.0, 1.0], [8.0, 18.5, 1.0]], 2.0)
    assert (none == -1).all()
    _, edge = spheres([[-1.0, 8.0, 5.0]], 2.0)                       # within the radius of the edge: drawn
    assert (edge[0, :, 0] == 0).any() and (edge[0, :, 1:] == -1).all()


def test_a_sphere_across_the_near_plane_is_clamped_to_zero():
    depth, winner = spheres([[8.0, 8.0, 2.0]], 4.0)                   # the front would be at t = 2 - 4 h < 0 in the middle
    assert depth[0, 8, 8] == 0.0 and not np.signbit(depth[0, 8, 8]) and (depth[0][winner[0] == 0] >= 0).all()
    assert (depth[0][winner[0] == 0] > 0).any()                       # the rim is behind the plane's clamp


def test_pinhole_twice_the_distance_is_half_the_radius():
    cam = R.cam_row(scale=16.0, cx=16.0, cy=16.0, near=0.5, far=100.0, mode=R.PINHOLE)
    assert np.array_equal(S.pixel_radius(np.array([4.0, 8.0], F32), cam, 1.0), np.array([4.0, 2.0], F32))
    widths = []
    for z in (4.0, 8.0):
        _, winner = spheres([[0.0, 0.0, z]], 1.0, cams=cam, W=32, H=32)
        widths.append(int((winner[0, 16] == 0).sum()))
    assert widths == [8, 4]


def test_the_radius_is_capped_at_64_pixels_with_the_true_bulge():
    cam = R.cam_row(scale=100.0, cx=75.0, cy=75.0, far=100.0)         # rp = 100 -> 64
    depth, winner = spheres([[0.0, 0.0, 5.0]], 1.0, cams=cam, W=150, H=150)
    assert (winner[0, 75] == 0).sum() == 128 and (winner[0, :, 75] == 0).sum() == 128
    d = F32(0.5) / F32(64.0)
    assert depth[0, 75, 75] == F32(5.0) - F32(1.0) * np.sqrt(F32(1.0) - (d * d + d * d))
    assert abs(depth[0, 75, 75] - 4.0) < 1e-4 and winner[0, 75, 5] == -1


# ---- (b) smoothing ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_smoothing_known_answers(k):
    assert S.binomial_row(1) == [1, 2, 1] and S.binomial_row(2) == [1, 4, 6, 4, 1] and max(S.binomial_row(4)) == 70
    plane = np.full((1, 11, 13), 2.0, F32)
    assert np.array_equal(S.smooth_rule(plane, k, 0.1), plane)                          # exactly, at the edges too
    rng = np.random.default_rng(k)
    step = np.where(np.arange(13) < 6, 2.0, 3.0).astype(F32) + rng.uniform(0, 0.01, (1, 11, 13)).astype(F32)
    out = S.smooth_rule(step, k, 0.5)                                                   # the step of 1 exceeds delta
    flat = np.where(np.arange(13) < 6, 2.0, 3.0).astype(F32) * np.ones((1, 11, 13), F32)
    assert np.array_equal(S.smooth_rule(flat, k, 0.5), flat)                            # both sides bit for bit
    assert (out[..., :6] < 2.02).all() and (out[..., 6:] > 2.99).all()                  # and nothing is smeared across
    holes = step.copy()
    holes[0, 2:5, 3:9] = np.inf
    holes[0, 8, 1] = np.nan
    smoothed = S.smooth_rule(holes, k, 0.5)
    assert np.array_equal(np.isfinite(smoothed), np.isfinite(holes))                    # the background mask is invariant
    assert np.isnan(smoothed[0, 8, 1]) and np.isinf(smoothed[0, 3, 4])
    alone = np.full((1, 9, 9), np.inf, F32)
    alone[0, 4, 4] = 1.2345
    alone[0, 4, 5] = 7.0                                                                # a neighbour beyond delta
    assert np.array_equal(S.smooth_rule(alone, k, 0.5), alone)                          # an isolated pixel is unchanged


# ---- (c) shading ------------------------------------------------------------------------------------------------------
def test_a_camera_facing_plane_has_one_colour_the_closed_form():
    from tpgan_amd import ops
    shade = ops.surface_shade()
    cam = R.cam_row(scale=3.0, cx=4.0, cy=3.0, far=10.0)
    depth = np.full((1, 6, 8), 2.5, F32)
    normals = S.normals_rule(depth, cam)
    assert np.array_equal(normals, np.broadcast_to(np.array([0, 0, -1], F32), normals.shape))
    lut = R.code_lut()
    image = S.shade_rule(depth, np.zeros((1, 6, 8), np.int32), cam, lut, R.BG, shade)
    level = int(F32(2.5) * (F32(255.0) / F32(10.0)) + F32(0.5))
    sp = max(-float(shade[5]), 0.0) ** (2 ** int(shade[10]))
    want = lut[level].astype(np.float64) * (shade[6] + shade[7] * max(-float(shade[2]), 0.0)) + 255.0 * shade[8] * sp
    assert (image == image[0, 0, 0]).all()
    assert np.abs(image[0, 0, 0].astype(np.float64) - np.clip(want, 0, 255)).max() <= 0.5 + 1e-3
    bg = S.shade_rule(np.full((1, 6, 8), np.inf, F32), np.full((1, 6, 8), -1, np.int32), cam, lut, R.BG, shade)
    assert (bg == np.array(R.BG, np.uint8)).all()


@pytest.mark.parametrize("alpha,beta", [(0.5, -0.25), (0.0, 0.75), (-1.5, 0.0)])
def test_an_ortho_plane_of_known_slope_has_the_analytic_normal(alpha, beta):
    cam = R.cam_row(scale=1.0, cx=0.5, cy=0.5, far=100.0)            # a = x, b = y in world units
    ys, xs = np.meshgrid(np.arange(9), np.arange(12), indexing="ij")
    depth = (20.0 + alpha * xs + beta * ys).astype(F32)[None]        # Zv = 20 + alpha a + beta b, exact in fp32
    want = np.array([alpha, beta, -1.0]) / np.sqrt(alpha * alpha + beta * beta + 1.0)
    normals = S.normals_rule(depth, cam)
    assert np.abs(normals.astype(np.float64) - want).max() < 1e-6
    lone = np.full((1, 5, 5), np.inf, F32)
    lone[0, 2, 2] = 3.0                                              # no neighbour: faces the camera
    assert np.array_equal(S.normals_rule(lone, cam)[0, 2, 2], np.array([0, 0, -1], F32))


def test_surface_shade_table():
    from tpgan_amd import ops
    table = ops.surface_shade()
    assert table.dtype == np.float32 and table.shape == (ops.SURFACE_SHADE_FLOATS,)
    L, Hh = table[0:3].astype(np.float64), table[3:6].astype(np.float64)
    assert abs(np.linalg.norm(L) - 1) < 1e-6 and abs(np.linalg.norm(Hh) - 1) < 1e-6
    assert np.allclose(L, np.array([-0.4, -0.6, -0.7]) / np.linalg.norm([-0.4, -0.6, -0.7]), atol=1e-7)
    half = L + np.array([0, 0, -1.0])
    assert np.allclose(Hh, half / np.linalg.norm(half), atol=1e-6)
    assert np.allclose(table[6:], [0.25, 0.65, 0.35, 0.25, 5.0])
    assert ops.surface_shade((0, -1, 0), p=3)[10] == 3.0
    for bad in (dict(light=(0, 0, 0)), dict(light=(0, 0, 1)), dict(p=9), dict(p=2.5), dict(light=(np.nan, 0, 0))):
        with pytest.raises(RuntimeError):
            ops.surface_shade(**bad)


# ---- the C entries' argument checks: no device is touched -------------------------------------------------------------
def test_surface_entries_reject_bad_arguments_before_any_launch(hip_lib):
    from tpgan_amd import ops
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    q = C.c_void_p(p.value + 128)
    cam, pin = R.cam_row(), R.cam_row(mode=R.PINHOLE, near=0.0)
    bad_cam = cam.copy()
    bad_cam[4] = np.nan
    nan, inf = float("nan"), float("inf")

    def spheres_(points=p, F=1, N=4, cams=cam, ncam=1, W=8, H=8, rad=0.1, keys=p, depth=p, winner=p):
        return hip_lib.tpg_render_spheres_f32(points, None, F, N, cams.ctypes.data, ncam, W, H, rad, keys, depth, winner,
                                              None)
    assert spheres_(depth=None) == -1 and spheres_(winner=None) == -1
    assert spheres_(rad=0.0) == -1 and spheres_(rad=-1.0) == -1 and spheres_(rad=nan) == -1 and spheres_(rad=inf) == -1
    assert spheres_(W=0) == -1 and spheres_(H=-3) == -1 and spheres_(F=-1) == -1 and spheres_(N=-1) == -1
    assert spheres_(F=0) == 0 and spheres_(N=0) == 0 and spheres_(F=0, points=None, keys=None) == 0
    assert spheres_(points=None) == -1 and spheres_(keys=None) == -1
    assert spheres_(keys=C.c_void_p(p.value + 4)) == -1               # the key buffer holds 64-bit words
    assert spheres_(cams=pin) == -1 and spheres_(cams=bad_cam) == -1 and spheres_(ncam=2) == -1
    assert spheres_(W=16385) == -3 and spheres_(H=16385) == -3 and spheres_(F=65536) == -3

    def smooth_(in_=p, F=1, W=8, H=8, k=2, delta=0.1, out=q):
        return hip_lib.tpg_surface_smooth_f32(in_, F, W, H, k, delta, out, None)
    assert smooth_(out=None) == -1 and smooth_(in_=None) == -1 and smooth_(out=p) == -1
    assert smooth_(k=0) == -1 and smooth_(k=5) == -1 and smooth_(k=-1) == -1
    assert smooth_(delta=0.0) == -1 and smooth_(delta=-0.5) == -1 and smooth_(delta=nan) == -1 and smooth_(delta=inf) == -1
    assert smooth_(W=0) == -1 and smooth_(H=0) == -1 and smooth_(F=-1) == -1
    assert smooth_(F=0) == 0 and smooth_(F=0, in_=None) == 0
    assert smooth_(W=16385) == -3 and smooth_(F=65536) == -3

    table = ops.surface_shade()

    def shade_(depth=p, winner=p, F=1, N=4, cams=cam, ncam=1, W=8, H=8, lo=0.0, hi=1.0, lut=p, bg=p, shade=table, image=p,
               **change):
        shade = None if shade is None else shade.copy()
        for j, value in change.items():
            shade[int(j[1:])] = value
        return hip_lib.tpg_surface_shade_f32(depth, winner, None, F, N, cams.ctypes.data, ncam, W, H, lo, hi, lut, bg,
                                             None if shade is None else shade.ctypes.data, image, None)
    assert shade_(image=None) == -1 and shade_(shade=None) == -1
    assert shade_(s10=9.0) == -1 and shade_(s10=-1.0) == -1 and shade_(s10=2.5) == -1 and shade_(s10=nan) == -1
    assert shade_(s0=nan) == -1 and shade_(s7=inf) == -1
    assert shade_(hi=0.0) == -1 and shade_(lo=2.0, hi=1.0) == -1 and shade_(hi=nan) == -1
    assert shade_(W=0) == -1 and shade_(H=0) == -1 and shade_(F=-1) == -1 and shade_(N=-1) == -1
    assert shade_(F=0) == 0 and shade_(N=0) == 0 and shade_(F=0, depth=None, winner=None, lut=None) == 0
    assert shade_(depth=None) == -1 and shade_(winner=None) == -1 and shade_(lut=None) == -1 and shade_(bg=None) == -1
    assert shade_(cams=pin) == -1 and shade_(cams=bad_cam) == -1 and shade_(ncam=2) == -1
    assert shade_(W=16385) == -3 and shade_(F=65536) == -3


# ---- the Python layer ---------------------------------------------------------------------------------------------------
def test_render_surface_validates_and_fills_empty_batches(oracle_cpu):
    from tpgan_amd import ops
    lut, pts = torch.from_numpy(R.code_lut()), torch.zeros(1, 4, 3)

    def call(points=pts, cams=None, radius=0.1, **kw):
        return ops.render_surface(points, R.cam_row() if cams is None else cams, 8, 8, lut, radius, **kw)
    for match, kw in [("radius", dict(radius=0.0)), ("radius", dict(radius=float("nan"))),
                      ("half_width", dict(half_width=0)), ("half_width", dict(half_width=5)), ("iters", dict(iters=-1)),
                      ("delta", dict(delta=0.0)), ("shade", dict(shade=np.zeros(10, np.float32))),
                      ("shade", dict(shade=np.full(11, np.nan, np.float32))),
                      ("near", dict(cams=R.cam_row(mode=R.PINHOLE, near=0.0))),
                      ("cameras", dict(cams=np.stack([R.cam_row()] * 3))),
                      ("range", dict(scalar=torch.zeros(1, 4), lo=1.0, hi=1.0)),
                      ("lo / hi", dict(scalar=torch.zeros(1, 4))), ("float tensor", dict(points=pts.double())),
                      ("max_key_bytes", dict(max_key_bytes=0)), ("background", dict(background=(1, 2, 256)))]:
        with pytest.raises(RuntimeError, match=match):
            call(**kw)
    with pytest.raises(RuntimeError, match="no render_surface"):    # the checker backend has no statement of it
        call()
    for empty in (torch.zeros(0, 4, 3), torch.zeros(2, 0, 3)):
        image, depth, winner = ops.render_surface(empty, R.cam_row(), 8, 6, lut, 0.1, background=R.BG)
        assert image.shape == (empty.shape[0], 6, 8, 3) and (image == torch.tensor(R.BG, dtype=torch.uint8)).all()
        assert depth.shape == winner.shape == (empty.shape[0], 6, 8) and (winner == -1).all() and torch.isinf(depth).all()


def test_cpu_tensors_are_refused_without_a_checker():
    from tpgan_amd import ops
    with pytest.raises(RuntimeError):
        ops.render_surface(torch.zeros(1, 4, 3), R.cam_row(), 8, 8, torch.from_numpy(R.code_lut()), 0.1)


def test_cli_takes_the_surface_options_and_defaults_to_points(tmp_path):
    from tpgan_amd import analysis, render
    ap = argparse.ArgumentParser()
    render.add_render_options(ap)
    a = ap.parse_args([])
    assert (a.style, a.particle_radius, a.smooth_iters, a.smooth_half_width) == ("points", 0.025, 3, 2)
    assert a.particle_radius == analysis.BASE_RADIUS and a.size == 3
    b = ap.parse_args(["--style", "surface", "--particle_radius", "0.05", "--smooth_iters", "0", "--smooth_half_width", "4"])
    assert (b.style, b.particle_radius, b.smooth_iters, b.smooth_half_width) == ("surface", 0.05, 0, 4)
    with pytest.raises(SystemExit):
        ap.parse_args(["--style", "mesh"])
    seq = render.renderer_from(b, str(tmp_path / "png"), "cpu")
    assert (seq.style, seq.particle_radius, seq.smooth_iters, seq.half_width) == ("surface", 0.05, 0, 4)
    assert render.renderer_from(a, str(tmp_path / "png"), "cpu").style == "points"
    assert render.SequenceRenderer(str(tmp_path / "png"), device="cpu").style == "points"
    with pytest.raises(ValueError):
        render.SequenceRenderer(str(tmp_path / "png"), device="cpu", style="mesh")
