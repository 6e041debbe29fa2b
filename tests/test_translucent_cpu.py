"""The translucent fluid without a GPU: known answers of the numpy statement of its rule (tests/translucent_rule.py), the
compositions of torch ops behind `ops.render_thickness`, `ops.surface_smooth` and `ops.absorb_layers` against that
statement, `ops.absorb_table` and the default look, the two C entries' argument checks and the CLIs' new options."""
import argparse
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_rule as R  # noqa: E402
import surface_rule as S  # noqa: E402
import translucent_cases as cases  # noqa: E402
import translucent_rule as T  # noqa: E402

F32 = np.float32
W16 = H16 = 16


def units(points, rad, cams=None, W=W16, H=H16, lengths=None, limit=None):
    pts = np.asarray(points, dtype=F32)
    return T.thickness_units(pts[None] if pts.ndim == 2 else pts, R.cam_row(far=100.0) if cams is None else cams, W, H,
                             rad, lengths, limit)[0]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- (a) thickness: known answers of the rule --------------------------------------------------------------------------
def test_the_centre_pixel_of_one_sphere_holds_its_chord():
    cam = R.cam_row(scale=4.0, cx=8.0, cy=8.0, far=100.0)             # ortho: rad 1 -> rp = 4, on a pixel corner
    acc = units([[0.0, 0.0, 6.0]], 1.0, cams=cam)
    d = F32(0.5) / F32(4.0)
    h = np.sqrt(F32(1.0) - (d * d + d * d))
    half = F32(1.0) * h
    term = (F32(6.0) + half) - (F32(6.0) - half)
    assert term.dtype == F32 and abs(float(term) - 2 * math.sqrt(1 - 2 * 0.125 ** 2)) < 1e-6
    assert (acc[0, 7:9, 7:9] == int(term * F32(16777216.0))).all()
    assert same_bits(T.resolve(acc)[0, 7:9, 7:9], np.full((2, 2), F32(int(term * F32(16777216.0))) * F32(2.0 ** -24)))
    covered = acc[0] > 0
    assert covered.sum() == 52 and np.array_equal(covered, S.spheres_rule(
        np.array([[[0.0, 0.0, 6.0]]], F32), cam, W16, H16, 1.0)[1][0] == 0)      # the discs of the two passes agree
    assert np.array_equal(acc[0], acc[0][::-1]) and np.array_equal(acc[0], acc[0].T)


def test_the_thickness_image_integrates_to_the_sphere_s_volume():
    """Sum over pixels x pixel area = the midpoint rule of the chord length g over the image plane.  g falls with the
    distance from the disc's centre, so with d = p / sqrt(2), half a pixel's diagonal (p = 1 / scale, the pixel's size in
    world units), every pixel has  integral of g(|x| + d) <= p^2 g(centre) <= integral of g(max(|x| - d, 0)),  and both
    bounds have closed forms: the sum differs from the volume V by at most  pi^2 r^2 d + 2 pi r d^2.  (Truncation to
    2^-24 units and fp32 rounding add less than 1e-5 of V; 1e-3 is allowed for them.)"""
    scale, r, W = 32.0, 1.0, 80
    cam = R.cam_row(scale=scale, cx=40.3, cy=39.6, far=100.0)
    thick = T.thickness_rule(np.array([[[0.0, 0.0, 5.0]]], F32), cam, W, W, r)
    total = float(thick.astype(np.float64).sum()) / scale ** 2
    d = 1.0 / scale / math.sqrt(2.0)
    bound = math.pi ** 2 * r * r * d + 2 * math.pi * r * d * d
    volume = 4.0 / 3.0 * math.pi * r ** 3
    print(f"sum / scale^2 = {total:.5f}, volume = {volume:.5f}, bound = {bound:.5f}")
    assert abs(total - volume) <= bound + 1e-3 * volume
    assert float(thick.max()) <= 2.0 * r and float(thick.max()) > 1.99 * r


@pytest.mark.parametrize("k", [2, 7, 4096])
def test_coincident_points_add_exactly(k):
    p = [5.2, 6.1, 5.0]
    one = units([p], 2.0)
    many = units([p] * k, 2.0)
    assert (one > 0).sum() > 4 and np.array_equal(many, k * one)
    want = np.array([[F32(float(k * int(q))) * F32(2.0 ** -24) for q in row] for row in one[0]], F32)   # k q < 2^53: exact
    assert same_bits(T.resolve(many)[0], want)
    assert (k * one).max() > 2 ** 24 or k < 4096                     # 4096 terms: the sum is beyond fp32's integers


def test_a_permutation_of_the_points_gives_the_same_bits():
    args, limit, thick, _ = cases.random_case("pinhole", "37x23")
    perm = np.random.default_rng(3).permutation(211)
    pts = args["points"][1:2, :211][:, perm]
    got = T.thickness_rule(pts, args["cams"][1], args["W"], args["H"], args["rad"], limit=limit[1:2])
    assert same_bits(got[0], thick[1])


def test_limit_leaves_out_clips_or_keeps_the_chord():
    cam = R.cam_row(scale=4.0, cx=8.0, cy=8.0, far=100.0)
    p = [[0.0, 0.0, 6.0]]                                             # fronts at 5 .. 6, backs at 6 .. 7
    free = units(p, 1.0, cams=cam)
    for value, want in ((np.inf, free), (7.5, free), (4.0, 0 * free), (5.0, 0 * free), (-1.0, 0 * free), (np.nan, free),
                        (-np.inf, 0 * free)):
        assert np.array_equal(units(p, 1.0, cams=cam, limit=np.full((1, 16, 16), value, F32)), want), value
    cut = units(p, 1.0, cams=cam, limit=np.full((1, 16, 16), 6.5, F32))
    d = F32(0.5) / F32(4.0)
    half = F32(1.0) * np.sqrt(F32(1.0) - (d * d + d * d))
    assert cut[0, 8, 8] == int((F32(6.5) - (F32(6.0) - half)) * F32(16777216.0))      # the clipped chord
    assert ((cut < free) & (cut > 0)).sum() > 20 and (cut <= free).all()
    rim = (free > 0) & (cut == free)                                  # near the rim the back lies in front of the limit
    assert rim.any()


def test_a_sphere_across_the_near_plane_is_clamped():
    acc = units([[8.0, 8.0, 2.0]], 4.0)                               # identity camera: fronts at 2 - 4 h < 0 in the middle
    d = F32(0.5) / F32(4.0)
    half = F32(4.0) * np.sqrt(F32(1.0) - (d * d + d * d))
    assert acc[0, 8, 8] == int(((F32(2.0) + half) - F32(0.0)) * F32(16777216.0))
    whole = units([[8.0, 8.0, 6.0]], 4.0)
    assert (acc <= whole).all() and (acc[whole > 0] > 0).all() and (acc == whole).any() and (acc < whole).any()


def test_dropped_rows_add_nothing():
    args, _, _, free = cases.random_case("ortho", "37x23")
    keep = np.r_[0:50, 60:211]                                        # frame 1 without its ten rows of NaN / inf / 999
    got = T.thickness_rule(args["points"][1:2, keep], args["cams"][1], args["W"], args["H"], args["rad"])
    assert same_bits(got[0], free[1])


# ---- the compositions of torch ops, through the public interface ---------------------------------------------------------
@pytest.mark.parametrize("size", sorted(cases.SIZES))
@pytest.mark.parametrize("mode", sorted(cases.MODES))
def test_render_thickness_on_cpu_tensors_equals_the_rule(oracle_cpu, mode, size):
    from tpgan_amd import ops
    args, limit, thick, free = cases.random_case(mode, size)
    pts = torch.from_numpy(np.ascontiguousarray(args["points"]))
    call = lambda **kw: ops.render_thickness(pts, args["cams"], args["W"], args["H"], args["rad"],      # noqa: E731
                                             lengths=args["lengths"], **kw).numpy()
    assert same_bits(call(limit=torch.from_numpy(limit.copy())), thick)
    assert same_bits(call(), free)
    assert same_bits(call(limit=torch.full(limit.shape, float("inf"))), free)
    small = ops._render_thickness_torch(pts, None, np.asarray(args["cams"], F32), args["W"], args["H"], args["rad"], None,
                                        pairs_per_chunk=7 * args["W"] * args["H"])
    assert same_bits(small.numpy()[0], free[0])                       # the chunking of the pairs changes nothing


def test_render_thickness_validates_and_fills_empty_batches(oracle_cpu):
    from tpgan_amd import ops
    pts = torch.zeros(1, 4, 3)
    for match, kw in [("radius", dict(radius=0.0)), ("radius", dict(radius=1025.0)), ("radius", dict(radius=float("nan"))),
                      ("limit", dict(limit=torch.zeros(1, 8, 9))), ("limit", dict(limit=torch.zeros(1, 8, 8).double())),
                      ("max_key_bytes", dict(max_key_bytes=0)), ("near", dict(cams=R.cam_row(mode=R.PINHOLE, near=0.0)))]:
        with pytest.raises(RuntimeError, match=match):
            ops.render_thickness(pts, kw.pop("cams", R.cam_row()), 8, 8, kw.pop("radius", 0.1), **kw)
    for empty in (torch.zeros(0, 4, 3), torch.zeros(2, 0, 3)):
        out = ops.render_thickness(empty, R.cam_row(), 8, 6, 0.1)
        assert out.shape == (empty.shape[0], 6, 8) and out.dtype == torch.float32 and (out == 0).all()
    assert ops.render_thickness(pts, R.cam_row(), 8, 8, 1024.0).shape == (1, 8, 8)


@pytest.mark.parametrize("k", [1, 2, 4])
def test_a_blur_is_the_surface_smoothing_with_the_largest_delta(k):
    from tpgan_amd import ops
    thick = cases.random_case("pinhole", "37x23")[2]
    want = T.blur_rule(thick, k, 2)
    got = ops.surface_smooth(torch.from_numpy(thick.copy()), k, None, 2).numpy()
    assert same_bits(got, want)
    assert ((thick == 0) & (want > 0)).any()                          # zeros take part: the outline fades out
    flat = np.full((1, 9, 11), 0.375, F32)
    assert np.array_equal(T.blur_rule(flat, k), flat)                 # pixels outside the image are left out, not zeros
    depth = cases.surface_case("pinhole", "37x23")[1]                  # and with a real delta it is the surface's pass
    got = ops.surface_smooth(torch.from_numpy(depth.copy()), k, 0.05, 1).numpy()
    assert same_bits(got, S.smooth_rule(depth, k, 0.05))
    assert ops.SMOOTH_ALL == T.FLT_MAX


def test_absorb_layers_on_cpu_tensors_equals_the_rule():
    from tpgan_amd import ops
    case, branch = cases.absorb_case()
    assert np.array_equal(ops.absorb_table(cases.SIGMA, cases.TH_MAX), case["table"])
    want_image, want_depth = T.absorb_rule(**case)
    image, depth = ops.absorb_layers(*(torch.from_numpy(case[k].copy()) for k in
                                       ("fluid", "fdepth", "thickness", "behind", "bdepth")), case["table"], case["th_max"])
    assert image.dtype == torch.uint8 and depth.dtype == torch.float32
    assert np.array_equal(image.numpy(), want_image) and same_bits(depth.numpy(), want_depth)
    # what the rule says in words, branch by branch
    back = branch["fdepth +inf"] | branch["bdepth < fdepth"]
    assert np.array_equal(want_image[back], case["behind"][back]) and same_bits(want_depth[back], case["bdepth"][back])
    for name in ("bdepth == fdepth", "bdepth +inf", "thickness 0", "thickness >= th_max", "between"):
        assert same_bits(want_depth[branch[name]], case["fdepth"][branch[name]]), name
    zero = branch["thickness 0"]
    assert np.array_equal(want_image[zero], case["behind"][zero])      # level 0: T = 1 exactly
    full = branch["thickness >= th_max"]
    T255 = case["table"][255]
    mix = case["fluid"][full].astype(F32) * (F32(1) - T255) + case["behind"][full].astype(F32) * T255
    assert np.array_equal(want_image[full], np.floor(mix + F32(0.5)).astype(np.uint8))
    between = branch["between"]
    assert (want_image[between] != case["behind"][between]).any() and (want_image[between] != case["fluid"][between]).any()


def test_the_level_rule_of_the_thickness():
    th = np.array([0.0, -1.0, np.nan, 0.001, 0.25, 0.5, 0.75, np.inf, 0.5 * 0.5 / 255, 0.5 * 1.5 / 255 + 1e-6], F32)
    assert T.level_rule(th, 0.5).tolist() == [0, 0, 0, 1, 128, 255, 255, 255, 1, 2]


def test_absorb_layers_validates():
    from tpgan_amd import ops
    img, dep = torch.zeros(1, 4, 5, 3, dtype=torch.uint8), torch.zeros(1, 4, 5)
    table = ops.absorb_table((1.0, 1.0, 1.0), 1.0)

    def call(fluid=img, fdepth=dep, thickness=dep, behind=img, bdepth=dep, table=table, th_max=1.0):
        return ops.absorb_layers(fluid, fdepth, thickness, behind, bdepth, table, th_max)
    bad = table.copy()
    bad[3, 1] = 1.5
    nan = table.copy()
    nan[0, 0] = np.nan
    for match, kw in [("fluid_image", dict(fluid=img.float())), ("behind_image", dict(behind=img[:, :3])),
                      ("share", dict(thickness=torch.zeros(1, 4, 6))), ("float tensor", dict(bdepth=dep.double())),
                      ("table", dict(table=bad)), ("table", dict(table=nan)), ("table", dict(table=table[:100])),
                      ("th_max", dict(th_max=0.0)), ("th_max", dict(th_max=float("inf"))), ("th_max", dict(th_max=1e-45))]:
        with pytest.raises(RuntimeError, match=match):
            call(**kw)
    image, depth = call()
    assert image.shape == (1, 4, 5, 3) and depth.shape == (1, 4, 5)
    empty = call(fluid=img[:0], fdepth=dep[:0], thickness=dep[:0], behind=img[:0], bdepth=dep[:0])
    assert empty[0].shape == (0, 4, 5, 3) and empty[1].shape == (0, 4, 5)


# ---- the table and the default look ------------------------------------------------------------------------------------
def test_absorb_table_is_beer_lambert_in_float64_rounded_once():
    from tpgan_amd import ops
    table = ops.absorb_table((2.0, 0.5, 0.0), 0.8)
    assert table.dtype == np.float32 and table.shape == (256, 3)
    assert (table[0] == 1.0).all() and (table[:, 2] == 1.0).all()
    for level in (1, 77, 255):
        for c, sigma in enumerate((2.0, 0.5)):
            assert table[level, c] == F32(math.exp(-sigma * 0.8 * level / 255.0))
    assert (np.diff(table[:, 0]) < 0).all() and ((table >= 0) & (table <= 1)).all()
    for bad in (dict(sigma=(1.0, 1.0)), dict(sigma=(-0.1, 0, 0)), dict(sigma=(np.nan, 0, 0)), dict(sigma=(np.inf, 0, 0)),
                dict(th_max=0.0), dict(th_max=-1.0), dict(th_max=float("inf"))):
        with pytest.raises(RuntimeError):
            ops.absorb_table(**{"sigma": (1.0, 1.0, 1.0), "th_max": 1.0, **bad})


def test_the_default_absorption_keeps_a_splash_clear_and_a_pool_dark():
    """One particle diameter transmits at least 0.8 on every channel; twenty diameters at most 0.1 on red: asserted on
    the table `render.render_surface` builds, at the levels the rule looks those thicknesses up at."""
    from tpgan_amd import analysis, ops, render
    diameter = 2.0 * analysis.BASE_RADIUS
    th_max = render.THICKNESS_DIAMETERS * diameter
    assert render.THICKNESS_DIAMETERS == 40.0
    table = ops.absorb_table(np.asarray(render.ABSORPTION, np.float64) / diameter, th_max)
    one, twenty = (int(T.level_rule(np.array([n * diameter], F32), th_max)[0]) for n in (1, 20))
    assert (one, twenty) in ((6, 127), (6, 128))
    assert (table[one] >= 0.8).all() and (table[one + 1] >= 0.8).all()
    assert table[twenty, 0] <= 0.1 and table[twenty - 1, 0] <= 0.1
    assert all(math.exp(-a) >= 0.8 for a in render.ABSORPTION) and math.exp(-20.0 * render.ABSORPTION[0]) <= 0.1
    assert render.ABSORPTION[0] > render.ABSORPTION[1] > render.ABSORPTION[2] > 0      # red goes first, as in water


# ---- the C entries' argument checks: no device is touched -----------------------------------------------------------------
def test_translucent_entries_reject_bad_arguments_before_any_launch(hip_lib):
    from tpgan_amd import ops
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    cam, pin = R.cam_row(), R.cam_row(mode=R.PINHOLE, near=0.0)
    bad_cam = cam.copy()
    bad_cam[4] = np.nan
    nan, inf = float("nan"), float("inf")

    def thick_(points=p, F=1, N=4, cams=cam, ncam=1, W=8, H=8, rad=0.1, limit=None, acc=p, out=p):
        return hip_lib.tpg_render_thickness_f32(points, None, F, N, cams.ctypes.data, ncam, W, H, rad, limit, acc, out, None)
    assert thick_(out=None) == -1
    assert thick_(rad=0.0) == -1 and thick_(rad=-1.0) == -1 and thick_(rad=nan) == -1 and thick_(rad=inf) == -1
    assert thick_(rad=1024.5) == -1 and thick_(rad=1024.0, F=0) == 0
    assert thick_(W=0) == -1 and thick_(H=-3) == -1 and thick_(F=-1) == -1 and thick_(N=-1) == -1
    assert thick_(F=0) == 0 and thick_(N=0) == 0 and thick_(F=0, points=None, acc=None) == 0
    assert thick_(points=None) == -1 and thick_(acc=None) == -1
    assert thick_(acc=C.c_void_p(p.value + 4)) == -1                  # the sums are 64-bit words
    assert thick_(cams=pin) == -1 and thick_(cams=bad_cam) == -1 and thick_(ncam=2) == -1
    assert thick_(W=16385) == -3 and thick_(H=16385) == -3 and thick_(F=65536) == -3
    assert thick_(N=(1 << 27) + 1) == -3 and thick_(N=(1 << 27) + 1, rad=2000.0) == -1

    table = ops.absorb_table((1.0, 2.0, 3.0), 1.0)

    def absorb_(fluid=p, fdepth=p, thickness=p, behind=p, bdepth=p, F=1, W=4, H=4, th_max=1.0, tab=table, image=p, depth=p,
                **change):
        tab = None if tab is None else tab.copy()
        for j, value in change.items():
            tab.reshape(-1)[int(j[1:])] = value
        return hip_lib.tpg_surface_absorb_u8(fluid, fdepth, thickness, behind, bdepth, F, W, H, th_max,
                                             None if tab is None else tab.ctypes.data, image, depth, None)
    assert absorb_(image=None) == -1 and absorb_(depth=None) == -1 and absorb_(tab=None) == -1
    assert absorb_(t0=nan) == -1 and absorb_(t767=inf) == -1 and absorb_(t5=-0.001) == -1 and absorb_(t400=1.001) == -1
    assert absorb_(th_max=0.0) == -1 and absorb_(th_max=-1.0) == -1 and absorb_(th_max=nan) == -1 and absorb_(th_max=inf) == -1
    assert absorb_(th_max=1e-45) == -1                                # 255 / th_max is not finite
    assert absorb_(W=0) == -1 and absorb_(H=0) == -1 and absorb_(F=-1) == -1
    assert absorb_(F=0) == 0 and absorb_(F=0, fluid=None, fdepth=None, thickness=None, behind=None, bdepth=None) == 0
    assert absorb_(F=0, t0=nan) == -1                                 # the table is checked before the empty batch returns
    for name in ("fluid", "fdepth", "thickness", "behind", "bdepth"):
        assert absorb_(**{name: None}) == -1, name
    assert absorb_(W=16385) == -3 and absorb_(F=65536) == -3


# ---- the command lines --------------------------------------------------------------------------------------------------
def test_cli_takes_the_translucency_options(tmp_path):
    from tpgan_amd import render
    ap = argparse.ArgumentParser()
    render.add_render_options(ap)
    a = ap.parse_args([])
    assert (a.translucent, a.absorption, a.thickness_iters) == (False, None, 2)
    b = ap.parse_args(["--style", "surface", "--translucent", "--absorption", "0.3", "0.1", "0", "--thickness_iters", "0"])
    assert (b.translucent, b.absorption, b.thickness_iters) == (True, [0.3, 0.1, 0.0], 0)
    seq = render.renderer_from(b, str(tmp_path / "png"), "cpu")
    assert (seq.translucent, seq.absorption, seq.thickness_iters) == (True, (0.3, 0.1, 0.0), 0)
    assert seq._translucent() == dict(translucent=True, absorption=(0.3, 0.1, 0.0), thickness_iters=0)
    plain = render.renderer_from(a, str(tmp_path / "png"), "cpu")
    assert not plain.translucent and plain._translucent() == {}       # the route of before gets no new argument
    render.check_render_options(ap, a)
    render.check_render_options(ap, b)
    for style in ("points", "surface_mesh"):
        with pytest.raises(ValueError, match="translucent"):
            render.SequenceRenderer(str(tmp_path / "png"), device="cpu", style=style, translucent=True)
    with pytest.raises(ValueError, match="absorption"):
        render.SequenceRenderer(str(tmp_path / "png"), device="cpu", style="surface", absorption=(1.0, -1.0, 0.0))
    with pytest.raises(ValueError, match="thickness_iters"):
        render.SequenceRenderer(str(tmp_path / "png"), device="cpu", style="surface", thickness_iters=-1)


FLAGS = ["--translucent", "--absorption", "0.2", "0.1", "0.05", "--thickness_iters", "1"]


@pytest.mark.parametrize("module,argv,message", [
    ("render", ["--frames", "f_{i}.npy", "--count", "1", "--out", "o", "--style", "points"],
     "--translucent needs --style surface"),
    ("render", ["--frames", "f_{i}.npy", "--count", "1", "--out", "o", "--style", "surface_mesh"],
     "--translucent needs --style surface"),
    ("rollout", ["--checkpoint", "c.ckpt", "--frames", "f_{i}.npz", "--count", "1", "--out", "o"],
     "--translucent needs --style surface"),
    ("mesh", ["--frames", "f_{i}.npy", "--count", "1", "--out", "o", "--style", "surface"], "draws the mesh, which is opaque"),
    ("train", [], "--translucent needs --samples_style surface"),
    ("train_action", [], "--translucent needs --samples_style surface"),
])
def test_every_parser_takes_the_flags_and_refuses_them_for_other_styles(capsys, module, argv, message):
    import importlib
    mod = importlib.import_module(f"tpgan_amd.{module}")
    entry = getattr(mod, "parse_args", None) or mod.main
    with pytest.raises(SystemExit) as stop:
        entry(argv + FLAGS)
    err = capsys.readouterr().err
    assert stop.value.code == 2 and message in err and "unrecognized" not in err


def test_the_trainers_pass_the_options_on():
    from tpgan_amd import train, train_action
    opt = train.parse_args(["--samples_style", "surface", "--particle_radius", "0.05"] + FLAGS)
    assert train.sample_surface_options(opt) == dict(particle_radius=0.05, translucent=True, absorption=[0.2, 0.1, 0.05],
                                                     thickness_iters=1)
    assert train.sample_surface_options(train.parse_args(["--samples_style", "surface"])) == dict(particle_radius=0.025)
    assert train.sample_surface_options(train.parse_args([])) is None                  # splats, as before
    assert train.sample_surface_options(train_action.parse_args([])) is None
    assert train.sample_surface_options(argparse.Namespace()) is None
