"""The mesh renderer on the GPU: tpg_render_mesh_f32 and tpg_mesh_shade_f32 through `ops.render_mesh` against the numpy
statement of their rule (tests/mesh_render_rule.py).  Depth bits, winner map and picture must be EQUAL to it, with no
tolerance and no cap on differing pixels; then the kernel's class edges (tests/mesh_render_cases.py), repeatability,
batch position, chunking, composition with the other picture ops, and the layers above."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_render_cases as MC  # noqa: E402
import mesh_render_rule as MR  # noqa: E402
import render_rule as R  # noqa: E402
import surface_rule as S  # noqa: E402
from test_render_cpu import read_png  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def shade_table():
    from tpgan_amd import ops
    return ops.surface_shade()


def run(dev, args, **kw):
    from tpgan_amd import ops
    a = dict(args)
    v, f = (torch.from_numpy(np.array(a.pop(k))).to(dev) for k in ("vertices", "faces"))
    cams, W, H = np.array(a.pop("cams")), a.pop("W"), a.pop("H")
    kw = {k: torch.from_numpy(np.array(x)).to(dev) if k in ("normals", "scalar") else x for k, x in kw.items()}
    image, depth, winner = ops.render_mesh(v, f, cams, W, H, torch.from_numpy(R.code_lut()), background=R.BG, **a, **kw)
    assert image.dtype == torch.uint8 and depth.dtype == torch.float32 and winner.dtype == torch.int32
    assert image.is_cuda and depth.is_cuda and winner.is_cuda
    return image.cpu().numpy(), depth.cpu().numpy(), winner.cpu().numpy()


def compare(got, want, what):
    image, depth, winner = got
    want_image, want_depth, want_winner = want
    diff = (int((winner != want_winner).sum()), int((depth.view(np.uint32) != want_depth.view(np.uint32)).sum()),
            int((image != want_image).any(-1).sum()))
    print(f"{what}: pixels whose winner / depth bits / colour differ from the rule: {diff[0]} / {diff[1]} / {diff[2]} of "
          f"{winner.size}; surface {int(np.isfinite(want_depth).sum())}")
    assert np.array_equal(winner, want_winner), what
    assert np.array_equal(depth.view(np.uint32), want_depth.view(np.uint32)), what
    assert np.array_equal(image, want_image), what


def rule_image(args, depth, winner, **kw):
    return MR.shade_rule(depth, winner, args["vertices"], args["faces"], args["cams"], R.code_lut(), R.BG, shade_table(),
                         args.get("vlengths"), args.get("flengths"), **kw)


# ---- random meshes against the rule ----------------------------------------------------------------------------------
@pytest.mark.parametrize("size", sorted(MC.SIZES))
@pytest.mark.parametrize("mode", sorted(MC.MODES))
def test_random_meshes_equal_the_rule(dev, mode, size):
    """Depth and winner, then the picture with and without normals, with a scalar, with a base colour, with neither."""
    args, depth, winner, extra = MC.random_case(mode, size)
    assert np.isfinite(depth).mean() >= 0.10 and np.isinf(depth).any()
    for kw in (dict(), dict(normals=extra["normals"]), dict(scalar=extra["scalar"], lo=-1.0, hi=1.5),
               dict(base=(200, 100, 50)), dict(normals=extra["normals"], scalar=extra["scalar"], lo=-1.0, hi=1.5),
               dict(normals=extra["normals"], base=(200, 100, 50))):
        compare(run(dev, args, **kw), (rule_image(args, depth, winner, **kw), depth, winner), f"{mode} {size} {sorted(kw)}")


def test_other_lights_equal_the_rule(dev):
    from tpgan_amd import ops
    args, depth, winner, extra = MC.random_case("pinhole", "70x50")
    for shade in (ops.surface_shade((0.7, 0.2, -0.3), 0.1, 0.9, 0.8, 0.6, 0), ops.surface_shade((0.0, -1.0, -0.2), p=8)):
        want = MR.shade_rule(depth, winner, args["vertices"], args["faces"], args["cams"], R.code_lut(), R.BG, shade,
                             args["vlengths"], args["flengths"], normals=extra["normals"])
        compare(run(dev, args, normals=extra["normals"], shade=shade), (want, depth, winner), "light")


# ---- the class edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.EDGE_NAMES)
def test_class_edges_equal_the_rule(dev, name):
    """Boxes of exactly SMALL and SMALL + 1 pixels, every lane layout of the wave's path, a box taller than wide, a quad
    clipped on all four sides, sub-pixel triangles, boxes of exactly HUGE pixels and more (the tile launch), more huge faces
    than a frame's list holds, a full ballot and one that spills (the sizes are asserted where the
    cases are built)."""
    from tpgan_amd import ops
    assert (ops.MESH_SMALL, ops.MESH_HUGE, ops.MESH_LIST) == (MC.SMALL, MC.HUGE, MC.LIST)
    args, depth, winner = MC.edge_case_answers()[name]
    compare(run(dev, args), (rule_image(args, depth, winner), depth, winner), name)


# ---- one mesh in many frames, batch position, chunking, repeatability ------------------------------------------------
@functools.lru_cache(maxsize=None)
def shared_case():
    """The torus of the random case under three cameras."""
    args, _, _, extra = MC.random_case("pinhole", "70x50")
    W, H = args["W"], args["H"]
    px = 0.42 * min(W, H)
    cams = np.stack([args["cams"][1], args["cams"][0], R.tilted_cam(W, H, R.PINHOLE, eye=(0.3, 2.5, 1.8), scale=px)])
    one = dict(vertices=args["vertices"][1:], faces=args["faces"][1:], cams=cams, W=W, H=H,
               vlengths=args["vlengths"][1:], flengths=args["flengths"][1:])
    depth, winner = MR.raster_rule(**one)
    assert depth.shape[0] == 3 and all(np.isfinite(d).mean() > 0.1 for d in depth)
    return one, depth, winner, extra["normals"][1:]


def test_one_mesh_shared_by_three_frames(dev):
    one, depth, winner, normals = shared_case()
    got = run(dev, one, normals=normals)
    compare(got, (rule_image(one, depth, winner, normals=normals), depth, winner), "M = 1, F = 3")
    three = dict(one, vertices=np.repeat(one["vertices"], 3, 0), faces=np.repeat(one["faces"], 3, 0),
                 vlengths=one["vlengths"] * 3, flengths=one["flengths"] * 3)
    for a, b in zip(run(dev, three, normals=np.repeat(normals, 3, 0)), got):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_repeatability_batch_position_and_chunking(dev):
    args, _, _, extra = MC.random_case("pinhole", "70x50")
    W, H = args["W"], args["H"]
    order = [1, 0, 1]
    kw = dict(vertices=args["vertices"][order], faces=args["faces"][order], cams=args["cams"][order], W=W, H=H,
              vlengths=[args["vlengths"][m] for m in order], flengths=[args["flengths"][m] for m in order])
    colour = dict(normals=extra["normals"][order], scalar=extra["scalar"][order], lo=-1.0, hi=1.5)
    first, again = run(dev, kw, **colour), run(dev, kw, **colour)
    for a, b in zip(first, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))             # the same bits on every run
    alone = run(dev, dict(kw, vertices=kw["vertices"][1:2], faces=kw["faces"][1:2], cams=kw["cams"][1],
                          vlengths=kw["vlengths"][1:2], flengths=kw["flengths"][1:2]),
                **dict(colour, normals=colour["normals"][1:2], scalar=colour["scalar"][1:2]))
    for a, b in zip(alone, first):
        assert np.array_equal(a[0].view(np.uint8), b[1].view(np.uint8))       # alone = at position 1 of 3
    for cap in (8 * W * H, 2 * 8 * W * H + 3):                                # 1 and 2 frames per call
        part = run(dev, kw, **colour, max_key_bytes=cap)
        for a, b in zip(part, first):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), cap
    one, depth, winner, normals = shared_case()                                # one mesh, chunked: still mesh 0 every time
    whole = run(dev, one, normals=normals)
    for a, b in zip(run(dev, one, normals=normals, max_key_bytes=8 * W * H), whole):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_a_frame_without_faces_is_background(dev):
    args, depth, winner, _ = MC.random_case("ortho", "37x23")
    image, d, w = run(dev, dict(args, flengths=[args["flengths"][0], 0]))
    assert np.array_equal(w[0], winner[0]) and np.array_equal(d[0].view(np.uint32), depth[0].view(np.uint32))
    assert (w[1] == -1).all() and np.isinf(d[1]).all() and (image[1] == R.BG).all()
    image, d, w = run(dev, dict(args, vlengths=[0, args["vlengths"][1]]))
    assert (w[0] == -1).all() and np.array_equal(w[1], winner[1])


# ---- composition -----------------------------------------------------------------------------------------------------
def test_mesh_composed_with_raw_sphere_fronts_equals_the_composed_rule(dev):
    from tpgan_amd import ops
    args, depth, winner, extra = MC.random_case("pinhole", "70x50")
    W, H, cams = args["W"], args["H"], np.array(args["cams"])
    rng = np.random.default_rng(12)
    pts = (R.random_cloud(rng, 2, 300, spread=0.6) + F32([0.05, -0.02, 0.1])).astype(F32)
    rad = 4.0 / (0.42 * min(W, H))
    lut = torch.from_numpy(R.code_lut())
    fluid = ops.render_surface(torch.from_numpy(pts).to(dev), cams, W, H, lut, rad, iters=0, background=R.BG)
    v, f = (torch.from_numpy(np.array(args[k])).to(dev) for k in ("vertices", "faces"))
    solid = ops.render_mesh(v, f, cams, W, H, lut, args["vlengths"], args["flengths"], base=(90, 90, 90), background=R.BG)
    image, d = ops.compose_layers([(fluid[0], fluid[1]), (solid[0], solid[1])])
    want_fluid = S.surface_rule(pts, cams, W, H, rad, R.code_lut(), R.BG, shade_table(), iters=0)
    want_solid = rule_image(args, depth, winner, base=(90, 90, 90))
    want_image, want_depth = MR.compose_rule([(want_fluid[0], want_fluid[1]), (want_solid, depth)])
    assert np.array_equal(image.cpu().numpy(), want_image)
    assert np.array_equal(d.cpu().numpy().view(np.uint32), want_depth.view(np.uint32))
    from_fluid = (want_fluid[1] <= depth) & np.isfinite(want_fluid[1])
    from_solid = depth < want_fluid[1]
    assert from_fluid.mean() > 0.03 and from_solid.mean() > 0.03, "both layers are seen"
    assert (np.isfinite(want_fluid[1]) & np.isfinite(depth)).mean() > 0.03, "and they overlap"


# ---- the layers above ------------------------------------------------------------------------------------------------
def _lattice_clouds():
    rng = np.random.default_rng(21)
    g = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.025
    return [(g + rng.normal(size=g.shape) * 0.001 + 0.01 * i).astype(F32) for i in range(2)]


def test_sequence_renderer_mesh_style_writes_the_rules_pictures(dev, tmp_path):
    from tpgan_amd import mesh, render
    clouds = _lattice_clouds()
    cam = render.Camera.fit(clouds, width=37, height=23)
    seq = render.SequenceRenderer(str(tmp_path / "mesh"), width=37, height=23, camera=cam, device=dev, style="surface_mesh",
                                  mesh_options=dict(iso=0.4))
    seq.push(clouds, 3)
    for t, cloud in enumerate(clouds):
        m = mesh.surface_mesh(torch.from_numpy(cloud).to(dev), iso=0.4)
        assert m.faces.shape[0] > 1000
        want = MR.mesh_rule(m.vertices.cpu().numpy()[None], m.faces.cpu().numpy()[None], cam.row(), 37, 23,
                            render.default_lut(), (255, 255, 255), shade_table(), normals=m.normals.cpu().numpy()[None])
        assert 0.1 < np.isfinite(want[1]).mean() < 1.0
        assert np.array_equal(read_png(str(tmp_path / "mesh" / f"pcd_{3 + t:04d}.png"))[0], want[0][0])


def test_solids_in_both_styles_write_the_composed_rules_pictures(dev, tmp_path):
    from tpgan_amd import mesh, render
    clouds = _lattice_clouds()
    cam = render.Camera.fit(clouds, width=37, height=23)
    v, f = mesh.make_torus(0.09, 0.03, 12, 8)
    v = (v + F32([0.07, 0.07, 0.07])).astype(F32)                     # a ring through the block of particles
    grey, white, lut = (120, 130, 140), (255, 255, 255), render.default_lut()
    solid = MR.mesh_rule(v[None], f[None], cam.row(), 37, 23, lut, white, shade_table(), F=2, base=grey)
    pts, lengths = render.pad_frames(clouds, "cpu")
    pts = pts.numpy()
    image, winner = R.render_rule(pts, cam.row(), 37, 23, 3, lut, white)
    t = np.full(winner.shape, np.inf, F32)
    for k in range(2):
        t[k][winner[k] >= 0] = R.project(pts[k], cam.row())[3][winner[k][winner[k] >= 0]]
    want = {"points": MR.compose_rule([(image, t), (solid[0], solid[1])])[0]}
    fluid = S.surface_rule(pts, cam.row(), 37, 23, 0.025, lut, white, shade_table(), half_width=2, iters=3)
    want["surface"] = MR.compose_rule([(fluid[0], fluid[1]), (solid[0], solid[1])])[0]
    for style in ("points", "surface"):
        seq = render.SequenceRenderer(str(tmp_path / style), 3, 37, 23, camera=cam, device=dev, style=style,
                                      particle_radius=0.025, solids=(v, f), solids_color=grey)
        seq.push(clouds, 0)
        got = np.stack([read_png(str(tmp_path / style / f"pcd_{k:04d}.png"))[0] for k in range(2)])
        assert np.array_equal(got, want[style]), style
        bare = render.SequenceRenderer(str(tmp_path / (style + "_bare")), 3, 37, 23, camera=cam, device=dev, style=style,
                                       particle_radius=0.025)
        bare.push(clouds, 0)
        plain = np.stack([read_png(str(tmp_path / (style + "_bare") / f"pcd_{k:04d}.png"))[0] for k in range(2)])
        shown = (got != plain).any(-1)
        assert 0.01 < shown.mean() < 0.6, "the ring shows where it is in front, the fluid where the fluid is"
        assert ((solid[2] >= 0) & ~shown).any()


def test_without_the_new_options_the_launches_are_what_they_were(dev, tmp_path, monkeypatch):
    from tpgan_amd import mesh, ops, render
    be = ops.backend_for(torch.zeros(1, device=dev))
    seen, call = [], be._call

    def spy(symbol, *a, **kw):
        seen.append(symbol)
        return call(symbol, *a, **kw)
    monkeypatch.setattr(be, "_call", spy)

    def launches(fn):
        seen.clear()
        fn()
        return list(seen)
    clouds = _lattice_clouds()
    cam = render.Camera.fit(clouds, width=37, height=23)
    batch, lengths = render.pad_frames(clouds, dev)
    points, surface = ["tpg_render_points_f32"], (["tpg_render_spheres_f32"] + ["tpg_surface_smooth_f32"] * 3
                                                   + ["tpg_surface_shade_f32"])
    meshes = ["tpg_render_mesh_f32", "tpg_mesh_shade_f32"]
    assert launches(lambda: render.render(batch, cam, lengths=lengths)) == points
    assert launches(lambda: render.render(batch, cam, lengths=lengths, return_winner=True)) == points
    assert launches(lambda: render.render_surface(batch, cam, lengths=lengths)) == surface
    for style, want in (("points", points), ("surface", surface)):
        seq = render.SequenceRenderer(str(tmp_path / style), 3, 37, 23, camera=cam, device=dev, style=style)
        assert launches(lambda: seq.push(clouds, 0)) == want
    solid = mesh.make_icosphere(1)
    assert launches(lambda: render.render(batch, cam, lengths=lengths, solids=solid)) == points + meshes
    assert launches(lambda: render.render_surface(batch, cam, lengths=lengths, solids=solid)) == surface + meshes
    assert launches(lambda: render.render_mesh(solid, cam, device=dev)) == meshes
