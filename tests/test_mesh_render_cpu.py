"""The mesh renderer without a GPU: properties of the numpy statement of its rule (tests/mesh_render_rule.py), the torch
statement (`ops._render_mesh_torch`, `ops._mesh_shade_torch`) on CPU tensors against it bit for bit, `compose_layers`
and `return_depth` against their definitions, the layers above over the torch statement, and the C entries' status
codes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_render_cases as MC  # noqa: E402
import mesh_render_rule as MR  # noqa: E402
import render_rule as R  # noqa: E402
from test_render_cpu import read_png  # noqa: E402

F32 = np.float32


@pytest.fixture(autouse=True)
def _checker_for_cpu_tensors(oracle_cpu):
    """CPU tensors go to the registered checker backend; it has no mesh entry, so the ops take the torch statement."""
    yield


def shade_table():
    from tpgan_amd import ops
    return ops.surface_shade()


def run(args, **kw):
    """`ops.render_mesh` on CPU tensors (the torch statement: the checker backend has no mesh entry)."""
    from tpgan_amd import ops
    a = dict(args)
    v, f = (torch.from_numpy(np.array(a.pop(k))) for k in ("vertices", "faces"))
    cams, W, H = np.array(a.pop("cams")), a.pop("W"), a.pop("H")
    kw = {k: torch.from_numpy(np.array(x)) if k in ("normals", "scalar") else x for k, x in kw.items()}
    image, depth, winner = ops.render_mesh(v, f, cams, W, H, torch.from_numpy(R.code_lut()), background=R.BG, **a, **kw)
    assert image.dtype == torch.uint8 and depth.dtype == torch.float32 and winner.dtype == torch.int32
    return image.numpy(), depth.numpy(), winner.numpy()


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


# ---- properties of the rule ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MC.MODES))
def test_a_closed_mesh_covers_every_pixel_zero_or_two_times(mode):
    from tpgan_amd import mesh
    v, f = mesh.make_icosphere(2)
    for W, H in MC.SIZES.values():
        cam = R.tilted_cam(W, H, MC.MODES[mode], scale=0.42 * min(W, H))
        count = MR.coverage_count(v + F32([0.05, -0.02, 0.1]), f, cam, W, H)
        assert set(np.unique(count)) == {0, 2}, np.unique(count)


def _on_shared(case):
    """Pixel centres that lie on an edge of two or more faces, and those that lie on a vertex of three or more."""
    W, H = case["W"], case["H"]
    s = MR.Setup(case["vertices"][0], case["faces"][0], np.asarray(case["cams"], F32), W, H, case["vertices"].shape[1],
                 case["faces"].shape[1])
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    edges, corners = np.zeros((H, W), int), np.zeros((H, W), int)
    for k in range(len(s.index)):
        w = s.weights(k, xs, ys)
        inside = np.all([wi >= 0 for wi in w], 0)
        zeros = np.sum([wi == 0 for wi in w], 0)
        edges += inside & (zeros == 1)
        corners += inside & (zeros == 2)
    return edges >= 2, corners >= 3


def test_centres_on_shared_edges_and_vertices_belong_to_exactly_one_face():
    fan = MC.planar_fan()
    count = MR.coverage_count(fan["vertices"][0], fan["faces"][0], fan["cams"], fan["W"], fan["H"])
    _, corners = _on_shared(fan)
    assert corners[7, 8] and corners.sum() == 1                  # the hub IS the centre of pixel (8, 7)
    ys, xs = np.meshgrid(np.arange(fan["H"]), np.arange(fan["W"]), indexing="ij")
    well_inside = np.hypot(xs + 0.5 - 8.5, ys + 0.5 - 7.5) < 5.0 * np.cos(np.pi / 7) - 0.01
    assert count.max() == 1 and (count[well_inside] == 1).all() and count[7, 8] == 1

    grid = MC.planar_grid()
    count = MR.coverage_count(grid["vertices"][0], grid["faces"][0], grid["cams"], grid["W"], grid["H"])
    edges, corners = _on_shared(grid)
    assert edges.sum() >= 20 and corners.sum() >= 6              # horizontal, vertical and diagonal edges; inner corners
    want = np.zeros_like(count)
    want[1:7, 2:10] = 1          # x 2.5 .. 10.5, y 1.5 .. 7.5: the left and top borders own their centres, the others not
    assert np.array_equal(count, want)
    depth, winner = MR.raster_rule(**grid)
    assert np.array_equal(winner >= 0, want[None] == 1)


def _one(tris, **kw):
    return MC._soup(tris, 16, 16, **kw)


def test_ties_show_the_lower_index_and_a_face_without_area_draws_nothing():
    t = MC.box_triangle(2, 2, 6, 6, (3.0, 3.0, 3.0))
    flat = [[1.0, 1.0, 1.0], [5.0, 5.0, 1.0], [9.0, 9.0, 1.0]]                      # A == 0, nearer than everything
    point = [[4.5, 4.5, 1.0]] * 3
    depth, winner = MR.raster_rule(**_one([flat, t, point, t, t]))
    assert set(np.unique(winner)) == {-1, 1} and (winner == 1).sum() >= 10
    assert (depth[winner == 1] == 3.0).all() and np.isinf(depth[winner < 0]).all()
    compare(run(_one([flat, t, point, t, t])), (rule_image(_one([flat, t, point, t, t]), depth, winner), depth, winner), "ties")


def test_faces_with_bad_indices_or_dropped_vertices_draw_nothing():
    good = np.array(MC.box_triangle(2, 2, 6, 6, (3.0, 3.0, 3.0)), F32)
    nan, inf = np.nan, np.inf
    bad = [[nan, 3.0, 1.0], [3.0, inf, 1.0], [3.0, 3.0, -inf], [3.0, 3.0, nan], [3.0, 3.0, inf],
           [3.0, 3.0, np.nextafter(F32(0.5), F32(0))], [3.0, 3.0, np.nextafter(F32(10), F32(20))],     # near = 0.5, far = 10
           [32768.0, 3.0, 1.0], [3.0, -32768.0, 1.0], [1e30, 3.0, 1.0]]
    vertices = np.concatenate([good, np.array(bad, F32)])[None]
    V = vertices.shape[1]
    faces = [[0, 1, 2]] + [[0, 2, 3 + k] for k in range(len(bad))] + [[-1, 1, 2], [0, V, 2], [0, 1, 2 ** 31 - 1],
                                                                      [-2 ** 31, 1, 2]]
    args = dict(vertices=vertices, faces=np.array(faces, np.int32)[None], cams=R.cam_row(near=0.5), W=16, H=16)
    depth, winner = MR.raster_rule(**args)
    assert set(np.unique(winner)) == {-1, 0}
    compare(run(args), (rule_image(args, depth, winner), depth, winner), "dropped")
    # the guard band is a bound on |u|: just inside it the same face IS drawn, across the whole row
    inside = vertices.copy()
    inside[0, 10] = [np.nextafter(F32(32768), F32(0)), 3.0, 1.0]
    d2, w2 = MR.raster_rule(inside, args["faces"], args["cams"], 16, 16)
    assert (w2 == 8).any()
    # beyond the lengths nothing is read
    d3, w3 = MR.raster_rule(**args, vlengths=[2], flengths=[5])
    assert (w3 == -1).all()
    compare(run(args, vlengths=[2], flengths=[5]), (rule_image(dict(args, vlengths=[2], flengths=[5]), d3, w3), d3, w3), "lengths")


# ---- the torch statement against the rule ----------------------------------------------------------------------------
@pytest.mark.parametrize("size", sorted(MC.SIZES))
@pytest.mark.parametrize("mode", sorted(MC.MODES))
def test_torch_statement_equals_the_rule(mode, size):
    args, depth, winner, extra = MC.random_case(mode, size)
    for kw in (dict(), dict(normals=extra["normals"]), dict(scalar=extra["scalar"], lo=-1.0, hi=1.5),
               dict(normals=extra["normals"], base=(200, 100, 50))):
        compare(run(args, **kw), (rule_image(args, depth, winner, **kw), depth, winner), f"{mode} {size} {sorted(kw)}")


@pytest.mark.parametrize("name", MC.EDGE_NAMES)
def test_torch_statement_equals_the_rule_at_the_class_edges(name):
    args, depth, winner = MC.edge_case_answers()[name]
    compare(run(args), (rule_image(args, depth, winner), depth, winner), name)


def test_compose_layers_equals_its_definition():
    from tpgan_amd import ops
    rng = np.random.default_rng(3)
    layers = []
    for k in range(3):
        depth = rng.integers(0, 4, size=(2, 5, 7)).astype(F32)           # many ties
        depth[rng.random(depth.shape) < 0.3] = np.inf
        layers.append((np.full((2, 5, 7, 3), 10 * (k + 1), np.uint8), depth))
    layers[1][1][0, 0, 0] = np.nan                                       # never in front
    image, depth = ops.compose_layers([(torch.from_numpy(i), torch.from_numpy(d)) for i, d in layers])
    want_image, want_depth = MR.compose_rule(layers)
    assert np.array_equal(image.numpy(), want_image) and np.array_equal(depth.numpy(), want_depth, equal_nan=True)
    for at in np.ndindex(2, 5, 7):                                       # the definition, pixel by pixel
        best = 0
        for k in (1, 2):
            if layers[k][1][at] < layers[best][1][at]:                   # strictly nearer: the earlier layer keeps a tie
                best = k
        assert image[at][0] == 10 * (best + 1) and depth[at] == layers[best][1][at]
    with pytest.raises(RuntimeError):
        ops.compose_layers([])
    with pytest.raises(RuntimeError):
        ops.compose_layers([(torch.zeros(2, 2, 3), torch.zeros(2, 2)), (torch.zeros(2, 3, 3), torch.zeros(2, 3))])


def test_return_depth_is_the_winners_t(oracle_cpu):
    from tpgan_amd import ops
    rng = np.random.default_rng(8)
    W, H = 37, 23
    pts = R.random_cloud(rng, 2, 200, spread=0.4)
    for mode in (R.ORTHO, R.PINHOLE):
        cams = np.stack([R.tilted_cam(W, H, mode), R.tilted_cam(W, H, mode, eye=(-2.0, 0.4, 1.5))])
        want_image, want_winner = R.render_rule(pts, cams, W, H, 3, R.code_lut(), R.BG)
        want = np.full((2, H, W), np.inf, F32)
        for f in range(2):
            t = R.project(pts[f], cams[f])[3]
            want[f][want_winner[f] >= 0] = t[want_winner[f][want_winner[f] >= 0]]
        lut = torch.from_numpy(R.code_lut())
        image, winner, depth = ops.render_points(torch.from_numpy(pts), cams, W, H, lut, 3, background=R.BG, return_depth=True)
        assert np.array_equal(winner.numpy(), want_winner) and np.array_equal(image.numpy(), want_image)
        assert np.array_equal(depth.numpy().view(np.uint32), want.view(np.uint32)) and np.isfinite(want).any()
        plain = ops.render_points(torch.from_numpy(pts), cams, W, H, lut, 3, background=R.BG)
        assert len(plain) == 2 and torch.equal(plain[0], image) and torch.equal(plain[1], winner)
    empty = ops.render_points(torch.zeros(2, 0, 3), cams, W, H, lut, return_depth=True)
    assert len(empty) == 3 and bool(torch.isinf(empty[2]).all())


def test_render_mesh_validates_its_arguments():
    from tpgan_amd import ops
    v, f = torch.zeros(1, 4, 3), torch.zeros(1, 2, 3, dtype=torch.int32)
    lut, cam = torch.from_numpy(R.code_lut()), R.cam_row()
    for bad in (dict(vertices=torch.zeros(1, 4, 2)), dict(faces=torch.zeros(1, 2, 3, dtype=torch.int64)),
                dict(faces=torch.zeros(2, 2, 3, dtype=torch.int32)), dict(normals=torch.zeros(1, 3, 3)),
                dict(scalar=torch.zeros(1, 4)), dict(scalar=torch.zeros(1, 5), lo=0.0, hi=1.0), dict(base=(1, 2, 300)),
                dict(shade=np.zeros(10, F32)), dict(vlengths=[1, 2]), dict(max_key_bytes=0), dict(lo=1.0, hi=1.0),
                dict(cams=np.stack([cam] * 3), vertices=torch.zeros(2, 4, 3), faces=torch.zeros(2, 2, 3, dtype=torch.int32))):
        kw = dict(vertices=v, faces=f, cams=cam, width=8, height=8, lut=lut)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            ops.render_mesh(**kw)
    image, depth, winner = ops.render_mesh(v, torch.zeros(1, 0, 3, dtype=torch.int32), np.stack([cam] * 2), 8, 6, lut,
                                           background=R.BG)
    assert image.shape == (2, 6, 8, 3) and (image.numpy() == R.BG).all() and bool(torch.isinf(depth).all())
    assert bool((winner == -1).all())


# ---- the layers above, over the torch statement ----------------------------------------------------------------------
def test_render_layer_takes_meshes_tuples_and_lists():
    from tpgan_amd import mesh, ops, render
    v, f = mesh.make_icosphere(1)
    v2, f2 = mesh.make_torus(0.6, 0.25, 12, 8)
    n = v / np.linalg.norm(v, axis=1, keepdims=True)
    cam = render.Camera.fit(torch.from_numpy(v), width=40, height=30)
    lut = render.default_lut()
    image, depth, winner = ops.render_mesh(torch.from_numpy(v)[None], torch.from_numpy(f)[None], cam.row(), 40, 30, lut,
                                           normals=torch.from_numpy(n)[None])
    assert 0.1 < float(torch.isfinite(depth).float().mean()) < 1.0
    one = render.render_mesh((v, f, n), cam, return_depth=True, return_winner=True)
    assert one[0].shape == (30, 40, 3) and all(torch.equal(a, b[0]) for a, b in zip(one, (image, depth, winner)))
    m = mesh.Mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(n), None, 0.0)
    assert torch.equal(render.render_mesh(m, cam), image[0])
    flat = render.render_mesh((v, f), cam)                                       # no normals: every face its own
    assert flat.shape == (30, 40, 3) and not torch.equal(flat, image[0])
    grey = render.render_mesh((v, f, n), cam, base=(90, 90, 90))
    assert not torch.equal(grey, image[0]) and torch.equal((grey == 255).all(-1), (image[0] == 255).all(-1))
    both = render.render_mesh([(v, f, n), (v2, f2)], cam)                        # ragged; no normals unless all have them
    assert both.shape == (2, 30, 40, 3) and torch.equal(both[0], flat)
    assert torch.equal(both[1], render.render_mesh((v2, f2), cam))
    turn = render.render_mesh((v, f, n), [cam, render.Camera.fit(torch.from_numpy(v), direction=(1.0, 0.0, 0.0),
                                                                  width=40, height=30)])
    assert turn.shape == (2, 30, 40, 3) and torch.equal(turn[0], image[0])
    tint = render.render_mesh((v, f, n), cam, color=torch.from_numpy(v[:, 0]))
    assert torch.equal(tint, ops.render_mesh(torch.from_numpy(v)[None], torch.from_numpy(f)[None], cam.row(), 40, 30, lut,
                                             normals=torch.from_numpy(n)[None], scalar=torch.from_numpy(v[:, 0].copy())[None],
                                             lo=float(v[:, 0].min()), hi=float(v[:, 0].max()))[0][0])
    with pytest.raises(ValueError):
        render.render_mesh(v, cam)
    with pytest.raises(ValueError):
        render.render_mesh((v, f), cam, color="density")


def _fluid_and_wall():
    """A slab of points at z = 0 and a quad that crosses it: in front of it on the left, behind it on the right."""
    rng = np.random.default_rng(4)
    pts = np.concatenate([rng.uniform(-1, 1, (4000, 2)), np.zeros((4000, 1))], 1).astype(F32)
    wall = (np.array([[-0.8, -0.5, 0.5], [0.8, -0.5, -0.5], [0.8, 0.5, -0.5], [-0.8, 0.5, 0.5]], F32),
            np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    return pts, wall


def test_solids_occlude_the_fluid_and_are_occluded_by_it(oracle_cpu):
    from tpgan_amd import ops, render
    pts, wall = _fluid_and_wall()
    cam = render.Camera.look_at((0.0, 0.0, 3.0), (0.0, 0.0, 0.0), mode="ortho", width=40, height=30, scale=15.0, near=1.0,
                                far=5.0)
    p = torch.from_numpy(pts)
    plain, winner = render.render(p, cam, size=3, return_winner=True)
    image, depth = render.render(p, cam, size=3, solids=wall, solids_color=(7, 7, 7), return_depth=True)
    solid = render.render_mesh(wall, cam, base=(7, 7, 7), return_depth=True)
    fluid_depth = ops.render_points(p[None], cam.row(), 40, 30, render.default_lut(), 3, return_depth=True)[2][0]
    want_image, want_depth = MR.compose_rule([(plain.numpy(), fluid_depth.numpy()), (solid[0].numpy(), solid[1].numpy())])
    assert np.array_equal(image.numpy(), want_image) and np.array_equal(depth.numpy(), want_depth)
    # looking down -z the wall's left half (x < 0) is nearer than the slab, its right half is behind it
    left, right = (slice(12, 18), slice(10, 14)), (slice(12, 18), slice(26, 30))
    assert (solid[1][left] < fluid_depth[left]).all() and torch.equal(image[left], solid[0][left])
    assert (fluid_depth[right] < solid[1][right]).all() and torch.equal(image[right], plain[right])
    assert not torch.equal(image[left], plain[left])
    # without the option nothing changes, and the camera is fitted to the fluid alone
    assert torch.equal(render.render(p, cam, size=3), plain)


def test_sequence_renderer_draws_solids_and_the_cli_takes_them(oracle_cpu, tmp_path):
    import argparse

    from tpgan_amd import render
    pts, wall = _fluid_and_wall()
    cam = render.Camera.look_at((0.0, 0.0, 3.0), (0.0, 0.0, 0.0), mode="ortho", width=40, height=30, scale=15.0, near=1.0,
                                far=5.0)
    seq = render.SequenceRenderer(str(tmp_path / "a"), 3, 40, 30, camera=cam, device="cpu", solids=wall,
                                  solids_color=(7, 7, 7))
    seq.push([pts, pts[:2000]], 5)
    want = render.render(render.pad_frames([pts, pts[:2000]], "cpu")[0], cam, size=3, lengths=[4000, 2000], solids=wall,
                         solids_color=(7, 7, 7))
    for t in range(2):
        assert np.array_equal(read_png(str(tmp_path / "a" / f"pcd_{5 + t:04d}.png"))[0], want[t].numpy())
    bare = render.render(render.pad_frames([pts, pts[:2000]], "cpu")[0], cam, size=3, lengths=[4000, 2000])
    assert 0.02 < float((want != bare).any(-1).float().mean()) < 0.5         # the wall's near half shows, shaded
    ap = argparse.ArgumentParser()
    render.add_render_options(ap)
    a = ap.parse_args([])
    assert a.solids is None and tuple(a.solids_color) == render.SOLIDS_COLOR
    assert render.renderer_from(a, str(tmp_path / "b"), "cpu").solids is None
    b = ap.parse_args(["--solids", "icosphere:1", "--solids_color", "1", "2", "3", "--style", "surface_mesh"])
    seq = render.renderer_from(b, str(tmp_path / "b"), "cpu")
    assert seq.style == "surface_mesh" and seq.solids[1].shape == (80, 3) and seq.solids_color == (1, 2, 3) and seq.mesh_options == {}
    with pytest.raises(ValueError):
        render.SequenceRenderer(str(tmp_path / "c"), device="cpu", style="surface_mesh", color="density")


def test_mesh_cli_renders_what_it_wrote(oracle_cpu, tmp_path):
    from tpgan_amd import mesh, render
    rng = np.random.default_rng(2)
    g = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.025
    for i in range(2):
        np.save(tmp_path / f"pcd_{i}.npy", (g + rng.normal(size=g.shape) * 0.001 + 0.01 * i).astype(F32))
    argv = ["--frames", str(tmp_path / "pcd_{i}.npy"), "--count", "2", "--out", str(tmp_path / "m"), "--device", "cpu",
            "--width", "48", "--height", "40", "--mode", "ortho"]
    mesh.main(argv)
    assert not (tmp_path / "png").exists()
    mesh.main(argv + ["--render", str(tmp_path / "png")])
    v0, f0, n0 = mesh.read_ply(str(tmp_path / "m" / "pcd_0000.ply"))
    cam = render.Camera.fit(torch.from_numpy(v0), mode="ortho", width=48, height=40)
    for i in range(2):
        v, f, n = mesh.read_ply(str(tmp_path / "m" / f"pcd_{i:04d}.ply"))
        want = render.render_mesh((v, f, n), cam)
        got = read_png(str(tmp_path / "png" / f"pcd_{i:04d}.png"))[0]
        assert np.array_equal(got, want.numpy()) and 0.05 < (got != 255).any(-1).mean() < 0.95
    mesh.main(argv + ["--render", str(tmp_path / "png2"), "--solids", "torus:0.1,0.03,12,8", "--solids_color", "3", "3", "3"])
    with_solid, plain = (read_png(str(tmp_path / d / "pcd_0000.png"))[0] for d in ("png2", "png"))
    assert with_solid.shape == plain.shape and (with_solid != plain).any()


# ---- the C entries' status codes -------------------------------------------------------------------------------------
def test_mesh_entries_reject_bad_arguments_before_any_launch(hip_lib):
    """No GPU here: every call below is decided before anything is launched."""
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    cams = (C.c_float * 36)(*(list(R.cam_row()) * 2))
    pin = (C.c_float * 18)(*R.cam_row(mode=R.PINHOLE, near=0.0))
    nanc = (C.c_float * 18)(*([float("nan")] + list(R.cam_row())[1:]))
    shade = (C.c_float * 11)(*shade_table())
    badp = (C.c_float * 11)(*(list(shade_table())[:10] + [2.5]))

    def a(vertices=p, faces=p, M=1, V=4, T=2, F=1, cam=cams, ncam=1, W=8, H=8, keys=p, depth=p, winner=p, lst=p):
        return hip_lib.tpg_render_mesh_f32(vertices, None, faces, None, M, V, T, F, cam, ncam, W, H, keys, lst, depth, winner,
                                           None)

    def b(depth=p, winner=p, vertices=p, faces=p, M=1, V=4, T=2, F=1, cam=cams, ncam=1, W=8, H=8, lo=0.0, hi=1.0, lut=p,
          base=None, background=p, table=shade, image=p):
        return hip_lib.tpg_mesh_shade_f32(depth, winner, vertices, None, faces, None, None, None, M, V, T, F, cam, ncam, W,
                                          H, lo, hi, lut, base, background, table, image, None)
    for fn in (a, b):
        assert fn(F=-1) == -1 and fn(V=-1) == -1 and fn(T=-1) == -1 and fn(M=-1) == -1 and fn(W=0) == -1 and fn(H=0) == -1
        assert fn(F=0) == 0 and fn(T=0) == 0 and fn(V=0) == 0                   # nothing to draw: nothing written
        assert fn(F=0, vertices=None, faces=None, cam=None) == 0
        assert fn(vertices=None) == -1 and fn(faces=None) == -1 and fn(cam=None) == -1
        assert fn(M=2) == -1 and fn(M=3, F=2, ncam=2) == -1                     # M is 1 or F
        assert fn(ncam=2) == -1 and fn(cam=pin) == -1 and fn(cam=nanc) == -1
        assert fn(W=16385) == -3 and fn(H=16385) == -3 and fn(F=65536, M=1) == -3
        assert fn(F=40000, W=300, H=300) == -3                                  # more than 2^31 pixels
        assert fn(T=715827883) == -3 and fn(V=715827883) == -3                  # 2^31 / 3
        assert fn(M=2, F=2, ncam=2, W=16385) == -3
    assert a(depth=None) == -1 and a(winner=None) == -1 and a(keys=None) == -1 and a(lst=None) == -1
    assert a(keys=C.c_void_p(p.value + 4)) == -1                                # not 8-byte aligned
    assert a(F=0, keys=None) == 0
    assert b(image=None) == -1 and b(table=None) == -1 and b(table=badp) == -1 and b(hi=0.0) == -1
    assert b(lo=float("nan")) == -1 and b(lo=float("-inf")) == -1
    assert b(depth=None) == -1 and b(winner=None) == -1 and b(background=None) == -1 and b(lut=None) == -1
    assert b(F=0, table=badp) == -1 and b(F=0, hi=-1.0) == -1                   # the table and range come first
