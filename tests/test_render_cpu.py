"""The renderer without a GPU: the PNG writer, the cameras, the torch composition of `ops.render_points` against the numpy
statement of the rule (tests/render_rule.py), the C entry's argument checks and the trainers' flags."""
import ctypes as C
import os
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_rule as R  # noqa: E402


# ---- write_png ----------------------------------------------------------------------------------------------------------
def read_png(path):
    """Inflate by hand: -> (array (H,W,3), IHDR fields, the scanlines' filter bytes); every chunk's CRC is checked."""
    blob = open(path, "rb").read()
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(blob):
        n, kind = struct.unpack(">I4s", blob[at:at + 8])
        data = blob[at + 8:at + 8 + n]
        assert struct.unpack(">I", blob[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + data) & 0xFFFFFFFF
        chunks.append((kind, data))
        at += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    ihdr = struct.unpack(">IIBBBBB", chunks[0][1])
    w, h = ihdr[:2]
    raw = np.frombuffer(zlib.decompress(b"".join(d for k, d in chunks if k == b"IDAT")), np.uint8).reshape(h, 1 + 3 * w)
    return raw[:, 1:].reshape(h, w, 3), ihdr, raw[:, 0]


@pytest.mark.parametrize("shape", [(1, 1), (7, 13), (48, 64)])
def test_write_png_decodes_to_the_same_array(tmp_path, shape):
    from tpgan_amd import render
    rng = np.random.default_rng(shape[0])
    image = rng.integers(0, 256, size=(*shape, 3), dtype=np.uint8)
    path = str(tmp_path / "a.png")
    render.write_png(path, torch.from_numpy(image))
    got, ihdr, filters = read_png(path)
    assert np.array_equal(got, image)
    assert ihdr == (shape[1], shape[0], 8, 2, 0, 0, 0)          # width, height, 8 bits, RGB, deflate, filter 0, no interlace
    assert (filters == 0).all() and len(filters) == shape[0]
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as im:
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), image)


def test_write_png_refuses_other_layouts(tmp_path):
    from tpgan_amd import render
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 4), np.uint8)):
        with pytest.raises(ValueError):
            render.write_png(str(tmp_path / "b.png"), bad)


def test_default_lut_is_a_closed_form_ramp():
    from tpgan_amd import render
    lut = render.default_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    x = np.arange(256) / 255.0
    want = np.stack([np.clip(1.5 - np.abs(4 * x - k), 0, 1) for k in (3, 2, 1)], 1)
    assert np.abs(lut / 255.0 - want).max() <= 0.5 / 255 + 1e-12
    assert len({tuple(c) for c in lut.tolist()}) == 256          # every level its own colour
    assert lut[0, 2] > lut[0, 0] and lut[255, 0] > lut[255, 2]   # blue end, red end


# ---- cameras ------------------------------------------------------------------------------------------------------------
def orthonormal(cam, tol):
    m = np.stack([cam.r, cam.d, cam.f])
    return np.abs(m @ m.T - np.eye(3)).max() <= tol


@pytest.mark.parametrize("mode", ["ortho", "pinhole"])
@pytest.mark.parametrize("direction", [(0.0, 0.0, -1.0), (-0.4, -0.3, -1.0), (1.0, 0.2, 0.1)])
def test_fit_holds_every_valid_point_inside_the_margin(mode, direction):
    from tpgan_amd import render
    rng = np.random.default_rng(5)
    pts = (rng.normal(size=(3, 400, 3)) * [0.5, 0.2, 0.9] + [3.0, -1.0, 0.5]).astype(np.float32)
    W, H, margin = 96, 64, 0.1
    cam = render.Camera.fit(torch.from_numpy(pts), direction=direction, mode=mode, width=W, height=H, margin=margin)
    assert orthonormal(cam, 1e-12)
    row = cam.row()
    assert row.dtype == np.float32 and row.shape == (18,) and row[17] == (1 if mode == "pinhole" else 0)
    m32 = row[3:12].reshape(3, 3).astype(np.float64)
    assert np.abs(m32 @ m32.T - np.eye(3)).max() <= 4 * 2.0 ** -24           # the fp32 rows, rounded once
    assert np.allclose(np.cross(cam.r, cam.d), cam.f, atol=1e-12)           # right x down = forward
    u, v, t = cam.project(pts.reshape(-1, 3))
    eps = 1e-3                                                               # the camera's rounding to fp32, in pixels
    assert u.min() >= margin * W / 2 - eps and u.max() <= W - margin * W / 2 + eps
    assert v.min() >= margin * H / 2 - eps and v.max() <= H - margin * H / 2 + eps
    assert t.min() >= 0 and t.max() <= cam.far - cam.near
    # the fit is tight in one of the two directions
    slack = min(u.min() - margin * W / 2, W - margin * W / 2 - u.max(), v.min() - margin * H / 2,
                H - margin * H / 2 - v.max())
    assert slack <= 0.25 * min(W, H)


def test_fit_ignores_padding_nan_rows_and_rows_beyond_the_length():
    from tpgan_amd import render
    rng = np.random.default_rng(6)
    pts = rng.uniform(-1, 1, size=(2, 100, 3)).astype(np.float32)
    base = render.Camera.fit(torch.from_numpy(pts[:, :60].copy())).row()
    dirty = pts.copy()
    dirty[0, 60:70] = 999.0
    dirty[1, 60:65] = np.nan
    dirty[1, 65:70, 1] = -np.inf
    dirty[0, 70:, 0] = 950.0
    dirty[1, 70:] = [5.0, 900.0, -7.0]
    assert np.array_equal(render.Camera.fit(torch.from_numpy(dirty)).row(), base)
    big = pts.copy()
    big[:, 60:] *= 50.0
    assert np.array_equal(render.Camera.fit(torch.from_numpy(big), lengths=[60, 60]).row(), base)
    assert np.array_equal(render.Camera.fit([pts[0, :60], torch.from_numpy(pts[1, :60])]).row(), base)   # a list of clouds
    with pytest.raises(ValueError):
        render.Camera.fit(torch.full((4, 3), 999.0))


def test_look_at_ortho_and_pinhole_agree_at_the_target():
    from tpgan_amd import render
    eye, target = (2.0, 1.5, 4.0), (0.3, -0.2, 0.5)
    cams = {m: render.Camera.look_at(eye, target, mode=m, width=80, height=60, scale=25.0) for m in ("ortho", "pinhole")}
    for cam in cams.values():
        assert orthonormal(cam, 1e-12)
        u, v, t = cam.project(np.array([target]))
        assert abs(u[0] - 40) < 1e-4 and abs(v[0] - 30) < 1e-4 and t[0] > 0
    # the plane through the target maps alike in both modes: `scale` pixels per unit length
    o = cams["ortho"]
    plane = np.array(target) + 0.7 * o.r - 0.4 * o.d
    (uo, vo, _), (up, vp, _) = o.project(plane[None]), cams["pinhole"].project(plane[None])
    assert abs(uo[0] - up[0]) < 1e-3 and abs(vo[0] - vp[0]) < 1e-3
    assert abs(uo[0] - (40 + 0.7 * 25)) < 1e-3 and abs(vo[0] - (30 - 0.4 * 25)) < 1e-3
    # image-DOWN: a point above the target (world up) lands on a smaller v
    assert o.project(np.array([target]) + [0, 1.0, 0])[1][0] < 30
    with pytest.raises(ValueError):
        render.Camera.look_at(eye, target, mode="pinhole", near=0.0)


# ---- the torch composition against the numpy statement ---------------------------------------------------------------
def run_case(case, device):
    import tpgan_amd.ops as ops
    kw = {k: v for k, v in case.items() if k not in ("expect", "points", "cams", "W", "H", "lut", "background")}
    if "scalar" in kw:
        kw["scalar"] = torch.from_numpy(kw["scalar"]).to(device)
    image, winner = ops.render_points(torch.from_numpy(case["points"]).to(device), case["cams"], case["W"], case["H"],
                                      torch.from_numpy(case["lut"]), background=case["background"], **kw)
    assert image.dtype == torch.uint8 and winner.dtype == torch.int32
    return image.cpu().numpy(), winner.cpu().numpy()


def rule_of(case):
    return R.render_rule(**{k: v for k, v in case.items() if k != "expect"})


@pytest.mark.parametrize("name", sorted(R.small_cases()))
def test_torch_composition_equals_the_rule_on_the_small_cases(oracle_cpu, name):
    case = R.small_cases()[name]
    want_image, want_winner = rule_of(case)
    case["expect"](want_image, want_winner)                     # the statement itself says what the issue says
    image, winner = run_case(case, "cpu")
    assert np.array_equal(winner, want_winner) and np.array_equal(image, want_image)


@pytest.mark.parametrize("mode", [R.ORTHO, R.PINHOLE])
def test_torch_composition_equals_the_rule_on_a_random_cloud(oracle_cpu, mode):
    rng = np.random.default_rng(11 + mode)
    W, H = 40, 28
    pts = R.random_cloud(rng, 2, 300)
    pts[1, 100:130] = pts[1, 7]                                  # exact duplicates: the lowest index shows
    case = dict(points=pts, cams=np.stack([R.tilted_cam(W, H, mode), R.tilted_cam(W, H, mode, eye=(-2.0, 0.4, 1.5))]),
                W=W, H=H, size=3, lut=R.code_lut(), background=R.BG, lengths=[300, 211],
                scalar=rng.normal(size=(2, 300)).astype(np.float32), lo=-1.0, hi=1.5)
    want_image, want_winner = rule_of(case)
    assert (want_winner >= 0).mean() > 0.1
    image, winner = run_case(case, "cpu")
    assert np.array_equal(winner, want_winner) and np.array_equal(image, want_image)


def test_render_points_validates_and_fills_empty_batches(oracle_cpu):
    import tpgan_amd.ops as ops
    lut, pts = torch.from_numpy(R.code_lut()), torch.zeros(1, 4, 3)
    with pytest.raises(RuntimeError, match="size"):
        ops.render_points(pts, R.cam_row(), 8, 8, lut, size=17)
    with pytest.raises(RuntimeError, match="near"):
        ops.render_points(pts, R.cam_row(mode=R.PINHOLE, near=0.0), 8, 8, lut)
    with pytest.raises(RuntimeError, match="cameras"):
        ops.render_points(pts, np.stack([R.cam_row()] * 3), 8, 8, lut)
    with pytest.raises(RuntimeError, match="range"):
        ops.render_points(pts, R.cam_row(), 8, 8, lut, scalar=torch.zeros(1, 4), lo=1.0, hi=1.0)
    with pytest.raises(RuntimeError, match="float tensor"):
        ops.render_points(pts.double(), R.cam_row(), 8, 8, lut)
    for empty in (torch.zeros(0, 4, 3), torch.zeros(2, 0, 3)):
        image, winner = ops.render_points(empty, R.cam_row(), 8, 6, lut, background=R.BG)
        assert image.shape == (empty.shape[0], 6, 8, 3) and (image == torch.tensor(R.BG, dtype=torch.uint8)).all()
        assert winner.shape == (empty.shape[0], 6, 8) and (winner == -1).all()


def test_render_layer_colours_and_shapes(oracle_cpu):
    from tpgan_amd import render
    rng = np.random.default_rng(3)
    pts = torch.from_numpy(R.random_cloud(rng, 2, 200))
    cam = render.Camera.fit(pts, width=32, height=24)
    depth = render.render(pts, cam, size=2)
    assert depth.shape == (2, 24, 32, 3) and torch.equal(depth, render.render(pts, cam, "depth", size=2))
    assert torch.equal(render.render(pts[1], cam, size=2), depth[1])                       # (N,3) -> (H,W,3)
    vel = torch.from_numpy(rng.normal(size=(2, 200, 3)).astype(np.float32))
    speed = torch.sqrt((vel[..., 0] * vel[..., 0] + vel[..., 1] * vel[..., 1]) + vel[..., 2] * vel[..., 2])
    image, winner = render.render(pts, cam, "speed", size=2, velocity=vel, return_winner=True)
    again = render.render(pts, cam, speed, size=2, lo=float(speed.min()), hi=float(speed.max()))
    assert torch.equal(image, again) and (winner >= 0).any()
    want, _ = R.render_rule(pts.numpy(), cam.row(), 32, 24, 2, render.default_lut(), (255, 255, 255), scalar=speed.numpy(),
                            lo=float(speed.min()), hi=float(speed.max()))
    assert np.array_equal(image.numpy(), want)
    with pytest.raises(ValueError):
        render.render(pts, cam, "density")                                                # needs a cutoff


# ---- the C entry's argument checks: no device is touched ---------------------------------------------------------------
def test_render_entry_rejects_bad_arguments_before_any_launch(hip_lib):
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    cam = R.cam_row()
    pin = R.cam_row(mode=R.PINHOLE, near=0.0)

    def call(points=p, F=1, N=4, cams=cam, ncam=1, W=8, H=8, size=3, lo=0.0, hi=1.0, lut=p, bg=p, keys=p, image=p,
             winner=p):
        return hip_lib.tpg_render_points_f32(points, None, None, F, N, cams.ctypes.data, ncam, W, H, size, lo, hi, lut, bg,
                                             keys, image, winner, None)
    assert call(image=None) == -1 and call(winner=None) == -1
    assert call(size=0) == -1 and call(size=17) == -1
    assert call(W=0) == -1 and call(H=0) == -1 and call(H=-3) == -1
    assert call(hi=0.0) == -1 and call(lo=2.0, hi=1.0) == -1 and call(hi=float("nan")) == -1
    assert call(F=-1) == -1 and call(N=-1) == -1
    assert call(F=0) == 0 and call(N=0) == 0
    assert call(F=0, points=None, keys=None) == 0
    assert call(cams=pin) == -1                                   # pinhole needs near > 0
    assert call(points=None) == -1 and call(keys=None) == -1 and call(lut=None) == -1 and call(bg=None) == -1
    assert call(ncam=2) == -1                                     # one camera, or one per frame
    bad = cam.copy()
    bad[4] = np.nan
    assert call(cams=bad) == -1
    assert call(keys=C.c_void_p(p.value + 4)) == -1               # the key buffer holds 64-bit words
    assert call(W=16385) == -3 and call(F=65536) == -3


# ---- the trainers' flags ----------------------------------------------------------------------------------------------
def test_trainers_accept_the_sample_flags_with_their_defaults():
    from tpgan_amd import train, train_action
    opt = train.parse_args([])
    assert (opt.samples, opt.test_sequence_num, opt.dump_visualization) == (0, 4, False)
    assert opt.test_dataset_path == "../../data/test_data_0.025_fine"
    assert (opt.samples_width, opt.samples_height) == (512, 512)
    assert train.parse_args(["--dump_visualization"]).samples == 4
    assert train.parse_args(["--dump_visualization", "--samples", "2"]).samples == 2
    assert train.parse_args(["--dump_visualization", "--samples", "0"]).samples == 0
    assert train.parse_args(["--samples", "3", "--test_dataset_path", "x", "--test_sequence_num", "2"]).samples == 3
    act = train_action.parse_args([])
    assert (act.samples, act.samples_width, act.samples_height) == (0, 512, 512)
    assert train_action.parse_args(["--dump_visualization"]).samples == 0          # still accepted, still ignored
    assert train_action.parse_args(["--samples", "2"]).samples == 2


def test_fluid_test_pass_on_the_host_leaves_the_checkpoints_alone(oracle_cpu, tmp_path, capsys):
    """The GPU file's trainer check on CPU tensors over the oracle backend (the pass through the torch composition)."""
    import test_render_gpu as G
    from tpgan_amd import train
    G.check_samples(train.main, G.fluid_args(tmp_path, "cpu"), tmp_path, capsys, 2, 48, 32, lambda n: 256 <= n <= 2048)


def test_samples_0_constructs_no_test_data(oracle_cpu, tmp_path, monkeypatch):
    """Without --samples the run never asks for held-out clips: a test set that does not exist is not an error."""
    from test_data_cpu import write_dataset
    from tpgan_amd import train
    asked = []
    monkeypatch.setattr(train, "held_out_fluid_clips", lambda *a, **k: asked.append(a) or [])
    data = str(tmp_path / "data")
    write_dataset(data)
    args = ["--train_dataset_path", data, "--train_sequence_num", "2", "--sequence_length", "5", "--batch_size", "2",
            "--sample_num", "512", "--amp", "none", "--device", "cpu", "--ckpt_every", "1", "--iters", "1",
            "--test_dataset_path", str(tmp_path / "missing"), "--log_dir", str(tmp_path / "log")]
    assert train.main(args) == 0
    assert asked == [] and not os.path.exists(tmp_path / "log" / "samples")
