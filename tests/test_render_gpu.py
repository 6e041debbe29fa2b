"""The renderer on the GPU: tpg_render_points_f32 against the numpy statement of its rule (tests/render_rule.py: picture
AND winner map EQUAL, no cap on differing pixels), batch invariance, repeatability and chunking, the trainers' test pass
(bit-identical checkpoints with and without it), `rollout --render` and the render CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_rule as R  # noqa: E402
from test_render_cpu import read_png, rule_of, run_case  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def check(case, dev):
    want_image, want_winner = rule_of(case)
    image, winner = run_case(case, dev)
    diff = int((winner != want_winner).sum()), int((image != want_image).any(-1).sum())
    print(f"pixels whose winner / colour differs from the rule: {diff[0]} / {diff[1]} of {winner.size}; "
          f"covered {int((want_winner >= 0).sum())}")
    assert np.array_equal(winner, want_winner) and np.array_equal(image, want_image)
    return image, winner


# ---- the hand-made cases: one point, corners, occlusion, culling, colour ---------------------------------------------
@pytest.mark.parametrize("name", sorted(R.small_cases()))
def test_small_cases(dev, name):
    case = R.small_cases()[name]
    image, winner = check(case, dev)
    case["expect"](image, winner)


# ---- random clouds against the rule ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cloud():
    """5000 points (several workgroups), 64 of them exact duplicates of one point, and a scalar per point."""
    rng = np.random.default_rng(2024)
    pts = R.random_cloud(rng, 1, 5000)
    pts[0, 3000:3064] = pts[0, 41]
    return pts, rng.normal(size=(1, 5000)).astype(np.float32)


@pytest.mark.parametrize("mode", [R.ORTHO, R.PINHOLE])
@pytest.mark.parametrize("size", [1, 3, 5])
def test_random_cloud_equals_the_rule(dev, cloud, size, mode):
    pts, scalar = cloud
    W, H = 128, 96
    case = dict(points=pts, cams=R.tilted_cam(W, H, mode), W=W, H=H, size=size, lut=R.code_lut(), background=R.BG,
                scalar=scalar, lo=-2.0, hi=2.0)
    _, winner = check(case, dev)
    assert (winner >= 0).mean() > 0.1 and (winner < 0).any()    # not vacuous: 5000 points on 12288 pixels
    dup = np.isin(winner, np.arange(3000, 3064))
    assert not dup.any()                                        # of exact duplicates the lowest index (41) shows
    if size == 3:
        check({k: v for k, v in case.items() if k not in ("scalar", "lo", "hi")}, dev)     # coloured by depth


def test_ragged_batch_with_per_frame_cameras_equals_the_rule(dev):
    rng = np.random.default_rng(77)
    W, H = 128, 96
    pts = R.random_cloud(rng, 3, 2048)
    pts[1, 1:] = np.nan                                         # beyond the frames' lengths: never read
    pts[2, 777:] = 3e38
    cams = np.stack([R.tilted_cam(W, H, R.PINHOLE), R.tilted_cam(W, H, R.ORTHO, eye=(-2.0, 0.4, 1.5)),
                     R.tilted_cam(W, H, R.PINHOLE, eye=(0.3, 2.5, -1.0), scale=20.0)])
    case = dict(points=pts, cams=cams, W=W, H=H, size=3, lut=R.code_lut(), background=R.BG, lengths=[2048, 1, 777])
    _, winner = check(case, dev)
    assert (winner[1] >= 0).sum() <= 9 and winner[1].max() <= 0 and winner[2].max() < 777


# ---- batch invariance, repeatability, chunking -----------------------------------------------------------------------
def test_batch_invariance_repeatability_and_chunking(dev):
    import tpgan_amd.ops as ops
    rng = np.random.default_rng(5)
    W, H, F, N = 96, 64, 20, 3000
    pts = torch.from_numpy(R.random_cloud(rng, F, N)).to(dev)
    lengths = torch.from_numpy(rng.integers(1, N + 1, F))
    scalar = torch.from_numpy(rng.normal(size=(F, N)).astype(np.float32)).to(dev)
    cams = np.stack([R.tilted_cam(W, H, f % 2, eye=(1.1 + 0.1 * f, -0.7, 2.9)) for f in range(F)])   # 2 camera groups
    lut = torch.from_numpy(R.code_lut())
    kw = dict(size=3, lo=-2.0, hi=2.0, background=R.BG)
    image, winner = ops.render_points(pts, cams, W, H, lut, lengths=lengths, scalar=scalar, **kw)
    again = ops.render_points(pts, cams, W, H, lut, lengths=lengths, scalar=scalar, **kw)
    assert torch.equal(image, again[0]) and torch.equal(winner, again[1])
    for f in (0, 7, 16, 19):
        one = ops.render_points(pts[f:f + 1].contiguous(), cams[f], W, H, lut, lengths=lengths[f:f + 1],
                                scalar=scalar[f:f + 1].contiguous(), **kw)
        assert torch.equal(one[0][0], image[f]) and torch.equal(one[1][0], winner[f]), f
    for cap in (8 * W * H, 3 * 8 * W * H + 5, 1):               # 1, 3 and (cap below one frame) 1 frame per chunk
        part = ops.render_points(pts, cams, W, H, lut, lengths=lengths, scalar=scalar, max_key_bytes=cap, **kw)
        assert torch.equal(part[0], image) and torch.equal(part[1], winner), cap
    shared = ops.render_points(pts, cams[3], W, H, lut, lengths=lengths, scalar=scalar, max_key_bytes=5 * 8 * W * H, **kw)
    one = ops.render_points(pts[9:10].contiguous(), cams[3], W, H, lut, lengths=lengths[9:10],
                            scalar=scalar[9:10].contiguous(), **kw)
    assert torch.equal(shared[0][9], one[0][0]) and torch.equal(shared[1][9], one[1][0])


# ---- the trainers' test pass -----------------------------------------------------------------------------------------
def write_fluid_cases(root, cases, steps, n, seed):
    """case{c}/data_{s}.npz: a blob of n particles drifting with its velocities."""
    rng = np.random.default_rng(seed)
    for c in cases:
        os.makedirs(os.path.join(root, f"case{c}"), exist_ok=True)
        pos = (rng.uniform(size=(n, 3)) * [1.0, 0.6, 0.8]).astype(np.float32)
        vel = (rng.normal(size=(n, 3)) * 0.05).astype(np.float32)
        for s in range(steps):
            np.savez(os.path.join(root, f"case{c}", f"data_{s}.npz"), pos=pos + np.float32(0.1 * s) * vel, vel=vel)


def write_action_videos(root, seed):
    from test_action_data_cpu import save_video
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    for v, (subject, sizes) in enumerate([(1, (1500, 2048, 2600, 900)), (2, (3000, 2049, 700)), (6, (1800, 2500, 950, 2100)),
                                          (7, (2048, 777, 3000))]):
        frames = [np.stack([rng.integers(0, 240, n), rng.integers(0, 320, n), rng.integers(400, 600, n)], 1)
                  .astype(np.float64) for n in sizes]
        save_video(root, f"a{v + 1:02d}_s{subject:02d}_e01_sdepth.npz", frames)


def load_ckpt(log_dir, n_iter):
    return torch.load(os.path.join(log_dir, "model_ckpt", f"tpugan_checkpoint{n_iter}.ckpt"), map_location="cpu",
                      weights_only=True)


def same(a, b, where="ckpt"):
    """Every tensor and number of two checkpoints, recursively: bit for bit."""
    if isinstance(a, dict):
        assert a.keys() == b.keys(), where
        for k in a:
            same(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{where}[{i}]")
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and torch.equal(a, b), where
    else:
        assert a == b, where


def check_samples(main, common, tmp_path, capsys, samples, width, height, points_ok):
    """3 iterations with a checkpoint after each, with and without --samples: the same checkpoints (parameters, Adam
    state, schedulers and the `tpgan_amd` RNG block), 3 x 3 x samples pictures and one `test_cd` line per checkpoint."""
    a, b = str(tmp_path / "plain"), str(tmp_path / "sampled")
    assert main(common + ["--log_dir", a]) == 0
    capsys.readouterr()
    assert main(common + ["--log_dir", b, "--samples", str(samples), "--samples_width", str(width), "--samples_height",
                          str(height)]) == 0
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert not os.path.exists(os.path.join(a, "samples"))
    for n_iter in (1, 2, 3):
        same(load_ckpt(a, n_iter), load_ckpt(b, n_iter))
    tests = [l for l in lines if "test_cd" in l]
    assert [l["n_iter"] for l in tests] == [1, 2, 3]
    for l in tests:
        assert len(l["test_cd"]) == samples and all(np.isfinite(v) and v > 0 for v in l["test_cd"]), l
        assert len(l["test_points"]) == samples and all(points_ok(n) for n in l["test_points"]), l
    names = sorted(os.listdir(os.path.join(b, "samples")))
    assert names == sorted(f"{kind}_iter:{n}_{j}.png" for kind in ("gt", "input", "pred") for n in (1, 2, 3)
                           for j in range(samples))
    pictures = {}
    for name in names:
        image, ihdr, _ = read_png(os.path.join(b, "samples", name))
        assert ihdr[:2] == (width, height) and image.shape == (height, width, 3)
        drawn = (image != 255).any(-1)
        assert drawn.any() and not drawn.all(), name                         # points on a white background
        pictures[name] = image
    for j in range(samples):                                                 # the same clips at every checkpoint
        for kind in ("gt", "input"):
            assert np.array_equal(pictures[f"{kind}_iter:1_{j}.png"], pictures[f"{kind}_iter:3_{j}.png"])
        assert not np.array_equal(pictures[f"gt_iter:1_{j}.png"], pictures[f"input_iter:1_{j}.png"])
    return tests


def fluid_args(tmp_path, device):
    train_dir, test_dir = str(tmp_path / "train"), str(tmp_path / "test")
    write_fluid_cases(train_dir, (1, 2), 5, 1300, seed=1)
    write_fluid_cases(test_dir, (1, 2), 5, 2100, seed=2)                     # test patch: (2100 // 1024) * 1024 = 2048
    return ["--train_dataset_path", train_dir, "--train_sequence_num", "2", "--sequence_length", "5", "--batch_size", "2",
            "--sample_num", "512", "--amp", "none", "--device", device, "--ckpt_every", "1", "--log_every", "1", "--iters",
            "3", "--seed", "1", "--test_dataset_path", test_dir, "--test_sequence_num", "2"]


def action_args(tmp_path, device):
    data = str(tmp_path / "videos")
    write_action_videos(data, seed=3)
    return ["--data_dir", data, "--batch_size", "2", "--num_points", "2048", "--amp", "none", "--device", device,
            "--ckpt_every", "1", "--log_every", "1", "--iters", "3", "--seed", "1"]


def test_fluid_trainer_samples_leave_the_checkpoints_alone(dev, tmp_path, capsys):
    from tpgan_amd import train
    # hard masking keeps slot 0 of every input point: between 2048 / 8 and 2048 predicted points
    check_samples(train.main, fluid_args(tmp_path, "cuda"), tmp_path, capsys, 2, 96, 64,
                  lambda n: 256 <= n <= 2048)


def test_fluid_dump_visualization_alone_means_four_samples(dev, tmp_path, capsys):
    from tpgan_amd import train
    args = fluid_args(tmp_path, "cuda")
    args[args.index("--iters") + 1] = "1"
    assert train.main(args + ["--log_dir", str(tmp_path / "log"), "--dump_visualization", "--samples_width", "48",
                              "--samples_height", "48"]) == 0
    line = [json.loads(l) for l in capsys.readouterr().out.splitlines() if "test_cd" in l]
    assert len(line) == 1 and len(line[0]["test_cd"]) == 4
    assert len(os.listdir(tmp_path / "log" / "samples")) == 3 * 4


def test_action_trainer_samples_leave_the_checkpoints_alone(dev, tmp_path, capsys):
    from tpgan_amd import train_action
    check_samples(train_action.main, action_args(tmp_path, "cuda"), tmp_path, capsys, 2, 64, 96, lambda n: n == 2048)


# ---- rollout --render and the render CLI -----------------------------------------------------------------------------
def test_rollout_render_and_the_render_cli(dev, tmp_path):
    from tpgan_amd import render
    from tpgan_amd.srnet import SRNet
    rng = np.random.default_rng(9)
    frames, n = 4, 512
    base = (rng.uniform(size=(n, 3)) * [0.5, 0.3, 0.4]).astype(np.float32)
    for i in range(frames):
        np.savez(tmp_path / f"data_{i}.npz", pos=base + np.float32(0.02 * i) + np.float32(1.5))
    torch.manual_seed(4)
    ckpt = tmp_path / "g.ckpt"
    torch.save({"sr_net": SRNet(3, 128).state_dict(), "n_iter": 0}, ckpt)
    out, png = tmp_path / "out", tmp_path / "png"
    cmd = [sys.executable, "-m", "tpgan_amd.rollout", "--checkpoint", str(ckpt), "--frames", str(tmp_path / "data_{i}.npz"),
           "--count", str(frames), "--chunk", "2", "--out", str(out), "--render", str(png), "--width", "80", "--height",
           "56", "--size", "2", "--mode", "ortho", "--direction", "-0.3", "-0.2", "-1"]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert sorted(os.listdir(png)) == [f"pcd_{i:04d}.png" for i in range(frames)]
    clouds = [np.load(out / f"pcd_{i}.npy") for i in range(frames)]
    cam = render.Camera.fit(clouds[:2], direction=(-0.3, -0.2, -1.0), mode="ortho", width=80, height=56)   # first chunk
    for i in range(frames):
        want = render.render(torch.from_numpy(clouds[i]).to(dev), cam, size=2).cpu().numpy()
        assert (want != 255).any() and np.array_equal(read_png(png / f"pcd_{i:04d}.png")[0], want), i

    # the CLI on the rollout's own output: one camera from the first, middle and last frame, 3 frames per call
    cli = tmp_path / "cli"
    cmd = [sys.executable, "-m", "tpgan_amd.render", "--frames", str(out / "pcd_{i}.npy"), "--count", str(frames), "--out",
           str(cli), "--width", "72", "--height", "72", "--size", "3", "--frames_per_call", "3"]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert sorted(os.listdir(cli)) == [f"pcd_{i:04d}.png" for i in range(frames)]
    cam = render.Camera.fit([clouds[0], clouds[2], clouds[3]], width=72, height=72)
    for i in range(frames):
        want = render.render(torch.from_numpy(clouds[i]).to(dev), cam, size=3).cpu().numpy()
        assert np.array_equal(read_png(cli / f"pcd_{i:04d}.png")[0], want), i
