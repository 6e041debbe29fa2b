"""tpgan_amd.classify without a GPU: the video vote against the reference's own, one epoch + evaluation of the command
line on a toy dataset over the CPU checker backend, and the sampler's return_lowres keyword."""
import json
import os

import numpy as np
import pytest
import torch

from test_action_data_cpu import numpy_backend, save_video  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "action_cls.npz")


def test_video_vote_matches_the_reference():
    """Against the CAPTURED result of train_action/eval_tempo_feat.test() (tests/golden/capture_cls_goldens.py: a stub
    model returning the stored logits for 40 clips of 6 videos in batches of 16): the same total accuracy and the same
    per-class list, exactly.  Plus the properties the capture cannot show: float32 sums in clip order, first arg-max,
    nan for a class without a video."""
    from tpgan_amd.classify import video_vote
    g = np.load(GOLDEN)
    logits = torch.from_numpy(g["vote/logits"])
    prob = torch.exp(torch.log_softmax(logits, dim=-1)).numpy()
    total, per_class = video_vote(prob, g["vote/label"], g["vote/video"])
    assert total == float(g["vote/total_acc"]) and per_class == g["vote/class_acc"].tolist()
    assert 0.0 < total < 1.0                                           # the fixture has right and wrong videos
    # the order of the clips in memory does not matter, their order per video does (float32 sums): interleaved videos
    perm = np.argsort(np.arange(len(prob)) % 7, kind="stable")
    assert video_vote(prob[perm], g["vote/label"][perm], g["vote/video"][perm])[0] == total
    # sums are float32 and sequential: 1 + 2^-24 + 2^-24 stays 1 in float32 (it would win in float64 or pairwise)
    p = np.array([[1.0, 1.0], [2.0 ** -24, 0.0], [2.0 ** -24, 0.0]], np.float32)
    assert video_vote(p[[0, 1, 2]], [1, 1, 1], [0, 0, 0])[0] == 0.0    # tie -> first arg-max = class 0, label 1
    assert video_vote(p[[1, 2, 0]], [0, 0, 0], [0, 0, 0])[0] == 1.0    # 2^-23 + 1 is representable: class 0 wins
    acc, per_class = video_vote(np.eye(3, dtype=np.float32)[[0, 2]], [0, 2], [5, 9])
    assert acc == 1.0 and per_class[0] == 1.0 and np.isnan(per_class[1]) and per_class[2] == 1.0


def _toy_dataset(root, seed=0):
    """4 train videos (subjects 1-4) and 4 test videos (subjects 6-9) of 4-5 frames of 40-90 points."""
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    for v in range(8):
        sizes = rng.integers(40, 91, size=4 + v % 2)
        frames = [np.stack([rng.integers(0, 240, n), rng.integers(0, 320, n), rng.integers(400, 600, n)], 1)
                  .astype(np.float64) for n in sizes]
        save_video(root, f"a{v % 4 + 1:02d}_s{(v + 1) if v < 4 else (v + 2):02d}_e01_sdepth.npz", frames)


def test_one_epoch_and_an_evaluation_on_a_toy_dataset(numpy_backend, tmp_path, capsys):  # noqa: F811
    from tpgan_amd import classify
    from tpgan_amd.set_abstraction import ActionCls, ActionTempoDis
    data, log = os.path.join(str(tmp_path), "data"), os.path.join(str(tmp_path), "log")
    _toy_dataset(data)
    torch.manual_seed(7)
    trained = ActionTempoDis(3, sn=True)
    pre = os.path.join(str(tmp_path), "pretrained.ckpt")
    torch.save({"tempo_dis": trained.state_dict(), "n_iter": 1}, pre)
    npoints = (48, 32)
    argv = ["--data_path", data, "--pretrained_ckpt", pre, "--log_dir", log, "--epoch", "1", "--device", "cpu",
            "--amp", "none", "--num_points", "64", "--batch_size", "4", "--test_batch_size", "4", "--seed", "1",
            "--npoints", *map(str, npoints)]
    assert classify.main(argv) == 0
    lines = [json.loads(s) for s in capsys.readouterr().out.splitlines() if s.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    path = os.path.join(log, "checkpoints", "model_epoch:0.pth")
    assert line["epoch"] == 0 and line["checkpoint"] == path and np.isfinite(line["train_loss"]) and line["lr"] == 3e-4
    assert 0.0 <= line["video_acc"] <= 1.0 and len(line["class_acc"]) == 20
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    assert tuple(ckpt) == classify.CKPT_KEYS and ckpt["epoch"] == 0 and ckpt["total_acc"] == line["video_acc"]
    # the classifier as main() built it: same seed, same construction order
    torch.manual_seed(1)
    start = ActionCls(3, npoints=npoints)
    start.init_feature_extractor(trained)
    moved, frozen = 0, 0
    for name, p in start.named_parameters():
        same = torch.equal(p, ckpt["model_state_dict"][name])
        if p.requires_grad:
            moved += not same
        else:
            frozen += 1
            assert same, f"frozen parameter {name} changed"
    assert frozen > 0 and moved > 0.9 * sum(p.requires_grad for p in start.parameters())
    # Adam holds the trainable parameters only
    assert len(ckpt["optimizer_state_dict"]["param_groups"][0]["params"]) == sum(p.requires_grad for p in start.parameters())


def test_flags_are_the_reference_s_plus_ours():
    from tpgan_amd import classify
    opt = classify.parse_args(["--data_path", "d", "--pretrained_ckpt", "c"])
    assert (opt.epoch, opt.learning_rate, opt.optimizer, opt.log_dir, opt.decay_rate) == (201, 3e-4, "Adam", "./", 1e-4)
    assert (opt.seed, opt.amp, opt.device, opt.num_points, opt.batch_size, opt.test_batch_size, opt.eval_every) == \
        (1, "bf16", "cuda", 2048, 64, 128, 10)


def test_return_lowres_false_keeps_the_high_resolution_tensors(numpy_backend, tmp_path):  # noqa: F811
    """Draws of a batch, in order: clip indices, subset seeds, scales (train) and -- with return_lowres=True only -- the
    FPS starts, which come last: from the same generator state both settings give the same high-resolution tensors,
    labels (centres, video indices) bit for bit; False returns no low-resolution tensors and draws no starts."""
    from tpgan_amd.data import ActionClipSampler, ActionSequences
    data = os.path.join(str(tmp_path), "data")
    _toy_dataset(data)
    for train in (True, False):
        seq = ActionSequences(data, train=train, frames_per_clip=3, device="cpu")
        ga, gb = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
        full = ActionClipSampler(seq, 3, 64, generator=ga).sample()
        high = ActionClipSampler(seq, 3, 64, generator=gb, return_lowres=False).sample()
        assert len(full) == len(high) + 3
        for a, b in zip(full[:3] + full[6:], high):
            assert a.dtype == b.dtype and torch.equal(a, b)
        assert all(t.shape == (3, 64, 3) for t in high[:3])
        with pytest.raises(ValueError, match="no FPS"):                   # a first pick for an FPS that does not run
            ActionClipSampler(seq, 3, 64, generator=torch.Generator().manual_seed(5), return_lowres=False).sample(
                initial_idx=np.zeros((3, 3), np.int64))
        # one draw less: the starts of T * B frames
        torch.randint(64, (3, 3), generator=gb)
        assert torch.equal(ga.get_state(), gb.get_state())
