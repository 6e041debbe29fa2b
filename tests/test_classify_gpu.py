"""python -m tpgan_amd.classify on the GPU: one epoch and an evaluation on a toy dataset, starting from a checkpoint that
tpgan_amd.train_action itself wrote; the evaluation pass takes the one-launch eval tails under bf16."""
import json
import os

import numpy as np
import pytest
import torch

from test_action_data_cpu import STEP_GOLDEN
from test_classify_cpu import _toy_dataset

pytestmark = pytest.mark.gpu


def test_classify_from_a_train_action_checkpoint(tmp_path, capsys, monkeypatch):
    import tpgan_amd.ops as ops
    from tpgan_amd import classify, train_action
    data, run, log = (os.path.join(str(tmp_path), d) for d in ("data", "run", "log"))
    _toy_dataset(data)
    num_points = int(np.load(STEP_GOLDEN)["high"].shape[2])            # the smallest the action networks are known to run at
    assert train_action.main(["--data_dir", data, "--batch_size", "2", "--num_points", str(num_points), "--amp", "none",
                              "--iters", "1", "--log_dir", run, "--seed", "1"]) == 0
    capsys.readouterr()
    calls = []
    real = ops.gather_mlp_max
    monkeypatch.setattr(ops, "gather_mlp_max",
                        lambda *a, **k: (calls.append((torch.is_grad_enabled(), tuple(a[0].shape))), real(*a, **k))[1])
    assert classify.main(["--data_path", data, "--pretrained_ckpt", os.path.join(run, "model_ckpt"), "--log_dir", log,
                          "--epoch", "1", "--num_points", "1024", "--batch_size", "4", "--test_batch_size", "4",
                          "--amp", "bf16"]) == 0
    line = [json.loads(s) for s in capsys.readouterr().out.splitlines() if s.startswith("{")][-1]
    assert line["epoch"] == 0 and np.isfinite(line["train_loss"]) and 0.0 <= line["video_acc"] <= 1.0
    ckpt = torch.load(line["checkpoint"], map_location="cpu", weights_only=True)
    assert tuple(ckpt) == classify.CKPT_KEYS
    # training batches run in train mode (per-layer path); every evaluation batch takes the five fused tails
    assert calls and not any(grad for grad, _ in calls) and len(calls) % 5 == 0
    pre = torch.load(os.path.join(run, "model_ckpt", "tpugan_checkpoint1.ckpt"), map_location="cpu", weights_only=True)
    w = "coarse_graining_module.0.mlps.0.0.weight"
    assert torch.equal(ckpt["model_state_dict"][w], pre["tempo_dis"][w + "_orig"])             # frozen, un-normalised
