"""Both trainers under --graph: the step replays from hipGraphs captured on the first batch, a resumed run repeats the
uninterrupted one bit for bit, and the captured Adam follows the learning-rate schedule (a device tensor the scheduler
fills in place)."""
import copy
import json
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_action_data_cpu as action_cpu  # noqa: E402
import test_data_cpu as fluid_cpu  # noqa: E402

pytestmark = pytest.mark.gpu


def _log_lines(capsys):
    return [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]


def test_action_trainer_replays_every_step_and_resumes_bit_exactly(tmp_path, capsys):
    """6 iterations at the step_action golden's cloud size, batch 2, bf16 off, a checkpoint after every one; resumed from
    iteration 3: parameters and Adam moments equal bit for bit.  Every logged step was a replay."""
    from tpgan_amd import train, train_action
    iters, resume_at = 6, 3
    num_points = int(np.load(action_cpu.STEP_GOLDEN)["high"].shape[2])
    data = os.path.join(str(tmp_path), "data")
    action_cpu.write_random_dataset(data, [(1500, 2048, 2600, 900), (3000, 2049, 700, 2500, 1800)])
    common = ["--data_dir", data, "--batch_size", "2", "--num_points", str(num_points), "--amp", "none", "--device", "cuda",
              "--ckpt_every", "1", "--log_every", "1", "--iters", str(iters), "--seed", "1", "--graph"]
    a, b = os.path.join(str(tmp_path), "a"), os.path.join(str(tmp_path), "b")
    assert train_action.main(common + ["--log_dir", a]) == 0
    lines = _log_lines(capsys)
    assert [l["n_iter"] for l in lines] == list(range(1, iters + 1))
    assert all(l["replayed"] == 1 for l in lines) and all(np.isfinite(v) for l in lines for v in l.values())
    ck = os.path.join(a, "model_ckpt")
    full = torch.load(os.path.join(ck, f"tpugan_checkpoint{iters}.ckpt"), map_location="cpu", weights_only=True)
    assert set(full) == set(train.CKPT_KEYS) and full["n_iter"] == iters
    first = torch.load(os.path.join(ck, "tpugan_checkpoint1.ckpt"), map_location="cpu", weights_only=True)
    assert any(not torch.equal(x, y) for x, y in zip(action_cpu._params(first), action_cpu._params(full)))
    assert train_action.main(common + ["--log_dir", b, "--resume", "--path_to_resume",
                                       os.path.join(ck, f"tpugan_checkpoint{resume_at}.ckpt")]) == 0
    lines = _log_lines(capsys)
    assert [l["n_iter"] for l in lines] == list(range(resume_at + 1, iters + 1)) and all(l["replayed"] == 1 for l in lines)
    again = torch.load(os.path.join(b, "model_ckpt", f"tpugan_checkpoint{iters}.ckpt"), map_location="cpu",
                       weights_only=True)
    for x, y in zip(action_cpu._params(full), action_cpu._params(again)):
        assert torch.equal(x, y)
    for k in ("sr_optim", "tempo_optim", "spatial_optim"):
        assert full[k]["state"].keys() == again[k]["state"].keys()
        for i, st in full[k]["state"].items():
            for name, v in st.items():
                assert torch.equal(torch.as_tensor(v), torch.as_tensor(again[k]["state"][i][name])), (k, i, name)
        assert float(full[k]["param_groups"][0]["lr"]) == float(again[k]["param_groups"][0]["lr"]) > 0


def test_fluid_trainer_with_graph_resumes_bit_exactly(tmp_path, capsys):
    """14 iterations (the n_iter <= 10 regime takes the eager step, the others try the replay), resumed from iteration 9:
    parameters and Adam moments equal bit for bit; every log line is finite and counts its replays."""
    fluid_cpu.check_trainer(tmp_path, "cuda", 14, 9, extra=["--graph"])
    lines = _log_lines(capsys)
    assert [l["n_iter"] for l in lines][:14] == list(range(1, 15))
    assert all(np.isfinite(v) for l in lines for v in l.values())
    assert all(l["replayed"] in (0, 1) for l in lines) and all(l["replayed"] == 0 for l in lines if l["n_iter"] <= 10)


@pytest.fixture(scope="module")
def scheduled_twins():
    """Two action steppers whose optimisers carry StepLR(2, 0.5), three iterations each from identical state with identical
    draws: one replays, its twin launches the same body kernel by kernel -> (per iteration: losses a, losses b, state
    tensors that differ), the learning-rate tensors after the third, their addresses before and after."""
    from tpgan_amd.gan_step_graph import GraphedActionStep
    from tpgan_amd.set_abstraction import ActionSpatialDis, ActionTempoDis
    from tpgan_amd.srnet import NoMaskSRNet
    from tpgan_amd.synthetic import action_clip
    from test_graph_padded_gpu import _differing, _same_draws, _state
    dev = torch.device("cuda", 0)
    torch.manual_seed(5)
    A = (NoMaskSRNet(3, 128, upsample_ratio=16).to(dev), ActionSpatialDis().to(dev), ActionTempoDis(3).to(dev))
    for m in list(A[1].modules()) + list(A[2].modules()):
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    Bm = copy.deepcopy(A)
    base = (3e-4, 1e-4, 1e-4)

    def optims(G, Ds, Dt):
        return tuple(torch.optim.Adam(m.parameters(), lr=torch.tensor(lr, device=dev), capturable=True)
                     for m, lr in zip((G, Dt, Ds), base))
    oa, ob = optims(*A), optims(*Bm)
    scheds = [torch.optim.lr_scheduler.StepLR(o, 2, gamma=0.5) for o in oa + ob]
    where = [o.param_groups[0]["lr"].data_ptr() for o in oa]
    opt = Namespace(R=2.0, w=2.0)
    low, high = action_clip(4, 2048, 16, 3, seed=1, device=dev)
    sa = GraphedActionStep(A[0], A[1], A[2], oa, opt, low, high, 1.0, None, None)
    sb = GraphedActionStep(Bm[0], Bm[1], Bm[2], ob, opt, low, high, 1.0, None, None)
    rows = []
    for it in (1, 2, 3):
        _same_draws(30 + it)
        la = sa(low, high, it)
        _same_draws(30 + it)
        lb = sb(low, high, it, launch_eagerly=True)
        for s in scheds:
            s.step()
        diff = _differing(_state(A, oa), _state(Bm, ob))
        print(f"iteration {it}: replay {la}\niteration {it}: eager  {lb}\niteration {it}: {len(diff)} state tensors differ",
              diff[:4], "lr", [float(o.param_groups[0]["lr"]) for o in oa])
        rows.append((it, la, lb, diff))
        with torch.no_grad():
            theirs = _state(Bm, ob)
            for k, v in _state(A, oa).items():
                theirs[k].copy_(v)
    assert sa.replays == 3
    return rows, [[o.param_groups[0]["lr"] for o in os_] for os_ in (oa, ob)], base, where


def test_learning_rate_tensor_halves_in_place_after_three_replays(scheduled_twins):
    _, lrs, base, where = scheduled_twins
    for group in lrs:
        for lr, lr0 in zip(group, base):
            assert torch.is_tensor(lr) and lr.is_cuda and float(lr) == float(np.float32(lr0) * np.float32(0.5))
    assert [lr.data_ptr() for lr in lrs[0]] == where


def test_replayed_adam_follows_the_schedule_discriminators(scheduled_twins):
    """Losses and both discriminators' parameters, buffers and Adam moments equal the eager twin's, bit for bit --
    iteration 3 included, whose update takes the halved rate."""
    for it, la, lb, diff in scheduled_twins[0]:
        assert la == lb, (it, la, lb)
        assert not [d for d in diff if not d[0].startswith(("G.", "og."))], (it, diff[:4])


def test_replayed_adam_follows_the_schedule_generator(scheduled_twins):
    for it, la, lb, diff in scheduled_twins[0]:
        assert not [d for d in diff if d[0].startswith(("G.", "og."))], (it, diff[:4])
