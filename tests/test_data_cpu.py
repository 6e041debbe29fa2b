"""Training from sequences on disk, on the host: the sampler's rule against the reference's own dataset class
(tests/golden/dataset.npz; capture_dataset_goldens.py), the index map, the collate rule, determinism, the prefetcher
and the trainer's checkpoint / resume -- through the torch compositions in ops on the oracle backend (CPU tensors).

The fixture stores, per case, frame 0's positions and the velocity field; frame s is pos0 + float32(s * 0.025) * vel in
float32 numpy, written to a temporary directory as the .npz files the loader reads (`write_dataset`).  Per kept item
it stores the reference's seed particle, `patch_idx`, `fps_idx` and float32 centroid; the reference's 12 arrays are the
gathers of the frames by those lists (positions minus that centroid), which the capture script checked array by array.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "dataset.npz")


def golden_frame(g, case, s):
    return g[f"case{case}/pos0"] + np.float32(s * float(g["spacing"])) * g[f"case{case}/vel"]


def write_dataset(root, g=None, cases=(1, 2), drop_last_particle_of=None):
    g = g if g is not None else np.load(GOLDEN)
    for c in cases:
        os.makedirs(os.path.join(root, f"case{c}"), exist_ok=True)
        for s in range(int(g["case_steps"])):
            pos, vel = golden_frame(g, c, s), g[f"case{c}/vel"]
            if drop_last_particle_of == (c, s):
                pos, vel = pos[:-1], vel[:-1]
            np.savez(os.path.join(root, f"case{c}", f"data_{s}.npz"), pos=pos, vel=vel)
    return g


def reference_outputs(g, idx):
    """The 12 arrays SiamData.__getitem__(idx) returned (jitter 0), rebuilt from the stored lists and centroid."""
    steps = int(g["case_steps"])
    case, step = idx // steps + 1, idx % (steps - 2)
    frames = [golden_frame(g, case, step + t) for t in range(3)]
    vel = g[f"case{case}/vel"]
    patch, fps, m = g[f"item{idx}/patch_idx"], g[f"item{idx}/fps_idx"], g[f"item{idx}/centroid_ref"]
    high = [f[patch] - m for f in frames]
    return high + [vel[patch]] * 3 + [h[fps] for h in high] + [vel[fps]] * 3, max(np.abs(f).max() for f in frames)


def check_golden_items(device, tmp_path):
    """Item 1 of the issue, on `device`'s backend: the patch SET equals the reference's; with the reference's patch order
    and first FPS pick fed in, the FPS picks and the velocities are equal and the centred positions agree within
    16 * 2^-24 * max|pos| (the only difference is the centroid: float64-accumulated here, a float32 sum there)."""
    from tpgan_amd.data import ClipSampler, FluidSequences
    g = write_dataset(str(tmp_path))
    seq = FluidSequences(str(tmp_path), 2, int(g["case_steps"]), device=device)
    sampler = ClipSampler(seq, 1, int(g["sample_num"]), jitter=0.0)
    assert len(g["items"]) >= 3
    for idx in (int(i) for i in g["items"]):
        assert float(g[f"item{idx}/gap"]) >= 1e-6
        sampler.sample(indices=[idx], seed_idx=[int(g[f"item{idx}/seed"])], initial_idx=[0])
        got = sampler.last["patch_idx"][0].cpu().numpy()
        assert got[0] == int(g[f"item{idx}/seed"])
        assert np.array_equal(np.sort(got), np.sort(g[f"item{idx}/patch_idx"])), f"item {idx}: patch set"
        ref_patch = torch.from_numpy(g[f"item{idx}/patch_idx"]).to(device).view(1, -1)
        out = sampler.sample(indices=[idx], seed_idx=[int(g[f"item{idx}/seed"])],
                             initial_idx=[int(g[f"item{idx}/fps_idx"][0])], patch_idx=ref_patch)
        assert np.array_equal(sampler.last["fps_idx"][0].cpu().numpy(), g[f"item{idx}/fps_idx"]), f"item {idx}: FPS picks"
        want, scale = reference_outputs(g, idx)
        bound = 16 * 2.0 ** -24 * scale
        assert float(out[12][0]) == float(g[f"item{idx}/h"]) == 1.0
        for j, (a, b) in enumerate(zip(out[:12], want)):
            a = a[0].cpu().numpy()
            assert a.dtype == np.float32 and a.shape == b.shape
            if 3 <= j < 6 or j >= 9:
                assert np.array_equal(a, b), f"item {idx}: velocity array {j}"
            else:
                err = float(np.abs(a - b).max())
                print(f"item {idx} array {j}: max |difference| {err:.3e} (bound {bound:.3e})")
                assert err <= bound, f"item {idx}: position array {j} off by {err} > {bound}"
                assert np.abs(b).max() > 1000 * bound          # the bound is not vacuous: the patch is ~0.25 wide


def test_selection_and_outputs_match_the_reference_dataset(oracle_cpu, tmp_path):
    check_golden_items(torch.device("cpu"), tmp_path)


def test_index_map_is_the_reference_s(oracle_cpu, tmp_path):
    from tpgan_amd.data import FluidSequences
    g = write_dataset(str(tmp_path))
    seq = FluidSequences(str(tmp_path), 2, int(g["case_steps"]), device="cpu")
    assert len(seq) == int(g["len"]) == 6
    assert [list(seq.keys(i)) for i in range(len(seq))] == g["keys"].tolist()
    assert seq.keys(3)[0] == "case1/data_0.npz" and seq.keys(5)[0] == "case2/data_2.npz"      # the // and % quirk
    with pytest.raises(IndexError):
        seq.clip(len(seq))
    for c in (1, 2):                                   # centroids: float64 mean, one rounding
        for s in range(int(g["case_steps"])):
            want = golden_frame(g, c, s).astype(np.float64).mean(0).astype(np.float32)
            assert np.array_equal(seq.centroids[(c - 1) * int(g["case_steps"]) + s].numpy(), want)


def test_unequal_particle_counts_in_a_case_raise(tmp_path):
    from tpgan_amd.data import FluidSequences
    write_dataset(str(tmp_path), drop_last_particle_of=(2, 3))
    with pytest.raises(ValueError, match=r"case2[/\\]data_3\.npz"):
        FluidSequences(str(tmp_path), 2, 5, device="cpu")


def _small_case(root, case, n, steps=5, seed=0):
    rng = np.random.RandomState(seed + n)
    os.makedirs(os.path.join(root, f"case{case}"), exist_ok=True)
    pos = rng.uniform(0.0, 0.5, (n, 3)).astype(np.float32) + np.float32(1.0)
    vel = rng.normal(0.0, 0.1, (n, 3)).astype(np.float32)
    for s in range(steps):
        np.savez(os.path.join(root, f"case{case}", f"data_{s}.npz"), pos=pos + np.float32(0.01 * s) * vel, vel=vel)


def test_scene_smaller_than_the_smallest_patch_raises(oracle_cpu, tmp_path):
    from tpgan_amd.data import ClipSampler, FluidSequences
    _small_case(str(tmp_path), 1, 3000)
    seq = FluidSequences(str(tmp_path), 1, 5, device="cpu")
    with pytest.raises(ValueError, match="3000 particles cannot give a patch of 4096"):
        ClipSampler(seq, 2, 9216).sample()


def test_mixed_patch_sizes_follow_the_collate_rule(oracle_cpu, tmp_path):
    """my_collate: the clips of size sample_num; if at most one is left, the clips of size 4096."""
    from tpgan_amd.data import ClipSampler, FluidSequences
    _small_case(str(tmp_path), 1, 5200)                # > 5000: patch 5000
    _small_case(str(tmp_path), 2, 4300)                # <= 5000: patch 4096
    seq = FluidSequences(str(tmp_path), 2, 5, device="cpu")
    sampler = ClipSampler(seq, 3, 5000, jitter=0.0)
    big, small = 0, 5                                  # clip 0 is case 1, clip 5 is case 2 (5 // 5)
    out = sampler.sample(indices=[big, small, big])
    assert out[1].shape == (2, 5000, 3) and out[7].shape == (2, 625, 3) and sampler.last["indices"] == [big, big]
    out = sampler.sample(indices=[big, small, small])
    assert out[1].shape == (2, 4096, 3) and out[7].shape == (2, 512, 3) and sampler.last["indices"] == [small, small]
    out = sampler.sample(indices=[small, small, small])
    assert out[1].shape == (3, 4096, 3) and out[12].shape == (3,)


def _batches(sampler, n):
    return [sampler.sample() for _ in range(n)]


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_same_seed_same_batches_and_prefetch_equals_plain(oracle_cpu, tmp_path):
    """Determinism from the one generator, and the prefetcher against the plain loop.  No device here: `prefetch` runs its
    stream-less form on CPU tensors (batches produced one ahead, same generator order); the stream hand-off itself is
    tested on the GPU (tests/test_data_gpu.py)."""
    from tpgan_amd.data import ClipSampler, FluidSequences, prefetch
    g = write_dataset(str(tmp_path))
    seq = FluidSequences(str(tmp_path), 2, int(g["case_steps"]), device="cpu")

    def make(seed):
        return ClipSampler(seq, 2, 4096, jitter=0.003, generator=torch.Generator().manual_seed(seed))
    a, b, c = _batches(make(5), 3), _batches(make(5), 3), _batches(make(6), 3)
    assert all(_equal(x, y) for x, y in zip(a, b))
    assert not any(_equal(x, y) for x, y in zip(a, c))
    assert not torch.equal(a[0][7], a[0][1][:, :512])                          # jitter applied
    it = prefetch(make(5))
    states = []
    for want in a:
        states.append(it.resume_state)
        assert _equal(next(it), want)
    again = make(1)
    again.generator.set_state(states[2])                                        # what a checkpoint after batch 2 holds
    assert _equal(again.sample(), a[2])
    # low = high rows + noise * jitter; left / right frames use the centre frame's lists
    s = make(9)
    out = s.sample()
    fps = s.last["fps_idx"].long()
    for f in range(3):
        rows = torch.gather(out[f], 1, fps.unsqueeze(-1).expand(-1, -1, 3))
        assert float((out[6 + f] - rows).abs().max()) < 6 * 0.003 and not torch.equal(out[6 + f], rows)


def _params(ckpt):
    return [ckpt[k][n] for k in ("sr_net", "tempo_dis", "spatial_dis") for n in sorted(ckpt[k])]


def check_trainer(tmp_path, device, iters, resume_at, extra=()):
    """Train `iters` iterations with a checkpoint after every one; resume from iteration `resume_at` in a second log
    directory and run to `iters`: the eleven keys, weights_only loading, rollout.load_generator, and parameters and Adam
    moments equal bit for bit."""
    from tpgan_amd import rollout, train
    data = os.path.join(str(tmp_path), "data")
    write_dataset(data)
    common = ["--train_dataset_path", data, "--train_sequence_num", "2", "--sequence_length", "5", "--batch_size", "2",
              "--sample_num", "512", "--amp", "none", "--device", device, "--ckpt_every", "1", "--log_every", "1",
              "--iters", str(iters), "--seed", "1", *extra]
    a, b = os.path.join(str(tmp_path), "a"), os.path.join(str(tmp_path), "b")
    assert train.main(common + ["--log_dir", a]) == 0
    ck = os.path.join(a, "model_ckpt")
    assert open(os.path.join(ck, "latest_checkpoint.txt")).readline().strip() == f"tpugan_checkpoint{iters}.ckpt"
    full = torch.load(os.path.join(ck, f"tpugan_checkpoint{iters}.ckpt"), map_location="cpu", weights_only=True)
    assert set(full) == set(train.CKPT_KEYS) and len(train.CKPT_KEYS) == 11 and full["n_iter"] == iters
    net = rollout.load_generator(os.path.join(ck, f"tpugan_checkpoint{iters}.ckpt"), 3, torch.device("cpu"))
    assert all(torch.equal(p.cpu(), full["sr_net"][n]) for n, p in net.state_dict().items())
    first = torch.load(os.path.join(ck, "tpugan_checkpoint1.ckpt"), map_location="cpu", weights_only=True)
    assert any(not torch.equal(x, y) for x, y in zip(_params(first), _params(full))), "parameters did not move"
    assert train.main(common + ["--log_dir", b, "--resume", "--path_to_resume",
                                os.path.join(ck, f"tpugan_checkpoint{resume_at}.ckpt")]) == 0
    again = torch.load(os.path.join(b, "model_ckpt", f"tpugan_checkpoint{iters}.ckpt"), map_location="cpu",
                       weights_only=True)
    for x, y in zip(_params(full), _params(again)):
        assert torch.equal(x, y)
    for k in ("sr_optim", "tempo_optim", "spatial_optim"):
        assert full[k]["state"].keys() == again[k]["state"].keys()
        for i, st in full[k]["state"].items():
            for name, v in st.items():
                assert torch.equal(torch.as_tensor(v), torch.as_tensor(again[k]["state"][i][name])), (k, i, name)
    return full


def test_trainer_checkpoint_and_resume_on_the_host(oracle_cpu, tmp_path, capsys):
    """3 iterations of the eager step on CPU tensors (patches of 512 points of the golden's scenes, batch 2)."""
    check_trainer(tmp_path, "cpu", 3, 2)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    import json
    assert [json.loads(l)["n_iter"] for l in lines] == [1, 2, 3, 3]
    assert all(np.isfinite(v) for l in lines for v in json.loads(l).values())


def test_host_tables_and_argument_checks(oracle_cpu):
    import tpgan_amd.ops as ops
    pts = torch.rand(100, 3)
    with pytest.raises(RuntimeError, match="exceeds"):
        ops.patch_select(pts, [0], [50], [0], 51)
    with pytest.raises(RuntimeError, match="seed"):
        ops.patch_select(pts, [0], [50], [50], 10)
    with pytest.raises(RuntimeError, match="slice"):
        ops.patch_select(pts, [60], [50], [0], 10)
    with pytest.raises(RuntimeError, match="float tensor"):
        ops.patch_select(pts.double(), [0], [50], [0], 10)
    idx = ops.patch_select(pts, torch.tensor([0, 50], dtype=torch.int32), np.array([50, 50]), [3, 4], 10)
    assert idx.dtype == torch.int32 and idx.shape == (2, 10) and idx[0, 0] == 3 and idx[1, 0] == 4


def test_new_entries_reject_bad_arguments_before_any_launch(hip_lib):
    """The C-ABI's own checks (no GPU here): per-scene conditions on the host tables are TPG_ERR_ARG with nothing
    launched, K above the LDS sort's capacity TPG_ERR_UNSUPPORTED, empty work TPG_OK."""
    import ctypes as C
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)

    def ints(*v):
        return C.cast((C.c_int32 * len(v))(*v), C.c_void_p)

    def select(first=0, count=5000, seed=0, K=4096, P=5000, ws=p, B=1):
        return hip_lib.tpg_patch_select_f32(p, P, ints(first), ints(count), ints(seed), B, K, p, ws, None)
    assert select(K=5001) == -1 and select(K=0) == -1 and select(K=-3) == -1
    assert select(seed=5000) == -1 and select(seed=-1) == -1
    assert select(first=1) == -1 and select(first=-1) == -1 and select(count=0) == -1
    assert select(ws=None) == -1 and select(ws=C.c_void_p(p.value + 4)) == -1
    assert select(K=16385, count=20000, P=20000) == -3 and hip_lib.tpg_patch_select_max_k() == 16384
    assert select(B=0) == 0
    assert hip_lib.tpg_patch_select_workspace_bytes(8, 80000, 9216) > 8 * 9216 * 8
    assert hip_lib.tpg_patch_select_workspace_bytes(0, 80000, 9216) == 0

    def high(first=(0, 100, 200), count=100, crow=0, T=3, P=300, F=1, vel=p, hv=p):
        return hip_lib.tpg_clip_gather_high_f32(p, vel, P, ints(*first), ints(count), p, F, ints(crow), p, T, 1, 16, p, hv,
                                                None)
    assert high(first=(0, 100, 201)) == -1 and high(crow=1) == -1 and high(hv=None) == -1 and high(count=0) == -1
    assert high(T=9, first=(0,) * 9) == -3 and high(T=0) == 0

    def low(vel=p, lv=p, first=(0, 100, 200), count=100, T=3, P=300, K=16):
        return hip_lib.tpg_clip_gather_low_f32(p, p, None, 0.003, vel, P, ints(*first), ints(count), T, 1, K, 2, p, lv, None)
    assert low(lv=None) == -1 and low(first=(0, 100, 201)) == -1 and low(K=0) == -1 and low(T=0) == 0
