"""tpg_replace_dummy_centres on the GPU: the kernel against the torch statement of its rule (ops._replace_dummy_centres_torch,
itself held to a numpy restatement in tests/test_dummy_centres_cpu.py), bit for bit, and the set-abstraction levels'
device rule (set_abstraction.device_dummy_draws) inside the discriminators' index plans."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dummy_centres_cpu import cloud, small_cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def fps_case(B, N, S, dummies, seed):
    """Clouds whose listed rows are 999-padding, with the centres FPS itself picks: the dummies coincide, so FPS takes one
    of them early and no other while a point at a positive distance is left."""
    import tpgan_amd.ops as ops
    xyz = torch.from_numpy(cloud(B, N, dummies, seed)).cuda()
    return xyz, ops.furthest_point_sample(xyz, S)


def shuffled_case(B, N, S, dummies, seed):
    """The same clouds with S distinct centres in a random order: every dummy among them is a hit."""
    rs = np.random.RandomState(seed)
    centres = np.stack([rs.permutation(N)[:S] for _ in range(B)]).astype(np.int32)
    return torch.from_numpy(cloud(B, N, dummies, seed)).cuda(), torch.from_numpy(centres).cuda()


def big_cases():
    rs = np.random.RandomState(11)
    return {
        # 28..70 dummies per cloud, every one a hit, N = S = one slot per thread
        "3x1024x1024": lambda: shuffled_case(3, 1024, 1024, [rs.permutation(1024)[:n] for n in (28, 70, 41)], 1),
        # N > S, FPS centres: one hit per cloud, the pool holds the other dummies
        "4x2048x1024": lambda: fps_case(4, 2048, 1024, [rs.permutation(2048)[:n] for n in (30, 64, 1, 50)], 2),
        # N not a multiple of the workgroup, five candidates per thread in the last round
        "2x4097x1024": lambda: fps_case(2, 4097, 1024, [rs.permutation(4097)[:n] for n in (100, 7)], 3),
        # S = 2048: two slots per thread in the compaction, hundreds of hits, a 1024-key sort
        "2x4096x2048": lambda: shuffled_case(2, 4096, 2048, [rs.permutation(4096)[:n] for n in (1500, 300)], 4),
    }


def both(xyz, centres, key, site, with_flag=True):
    import tpgan_amd.ops as ops
    B = xyz.shape[0]
    f1 = torch.ones(B, dtype=torch.int32, device=xyz.device) if with_flag else None
    f2 = None if f1 is None else f1.clone()
    got = ops.replace_dummy_centres(xyz, centres, key, site, f1)
    want = ops._replace_dummy_centres_torch(xyz, centres, key, site, f2)
    return got, want, f1, f2


@pytest.mark.parametrize("name", sorted(small_cases()))
def test_kernel_equals_the_torch_statement_small(dev, name):
    xyz, centres = small_cases()[name]
    xyz, centres = torch.from_numpy(xyz).to(dev), torch.from_numpy(centres).to(dev)
    for seed, n_iter, site in ((0, 12, 0), (7 + (3 << 32), 1 << 33, 5), (-2, 13, 1)):
        key = torch.tensor([seed, n_iter], dtype=torch.int64, device=dev)
        (out, short), (want, want_short), f1, f2 = both(xyz, centres, key, site)
        assert out.dtype == torch.int32 and out.shape == centres.shape and tuple(short.shape) == (1,)
        assert torch.equal(out, want) and torch.equal(short, want_short) and torch.equal(f1, f2), name
    assert int(short) == (1 if name in ("all_dummy_short", "more_centres_than_points") else 0)
    out, _ = both(xyz, centres, key, site, with_flag=False)[0]
    assert torch.equal(out, want)


@pytest.mark.parametrize("name", sorted(big_cases()))
def test_kernel_equals_the_torch_statement_large(dev, name):
    import tpgan_amd.ops as ops
    xyz, centres = big_cases()[name]()
    hits = (torch.gather(xyz[:, :, 0], 1, centres.long()) == 999.0).sum(1).tolist()
    print(name, "hits per cloud:", hits)
    assert min(hits) >= 1
    if name == "3x1024x1024":
        assert hits == [28, 70, 41]
    if name == "4x2048x1024":
        assert hits == [1, 1, 1, 1]
    key = torch.tensor([123456789012345, 77], dtype=torch.int64, device=dev)
    (out, short), (want, want_short), f1, f2 = both(xyz, centres, key, 3)
    assert torch.equal(out, want) and int(short) == 0 == int(want_short) and torch.equal(f1, f2) and not f1.any()
    # two runs, the same bits
    again, _ = ops.replace_dummy_centres(xyz, centres, key, 3)
    assert torch.equal(again, out)
    # a row depends on its own cloud and its index b in the call alone: other neighbours, another batch size
    other = torch.cat([xyz[:1].flip(1), xyz[1:2], xyz[:1]])
    other_c = torch.cat([centres[:1], centres[1:2], centres[:1]])
    moved, _ = ops.replace_dummy_centres(other.contiguous(), other_c.contiguous(), key, 3)
    assert torch.equal(moved[1], out[1])
    # another site, another iteration: other draws (the survivors stay)
    for k2, site in ((key, 4), (key + torch.tensor([0, 1], device=dev), 3)):
        diff, _ = ops.replace_dummy_centres(xyz, centres, k2, site)
        assert not torch.equal(diff, out)
        for b, k in enumerate(hits):
            assert torch.equal(diff[b, :centres.shape[1] - k], out[b, :centres.shape[1] - k])


def test_status_codes_without_a_launch(dev):
    import tpgan_amd.ops as ops
    hip = ops.backend_for(torch.zeros(1, device=dev))
    xyz, centres = fps_case(2, 64, 16, [[1], [2]], 0)
    key = torch.tensor([1, 2], dtype=torch.int64, device=dev)
    out = torch.full_like(centres, -7)
    short = torch.full((1,), -7, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(xyz_p=xyz.data_ptr(), cen_p=centres.data_ptr(), key_p=key.data_ptr(), site=0, B=2, N=64, S=16,
             out_p=out.data_ptr(), short_p=short.data_ptr()):
        ptr = [None if p is None else C.c_void_p(p) for p in (xyz_p, cen_p, key_p, out_p, short_p)]
        return hip.lib.tpg_replace_dummy_centres(ptr[0], ptr[1], ptr[2], site, B, N, S, ptr[3], None, ptr[4], stream)
    assert call(N=0) == -1 and call(site=-1) == -1 and call(B=-1) == -1
    assert call(xyz_p=None) == -1 and call(key_p=None) == -1 and call(short_p=None) == -1
    assert call(out_p=centres.data_ptr()) == -1
    big = hip.lib.tpg_patch_select_max_k() + 1
    assert call(N=big, S=big) == -3
    assert call(B=0) == 0 and call(S=0) == 0
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and int(short) == -7          # nothing was written
    with pytest.raises(RuntimeError, match="capacity"):
        ops.replace_dummy_centres(torch.zeros(1, big, 3, device=dev), torch.zeros(1, big, dtype=torch.int32, device=dev),
                                  key, 0)
    assert call() == 0
    torch.cuda.synchronize()
    assert int(short) == 0 and torch.equal(out, ops._replace_dummy_centres_torch(xyz, centres, key, 0)[0])


def padded_clouds(dev, B, N, seed):
    """Generator-like clouds of N points with 999-rows the way hard masking writes them (different counts per cloud)."""
    rs = np.random.RandomState(seed)
    return torch.from_numpy(cloud(B, N, [rs.permutation(N)[:n] for n in rs.randint(20, 80, size=B)], seed)).to(dev)


def check_first_two_levels(plan, xyz, key, site0, npoint2):
    """Level 1 = the torch statement applied to plain FPS; level 2 = plain FPS of the new centres: the prefix shortcut would
    answer 0..m-1, which is right only while the centres are in pick order (it may still be the answer: coinciding dummies
    decide no other pick, so the survivors of S = N centres are in the order FPS gives them without the dummies)."""
    import tpgan_amd.ops as ops
    c1 = plan["sa"][0][0]
    want, _ = ops._replace_dummy_centres_torch(xyz, ops.furthest_point_sample(xyz, c1.shape[1]), key, site0)
    assert torch.equal(c1, want)
    new_xyz = torch.gather(xyz, 1, c1.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
    c2 = plan["sa"][1][0]
    assert c2.shape[1] == npoint2 and torch.equal(c2, ops.furthest_point_sample(new_xyz, npoint2))
    return c1


@pytest.mark.parametrize("N", [1024, 2048])
def test_index_plans_under_device_dummy_draws(dev, N):
    from tpgan_amd.set_abstraction import FluidSpatialDis, FluidTempoDis, device_dummy_draws
    torch.manual_seed(0)
    Ds, Dt = FluidSpatialDis().to(dev), FluidTempoDis(3).to(dev)
    key = torch.tensor([5, 12], dtype=torch.int64, device=dev)
    xs = padded_clouds(dev, 4, N, 1)
    frames = [padded_clouds(dev, 2, N, 10 + t) for t in range(3)]
    with device_dummy_draws(key) as ctx:
        plan_s = Ds.index_plan(xs)
        assert ctx.next_site() == 1
        plan_t = Dt.index_plan(frames, 0.10)
        assert len(ctx.shorts) == 2 and not any(int(s) for s in ctx.shorts)
    check_first_two_levels(plan_s, xs, key, 0, 512)
    c1 = check_first_two_levels(plan_t, torch.cat(frames), key, 2, 256)
    x = torch.gather(torch.cat(frames)[:, :, 0], 1, c1.long())
    assert N > 1024 or bool((x == 999.0).sum() < (torch.cat(frames)[:, :, 0] == 999.0).sum())    # dummies were swapped out
    # entering the context again starts the ordinals at 0: the same plan, bit for bit
    with device_dummy_draws(key) as ctx:
        again = Ds.index_plan(xs)
    assert torch.equal(again["sa"][0][0], plan_s["sa"][0][0]) and torch.equal(again["sa"][1][0], plan_s["sa"][1][0])
    # outside the context the host rule is untouched: a hit-free cloud gives plain FPS and the prefix chain
    clean = torch.from_numpy(cloud(2, N, [[], []], 3)).to(dev)
    import tpgan_amd.ops as ops
    plain = Ds.index_plan(clean)
    assert torch.equal(plain["sa"][0][0], ops.furthest_point_sample(clean, 1024))
