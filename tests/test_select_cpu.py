"""The cases of tests/select_cases.py have the properties they are named for (which bins of the radix select the K-th
key falls in, how many keys lie below it, where its ties sit, which rows are taken and which left out) -- or the GPU
tests built on them (tests/test_select_gpu.py) check nothing new -- and `ops.patch_select` on CPU tensors (the torch
composition behind backends without the kernel) equals the numpy rule on every one of them."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import select_cases as cases  # noqa: E402
from select_rule import CHUNK, NAN_KEY, keys, patch_keys, patch_rule, patch_trace, subset  # noqa: E402

INF_KEY = 0x7F800000


@pytest.fixture(scope="module")
def patch_cases():
    return cases.patch_cases(capacity=[(16385, cases.MAX_K)])


def chunks(n):
    return -(-n // CHUNK)


# ---- the trace itself -----------------------------------------------------------------------------------------------------
def test_trace_on_a_cloud_worked_by_hand():
    """Seed at the origin, every other point on the x axis: d2 = x^2, exact.  Keys 0, 2^-2 (twice), 1, 4 (twice)."""
    pts = np.zeros((6, 3), np.float32)
    pts[:, 0] = (0.0, 2.0, 0.5, 1.0, -0.5, -2.0)
    assert patch_keys(pts, 0).tolist() == [0, 0x40800000, 0x3E800000, 0x3F800000, 0x3E800000, 0x40800000]
    t = patch_trace(pts, 0, 5)
    assert t == {"kth": 0x40800000, "digits": (0x204, 0, 0), "below": 4, "krem": 1, "equal": 2, "ties": [2]}
    assert patch_rule(pts, 0, 5).tolist() == [0, 2, 4, 3, 1]
    t = patch_trace(pts, 0, 2)
    assert (t["kth"], t["below"], t["krem"], t["equal"]) == (0x3E800000, 1, 1, 2)
    one = np.float32(1.0).view(np.uint32)
    assert (int(one) >> 21, (int(one) >> 10) & 2047, int(one) & 1023) == (0x1FC, 0, 0)


# ---- launch groups --------------------------------------------------------------------------------------------------------
def test_group_cases_put_the_widest_scene_where_they_say():
    scenes, seeds, K = cases.groups_33()
    n = [len(s) for s in scenes]
    assert len(n) == 33 and K == 7 and min(n) == K
    assert max(chunks(c) for c in n[:32]) == 1 and 1024 in n[:32] and chunks(n[32]) == 3
    scenes, seeds, K = cases.groups_65()
    n = [len(s) for s in scenes]
    assert len(n) == 65 and K == 7 and min(n) == K
    assert max(chunks(c) for c in n[:32]) == 3 and chunks(n[64]) == 1 and len({chunks(c) for c in n}) == 3
    for make in cases.GROUPS.values():
        scenes, seeds, K = make()
        assert all(0 <= s < len(p) and len(p) >= K for p, s in zip(scenes, seeds))
        assert len({int(patch_rule(p, s, K)[-1]) for p, s in zip(scenes, seeds)}) > 8     # the scenes' answers differ


# ---- small and capacity -----------------------------------------------------------------------------------------------------
def test_small_and_capacity_cases_sit_on_the_sort_s_sizes(patch_cases):
    assert {(1, 1), (2, 2), (1024, 1024), (1025, 1025)} <= set(cases.SMALL)               # K = N: everything is taken
    assert {K for _, K in cases.SMALL} >= {1, 1023, 1024, 1025}                           # around the 1024 sort threads
    assert [K for _, K in cases.CAPACITY] == [cases.MAX_K] * 3 and [N for N, _ in cases.CAPACITY] == [16384, 16385, 40000]
    for N, K in cases.SMALL + [(16385, cases.MAX_K)]:
        (pts,), (seed,), k = patch_cases[f"small_{N}_{K}" if K < cases.MAX_K else f"capacity_{N}"]
        assert pts.shape == (N, 3) and k == K and 0 <= seed < N
        t = patch_trace(pts, seed, K)
        assert t["below"] + t["krem"] == K and len(t["ties"]) == chunks(N)


# ---- digits -------------------------------------------------------------------------------------------------------------
def test_all_identical_is_bin_zero_of_every_pass(patch_cases):
    (pts,), (seed,), K = patch_cases["all_identical"]
    t = patch_trace(pts, seed, K)
    assert (len(pts), K) == (3 * 1024 + 5, 2049)
    assert t["kth"] == 0 and t["digits"] == (0, 0, 0) and t["below"] == 0 and t["krem"] == K
    assert t["equal"] == len(pts) and t["ties"] == [1024, 1024, 1024, 5]
    assert np.array_equal(patch_rule(pts, seed, K), np.arange(K))


def test_digit_cases_hit_their_bins(patch_cases):
    found = {name: patch_trace(*[a[0] for a in patch_cases[name][:2]], patch_cases[name][2]) for name in cases.DIGIT_WANTED}
    assert found["pass2_last_bin"]["digits"][2] == 1023
    assert found["pass1_last_bin"]["digits"][1] == 2047
    assert found["low_digits_zero"]["digits"][1:] == (0, 0) and found["low_digits_zero"]["kth"] == 0x3D800000
    for name, t in found.items():
        (pts,), _, K = patch_cases[name]
        assert len(pts) == 3000 and t["kth"] != 0 and 0 < t["below"] == K - 1 and t["krem"] == 1, name
    assert patch_rule(*[a[0] for a in patch_cases["low_digits_zero"][:2]], patch_cases["low_digits_zero"][2])[-1] == 1


def test_denormal_case_is_pass_zero_bin_zero_with_lower_digits(patch_cases):
    (pts,), (seed,), K = patch_cases["denormal"]
    key = patch_keys(pts, seed)
    t = patch_trace(pts, seed, K)
    assert t["digits"][0] == 0 and t["kth"] != 0 and t["digits"][1:] != (0, 0)
    near = patch_rule(pts, seed, 2 * K)
    tiny = np.float32(np.finfo(np.float32).tiny).view(np.uint32)
    assert (key[near] < tiny).all() and (key[near] != 0).sum() >= 2 * K - 8               # denormal, all but a few zeros
    assert len(np.unique(key[near])) > K // 2                                             # many distinct denormals
    # what flushing to zero would give: the zeros in index order -- another answer than the rule's
    flushed = np.lexsort((np.arange(len(key)), np.where(key < tiny, 0, key)))[:K]
    assert np.array_equal(flushed, np.arange(K)) and not np.array_equal(flushed, patch_rule(pts, seed, K))


def test_non_finite_cases_take_one_tie_and_leave_one_out(patch_cases):
    for name, kth, taken, left in (("kth_is_inf", INF_KEY, 7, 300), ("kth_is_nan", NAN_KEY, 100, 4000)):
        (pts,), (seed,), K = patch_cases[name]
        t = patch_trace(pts, seed, K)
        assert t["kth"] == kth and t["krem"] == 1 and t["equal"] == 2 and t["below"] == K - 1, name
        assert sorted(i for i, c in enumerate(t["ties"]) if c) == sorted({taken // CHUNK, left // CHUNK})
        want = patch_rule(pts, seed, K)
        assert want[-1] == taken and left not in want, name
    key = patch_keys(*[a[0] for a in patch_cases["kth_is_nan"][:2]])
    assert (key[[7, 300]] == INF_KEY).all() and (key[[100, 4000]] == NAN_KEY).all()
    assert (key < INF_KEY).sum() == 4996


# ---- the torch composition ------------------------------------------------------------------------------------------------
def test_the_torch_composition_equals_the_rule_on_every_case(oracle_cpu, patch_cases):
    """ops.patch_select on CPU tensors: no backend for them has the kernel, so this is ops._patch_select_torch."""
    import tpgan_amd.ops as ops
    assert not hasattr(ops.backend_for(torch.zeros(1)), "patch_select")
    assert len(patch_cases) == 2 + len(cases.SMALL) + 1 + 1 + 3 + 3
    for name, (scenes, seeds, K) in patch_cases.items():
        count = [len(s) for s in scenes]
        first = np.concatenate([[0], np.cumsum(count)[:-1]])
        got = ops.patch_select(torch.from_numpy(np.concatenate(scenes)), first, count, seeds, K)
        assert got.dtype == torch.int32 and tuple(got.shape) == (len(scenes), K), name
        for b, (pts, seed) in enumerate(zip(scenes, seeds)):
            assert np.array_equal(got[b].numpy(), patch_rule(pts, seed, K)), (name, b)


# ---- frame subset -------------------------------------------------------------------------------------------------------
def check_subset(n, K, seed):
    """A repetition of 0..n-1 plus a residue of distinct picks, or K distinct picks: the smallest keys, ascending."""
    got = subset(n, K, seed)
    assert got.shape == (K,) and got.dtype == np.int32 and got.min() >= 0 and got.max() < n
    lead, picks = (0, K) if n > K else (K // n * n, K % n)
    assert picks == cases.selected(n, K)
    assert np.array_equal(got[:lead], np.tile(np.arange(n), K // n) if lead else got[:0])
    tail = got[lead:]
    assert len(tail) == picks and len(np.unique(tail)) == picks
    key = keys(n, seed)
    assert (np.diff(key[tail].astype(np.int64)) > 0).all()
    assert picks == 0 or (np.delete(key, tail) > key[tail].max()).all()
    return got


def test_subset_cases_are_prefixes_or_repetitions_with_distinct_picks():
    assert [(n, K, cases.selected(n, K)) for n, K in cases.SUBSET if K < 10] == \
        [(1, 1, 0), (2, 1, 1), (5, 1, 1), (2, 3, 1), (3, 2, 2), (4, 3, 3)]
    assert [(n, cases.selected(n, K)) for n, K in cases.SUBSET if K == cases.MAX_K] == \
        [(3, 1), (16384, 0), (16385, 16384), (50000, 16384)]
    for n, K in cases.SUBSET:
        got = check_subset(n, K, cases.subset_seed(n, K))
        if n == K:
            assert np.array_equal(got, np.arange(n))
        if n == K + 1:
            assert np.array_equal(np.setdiff1d(np.arange(n), got), [np.argmax(keys(n, cases.subset_seed(n, K)))])


def test_subset_batch_sorts_another_size_in_every_launch():
    count, seeds, K = cases.subset_batch()
    assert len(count) == 65 and len(seeds) == 65 and len(set(seeds.tolist())) == 65
    most = [max(cases.selected(int(n), K) for n in count[g:g + cases.GROUP]) for g in range(0, 65, cases.GROUP)]
    assert most == [16, 31, 64] and cases.selected(int(count[64]), K) == 64
    assert cases.selected(int(count[0]), K) == 0 and count[5] == K                       # nothing to select next to work
    for f in range(65):
        check_subset(int(count[f]), K, seeds[f])
