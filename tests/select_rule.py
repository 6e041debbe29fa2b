"""The two samplers' selection rules in numpy, importable without a GPU (tests/test_select_cpu.py,
tests/test_select_gpu.py, tests/test_data_gpu.py): `patch_rule` is include/tpgan_ops.h's statement of
tpg_patch_select_f32, `patch_trace` describes an input in the terms of that statement's radix select (which digits the
K-th key has, how many keys lie below it, where its ties sit), and `subset` / `keys` are tpg_frame_subset's rule, stated
once in tests/test_action_data_cpu.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_action_data_cpu import keys, subset  # noqa: E402,F401

NAN_KEY = 0x7FC00000
CHUNK = 1024                            # candidates per workgroup of the select (csrc/clip_sample.hip, SEL_CHUNK)


def patch_rule(points, seed, K):
    """The selection rule in numpy: fp32 d2 = (dx*dx + dy*dy) + dz*dz, each operation rounded; the K smallest in
    ascending (d2, index); a NaN d2 ranks as the bit pattern 0x7FC00000 (after +inf)."""
    with np.errstate(all="ignore"):
        d = points - points[seed]
        d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)
    index = np.arange(len(d2))
    if np.isfinite(d2).all():
        return np.lexsort((index, d2))[:K].astype(np.int32)
    key = np.where(np.isnan(d2), np.uint32(NAN_KEY), d2.view(np.uint32))
    return np.lexsort((index, key))[:K].astype(np.int32)


def patch_keys(points, seed):
    """The 32-bit selection key of every candidate: the bits of the rule's fp32 d2 (a sum of squares: never negative,
    so it orders like its bit pattern), 0x7FC00000 for a NaN."""
    assert points.dtype == np.float32
    with np.errstate(all="ignore"):
        d = points - points[seed]
        d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)
    return np.where(np.isnan(d2), np.uint32(NAN_KEY), d2.view(np.uint32)).astype(np.uint32)


def patch_trace(points, seed, K):
    """Where the K-th smallest key of (points, seed) lies, from the rule's own d2 bits:
      kth            the K-th smallest key;
      digits         its three radix digits (bits 31..21, 20..10, 9..0);
      below, krem    the keys strictly under it, and K - below: the ties that are taken (by ascending index);
      equal          the keys equal to it (equal - krem ties are left out);
      ties           the keys equal to it in each chunk of 1024 consecutive candidates."""
    key = patch_keys(points, seed)
    assert 1 <= K <= len(key)
    kth = int(np.sort(key)[K - 1])
    below, equal = int((key < kth).sum()), int((key == kth).sum())
    chunks = -(-len(key) // CHUNK)
    ties = np.bincount(np.flatnonzero(key == kth) // CHUNK, minlength=chunks)
    assert below < K <= below + equal
    return {"kth": kth, "digits": (kth >> 21, (kth >> 10) & 2047, kth & 1023), "below": below, "krem": K - below,
            "equal": equal, "ties": ties.tolist()}
