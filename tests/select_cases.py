"""Named, seeded, small inputs for the two samplers' selections at their launch-group, digit and capacity edges
(tests/test_select_cpu.py asserts that every case has the property it is named for; tests/test_select_gpu.py runs the
kernels on them).

A patch-select case is (scenes, seeds, K): a ragged batch of (n,3) fp32 clouds, one seed row per scene, one K.
The select (csrc/clip_sample.hip) launches 32 scenes at a time, walks a scene in chunks of 1024 candidates, finds the
K-th key by 11 + 11 + 10-bit digits and sorts K keys with 1024 threads in at most 16384 slots of LDS: the sizes below sit
on those numbers."""
import numpy as np

from select_rule import patch_keys, patch_rule

CENTRE = np.asarray((1.0, 0.5, 2.0), np.float32)
MAX_K = 16384                           # include/tpgan_ops.h, TPG_PATCH_SELECT_MAX_K
GROUP = 32                              # scenes / clips / frames per launch


def ball(rng, n, centre=CENTRE):
    v = rng.normal(size=(n, 3))
    v *= (rng.uniform(size=(n, 1)) ** (1 / 3)) / np.linalg.norm(v, axis=1, keepdims=True)
    return (0.4 * v + np.asarray(centre)).astype(np.float32)


# ---- launch groups ------------------------------------------------------------------------------------------------------
def _ragged(rng, sizes):
    sizes = [int(n) for n in sizes]
    return [ball(rng, n, centre=rng.uniform(-2, 2, 3)) for n in sizes], [int(rng.integers(n)) for n in sizes]


def groups_33():
    """33 scenes, K = 7: the first launch group holds one-chunk scenes only (7 .. 1024 points; a scene cannot be smaller
    than K), the second group is ONE scene of 3000 points (3 chunks).  The workspace stride is that of 3 chunks, the first
    group's grid is 1 chunk wide, and scene 32 is slot 0 of its launch."""
    rng = np.random.default_rng(33)
    sizes = rng.integers(7, 1025, size=33)
    sizes[[0, 5, 31]] = (7, 1024, 8)
    sizes[32] = 3000
    scenes, seeds = _ragged(rng, sizes)
    return scenes, seeds, 7


def groups_65():
    """65 scenes, K = 7, the reverse: a first group with 3-chunk scenes (and one of 7 points), a ragged middle group, and
    a last group of a single one-chunk scene, whose grid (1 chunk) is narrower than the workspace stride (3 chunks)."""
    rng = np.random.default_rng(65)
    sizes = rng.integers(7, 3001, size=65)
    sizes[[0, 3, 31, 32, 63]] = (3000, 7, 2049, 1025, 2999)
    sizes[64] = 700
    scenes, seeds = _ragged(rng, sizes)
    return scenes, seeds, 7


GROUPS = {"groups_33": groups_33, "groups_65": groups_65}

# ---- small and capacity ---------------------------------------------------------------------------------------------------
SMALL = [(1, 1), (2, 1), (2, 2), (5, 3), (1024, 1024), (1025, 1), (1025, 1025), (3000, 1023), (3000, 1024), (3000, 1025)]
CAPACITY = [(16384, MAX_K), (16385, MAX_K), (40000, MAX_K)]


def single(N, K):
    """One ball of N points, a seed drawn from it."""
    rng = np.random.default_rng(1000 * N + K)
    pts = ball(rng, N)
    return [pts], [int(rng.integers(N))], K


# ---- digits -----------------------------------------------------------------------------------------------------------
def all_identical():
    """3 * 1024 + 5 copies of one point, K = 2049: every key is 0 (bin 0 of every pass), nothing lies below the K-th key,
    and all four chunks hold ties, of which the first 2049 by index are taken."""
    return [np.tile(CENTRE, (3 * 1024 + 5, 1))], [5], 2049


DIGIT_WANTED = {                                        # name -> what (pass-1 digit, pass-2 digit) of the K-th key must be
    "pass2_last_bin": lambda d1, d2: d2 == 1023,
    "pass1_last_bin": lambda d1, d2: d1 == 2047,
    "low_digits_zero": lambda d1, d2: (d1 == 0) & (d2 == 0),
}


def digit_last_bins():
    """name -> (scenes, seeds, K) on 3000-point balls around their seed point (row 0, the ball's centre).  Row 1 sits
    0.25 from the seed along x: d2 = 2^-4 exactly, a non-zero key whose two lower digits are 0.  The ranks K are found
    by search: the first key, in ascending order, whose digits are the wanted ones; the first generator seed whose cloud
    offers all three is kept."""
    for s in range(64):
        rng = np.random.default_rng(2047 + s)
        pts = ball(rng, 3000)
        pts[0] = CENTRE
        pts[1] = CENTRE + np.asarray((0.25, 0.0, 0.0), np.float32)
        key = patch_keys(pts, 0)
        order = patch_rule(pts, 0, len(pts))
        d1, d2 = (key[order] >> 10) & 2047, key[order] & 1023
        ranks = {}
        for name, wanted in DIGIT_WANTED.items():
            hit = np.flatnonzero(wanted(d1, d2) & (key[order] != 0))
            if len(hit):
                ranks[name] = int(hit[0]) + 1
        if len(ranks) == len(DIGIT_WANTED):
            return {name: ([pts], [0], K) for name, K in ranks.items()}
    raise AssertionError("no generator seed offers a key in every wanted bin")


def denormal():
    """3000 points, K = 1025, seed = row 0 at the ORIGIN (so that the offsets survive the subtraction): rows 1 .. 2099
    are offset from it by up to 2^-70 per axis, so their d2 is below 3 * 2^-140, an fp32 denormal (or 0), whatever
    the rounding; the other rows are an ordinary ball.  The 2K nearest candidates are all among the first 2100 rows."""
    rng = np.random.default_rng(70)
    pts = ball(rng, 3000, centre=(0.0, 0.0, 0.0))
    pts[:2100] = np.ldexp(rng.uniform(-1, 1, size=(2100, 3)), -70).astype(np.float32)
    pts[0] = 0.0
    return [pts], [0], 1025


def non_finite_cloud():
    """The cloud of test_patch_select_non_finite_coordinates (tests/test_data_gpu.py), seed 50: d2 is +inf for rows 7 and
    300, NaN for rows 100 and 4000, finite for the other 4996."""
    rng = np.random.default_rng(3)
    pts = ball(rng, 5000)
    pts[100, 1] = np.nan
    pts[7, 0] = np.inf
    pts[4000] = np.nan
    pts[300, 2] = -np.inf
    return pts


def kth_is_inf():
    """K = 4997: the K-th key is +inf (0x7F800000); row 7 is taken, its tie row 300 is left out."""
    return [non_finite_cloud()], [50], 4997


def kth_is_nan():
    """K = 4999: the K-th key is the NaN key 0x7FC00000; row 100 is taken, its tie row 4000 is left out."""
    return [non_finite_cloud()], [50], 4999


def patch_cases(capacity=CAPACITY):
    """name -> (scenes, seeds, K), every patch-select case; `capacity`: which of the (N, 16384) variants."""
    cases = {name: make() for name, make in GROUPS.items()}
    cases.update({f"small_{N}_{K}": single(N, K) for N, K in SMALL})
    cases.update({f"capacity_{N}": single(N, K) for N, K in capacity})
    cases["all_identical"] = all_identical()
    cases.update(digit_last_bins())
    cases.update({"denormal": denormal(), "kth_is_inf": kth_is_inf(), "kth_is_nan": kth_is_nan()})
    return cases


# ---- frame subset ---------------------------------------------------------------------------------------------------------
# (n, K): one point (nothing left to select); one of 2 and one of 5 (far fewer points than threads, a sort of 2 slots);
# a repetition of 0, 1 and a residue of 1; two of 3 and all but one of 4; then the capacity: a residue of 1 after 5461
# repetitions, the identity, all but one point, and a large frame -- the last two sort 16384 slots on top of the
# kernel's static LDS
SUBSET = [(1, 1), (2, 1), (5, 1), (2, 3), (3, 2), (4, 3), (3, MAX_K), (16384, MAX_K), (16385, MAX_K), (50000, MAX_K)]


def subset_seed(n, K):
    return int(np.random.default_rng(n + K).integers(0, 2 ** 64, dtype=np.uint64))


def subset_batch():
    """(count, seeds, K): 65 ragged frames, K = 64.  Every frame of the first two groups has n <= K and selects only its
    residue K % n: at most 16 in group 0 (n = 48 .. 64, and one frame of a single point), at most 31 in group 1
    (n = 24 .. 64, and one frame of 3 points).  The only frame that
    selects all 64 (n = 5000 > K) is frame 64, alone in the last group: the three launches sort 16, 32 and 64 slots."""
    rng = np.random.default_rng(6565)
    K = 64
    count = np.concatenate([rng.integers(48, 65, size=32), rng.integers(24, 65, size=32), [5000]])
    count[[0, 5, 9, 31]] = (1, 64, 48, 63)              # residues 0 (nothing to select), 0 (the identity), 16, 1
    count[[32, 40, 63]] = (33, 3, 24)                   # residues 31, 1 (after 21 repetitions), 16
    seeds = rng.integers(0, 2 ** 64, size=65, dtype=np.uint64)
    return count.astype(np.int64), seeds, K


def selected(n, K):
    """Points of a frame that the keyed order selects: K of n > K, else the residue K % n."""
    return K if n > K else K % n
