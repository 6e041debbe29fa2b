"""The launch grid of the fused MLP forward (tpg_mlp_fwd: mlp_fwd_kernel + mlp_stats_finalize_kernel) shared by
tests/test_mlp_gpu.py (the kernels against the fp64 oracle) and tests/test_oracle_cpu.py (the restated geometry against
the launcher, the planted defects): every channel pair x the smallest shapes that reach each launch edge, and what each
shape must reach, asserted from oracle.ref_ops.mlp_fwd_geometry so that a retuned launch constant fails here instead
of hollowing a case out."""
from oracle import ref_ops as R

PAIRS = [(64, 64), (64, 128), (128, 64), (128, 128), (128, 256), (256, 128), (256, 256)]

# rows per segment, nseg, per-segment weight, the edge
SHAPES = [
    (4096, 1, False, "one_tile"),       # baseline: whole tiles, one per workgroup
    (1000, 1, False, "partial_tile"),   # partial last tile of the 64- and the 128-row tiles
    (37, 1, False, "short"),            # less than one tile: waves without rows (pivot from a clamped row, n = 0)
    (1, 1, False, "one_row"),           # N = 1: variance 0, rstd = 1 / sqrt(eps), the running variance's biased branch
    (70001, 1, False, "multi_tile"),    # above every cap: 2 and 1, 3 and 2 or 5 and 4 tiles, the last one partial
    (2997, 3, True, "ragged"),          # ragged segments with their own weights, one dead lane group
    (2997, 3, False, "ragged"),         # ... and one weight for all
    (16600, 3, False, "refetch"),       # the finalize's !fits path at L = 16 (G = 130 / 170; 85 where the cap is 256)
    (1100, 70, True, "two_sweeps"),     # 64 + 6 segments, L = 1, G = 9 or 16 > FIN_R: !fits, the chain across sweeps
    (192, 5, False, "dead_groups"),     # SP = 8 with three dead lane groups
]


def check_reaches(geo, edge):
    """Assert that the launch of `geo` reaches what its row of SHAPES says."""
    P, bm, t = geo["P"], geo["BM"], geo["tiles_wg"]
    lo, hi = int(t.min()), int(t.max())
    if edge == "one_tile":
        assert hi == 1 and P % bm == 0 and geo["fits"] and geo["sweeps"] == 1
    elif edge == "partial_tile":
        assert hi == 1 and P % bm != 0 and geo["tiles"] > 1
    elif edge == "short":
        assert geo["tiles"] == 1 and P < bm and int((geo["n_wave"] == 0).sum()) >= 1 and P % (geo["STRIPS"] * 16) != 0
    elif edge == "one_row":
        assert P == 1 and geo["G"] == 1
    elif edge == "multi_tile":
        assert geo["G"] == geo["slots"] and (hi, lo) in ((2, 1), (3, 2), (5, 4))
        assert P % bm != 0 and int(t[geo["last_wg"]]) == hi         # the partial tile ends a multi-tile walk
    elif edge == "ragged":
        assert P % bm != 0 and geo["fin_SP"] == 4 and geo["dead"] == 1
    elif edge == "refetch":
        assert geo["fin_L"] == 16
        if geo["slots"] == 512:
            assert geo["G"] in (130, 170) and not geo["fits"]
        else:
            assert geo["G"] == 85 and geo["fits"]
    elif edge == "two_sweeps":
        assert geo["sweeps"] == 2 and geo["fin_L"] == 1 and geo["dead"] == 58
        assert geo["G"] in (9, 16) and geo["G"] > R.TPG_BN_FIN_R and not geo["fits"]
        assert (hi, lo) == ((2, 1) if geo["G"] == 16 else (1, 1))
    elif edge == "dead_groups":
        assert geo["fin_SP"] == 8 and geo["dead"] == 3 and geo["sweeps"] == 1
    else:
        raise AssertionError(edge)
