"""Inputs of the row BatchNorm kernels (csrc/rowbn.hip) shared by tests/test_rowbn_cpu.py and tests/test_rowbn_gpu.py,
with the oracle's restatements (oracle.ref_ops.rowbn_*) computed once per case.

SHAPES: (rows per segment P, K, C, input type, output / gradient type, segments) -> the launch edge the shape is the
smallest to reach, as entries of oracle.ref_ops.rowbn_geometry (tests/test_rowbn_cpu.py re-asserts every one, so a
retuned launcher constant fails there instead of silently un-testing the edge).

Family `dyadic`: x = k/16 (|k| <= 16, planted rows 17/16), given mean and beta = k/16 (|k| <= 8), given rstd in
{1/2, 1, 2}, gamma = +-{1/4, 1/2, 1, 2}, gy = k/8 (|k| <= 8), slope 0, 1/4 or 1.  Every summed quantity is then an integer
count of one power of two per channel and below 2^24 counts in total: exact in fp32 in ANY order (`dyadic_exactness`
raises otherwise), so the kernels must equal the fp32 restatement bit for bit, sums included.  Groups carry planted exact
ties (see `_plant`).  Family `random`: N(0, 1.7) rows with per-channel offsets, judged per element against the derived
bounds; `random_case` asserts on the FP64 twin alone that at most 1 % of the elements sit within the fp32 error of the
LeakyReLU kink and at most 1 % of the (group, channel) maxima within it of their runner-up.

Channels with an edge of their own (C >= 24; K > 0 for the guard of rowbn_bwd_reduce_max_kernel's (gy, y) form):
  0: beta == 4 gamma exactly (the guard's boundary, stored-output form)    1: beta one ulp above (gather form)
  2: gamma == 0, beta != 0      3: gamma == 0, beta == 0      4: gamma denormal (2^-130: 1/gamma overflows), beta == 0
  random only -- 5: gamma 1e-3;  6: rows scaled by 1e-3;  7: a constant column;  C-1: mean 1e3, deviation 1e-2;
  C-2: the first row (the statistics' pivot) 1e4 away from the rest."""
import functools

import torch

from oracle import ref_ops as R

F32, BF16 = torch.float32, torch.bfloat16
EXACT_UNITS = 2.0 ** 24
EPS, MOMENTUM = 1e-5, 0.1
DENORMAL = 2.0 ** -130

# P, K, C, din, dother, nseg, dyadic slope, geometry claims
SHAPES = [
    (150, 3, 24, F32, F32, 1, 0.25, dict(U_fwd=1, U_bwd=1, cpr=6, idle=4, grid_fwd=2)),
    (185, 5, 40, BF16, BF16, 1, 0.0, dict(U_fwd=1, U_bwd=1, cpr=5, idle=1)),
    (765, 255, 64, F32, F32, 1, 0.25, dict(U_fwd=1, U_bwd=1, L_fwd=1)),
    (7, 1, 8, F32, F32, 1, 0.25, dict(U_fwd=1, grid_fwd=1, rpi=128)),
    (18, 2, 8, F32, F32, 1, 0.0, dict(U_fwd=2, grid_fwd=1, rpi=128)),
    (240, 6, 72, F32, F32, 1, 1.0, dict(U_fwd=2, U_bwd=2, idle=4)),
    (330, 10, 64, BF16, BF16, 3, 0.25, dict(U_fwd=2, U_bwd=2, fin_L=16)),
    (330, 10, 64, BF16, F32, 3, 0.0, dict(U_fwd=2, ne=8)),
    (330, 10, 64, F32, BF16, 3, 0.25, dict(U_fwd=2, ne=8, ne_stats=4)),
    (330, 10, 64, F32, F32, 3, 1.0, dict(U_fwd=2, ne=4)),
    (32, 32, 64, F32, F32, 1, 0.25, dict(L_fwd=8, L_bwd=8, U_fwd=4)),
    (72, 24, 24, F32, F32, 1, 0.0, dict(L_fwd=2, L_bwd=2, U_fwd=4, idle=4)),
    (96, 48, 40, BF16, BF16, 2, 0.25, dict(L_fwd=4, L_bwd=4, U_fwd=4, idle=1)),
    (512, 256, 256, F32, F32, 1, 0.25, dict(L_fwd=64, L_bwd=64, grid_fwd=32)),
    (512, 256, 1024, BF16, BF16, 1, 0.25, dict(L_fwd=64, rpi=2, rpi_stats=2)),
    (600, 2, 512, F32, F32, 4, 0.25, dict(grid_fwd=128, grid_bwd=128, per_fwd=(1, 2), per_bwd=(1, 2))),
    (2200, 2, 1024, F32, F32, 1, 0.0, dict(grid_fwd=1024, per_fwd=(1, 2), rpi=1)),
    (707, 0, 1024, F32, F32, 4, 0.25, dict(per_stats=(30, 31), per_fwd=(11, 12), per_reduce=(30, 31))),
    (2819, 0, 1024, F32, F32, 1, 0.25, dict(G_stats=256, grid_fwd=256, per_stats=(11, 12), per_fwd=(11, 12))),
    (1025, 0, 1024, F32, F32, 9, 0.0, dict(G_stats=33, G_bwd=33, fin_L=4, fin_blocks_stats=2, fin_blocks_bwd=2)),
    (269, 0, 1024, F32, F32, 33, 0.25, dict(G_stats=9, G_bwd=9, fin_L=1, fin_blocks_stats=2, fin_blocks_bwd=2)),
    (1, 0, 8, F32, F32, 1, 0.25, dict(per_stats=(1, 1))),
    (1, 0, 8, F32, F32, 3, 0.25, dict(per_stats=(1, 1), fin_L=16)),
    (37, 0, 48, F32, F32, 1, 0.25, dict(ne=4, idle=4)),
    (37, 0, 48, F32, BF16, 1, 0.0, dict(ne=8, ne_stats=4, idle_stats=4, idle=4)),
    (37, 0, 48, BF16, F32, 1, 1.0, dict(ne=8, ne_stats=8)),
    (37, 0, 48, BF16, BF16, 1, 0.25, dict(ne=8)),
]
_TAG = {F32: "f32", BF16: "bf16"}
IDS = [f"{P}x{K}x{C}-{_TAG[a]}-{_TAG[b]}-s{n}" for P, K, C, a, b, n, _, _ in SHAPES]
INDEX = list(range(len(SHAPES)))
SMALL = [i for i in INDEX if SHAPES[i][0] * SHAPES[i][5] * SHAPES[i][2] <= 70000]       # what the CPU file runs in full
RANDOM_SLOPE = 0.2
# (case, variant): no affine parameters, eval-mode statistics, constants one float past a 16-byte boundary
VARIANTS = ["plain", "no_affine", "misaligned"]
VARIANT_CASES = [IDS.index(s) for s in ("150x3x24-f32-f32-s1", "330x10x64-bf16-bf16-s3", "96x48x40-bf16-bf16-s2",
                                        "37x0x48-f32-f32-s1", "37x0x48-bf16-bf16-s1", "600x2x512-f32-f32-s4")]


def special_channels(K, C):
    return C >= 24 and K > 0, C >= 24


def _plant(x, P, K, C, nseg, L, sign_a):
    """Exact ties by construction, one plan per group from group 0 on (as many as the case has groups), M = 17/16 on
    the side of the channel's maximum: `straddle` rows K/L - 1 and K/L (the last of run 0, the first of run 1) both M;
    `last` only row K - 1 is M (the byte K - 1: 254 or 255 at K = 255, 256); `firstlast` rows 0 and K - 1 both M;
    `neg` every row -M (with slope 0 and beta <= 0 the whole group is 0: arg 0); `dup` row 1 copied to row K - 1 and
    row 0 to row 1 (duplicate rows inside a group).  -> the plans in group order."""
    plans = (["straddle"] if L > 1 else []) + (["last"] if K >= 255 else []) + ["firstlast", "last", "neg", "dup"]
    plans = list(dict.fromkeys(plans))[:nseg * P // K]
    xg = x.view(-1, K, C)
    M = (17.0 / 16.0) * sign_a
    for g, plan in enumerate(plans):
        if plan == "straddle":
            xg[g, K // L - 1] = M
            xg[g, K // L] = M
        elif plan == "last":
            xg[g, K - 1] = M
        elif plan == "firstlast":
            xg[g, 0] = M
            xg[g, K - 1] = M
        elif plan == "neg":
            xg[g] = -M
        elif plan == "dup" and K >= 2:
            xg[g, K - 1] = xg[g, 1]
            xg[g, 1] = xg[g, 0]
    return plans


def _units(t, unit):
    """Largest sum |terms| per channel in counts of `unit` (C); raises unless every term is a whole count."""
    q = t.abs() / unit
    if not bool((q == q.round()).all()):
        raise AssertionError("a term is not a whole count of its unit")
    return q.sum(0)


def dyadic_exactness(c):
    """sum |terms| of every fp32 sum the kernels take on the case c, per segment and channel, counted in the terms' own
    last bit: {name: peak}.  Raises unless every count is an integer below 2^24: every partial sum in any order is then
    an fp32 number."""
    P, K, C, nseg = c["P"], c["K"], c["C"], c["nseg"]
    x = c["x"].double()
    rs = c["rstd"].double()
    s_unit = {0.0: 1.0, 1.0: 1.0, 0.25: 0.25}[c["slope"]]
    peaks = {}
    for s in range(nseg):
        xs = x[s * P:(s + 1) * P]
        d = xs - xs[0]
        peaks["d"] = max(peaks.get("d", 0.0), float(_units(d, 2.0 ** -4).max()))
        peaks["dd"] = max(peaks.get("dd", 0.0), float(_units(d * d, 2.0 ** -8).max()))
        rows = P // K if K else P
        b = c["bwd"]
        gg, xh = b["gg"][s * rows:(s + 1) * rows], b["xhat"][s * rows:(s + 1) * rows]
        peaks["gg"] = max(peaks.get("gg", 0.0), float(_units(gg, 2.0 ** -3 * s_unit).max()))
        u1 = 2.0 ** -7 * s_unit * rs[s].abs()[None]
        peaks["gg_xhat"] = max(peaks.get("gg_xhat", 0.0), float(_units(gg * xh, u1).max()))
        if K:
            by = c["bwd_y"]
            peaks["gg_xhat_y"] = max(peaks.get("gg_xhat_y", 0.0), float(_units(
                by["gg"][s * rows:(s + 1) * rows] * by["xhat"][s * rows:(s + 1) * rows], u1).max()))
    bad = {k: v for k, v in peaks.items() if not v < EXACT_UNITS}
    if bad:
        raise AssertionError(f"dyadic case {c['id']}: not exact in fp32: {bad}")
    return peaks


def _rt(t, dt):
    """Values of the row type, held in fp32."""
    return t.to(dt).float()


def _finish(c):
    """The restatements every test of the case shares: FP32 (what the kernels must produce) and the FP64 twin."""
    P, K, C, nseg = c["P"], c["K"], c["C"], c["nseg"]
    kw = dict(running_mean=c["rm0"], running_var=c["rv0"], num_batches_tracked=7, mean_shift=c["mean_shift"])
    c["stats"] = R.rowbn_stats_ref(c["x"], nseg, EPS, MOMENTUM, c["din"], **kw)
    c["stats64"] = R.rowbn_stats_ref(c["x"], nseg, EPS, MOMENTUM, c["din"], ar=R.FP64, **kw)
    c["stats_bound"] = R.rowbn_stats_bound(c["stats64"], c["rm0"], c["rv0"])
    return c


def _backward(c, mean, rstd):
    """apply + backward restatements with the GIVEN statistics mean, rstd (nseg, C) fp32."""
    K, nseg = c["K"], c["nseg"]
    bf_o, bf_i = c["dother"] == BF16, c["din"] == BF16
    args = (mean, rstd, c["gamma"], c["beta"], c["slope"])
    for tag, ar in (("", R.FP32), ("64", R.FP64)):
        f = R.rowbn_apply_ref(c["x"], K, *args, nseg, ar=ar)
        c["fwd" + tag] = f
    f = c["fwd"]
    c["y"] = R.rowbn_stored(f["y"], bf_o)                         # float64 carrier of the stored output
    c["arg"] = f["arg"]
    sums = (c["x"], c["arg"])
    tail = (K, *args, nseg, c["din"], c["dother"])
    c["bwd"] = R.rowbn_bwd_sums_ref(c["gy"], *sums, None, *tail)
    c["bwd64"] = R.rowbn_bwd_sums_ref(c["gy"], *sums, None, *tail, ar=R.FP64)
    if K:
        c["bwd_y"] = R.rowbn_bwd_sums_ref(c["gy"], *sums, c["y"], *tail)
    for tag, ar, b in (("", R.FP32, c["bwd"]), ("64", R.FP64, c["bwd64"])):
        c["dx" + tag] = R.rowbn_bwd_apply_ref(c["gy"], c["x"], c["arg"], K, *args, b["c12"], nseg, ar=ar)
    if K:
        c["dx_y"] = R.rowbn_bwd_apply_ref(c["gy"], c["x"], c["arg"], K, *args, c["bwd_y"]["c12"], nseg)
    c["dx_eval"] = R.rowbn_bwd_apply_ref(c["gy"], c["x"], c["arg"], K, *args, None, nseg)
    c["bf_in"], c["bf_other"] = bf_i, bf_o


def _base(i, variant):
    P, K, C, din, dother, nseg, slope, claims = SHAPES[i]
    return dict(i=i, id=IDS[i], variant=variant, P=P, K=K, C=C, din=din, dother=dother, nseg=nseg,
                geo_fwd=R.rowbn_geometry(P, K, C, din, dother, nseg))


@functools.lru_cache(maxsize=None)
def dyadic_case(i, variant="plain"):
    c = _base(i, variant)
    P, K, C, nseg = c["P"], c["K"], c["C"], c["nseg"]
    g = torch.Generator().manual_seed(100 + i)

    def q(lim, den, *shape):
        return torch.randint(-lim, lim + 1, shape, generator=g).float() / den
    x = q(16, 16, nseg * P, C)
    mean, beta = q(8, 16, nseg, C), q(8, 16, C)
    rstd = 2.0 ** torch.randint(-1, 2, (nseg, C), generator=g).float()
    gamma = 2.0 ** torch.randint(-2, 2, (C,), generator=g).float() * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
    guard, _ = special_channels(K, C)
    if guard:
        gamma[:5] = torch.tensor([0.125, -0.125, 0.0, 0.0, DENORMAL])
        beta[:5] = torch.tensor([0.5, torch.nextafter(torch.tensor(0.5), torch.tensor(1.0)).item(), 0.25, 0.0, 0.0])
    gamma[C - 3], beta[C - 3] = 1.0, -0.25          # NEG_CHANNEL: the `neg` plan's group is all-negative there for sure
    if variant == "no_affine":
        gamma = beta = None
    c["plans"] = _plant(x, P, K, C, nseg, c["geo_fwd"]["L_fwd"],
                        torch.ones(C) if gamma is None else torch.where(gamma < 0, -1.0, 1.0)) if K else []
    rows = nseg * P // K if K else nseg * P
    c.update(x=x, gamma=gamma, beta=beta, slope=SHAPES[i][6], gy=q(8, 8, rows, C), mean=mean, rstd=rstd,
             rm0=q(8, 16, C), rv0=q(8, 16, C).abs() + 0.5, mean_shift=q(8, 16, C), family="dyadic")
    if variant == "no_affine":
        c["mean_shift"] = None                                     # absent too: the finalize kernel's shift of 0
    _backward(c, mean, rstd)
    _finish(c)
    c["exact"] = dyadic_exactness(c)
    if K:                                                          # the planted ties decide what they were planted for
        arg = c["arg"].long().view(-1, C)
        live = torch.ones(C, dtype=torch.bool) if gamma is None else gamma.abs() >= 0.125
        for gi, plan in enumerate(c["plans"]):
            a = arg[gi][live]
            L = c["geo_fwd"]["L_fwd"]
            if plan == "straddle":
                assert bool((a == K // L - 1).any()), "straddling tie: the first run's last row"
            elif plan == "last":
                assert bool((a == K - 1).any()), "maximum at k = K - 1"
            elif plan == "firstlast":
                assert bool((a == 0).any()) and (K == 1 or not bool((a == K - 1).any())), "tie of the first and the last row"
            elif plan == "neg" and c["slope"] == 0.0 and gamma is not None:
                # channel C - 3 (gamma 1, beta -1/4): z = (-17/16 - mean) rstd - 1/4 < 0 on every row, v = 0, arg 0
                v, z = c["fwd"]["v"].view(-1, K, C)[gi, :, C - 3], c["fwd"]["z"].view(-1, K, C)[gi, :, C - 3]
                assert bool((z < 0).all()) and bool((v == 0).all()) and int(arg[gi, C - 3]) == 0, "an all-negative group"
        vk = c["fwd"]["v"].view(-1, K, C)
        c["ties"] = int(((vk == c["fwd"]["y"][:, None]).sum(1) > 1).sum())
        assert K == 1 or c["ties"] > 0
    return c


@functools.lru_cache(maxsize=None)
def random_case(i, variant="plain"):
    c = _base(i, variant)
    P, K, C, din, dother, nseg = c["P"], c["K"], c["C"], c["din"], c["dother"], c["nseg"]
    g = torch.Generator().manual_seed(500 + i)
    N = nseg * P
    x = torch.randn(N, C, generator=g) * 1.7 + torch.randn(C, generator=g) * 3.0
    gamma = (torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
    beta = 0.5 * torch.randn(C, generator=g)
    guard, edges = special_channels(K, C)
    if edges:
        gamma[5] = 1e-3
        x[:, 6] *= 1e-3
        x[:, 7] = x[0, 7]
        x[:, C - 1] = 1e3 + 1e-2 * torch.randn(N, generator=g)
        x[torch.arange(nseg) * P, C - 2] += 1e4
    if guard:
        gamma[:5] = torch.tensor([gamma[0].item(), gamma[1].item(), 0.0, 0.0, DENORMAL])
        beta[0] = 4.0 * gamma[0]
        beta[1] = torch.nextafter(4.0 * gamma[1].abs(), torch.tensor(100.0))
        beta[2:5] = torch.tensor([0.25, 0.0, 0.0])
    if variant == "no_affine":
        gamma = beta = None
    x = _rt(x, din)
    rows = N // K if K else N
    c.update(x=x, gamma=gamma, beta=beta, slope=RANDOM_SLOPE, gy=_rt(torch.randn(rows, C, generator=g), dother),
             rm0=torch.randn(C, generator=g), rv0=torch.rand(C, generator=g) * 1.5 + 0.5,
             mean_shift=None if variant == "no_affine" else 0.3 * torch.randn(C, generator=g), family="random")
    _finish(c)
    # the given statistics of the apply and backward launches: the batch's own (the twin's, as fp32 numbers)
    c["mean"], c["rstd"] = c["stats64"]["mean"].float(), c["stats64"]["rstd"].float()
    _backward(c, c["mean"], c["rstd"])
    f64 = c["fwd64"]
    c["kink"] = R.rowbn_kink(f64, x, c["mean"], nseg) & (f64["z"] != 0)
    share = float(c["kink"].double().mean())
    assert share <= 0.01, (c["id"], "near the kink", share)
    # `undecided` only documents that the seeds are well separated (on the FP64 twin alone): no check excludes by it, since
    # the apply launch is restated op for op and arg is required exact everywhere, near-ties included
    c["undecided"] = None
    if K > 1:
        Ev = R.ROWBN_SAFETY * R.U32 * (3.0 * (f64["z"] - (0.0 if beta is None else beta.double()[None])).abs() + 2.0 * f64["z"].abs())
        top = f64["v"].view(-1, K, C).topk(2, 1)[0]
        gap = top[:, 0] - top[:, 1]
        c["undecided"] = (gap > 0) & (gap <= 2.0 * Ev.view(-1, K, C).max(1)[0])
        share = float(c["undecided"].double().mean())
        assert share <= 0.01, (c["id"], "near-ties", share)
    rows_kink = c["kink"]
    if K:                                                          # the summed rows of the max variant: the arg-max rows
        rows_kink = c["kink"].view(-1, K, C).gather(1, c["arg"].long()[:, None])[:, 0]
    c["kink_rows"] = rows_kink
    stored = dict(gamma=c["gamma"], beta=c["beta"], bf16=c["bf_other"])
    c["sums_bound"] = R.rowbn_bwd_sums_bound(c["bwd64"], c["slope"], rows_kink)
    c["sums_bound_y"] = R.rowbn_bwd_sums_bound(c["bwd64"], c["slope"], rows_kink, stored) if K else None
    return c


def case(family, i, variant="plain"):
    return dyadic_case(i, variant) if family == "dyadic" else random_case(i, variant)
