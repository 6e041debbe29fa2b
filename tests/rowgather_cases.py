"""Inputs of the row-gather kernels (csrc/rowgather.hip) shared by tests/test_rowgather_cpu.py and
tests/test_rowgather_gpu.py, with the FP64 twins of oracle.ref_ops (rowcombine_*_twin) computed once per case.

SHAPES: one dict per case -- mode (GATHER / SUB / EDGE of tpg_rowcombine_*, FRONT = tpg_rowcombine_edge_*), type pair
(ff: f32 rows and f32 grouped tensor, fb: f32 rows / bf16 grouped, bb: both bf16), B, N, S, K, C, how idx is built, which
launches run, and `claims`: the entries of oracle.ref_ops.rowcombine_geometry that make the shape the smallest to reach
its edge (tests/test_rowgather_cpu.py re-asserts every one, so a retuned cap fails there instead of un-testing the edge).

Family `dyadic`: every value k / 16 with |k| <= 64, slopes 1/4 (edge) and 1/2 (node): every term of every sum is a whole
count of 2^-6 and the longest chain stays below 2^24 counts (`dyadic_exactness` raises otherwise), so every sum is exact
in fp32 in ANY order: f32 outputs must equal the twin bit for bit, bf16 outputs its round-to-nearest-even.  Differences
of E are 0 in about one entry in a hundred, and the kink cases put a tie on every row.
Family `random`: standard normal values rounded to the row type first, slopes 0.2 / 0.1; the forward against the fp32
restatement op for op, the backward per element against the derived bounds (oracle.ref_ops.rowcombine_bound).

idx builders: `random`; `oor` (random with negative, N, N + 50 and INT_MIN planted); `ladder` (destination rows with
exactly the list lengths LS, the remainder on one hub row, in a fixed permutation per cloud); `targets` (entries on
rows of the backward's LAST pass and on the first rows); `kink` (idx[:, n, 0] = n, for K = 1 on every second row)."""
import functools

import numpy as np
import torch

from oracle import ref_ops as R

F32, BF16 = torch.float32, torch.bfloat16
PAIRS = {"ff": (F32, F32), "fb": (F32, BF16), "bb": (BF16, BF16)}
MODE = {"GATHER": R.ROW_GATHER, "SUB": R.ROW_SUB, "EDGE": R.ROW_EDGE, "FRONT": R.ROW_EDGE}
EXACT_UNITS = 2.0 ** 24
SLOPES = {"dyadic": (0.25, 0.5), "random": (0.2, 0.1)}          # (slope / slope_e, slope_a)
THREAD_LS = (0, 1, 3, 4, 5, 7, 8, 9)                             # around the 4-entry unroll of the thread form
UNROLL_KS = (1, 3, 4, 5, 8, 9)
MIN_HUB = 64


def wave_ls(G):
    return (0, 1, G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1, 3 * G, 4 * G + 1)


def ladder_rows(ls, K, edge):
    """Smallest S (and N: S for EDGE, else 16) whose S * K entries hold the lists `ls` and a hub of at least
    max(MIN_HUB, S) entries (K = 1: MIN_HUB, a hub of S entries would leave none for the lists)."""
    S = 1
    while S * K - sum(ls) < max(MIN_HUB, S if K > 1 else 0) or (edge and S < len(ls) + 1):
        S += 1
    return (S if edge else 16), S


SHAPES = []


def _add(name, mode, pair, B, N, S, K, C, idx, claims, run=("fwd", "bwd"), big=False, ties=False):
    SHAPES.append(dict(id=f"{name}-{mode}-{pair}-{B}x{N}x{S}x{K}x{C}", mode=mode, pair=pair, B=B, N=N, S=S, K=K, C=C,
                       idx=idx, claims=claims, run=run, big=big, ties=ties))


def _ne(pair):
    return 4 if pair == "ff" else 8


# 1. a rounded-up forward grid under the XCD ordering: 65 workgroups launched as 72, the last of them partial
for _m in ("GATHER", "SUB", "EDGE"):
    _add("xcd", _m, "ff", 1, 165 if _m == "EDGE" else 50, 165, 100, 4, ("random",),
         dict(total=16500, wgs=65, wgs_launched=72, xcd=True, idle=7, passes_fwd=1), run=("fwd",))
# 2. the forward's grid-stride loop takes a second, partial pass
_add("fwd2", "SUB", "ff", 1, 64, 2049, 32, 256, ("random",),
     dict(total=4196352, wgs_launched=16384, xcd=True, passes_fwd=2), run=("fwd",), big=True)
_add("fwd2", "EDGE", "bb", 1, 4100, 4100, 32, 256, ("random",),
     dict(total=4198400, wgs_launched=16384, xcd=True, passes_fwd=2), run=("fwd",), big=True)
# 3. out-of-range indices: forward and backward agree on the clamped destination
for _m in ("GATHER", "SUB", "EDGE", "FRONT"):
    for _p in ("ff", "fb", "bb"):
        _add("oor", _m, _p, 2, 40, 40 if _m in ("EDGE", "FRONT") else 24, 5, 16, ("oor",), dict(cpr=16 // _ne(_p)))
# 4. wave form: the list-length ladder around G = 64 / cpr entries per step
for _cpr in (1, 2, 4, 8, 16, 32):
    for _p in ("ff", "fb", "bb"):
        for _m in ("GATHER", "SUB") + (("EDGE",) if _cpr >= 4 else ()):
            _n, _s = ladder_rows(wave_ls(64 // _cpr), 8, _m == "EDGE")
            _add("wave", _m, _p, 2, _n, _s, 8, _cpr * _ne(_p), ("ladder", wave_ls(64 // _cpr)),
                 dict(form="wave", cpr=_cpr, G=64 // _cpr, passes_bwd=1))
# 5. wave form: more than 65536 rows, a second pass
_add("wave2", "GATHER", "ff", 3, 21900, 32, 8, 4, ("targets",), dict(form="wave", G=64, grid_bwd=16384, passes_bwd=2),
     run=("bwd",), big=True)
_add("wave2", "EDGE", "ff", 1, 65600, 65600, 2, 16, ("kink",), dict(form="wave", G=16, grid_bwd=16384, passes_bwd=2),
     run=("bwd",), big=True)
# 6. + 8. thread form of GATHER / SUB: cpr that does not divide 64, and 64; lists and K around the 4-entry unroll
for _i, (_c, _p) in enumerate([(24, "ff"), (48, "ff"), (96, "ff"), (24, "bb"), (48, "bb"), (96, "bb"), (48, "fb"),
                               (256, "ff"), (512, "bb")]):
    for _m, _k in (("GATHER", UNROLL_KS[(_i + 3) % 6]), ("SUB", UNROLL_KS[_i % 6])):
        _n, _s = ladder_rows(THREAD_LS, _k, False)
        _add("thread", _m, _p, 2, _n, _s, _k, _c, ("ladder", THREAD_LS), dict(form="thread", cpr=_c // _ne(_p), G=None))
# 7. + 8. thread form of EDGE: one or two chunks per row; the centre loop's K around the unroll
for (_c, _p), _k in zip([(4, "ff"), (8, "ff"), (8, "bb"), (16, "bb"), (8, "fb"), (16, "fb")], UNROLL_KS):
    _n, _s = ladder_rows(THREAD_LS, _k, True)
    _add("thread", "EDGE", _p, 2, _n, _s, _k, _c, ("ladder", THREAD_LS), dict(form="thread", cpr=_c // _ne(_p)))
# 9. thread form: more than 1048576 chunks, a second pass
_add("thread2", "GATHER", "ff", 2, 87400, 64, 8, 24, ("targets",), dict(form="thread", cpr=6, grid_bwd=4096, passes_bwd=2),
     run=("bwd",), big=True)
_add("thread2", "EDGE", "ff", 8, 65600, 65600, 1, 8, ("kink",), dict(form="thread", cpr=2, grid_bwd=4096, passes_bwd=2),
     run=("bwd",), big=True)
# 10. rowsum_neg's second pass
_add("rowsum2", "SUB", "ff", 1, 8, 65600, 1, 256, ("random",), dict(form="thread", passes_rowsum=2), run=("bwd",), big=True)
# 11. the kink of EDGE mode: every point its own neighbour 0, a third of the E rows duplicated, -0.0 present
for _m in ("EDGE", "FRONT"):
    _add("kink", _m, "ff", 2, 48, 48, 6, 8, ("kink",), dict(form="thread", cpr=2), ties=True)
    _add("kink", _m, "ff", 2, 48, 48, 6, 64, ("kink",), dict(form="wave", cpr=16, G=4), ties=True)
# 12. the front end (row stride 2C, Uraw, slope_a): the wave ladder at cpr 4 and 16, the thread form's C
for _cpr in (4, 16):
    for _p in ("ff", "fb", "bb"):
        _n, _s = ladder_rows(wave_ls(64 // _cpr), 8, True)
        _add("wave", "FRONT", _p, 2, _n, _s, 8, _cpr * _ne(_p), ("ladder", wave_ls(64 // _cpr)),
             dict(form="wave", cpr=_cpr, G=64 // _cpr))
for (_c, _p), _k in zip([(4, "ff"), (8, "ff"), (8, "bb"), (16, "bb"), (8, "fb"), (16, "fb")], (5, 9, 4, 3, 1, 8)):
    _n, _s = ladder_rows(THREAD_LS, _k, True)
    _add("thread", "FRONT", _p, 2, _n, _s, _k, _c, ("ladder", THREAD_LS), dict(form="thread", cpr=_c // _ne(_p)))

IDS = [s["id"] for s in SHAPES]
assert len(set(IDS)) == len(IDS)
INDEX = list(range(len(SHAPES)))
SMALL = [i for i in INDEX if not SHAPES[i]["big"]]
FWD = [i for i in INDEX if "fwd" in SHAPES[i]["run"]]
BWD = [i for i in INDEX if "bwd" in SHAPES[i]["run"]]


def geometry(s):
    din, dout = PAIRS[s["pair"]]
    return R.rowcombine_geometry(MODE[s["mode"]], s["B"], s["N"], s["S"], s["K"], s["C"], din, dout)


def last_pass_row(s):
    """(cloud, n): the first destination row of the backward's last pass all of whose chunks lie in it."""
    geo = geometry(s)
    first = 4 * geo["grid_bwd"] if geo["form"] == "wave" else -(-256 * geo["grid_bwd"] // geo["cpr"])
    return first // s["N"], first % s["N"]


def build_idx(s, seed):
    B, N, S, K = s["B"], s["N"], s["S"], s["K"]
    rng = np.random.default_rng(seed)
    kind = s["idx"][0]
    idx = rng.integers(0, N, (B, S, K)).astype(np.int32)
    if kind == "oor":
        flat = idx.reshape(B, -1)
        flat[:, 1::7] = np.resize(np.array([-1, N, N + 50, -50, np.iinfo(np.int32).min, np.iinfo(np.int32).max], np.int32),
                                  flat[:, 1::7].shape)
    elif kind == "ladder":
        ls = s["idx"][1]
        for b in range(B):
            rows = np.random.default_rng(1000 + b).permutation(N)[:len(ls) + 1]
            dest = np.concatenate([np.full(L, r) for r, L in zip(rows, ls)] + [np.full(S * K - sum(ls), rows[-1])])
            idx[b] = dest[np.random.default_rng(2000 + b).permutation(S * K)].reshape(S, K)
            cnt = np.bincount(idx[b].ravel(), minlength=N)
            assert sorted(cnt[rows[:-1]]) == sorted(ls) and cnt[rows[-1]] >= max(MIN_HUB, S if K > 1 else 0)
            assert cnt.sum() == cnt[rows].sum()
    elif kind == "targets":
        b1, n1 = last_pass_row(s)
        assert b1 == B - 1 and n1 < N - 8
        idx[:] = rng.integers(0, N, (B, S, K))
        idx[B - 1, :, 0::2] = rng.integers(n1, N, idx[B - 1, :, 0::2].shape)
        idx[:, :, 1] = rng.integers(0, 8, (B, S))
        idx[B - 1, 0, 0], idx[B - 1, 1, 0] = N - 1, n1
    elif kind == "kink":
        own = np.arange(N, dtype=np.int32)
        if K > 1:
            idx[:, :, 0] = own[None]
        else:
            idx[:, ::2, 0] = own[None, ::2]
        if s["big"]:                                   # neighbours in the rows of the last pass too
            b1, n1 = last_pass_row(s)
            idx[b1, n1:, K - 1] = rng.integers(n1, N, N - n1)
    return idx


def _values(family, g, dt, *shape):
    if family == "dyadic":
        return torch.randint(-64, 65, shape, generator=g).float() / 16.0
    return torch.randn(*shape, generator=g).to(dt).float()


def dyadic_exactness(c):
    """The condition under which every sum the kernels take on the dyadic case c is exact in fp32 in any order: every
    input a whole count of 2^-4 (a bf16 number where the rows are bf16), the slopes whole counts of 1/4, so every term
    is a whole count of 2^-6; the longest chain (longest list + K + 1 terms) times the largest term stays below 2^24
    counts.  -> that peak count; raises otherwise."""
    peak_term = 0.0
    for name in ("U", "QE", "Y", "g"):
        t = c.get(name)
        if t is None:
            continue
        q = t.double() * 16.0
        if not bool((q == q.round()).all()):
            raise AssertionError(f"{c['id']}: {name} is not a whole count of 2^-4")
        if not torch.equal(t.to(BF16).float(), t.float()):
            raise AssertionError(f"{c['id']}: {name} is not a bf16 number")
        peak_term = max(peak_term, float(t.abs().max()))
    for sl in (c["slope"], c["slope_a"]):
        if sl * 4.0 != round(sl * 4.0) or sl <= 0:
            raise AssertionError("a slope is not a whole count of 1/4")
    chain = c["Lmax"] + c["K"] + 1
    peak = chain * 2.0 * peak_term * 64.0              # a forward term |E[n] - E[s]| reaches twice the largest input
    if not peak < EXACT_UNITS:
        raise AssertionError(f"{c['id']}: {chain} terms of up to {2 * peak_term} exceed 2^24 counts of 2^-6")
    return peak


def _stored32(v, bf16):
    """Values as the kernels store them, held in fp32 (v float64: exact values; float32: the kernel's own)."""
    if v.dtype == torch.float64:
        return R.rowbn_stored(v, bf16).float()
    return v.to(BF16).float() if bf16 else v


def _build(family, i, dev):
    s = SHAPES[i]
    c = dict(s, i=i, family=family, geo=geometry(s))
    B, N, S, K, C, mode = s["B"], s["N"], s["S"], s["K"], s["C"], s["mode"]
    din, dout = PAIRS[s["pair"]]
    g = torch.Generator().manual_seed((100 if family == "dyadic" else 500) + i)
    idx = build_idx(s, 7 + i)
    c.update(din=din, dout=dout, bf_in=din == BF16, bf_out=dout == BF16, slope=SLOPES[family][0], slope_a=SLOPES[family][1])
    rows = {}
    if mode == "FRONT":
        Y = _values(family, g, din, B, N, 2 * C)
        Y[:, :, C:][:, :, 0::5] = 0.0                   # lrelu'(0) of the node half: slope_a
        Y[:, 1::2, C:][:, :, 0::10] = -0.0
        rows["Y"] = Y
        E = Y[:, :, :C]
    else:
        rows["U"] = _values(family, g, din, B, N, C)
        if mode != "GATHER":
            rows["QE"] = _values(family, g, din, B, S, C)
        E = rows.get("QE")
    if s["ties"]:
        E[:, 1::3] = E[:, 0:-1:3]                       # exact ties between distinct rows
        E[:, 0::6, 0::2] = 0.0
        E[:, 1::6, 0::2] = -0.0                         # the duplicate of a +0.0 row holds -0.0
    c["g"] = _values(family, g, dout, B, S, K, C).to(dev) if "bwd" in s["run"] else None
    for k, v in rows.items():
        c[k] = v.to(dev)
    c["idx"] = torch.from_numpy(idx).to(dev)
    c["idxc"] = R.rowcombine_clamp(c["idx"], N).to(torch.int32)
    c["Lmax"] = max(int(np.bincount(row, minlength=N).max()) for row in c["idxc"].cpu().numpy().reshape(B, -1))
    sl, sa = c["slope"], c["slope_a"]
    if "fwd" in s["run"]:
        dt = torch.float64 if family == "dyadic" else torch.float32
        if mode == "FRONT":
            out = R.rowcombine_edge_fwd_twin(c["Y"], c["idx"], sa, sl, dt)
        else:
            out = R.rowcombine_fwd_twin(c["U"], c.get("QE"), c["idx"], MODE[mode], sl, 1.0, dt)
        c["out"] = _stored32(out, c["bf_out"])
    if "bwd" in s["run"]:
        if mode == "FRONT":
            c["bwd"] = R.rowcombine_edge_bwd_twin(c["g"], c["idx"], c["Y"], sa, sl)
        else:
            c["bwd"] = R.rowcombine_bwd_twin(c["g"], c["idx"], c.get("QE") if mode == "EDGE" else None, MODE[mode], N, sl)
    if family == "dyadic":
        c["exact"] = dyadic_exactness(c)
    return c


_cached = functools.lru_cache(maxsize=None)(_build)


def case(family, i, dev="cpu"):
    """The case with its tensors and twins on `dev` (the big ones are built per use, the others once)."""
    return _build(family, i, dev) if SHAPES[i]["big"] else _cached(family, i, dev)
