"""Anisotropic surface kernels without a GPU: the torch statements (`ops._aniso_kernels_torch`, `ops._aniso_field_torch`)
against the numpy statement of the rule (tests/aniso_rule.py) bit for bit, the rule's own properties on a full lattice,
a sheet, a row and degenerate clouds, the ripple of a jittered slab meshed both ways, the unchanged isotropic path, the
C entries' argument checks, and the CLI / rollout options under the oracle backend.

TOL: the rule's largest deviation from the float64 `numpy.linalg.eigh` statement of the same stages (`R.kernels_eigh`)
over the committed clouds is 6.4e-7 (entries of G absolutely, det relatively, a centre relative to max(rc, |x|): the
fp32 rounding of a position is relative to its magnitude); the tests allow 4 x that, 2.6e-6.  The field comparison is
relative: its fixed-point unit 2^-22 truncates every one of the ~60 terms of a node, 2e-6 of a value of 3 to 5."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aniso_cases as K  # noqa: E402
import aniso_rule as R  # noqa: E402
import iso_rule as IR  # noqa: E402
import test_mesh_cpu as M  # noqa: E402

F32 = np.float32
TOL = 2.6e-6
DEFAULTS = dict(lam=0.9, kr=4.0, s_min=0.125, s_max=2.0, kn=0.5, n_eps=25)
N_EPS = {"row": 5}                              # a row particle has 9 neighbours within rc: below the default n_eps


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def default_ks():
    from tpgan_amd import mesh
    return 1.0 / mesh.lattice_covariance(K.SPACING, K.RC)


def rule_params(name=None, **kw):
    args = dict(DEFAULTS, n_eps=N_EPS.get(name, 25))
    args.update(kw)
    return R.params(K.RC, default_ks(), **args)


def torch_params(prm):
    from tpgan_amd import ops
    return ops._aniso_params(float(prm.rc), float(prm.ks), float(prm.lam), float(prm.kr), float(prm.s_min), float(prm.s_max),
                             float(prm.kn), prm.n_eps)


@functools.lru_cache(maxsize=None)
def rule_kernels(name):
    """The rule's stage A of a committed cloud, computed once and shared; read-only."""
    out = R.kernels(K.cloud(name), rule_params(name))
    for a in out:
        a.setflags(write=False)
    return out


def queries(name):
    """Stage B queries of a cloud: beside its particles, a (9,7,5) lattice over its first 150 rows' bounding box padded
    by 0.06, a point beyond every reach, and a NaN."""
    x = K.cloud(name)
    lo, hi = x[:150].min(0).astype(np.float64) - 0.06, x[:150].max(0).astype(np.float64) + 0.06
    ax = [np.linspace(lo[a], hi[a], n) for a, n in enumerate((9, 7, 5))]
    nodes = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    extra = np.array([[lo[0] - 50.0, lo[1], lo[2]], [np.nan, 0.0, 0.0]])
    return np.concatenate([x[:200].astype(np.float64) + 0.01, nodes, extra]).astype(F32)


@functools.lru_cache(maxsize=None)
def rule_field(name):
    c, G, d, _ = rule_kernels(name)
    out = R.field(queries(name), c, G, d, K.SUPPORT, K.REACH)
    out.setflags(write=False)
    return out


# ---- the torch statements -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.CLOUDS)
def test_torch_statements_equal_the_rule(name):
    from tpgan_amd import ops
    x = K.cloud(name)
    rc, rG, rd, rn = rule_kernels(name)
    c, G, d, n = ops._aniso_kernels_torch(torch.from_numpy(x), torch_params(rule_params(name)))
    assert c.dtype == G.dtype == d.dtype == torch.float32 and n.dtype == torch.int32
    assert tuple(G.shape) == (x.shape[0], 6) and rn.min() >= 1                     # every particle is its own member
    assert np.array_equal(bits(c), bits(rc)) and np.array_equal(bits(G), bits(rG)) and np.array_equal(bits(d), bits(rd))
    assert np.array_equal(n.numpy(), rn)
    q = queries(name)
    f = ops._aniso_field_torch(torch.from_numpy(q), c, G, d, K.SUPPORT, K.REACH)
    rf = rule_field(name)
    assert rf.max() > 0.4 and rf[-1] == 0.0 and rf[-2] == 0.0 and np.isfinite(rf).all()
    assert np.array_equal(bits(f), bits(rf))
    # small chunks walk the statement's other paths: the same bits
    f2 = ops._aniso_field_torch(torch.from_numpy(q), c, G, d, K.SUPPORT, K.REACH, pairs_per_chunk=1000, query_rows=97)
    c2 = ops._aniso_kernels_torch(torch.from_numpy(x), torch_params(rule_params(name)), pairs_per_chunk=1000)
    assert np.array_equal(bits(f2), bits(rf)) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(c2[:3], (rc, rG, rd)))


def test_ops_dispatch_batches_lengths_and_validation(oracle_cpu):
    from tpgan_amd import ops
    ks = default_ks()
    names = ["random257", "one", "random64"]
    N = 257
    batch = torch.zeros((3, N, 3))
    for b, name in enumerate(names):
        x = K.cloud(name)
        batch[b, :x.shape[0]] = torch.from_numpy(x)
    lengths = torch.tensor([257, 0, 64])
    c, G, d, n = ops.anisotropic_kernels(batch, K.RC, ks, lengths=lengths)
    for b, name in ((0, "random257"), (2, "random64")):
        rc, rG, rd, rn = rule_kernels(name)
        m = rn.shape[0]
        assert np.array_equal(bits(c[b, :m]), bits(rc)) and np.array_equal(bits(G[b, :m]), bits(rG))
        assert np.array_equal(bits(d[b, :m]), bits(rd)) and np.array_equal(n[b, :m].numpy(), rn)
        assert float(G[b, m:].abs().sum()) == 0.0 and int(n[b, m:].sum()) == 0
    assert float(c[1].abs().sum()) == 0.0 and float(d[1].abs().sum()) == 0.0 and int(n[1].sum()) == 0
    q = torch.from_numpy(queries("random257"))
    f = ops.anisotropic_field(q.unsqueeze(0).expand(3, -1, -1).contiguous(), c, G, d, K.SUPPORT, lengths_q=torch.tensor([q.shape[0], 5, 7]),
                              lengths_p=lengths)
    assert np.array_equal(bits(f[0]), bits(rule_field("random257"))) and float(f[1].abs().sum()) == 0.0
    assert float(f[2, 7:].abs().sum()) == 0.0
    one = ops.anisotropic_kernels(torch.from_numpy(K.cloud("random64")), K.RC, ks)              # unbatched
    assert one[0].shape == (64, 3) and np.array_equal(bits(one[1]), bits(rule_kernels("random64")[1]))
    x = torch.from_numpy(K.cloud("random64"))
    for match, kw in [("cov_radius", dict(cov_radius=0.0)), ("cov_radius", dict(cov_radius=float("nan"))), ("ks", dict(ks=-1.0)),
                      ("smooth_lambda", dict(smooth_lambda=1.5)), ("kr", dict(kr=0.5)), ("s_min", dict(s_min=3.0)),
                      ("kn", dict(kn=0.0)), ("n_eps", dict(n_eps=-1)), ("\\(B,N,3\\)", dict(points=x[:, :2])),
                      ("float tensor", dict(points=x.long()))]:
        args = dict(points=x, cov_radius=K.RC, ks=ks)
        args.update(kw)
        with pytest.raises(RuntimeError, match=match):
            ops.anisotropic_kernels(**args)
    c, G, d, _ = one
    for match, kw in [("support", dict(support=0.0)), ("s_max", dict(s_max=float("inf"))), ("G \\(B,Np,6\\)", dict(G=G[:, :5])),
                      ("det", dict(det=d[:10])), ("float tensors", dict(det=d.long()))]:
        args = dict(query=x, centres=c, G=G, det=d, support=K.SUPPORT)
        args.update(kw)
        with pytest.raises(RuntimeError, match=match):
            ops.anisotropic_field(**args)
    ops.unregister_backend("cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.anisotropic_kernels(x, K.RC, ks)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.anisotropic_field(x, c, G, d, K.SUPPORT)


# ---- the rule's properties ------------------------------------------------------------------------------------------------
def centre_deviation(c, ref, x, rc):
    return float((np.abs(c.astype(np.float64) - ref) / np.maximum(np.abs(x.astype(np.float64)), rc)).max())


@pytest.mark.parametrize("name", K.CLOUDS)
def test_rule_deviates_from_the_eigh_statement_by_a_quarter_of_the_tolerance_at_most(name):
    x = K.cloud(name)
    prm = rule_params(name)
    c, G, d, n = rule_kernels(name)
    ec, eG, ed, en = R.kernels_eigh(x, prm)
    dev = max(float(np.abs(G - eG).max()), float(np.abs(d / ed - 1.0).max()), centre_deviation(c, ec, x, float(prm.rc)))
    print(f"{name}: deviation from the eigh statement {dev:.3e}")
    assert np.array_equal(n, en) and dev <= TOL / 4.0


@functools.lru_cache(maxsize=None)
def full_lattice():
    x = K.lattice((13, 13, 13))
    idx = np.stack(np.meshgrid(*[np.arange(13)] * 3, indexing="ij"), -1).reshape(-1, 3)
    inner = ((idx >= 4) & (idx <= 8)).all(1)                                       # at least rc = 4 spacings from the boundary
    return x, inner, R.kernels(x, rule_params())


def test_a_full_lattice_has_the_isotropic_kernel():
    from tpgan_amd import mesh
    assert abs(mesh.lattice_covariance(K.SPACING, K.RC) - 0.150571) < 1e-6
    x, inner, (c, G, d, n) = full_lattice()
    assert inner.sum() == 125 and n[inner].max() == 257 and n[inner].min() >= 251   # the rim (weight 0) is a matter of rounding
    e = R.extents(G)[inner]
    print(f"full lattice: extents within {np.abs(e - 1).max():.2e} of 1, det within {np.abs(d[inner] - 1).max():.2e}, "
          f"centres within {np.abs(c[inner] - x[inner]).max() / K.RC:.2e} rc")
    assert np.abs(e - 1.0).max() <= TOL and np.abs(d[inner].astype(np.float64) - 1.0).max() <= TOL
    assert np.abs(c[inner].astype(np.float64) - x[inner]).max() <= TOL * K.RC
    assert R.extents(G)[~inner].min() < 0.5                                        # the boundary is not isotropic


def test_field_identities_on_the_full_lattice():
    """At the 27 nodes of the lattice step spacing / 2 around the central particle the anisotropic field is the isotropic
    one (relatively: see the module's docstring); a node beyond reach of every centre gets exactly 0."""
    from tpgan_amd import mesh, ops
    x, inner, (c, G, d, n) = full_lattice()
    lat = mesh.Lattice(np.full(3, 6 * K.SPACING - K.SPACING / 2, F32), float(F32(K.SPACING / 2)), (3, 3, 3))
    nodes = mesh.lattice_nodes(lat, 0, 27, "cpu").numpy()
    fa = R.field(nodes, c, G, d, K.SUPPORT, K.REACH)
    fi = ops._radius_cubic_sums_torch(torch.from_numpy(nodes), torch.from_numpy(x), K.SUPPORT).numpy()
    print(f"field identity: relative difference {np.abs(fa / fi - 1).max():.2e}")
    assert fi.min() > 3.0 and np.abs(fa.astype(np.float64) / fi - 1.0).max() <= TOL
    far = np.array([[12 * K.SPACING + 1.01 * K.REACH, 0.15, 0.15], [-1.01 * K.REACH, 0.0, 0.0], [5.0, 5.0, 5.0]], F32)
    near = np.array([[11 * K.SPACING, 0.15, 0.15]], F32)       # (the face's centres have moved in by about a spacing)
    assert np.array_equal(R.field(far, c, G, d, K.SUPPORT, K.REACH), np.zeros(3, F32))
    assert R.field(near, c, G, d, K.SUPPORT, K.REACH)[0] > 0.0


def test_a_sheet_is_flat_and_a_row_is_thin():
    prm = rule_params()
    c, G, d, n = rule_kernels("sheet")
    idx = np.stack(np.meshgrid(np.arange(20), np.arange(20), indexing="ij"), -1).reshape(-1, 2)
    interior = ((idx >= 4) & (idx <= 15)).all(1)                                   # the full in-plane neighbourhood
    assert interior.sum() == 12 * 12 and n[interior].max() == 49 and n[interior].min() >= 45   # the rim has weight 0
    e = R.extents(G)[interior]
    # two equal extents, the third at the floor top / kr (nothing is clamped: 0.125 < e0, e2 < 2)
    assert np.abs(e[:, 2] - e[:, 1]).max() <= TOL and np.abs(e[:, 2] / e[:, 0] - float(prm.kr)).max() <= TOL * float(prm.kr)
    assert e[:, 0].min() > float(prm.s_min) and e[:, 2].max() < float(prm.s_max)
    M3 = np.zeros((3, 3))
    for k, (a, b) in enumerate(R.PAIRS):
        M3[a, b] = M3[b, a] = G[np.argmax(interior), k]
    w, v = np.linalg.eigh(M3)
    assert abs(abs(v[2, 2]) - 1.0) <= TOL                                          # the short axis is the sheet's normal
    assert np.abs(c[:, 2]).max() == 0.0                                            # centres stay in the plane
    c, G, d, n = rule_kernels("row")                                              # n_eps = 5 for this cloud
    assert 5 < n[4:36].min() and n.max() <= 9
    e = R.extents(G)[4:36]
    assert np.abs(e[:, 0] - e[:, 1]).max() <= TOL
    assert np.abs(e[:, 2] / e[:, 0] - float(prm.kr)).max() <= TOL * float(prm.kr)
    few = R.kernels(K.cloud("row"), rule_params())                                 # at the default n_eps the row is all kn
    assert np.array_equal(R.extents(few[1]), np.full((40, 3), 0.5))


@pytest.mark.parametrize("name", ["one", "pair", "coincident"])
def test_degenerate_counts_take_the_kn_branch(name):
    c, G, d, n = rule_kernels(name)
    x = K.cloud(name)
    assert n.tolist() == [x.shape[0]] * x.shape[0]
    assert np.array_equal(G, np.tile(np.array([2, 0, 0, 2, 0, 2], F32), (x.shape[0], 1))) and np.array_equal(d, np.full(x.shape[0], 8, F32))
    assert np.isfinite(c).all() and np.abs(c - x).max() <= 0.9 * K.RC
    if name == "coincident":                                                      # 30 > n_eps members, a zero covariance
        assert n[0] == 30 > 25 and np.array_equal(c, x)


# ---- the point of the feature ---------------------------------------------------------------------------------------------
def top_ripple(m, layers=3):
    v = m.vertices.numpy().astype(np.float64) / K.SPACING
    sel = (v[:, 0] >= 8) & (v[:, 0] <= 15) & (v[:, 1] >= 8) & (v[:, 1] <= 15) & (v[:, 2] > (layers - 1) / 2)
    return int(sel.sum()), float(v[sel, 2].std()), float(v[sel, 2].mean())


def test_the_anisotropic_surface_of_a_jittered_slab_ripples_less_than_half_as_much(oracle_cpu):
    """A 24 x 24 x 3 slab at spacing 0.025, jittered by +-0.3 spacings, meshed both ways at the defaults; the top side's
    vertices over the interior.  Measured: standard deviation of their height 0.1206 spacings isotropic, 0.0100
    anisotropic (ratio 0.083); mean height 0.47 spacings above the top layer's centres against 0.37 below."""
    from tpgan_amd import mesh
    p = torch.from_numpy(K.slab(3, 0.3))
    out = {}
    for kernel in mesh.KERNELS:
        m = mesh.surface_mesh(p, K.SPACING, kernel=kernel)
        faces = m.faces.numpy()
        assert faces.shape[0] > 10000 and IR.is_closed_oriented(faces, m.vertices.shape[0]) and mesh.volume(m) > 0.0
        out[kernel] = top_ripple(m)
        print(kernel, "vertices sampled %d, ripple %.4f spacings, mean height %.3f spacings above the top layer" %
              (out[kernel][0], out[kernel][1], out[kernel][2] - 2.0))
    print("ripple ratio %.3f" % (out["anisotropic"][1] / out["isotropic"][1]))
    assert min(out["isotropic"][0], out["anisotropic"][0]) > 500
    assert out["anisotropic"][1] < 0.5 * out["isotropic"][1]


# ---- the isotropic path is the one it was ---------------------------------------------------------------------------------
def test_the_isotropic_mesh_is_density_field_and_iso_surface_called_directly(oracle_cpu, tmp_path, capsys):
    from tpgan_amd import mesh, ops
    small = K.ball(3.3)
    rows = torch.from_numpy(np.concatenate([small, np.full((2, 3), 999.0, F32)]))
    support, step = 2 * K.SPACING, K.SPACING / 2
    lattice = mesh.lattice_for(rows, support, step)
    field = mesh.density_field(rows, lattice, support)
    level = float(F32(0.5 * mesh.lattice_value(K.SPACING, support)))
    v, f, n = ops.iso_surface(field, lattice.origin, lattice.step, level, True)
    for m in (mesh.surface_mesh(rows, K.SPACING), mesh.surface_mesh(rows, K.SPACING, kernel="isotropic", cov_radius=0.3, smooth_lambda=0.1)):
        assert m.lattice.shape == lattice.shape and np.array_equal(m.lattice.origin, lattice.origin) and m.iso == level
        assert np.array_equal(bits(m.vertices), bits(v)) and np.array_equal(bits(m.normals), bits(n)) and torch.equal(m.faces, f)
    np.save(tmp_path / "pcd_0.npy", rows.numpy())
    mesh.main(["--frames", str(tmp_path / "pcd_{i}.npy"), "--count", "1", "--out", str(tmp_path / "m"), "--device", "cpu"])
    record = json.loads(capsys.readouterr().out.strip())
    names, got, faces = M.read_ply(str(tmp_path / "m" / "pcd_0000.ply"))
    assert record["vertices"] == v.shape[0] > 0
    assert np.array_equal(bits(got[:, :3]), bits(v)) and np.array_equal(bits(got[:, 3:]), bits(n)) and np.array_equal(faces, f.numpy())
    wide = mesh.lattice_for(rows, support, step, reach=2 * support)
    assert all(a > b for a, b in zip(wide.shape, lattice.shape))
    with pytest.raises(RuntimeError, match="kernel must be"):
        mesh.surface_mesh(rows, K.SPACING, kernel="ellipsoid")
    with pytest.raises(ValueError, match="kernel must be"):
        mesh.SequenceMesher(str(tmp_path / "x"), kernel="ellipsoid")


def test_cli_and_rollout_write_closed_anisotropic_meshes(tmp_path, capsys, monkeypatch, oracle_cpu):
    from tpgan_amd import mesh
    small = K.ball(3.3)
    np.save(tmp_path / "pcd_0.npy", small)
    out = tmp_path / "meshes"
    common = ["--frames", str(tmp_path / "pcd_{i}.npy"), "--count", "1", "--device", "cpu"]
    mesh.main(common + ["--out", str(out / "iso")])
    mesh.main(common + ["--out", str(out / "aniso"), "--kernel", "anisotropic"])
    mesh.main(common + ["--out", str(out / "half"), "--kernel", "anisotropic", "--smooth_lambda", "0.5", "--cov_radius", "0.08"])
    iso, aniso, half = [json.loads(line) for line in capsys.readouterr().out.strip().split("\n")]
    for name in ("iso", "aniso", "half"):
        names, rows, faces = M.read_ply(str(out / name / "pcd_0000.ply"))
        assert faces.shape[0] > 500 and IR.is_closed_oriented(faces, rows.shape[0])
    direct = mesh.surface_mesh(torch.from_numpy(small), kernel="anisotropic")
    names, rows, faces = M.read_ply(str(out / "aniso" / "pcd_0000.ply"))
    assert np.array_equal(bits(rows[:, :3]), bits(direct.vertices)) and np.array_equal(faces, direct.faces.numpy())
    # the centre smoothing pulls the surface in, less so at a smaller lambda: a knob, not compensated for
    assert 0.0 < aniso["volume"] < half["volume"] < iso["volume"]
    with pytest.raises(SystemExit):
        mesh.main(common + ["--out", str(out / "bad"), "--kernel", "ellipsoid"])
    small, rolled = M._run_rollout(tmp_path, monkeypatch, ["--mesh", str(tmp_path / "rolled"), "--kernel", "anisotropic"])
    assert sorted(os.listdir(tmp_path / "rolled")) == ["pcd_0000.ply", "pcd_0001.ply", "pcd_0002.ply"]
    names, rows, faces = M.read_ply(str(tmp_path / "rolled" / "pcd_0001.ply"))
    assert faces.shape[0] > 500 and IR.is_closed_oriented(faces, rows.shape[0])
    centre = rows[:, :3].astype(np.float64).mean(0)
    assert np.abs(centre - (small.astype(np.float64).mean(0) + 0.01)).max() < 0.01


# ---- the C entries' argument checks: no device is touched -----------------------------------------------------------------
def test_aniso_entries_reject_bad_arguments_before_any_launch(hip_lib):
    buf = (C.c_float * 256)()
    p = C.c_void_p((C.addressof(buf) + 255) & ~255)
    odd = C.c_void_p(p.value + 64)
    nan, inf = float("nan"), float("inf")
    grid_bytes = hip_lib.tpg_frnn_grid_workspace_bytes(2, 1000)
    assert hip_lib.tpg_aniso_workspace_bytes(2, 1000) >= grid_bytes + 80 * 2000
    assert hip_lib.tpg_aniso_workspace_bytes(0, 8) == 0 and hip_lib.tpg_aniso_workspace_bytes(8, 0) == 0

    for fn in (hip_lib.tpg_aniso_kernels_f32, hip_lib.tpg_aniso_kernels_exhaustive_f32):
        def kernels(pos=p, B=1, N=8, rc=0.1, lam=0.9, ks=6.6, kr=4.0, s_min=0.125, s_max=2.0, kn=0.5, n_eps=25, stages=3,
                    centres=p, G=p, det=p, count=p, ws=p):
            return fn(pos, None, B, N, rc, lam, ks, kr, s_min, s_max, kn, n_eps, stages, centres, G, det, count, ws, None)
        assert kernels(B=-1) == -1 and kernels(N=-1) == -1
        assert kernels(rc=0.0) == -1 and kernels(rc=nan) == -1 and kernels(rc=inf) == -1 and kernels(ks=-1.0) == -1
        assert kernels(lam=-0.1) == -1 and kernels(lam=1.5) == -1 and kernels(lam=nan) == -1
        assert kernels(kr=0.5) == -1 and kernels(kr=nan) == -1 and kernels(kr=inf) == -1
        assert kernels(s_min=0.0) == -1 and kernels(s_max=inf) == -1 and kernels(s_min=3.0) == -1 and kernels(kn=0.0) == -1
        assert kernels(n_eps=-1) == -1 and kernels(stages=0) == -1 and kernels(stages=4) == -1
        assert kernels(centres=None) == -1 and kernels(G=None) == -1 and kernels(det=None) == -1 and kernels(count=None) == -1
        assert kernels(ws=None) == -1 and kernels(ws=odd) == -1
        assert kernels(B=0) == 0 and kernels(N=0) == 0 and kernels(N=0, ws=None, pos=None) == 0    # nothing to do
        assert kernels(B=70000) == -3 and kernels(B=70000, ws=None) == -1                           # the argument errors come first
        assert kernels(pos=None) == -1

    def field(fn, ws, query=p, centres=p, G=p, det=p, B=1, Nq=8, Np=8, support=0.05, reach=0.1, out=p):
        args = (query, centres, G, det, None, None, B, Nq, Np, support, reach, out)
        return fn(*args, ws, None) if ws is not False else fn(*args, None)
    for fn, ws in ((hip_lib.tpg_aniso_field_f32, p), (hip_lib.tpg_aniso_field_exhaustive_f32, False)):
        assert field(fn, ws, B=-1) == -1 and field(fn, ws, Nq=-1) == -1 and field(fn, ws, Np=-1) == -1
        assert field(fn, ws, support=0.0) == -1 and field(fn, ws, support=nan) == -1 and field(fn, ws, reach=inf) == -1
        assert field(fn, ws, reach=-1.0) == -1 and field(fn, ws, out=None) == -1
        assert field(fn, ws, B=0) == 0 and field(fn, ws, Nq=0) == 0 and field(fn, ws, Nq=0, query=None) == 0
        assert field(fn, ws, B=70000) == -3
        assert field(fn, ws, query=None) == -1 and field(fn, ws, centres=None) == -1 and field(fn, ws, G=None) == -1
        assert field(fn, ws, det=None) == -1
    assert field(hip_lib.tpg_aniso_field_f32, None) == -1 and field(hip_lib.tpg_aniso_field_f32, odd) == -1
    assert field(hip_lib.tpg_aniso_field_f32, None, Nq=0) == 0
