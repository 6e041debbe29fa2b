"""Anisotropic kernels on the GPU (csrc/aniso.hip through ops.anisotropic_kernels / ops.anisotropic_field) against the
numpy statement of the rule (tests/aniso_rule.py): centres, G, det, counts and field bit for bit, from the grid entry and
from the exhaustive entry, on every case: both sides use the same fp32 membership, so no case is excluded."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aniso_cases as K  # noqa: E402
import aniso_rule as R  # noqa: E402
import iso_rule as IR  # noqa: E402
from test_aniso_cpu import N_EPS, bits, default_ks, queries, rule_field, rule_kernels  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
F32 = np.float32


def device_kernels(x, name=None, grid=None, lengths=None):
    from tpgan_amd import ops
    return ops.anisotropic_kernels(torch.as_tensor(x).to(DEV), K.RC, default_ks(), n_eps=N_EPS.get(name, 25), lengths=lengths,
                                   _grid=grid)


def device_field(q, kernels, grid=None, **kw):
    from tpgan_amd import ops
    c, G, d = kernels[:3]
    return ops.anisotropic_field(torch.as_tensor(q).to(DEV), c, G, d, K.SUPPORT, _grid=grid, **kw)


def assert_kernels_equal(got, want):
    for g, w, what in zip(got, want, ("centres", "G", "det")):
        assert g.dtype == torch.float32 and tuple(g.shape) == w.shape, what
        assert np.array_equal(bits(g), bits(w)), what
    assert got[3].dtype == torch.int32 and np.array_equal(got[3].cpu().numpy(), want[3]), "count"


@pytest.mark.parametrize("grid", [False, True], ids=["exhaustive", "grid"])
@pytest.mark.parametrize("name", K.CLOUDS)
def test_kernels_and_field_equal_the_rule(name, grid):
    """Clouds of 1, 2, 63, 64, 65 and 257 points (the 64-candidate step's edges), the sheet, the row, the coincident
    cluster, the 2 000-particle ball, and two clusters 100 reaches apart (the 64-cells cap sets the cell edge); the
    queries hold a (9,7,5) lattice, a point far outside the grid and a NaN."""
    want = rule_kernels(name)
    assert want[3].min() >= 1 and np.isfinite(want[1]).all()
    got = device_kernels(K.cloud(name), name, grid)
    assert_kernels_equal(got, want)
    f = device_field(queries(name), got, grid)
    rf = rule_field(name)
    assert rf.max() > 0.4 and rf[-1] == 0.0 and rf[-2] == 0.0
    assert f.dtype == torch.float32 and np.array_equal(bits(f), bits(rf))


def test_a_ragged_batch_with_an_empty_cloud():
    names = ["random257", "one", "random65"]
    batch = np.full((3, 257, 3), 7.0, F32)                                         # the rows beyond a length are never read
    for b, name in enumerate(names):
        batch[b, :K.cloud(name).shape[0]] = K.cloud(name)
    lengths = torch.tensor([257, 0, 65], device=DEV)
    q = queries("random257")
    for grid in (False, True):
        got = device_kernels(batch, grid=grid, lengths=lengths)
        for b, name in ((0, "random257"), (2, "random65")):
            want = rule_kernels(name)
            m = want[3].shape[0]
            assert_kernels_equal([t[b, :m] for t in got], want)
            assert all(float(t[b, m:].abs().sum()) == 0.0 for t in got)
        assert all(float(t[1].abs().sum()) == 0.0 for t in got)
        f = device_field(np.stack([q, q, q]), got, grid, lengths_q=torch.tensor([q.shape[0], 9, 4], device=DEV), lengths_p=lengths)
        assert np.array_equal(bits(f[0]), bits(rule_field("random257"))) and float(f[1].abs().sum()) == 0.0
        c, G, d, _ = rule_kernels("random65")
        assert np.array_equal(bits(f[2, :4]), bits(R.field(q[:4], c, G, d, K.SUPPORT, K.REACH))) and float(f[2, 4:].abs().sum()) == 0.0


def test_two_runs_are_equal_and_the_grid_equals_the_exhaustive_entry():
    x = K.cloud("ball")
    q = queries("ball")
    runs = [device_kernels(x, grid=g) for g in (True, True, False)]
    for other in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], other))
    fields = [device_field(q, runs[0], g) for g in (True, True, False)]
    assert float(fields[0].max()) > 1.0 and torch.equal(fields[0], fields[1]) and torch.equal(fields[0], fields[2])
    assert np.array_equal(bits(fields[0]), bits(fields[2]))


def test_the_walk_and_the_finish_as_calls_of_their_own_equal_one_call():
    from tpgan_amd import ops
    x = torch.from_numpy(K.cloud("ball")).to(DEV).unsqueeze(0)
    be = ops.backend_for(x)
    prm = ops._aniso_params(K.RC, default_ks(), 0.9, 4.0, 0.125, 2.0, 0.5, 25)
    for grid in (True, False):
        out = be.aniso_kernels(x, None, prm, grid)
        for t in out:
            t.fill_(-3)
        be.aniso_kernels(x, None, prm, grid, stages=1, out=out)
        assert float(out[2].max()) == -3.0 and int(out[3].min()) >= 1               # the walk writes the counts only
        be.aniso_kernels(x, None, prm, grid, stages=2, out=out)
        assert_kernels_equal([t[0] for t in out], rule_kernels("ball"))


def test_a_small_cloud_after_a_large_one_in_the_same_workspace():
    from tpgan_amd import ops
    assert_kernels_equal(device_kernels(K.cloud("ball"), grid=True), rule_kernels("ball"))
    be = ops.backend_for(torch.zeros(1, device=DEV))
    before = [ws.data_ptr() for key, ws in be._ws.items() if key[0] == "aniso"]
    assert before
    for name in ("random65", "pair"):
        got = device_kernels(K.cloud(name), name, True)
        assert_kernels_equal(got, rule_kernels(name))
        assert np.array_equal(bits(device_field(queries(name), got, True)), bits(rule_field(name)))
    assert [ws.data_ptr() for key, ws in be._ws.items() if key[0] == "aniso"] == before     # the grow-only buffer was reused


def test_rows_at_999_are_dropped_by_the_mesher():
    from tpgan_amd import mesh
    x = K.cloud("random257")
    rows = np.concatenate([x[:100], np.full((3, 3), 999.0, F32), x[100:], np.full((2, 3), 999.0, F32)])
    lattice = mesh.Lattice(np.array([0.03, 0.04, 0.05], F32), float(F32(0.0125)), (9, 7, 5))
    got = mesh.anisotropic_field(torch.from_numpy(rows).to(DEV), lattice, K.SPACING, K.SUPPORT)
    c, G, d, _ = rule_kernels("random257")
    nodes = mesh.lattice_nodes(lattice, 0, 9 * 7 * 5, "cpu").numpy()
    want = R.field(nodes, c, G, d, K.SUPPORT, K.REACH)
    assert want.max() > 1.0 and tuple(got.shape) == (9, 7, 5) and np.array_equal(bits(got.reshape(-1)), bits(want))


def test_a_lattice_of_queries_that_spans_several_workgroups():
    """67 240 nodes: more than NODES_PER_CALL / 64, 16 810 workgroups of four queries, around the 257 centres (which the
    smoothing has drawn towards the middle of their small box: the outer nodes are beyond every reach)."""
    from tpgan_amd import mesh
    shape = (41, 41, 40)
    assert shape[0] * shape[1] * shape[2] > mesh.NODES_PER_CALL // 64
    lattice = mesh.Lattice(np.array([-0.005, -0.004, -0.003], F32), float(F32(0.004)), shape)
    nodes = mesh.lattice_nodes(lattice, 0, shape[0] * shape[1] * shape[2], "cpu").numpy()
    c, G, d, _ = rule_kernels("random257")
    want = R.field(nodes, c, G, d, K.SUPPORT, K.REACH)
    assert (want > 0).sum() > 20000 and (want == 0).sum() > 5000
    kernels = device_kernels(K.cloud("random257"))
    for grid in (True, False):
        assert np.array_equal(bits(device_field(nodes, kernels, grid)), bits(want))


def test_surface_mesh_on_the_device_equals_the_cpu_checker(oracle_cpu):
    from tpgan_amd import mesh
    ball = torch.from_numpy(K.cloud("ball"))
    assert 1900 <= ball.shape[0] <= 2100
    padded = torch.cat([ball, torch.full((5, 3), 999.0)])
    dev, cpu = (mesh.surface_mesh(p, kernel="anisotropic") for p in (padded.to(DEV), padded))
    assert dev.lattice.shape == cpu.lattice.shape and np.array_equal(dev.lattice.origin, cpu.lattice.origin)
    assert dev.faces.shape[0] > 1000 and dev.vertices.is_cuda and not cpu.vertices.is_cuda
    assert np.array_equal(bits(dev.vertices), bits(cpu.vertices)) and np.array_equal(bits(dev.normals), bits(cpu.normals))
    assert np.array_equal(IR.rotate_smallest_first(dev.faces.cpu().numpy()), IR.rotate_smallest_first(cpu.faces.numpy()))
    assert IR.is_closed_oriented(cpu.faces.numpy(), cpu.vertices.shape[0]) and mesh.volume(dev) > 0.0
