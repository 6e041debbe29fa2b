"""Isosurface kernels on the GPU (csrc/isosurface.hip through ops.iso_surface) against the numpy statement of the rule
(tests/iso_rule.py): vertices and normals bit for bit and in order, faces in order after rotating each to its smallest
index first.  Every case asserts that it is not vacuous; equality is over all vertices and faces."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iso_cases as K  # noqa: E402
import iso_rule as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
BIG = (70, 33, 35)


@functools.lru_cache(maxsize=None)
def rule(shape, kind):
    """The rule's mesh of a case, computed once and shared; read-only."""
    out = R.iso_surface(K.field(shape, kind), K.ORIGIN, K.STEP, K.ISO, normals=True)
    for a in out:
        a.setflags(write=False)
    return out


def device_mesh(shape, kind, normals=True):
    from tpgan_amd import ops
    f = torch.from_numpy(K.field(shape, kind)).to(DEV)
    return ops.iso_surface(f, K.ORIGIN, float(K.STEP), float(K.ISO), normals=normals)


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def assert_equals_rule(got, shape, kind, normals=True):
    v, f, n = got
    rv, rf, rn = rule(shape, kind)
    if K.is_empty(shape, kind):
        assert rv.shape[0] == 0 and rf.shape[0] == 0
    else:
        assert rf.shape[0] > 0 and rv.shape[0] > 0, "a vacuous case"
    assert v.dtype == torch.float32 and f.dtype == torch.int32
    assert tuple(v.shape) == rv.shape and tuple(f.shape) == rf.shape, (tuple(v.shape), rv.shape, tuple(f.shape), rf.shape)
    assert np.array_equal(bits(v), bits(rv))
    if normals:
        assert np.array_equal(bits(n), bits(rn))
    else:
        assert n is None
    assert np.array_equal(R.rotate_smallest_first(f.cpu().numpy()), R.rotate_smallest_first(rf))


@pytest.mark.parametrize("kind", K.FIELDS)
@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_equal_the_rule(shape, kind):
    assert_equals_rule(device_mesh(shape, kind), shape, kind)


def test_the_large_lattice_spans_several_scan_workgroups():
    from tpgan_amd import _lib
    nodes = BIG[0] * BIG[1] * BIG[2]
    assert nodes == 80850 and nodes % 2048 != 0 and nodes // 2048 >= 3          # 2048 nodes per scan workgroup
    assert _lib.load().tpg_iso_workspace_bytes(*BIG) >= 10 * nodes
    rv, rf, _ = rule(BIG, "random")
    assert rv.shape[0] > 2 * nodes and rf.shape[0] > 2 * nodes                   # the dense case is dense


@pytest.mark.parametrize("kind", ["random", "planted"])
def test_two_runs_are_equal(kind):
    a, b = device_mesh(BIG, kind), device_mesh(BIG, kind)
    assert a[1].shape[0] > 0
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[2]), bits(b[2]))


@pytest.mark.parametrize("shape", [(9, 7, 5), BIG], ids=lambda s: "x".join(map(str, s)))
def test_without_normals_the_mesh_is_the_same(shape):
    assert_equals_rule(device_mesh(shape, "planted", normals=False), shape, "planted", normals=False)


@pytest.mark.parametrize("shape", [(9, 7, 5), BIG], ids=lambda s: "x".join(map(str, s)))
def test_short_buffers_are_truncated_not_overrun(shape):
    from tpgan_amd import ops
    f = torch.from_numpy(K.field(shape, "random")).to(DEV)
    be = ops.backend_for(f)
    rv, rf, rn = rule(shape, "random")
    ws, V, F = be.iso_count(f, float(K.ISO))
    assert (V, F) == (rv.shape[0], rf.shape[0]) and V > 1 and F > 1
    guard_f, guard_i = 12345.0, -77
    vertices = torch.full((V, 3), guard_f, dtype=torch.float32, device=DEV)     # V - 1 rows and the guard row after them
    nrm = torch.full((V, 3), guard_f, dtype=torch.float32, device=DEV)
    faces = torch.full((F, 3), guard_i, dtype=torch.int32, device=DEV)
    be.iso_emit(f, K.ORIGIN, float(K.STEP), float(K.ISO), ws, V - 1, F - 1, vertices, nrm, faces)
    assert (vertices[V - 1] == guard_f).all() and (nrm[V - 1] == guard_f).all() and (faces[F - 1] == guard_i).all()
    assert np.array_equal(bits(vertices[:V - 1]), bits(rv[:V - 1])) and np.array_equal(bits(nrm[:V - 1]), bits(rn[:V - 1]))
    assert np.array_equal(R.rotate_smallest_first(faces[:F - 1].cpu().numpy()), R.rotate_smallest_first(rf[:F - 1]))


def test_a_small_lattice_after_a_large_one_in_the_same_workspace():
    from tpgan_amd import ops
    assert_equals_rule(device_mesh(BIG, "random"), BIG, "random")
    be = ops.backend_for(torch.zeros(1, device=DEV))
    before = [ws.data_ptr() for key, ws in be._ws.items() if key[0] == "iso"]
    assert before
    for kind in ("spheres", "random"):
        assert_equals_rule(device_mesh((9, 7, 5), kind), (9, 7, 5), kind)
    assert [ws.data_ptr() for key, ws in be._ws.items() if key[0] == "iso"] == before      # the grow-only buffer was reused


def test_surface_mesh_on_the_device_equals_the_cpu_checker(oracle_cpu):
    from tpgan_amd import mesh
    ball = torch.from_numpy(K.lattice_ball(7.8, 0.025))
    assert 1900 <= ball.shape[0] <= 2100
    padded = torch.cat([ball, torch.full((5, 3), 999.0)])                        # the 999 rows of hard masking are dropped
    dev, cpu = mesh.surface_mesh(padded.to(DEV)), mesh.surface_mesh(padded)
    assert dev.lattice.shape == cpu.lattice.shape and np.array_equal(dev.lattice.origin, cpu.lattice.origin)
    assert dev.faces.shape[0] > 1000 and dev.vertices.is_cuda and not cpu.vertices.is_cuda
    assert np.array_equal(bits(dev.vertices), bits(cpu.vertices))
    assert np.array_equal(bits(dev.normals), bits(cpu.normals))
    assert np.array_equal(R.rotate_smallest_first(dev.faces.cpu().numpy()), R.rotate_smallest_first(cpu.faces.numpy()))
    assert abs(mesh.volume(dev) - mesh.volume(cpu)) <= 1e-12 * mesh.volume(cpu) and mesh.volume(dev) > 0.0   # fp64 sums, other order


def test_count_of_a_lattice_without_cells_is_zero(hip_lib):
    counts = torch.full((2,), 7, dtype=torch.int64, device=DEV)
    field = torch.ones(25, device=DEV)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    assert hip_lib.tpg_iso_count_f32(field.data_ptr(), 5, 1, 5, 0.5, None, counts.data_ptr(), stream) == 0
    assert counts.tolist() == [0, 0]
