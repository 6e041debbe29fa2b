"""The signed-distance kernel (csrc/mesh_sdf.hip) against the numpy statement of its rule (tests/mesh_sdf_rule.py), bit
for bit, distances and faces, on the cases of tests/mesh_sdf_cases.py: closest features, the sign's edge cases, the tiling
of faces and queries, and the independence of the answer from the order and the split of the queries."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_sdf_cases as K  # noqa: E402
import mesh_sdf_rule as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def tiling():
    """(F, Q) -> (case, (dist, face) by the rule); the rule runs once per mesh, on the longest stream of queries."""
    cases = K.tiling_cases()
    out = {}
    for F in sorted({f for f, _ in cases}):
        d, face = R.mesh_sdf_rule(**cases[(F, 1000)])
        for (f, Q), c in cases.items():
            if f == F:
                out[(F, Q)] = (c, (d[:Q], face[:Q]))
    return out


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, F32)
    return np.ascontiguousarray(a).view(np.int32)


def _sdf(dev, case, query=None):
    from tpgan_amd import ops
    q = case["query"] if query is None else query
    return ops.mesh_sdf(_up(q, dev), _up(case["vertices"], dev), _up(case["faces"], dev))


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_mesh_sdf_equals_the_rule_distance_bits_and_face(dev, name):
    case = K.CASES[name]()
    wd, wf = R.mesh_sdf_rule(**case)
    d, f = _sdf(dev, case)
    assert d.dtype == torch.float32 and f.dtype == torch.int32 and d.shape == f.shape == (len(case["query"]),)
    assert np.array_equal(_bits(d), _bits(wd)), (name, d.cpu().numpy(), wd)
    assert np.array_equal(f.cpu().numpy(), wf), name


@pytest.mark.parametrize("F", [1, 256, 257, 773])
def test_every_tiling_of_faces_and_queries_equals_the_rule(dev, tiling, F):
    for Q in (1, 255, 256, 257, 1000):
        case, (wd, wf) = tiling[(F, Q)]
        d, f = _sdf(dev, case)
        assert np.array_equal(_bits(d), _bits(wd)) and np.array_equal(f.cpu().numpy(), wf), (F, Q)


def test_another_order_and_another_split_of_the_queries_give_the_same_bits(dev, tiling):
    case, (wd, wf) = tiling[(773, 1000)]
    perm = np.random.default_rng(9).permutation(1000)
    d, f = _sdf(dev, case, case["query"][perm])
    assert np.array_equal(_bits(d), _bits(wd[perm])) and np.array_equal(f.cpu().numpy(), wf[perm])
    parts = [_sdf(dev, case, case["query"][a:b]) for a, b in ((0, 3), (3, 300), (300, 301), (301, 1000))]
    assert np.array_equal(_bits(torch.cat([p[0] for p in parts])), _bits(wd))
    assert np.array_equal(torch.cat([p[1] for p in parts]).cpu().numpy(), wf)


def test_the_torch_statement_on_the_device_equals_the_kernel(dev, tiling):
    from tpgan_amd import ops
    case, (wd, wf) = tiling[(257, 1000)]
    box, inv_unit = ops.mesh_sdf_grid(case["vertices"])
    d, f = ops._mesh_sdf_torch(_up(case["query"], dev), _up(case["vertices"], dev), _up(case["faces"], dev), box, inv_unit)
    assert np.array_equal(_bits(d), _bits(wd)) and np.array_equal(f.cpu().numpy(), wf)


def test_bad_vertex_indices_are_clamped_by_the_kernel_and_refused_by_the_op(dev):
    """The C entry cannot check device faces: the kernel clamps them into [0, V-1] and answers as the rule does on the
    clamped faces.  The op itself refuses them on the host."""
    from tpgan_amd import ops
    case = dict(K.CASES["ray_edge"]())
    bad = case["faces"].copy()
    bad[3] = [-5, 2 ** 30, 7]
    bad[20] = [99, 16, -1]
    with pytest.raises(RuntimeError, match="vertex"):
        _sdf(dev, dict(case, faces=bad))
    be = ops.backend_for(torch.zeros(1, device=dev))
    box, inv_unit = ops.mesh_sdf_grid(case["vertices"])
    d, f = be.mesh_sdf(_up(case["query"], dev), _up(case["vertices"], dev), _up(bad, dev), box, inv_unit)
    wd, wf = R.mesh_sdf_rule(case["query"], case["vertices"], bad)
    assert np.array_equal(_bits(d), _bits(wd)) and np.array_equal(f.cpu().numpy(), wf)
