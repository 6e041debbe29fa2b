"""ops.replace_dummy_centres without a GPU: the torch statement of the rule (the path backends without the kernel take)
against a numpy restatement of include/tpgan_ops.h written here, the uniformity of its draws, the library's argument
checks, and the trainers' --graph argument rules."""
import ctypes as C

import numpy as np
import pytest
import torch

M = 0xFFFFFFFF


def _mix(h):
    h ^= h >> 16
    h = (h * 0x7FEB352D) & M
    h ^= h >> 15
    h = (h * 0x846CA68B) & M
    return h ^ (h >> 16)


def rule_numpy(xyz, centres, seed, n_iter, site, flag=None):
    """include/tpgan_ops.h, cloud by cloud, python integers: -> (out, short, flag)."""
    B, N, _ = xyz.shape
    S = centres.shape[1]
    out, short = centres.copy(), 0
    flag = None if flag is None else flag.copy()
    seed, n_iter = seed % (1 << 64), n_iter % (1 << 64)                    # two's complement words
    lo = _mix((seed & M) ^ _mix(((n_iter & M) * 0x9E3779B1 + site) & M))
    for b in range(B):
        hit = np.abs(xyz[b, centres[b], 0] - np.float32(999.0)) < np.float32(1e-4)
        k = int(hit.sum())
        if k == 0:
            continue
        pool = [j for j in range(N) if not (j < S and hit[j])]
        if len(pool) < k:
            short = 1
            continue
        hi = _mix((seed >> 32) ^ _mix((b * 0x85EBCA6B + site) & M))
        pool.sort(key=lambda j: (_mix(_mix((j * 0x9E3779B1 + lo) & M) ^ hi), j))
        out[b] = np.concatenate([centres[b][~hit], np.asarray(pool[:k], dtype=np.int32)])
        if flag is not None:
            flag[b] = 0
    return out, short, flag


def cloud(B, N, dummies, seed=0):
    """(B,N,3) fp32 points; rows listed in `dummies[b]` are 999-padding."""
    x = np.random.RandomState(seed).rand(B, N, 3).astype(np.float32)
    for b, rows in enumerate(dummies):
        x[b, list(rows)] = 999.0
    return x


def small_cases():
    """name -> (xyz, centres): the cases the rule distinguishes, N = 32."""
    rs = np.random.RandomState(5)

    def picks(N, S):
        return rs.permutation(N)[:S].astype(np.int32)
    cases = {}
    c = np.stack([picks(32, 8) for _ in range(2)])
    cases["no_hit"] = (cloud(2, 32, [[], []]), c)
    cases["one_hit"] = (cloud(2, 32, [[int(c[0, 3])], []]), c)
    # alternate slots are hits; the rows 8..31 a replacement can come from hold dummies too (a pick may be one)
    c = np.stack([np.arange(8, dtype=np.int32), np.arange(8, dtype=np.int32)[::-1].copy()])
    cases["alternate"] = (cloud(2, 32, [[0, 2, 4, 6, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20], [1, 3, 5, 7]]), c)
    cases["all_dummy_served"] = (cloud(1, 32, [range(32)]), picks(32, 16)[None])          # k = 16 = N - k
    cases["all_dummy_short"] = (cloud(2, 32, [range(32), [3]]), np.stack([picks(32, 32), np.arange(32, dtype=np.int32)]))
    # more centres than points (FPS of a cloud smaller than npoint repeats picks): slots beyond N bar no pool position
    c = np.stack([np.arange(48, dtype=np.int32) % 32, np.full(48, 5, dtype=np.int32)])
    cases["more_centres_than_points"] = (cloud(2, 32, [[1, 40 % 32, 30], [5]]), c)              # k = 5; k = 48 > pool
    return cases


@pytest.mark.parametrize("name", sorted(small_cases()))
def test_torch_statement_matches_the_rule(name):
    import tpgan_amd.ops as ops
    xyz, centres = small_cases()[name]
    B, S = centres.shape
    for seed, n_iter, site in ((0, 12, 0), (7 + (3 << 32), 1 << 33, 5), (-2, 13, 1)):
        flag0 = np.ones(B, dtype=np.int32)
        want, want_short, want_flag = rule_numpy(xyz, centres, seed, n_iter, site, flag0)
        flag = torch.from_numpy(flag0.copy())
        key = torch.tensor([seed, n_iter], dtype=torch.int64)
        got, short = ops._replace_dummy_centres_torch(torch.from_numpy(xyz), torch.from_numpy(centres), key, site, flag)
        assert got.dtype == torch.int32 and tuple(short.shape) == (1,) and short.dtype == torch.int32
        assert np.array_equal(got.numpy(), want), name
        assert int(short) == want_short and np.array_equal(flag.numpy(), want_flag)
        # survivors keep their slot order; the flag is cleared exactly where centres were replaced
        for b in range(B):
            hit = np.abs(xyz[b, centres[b], 0] - 999.0) < 1e-4
            k = int(hit.sum())
            served = 0 < k <= xyz.shape[1] - int(hit[:xyz.shape[1]].sum())
            assert flag[b] == (0 if served else 1)
            if served:
                assert np.array_equal(got[b, :S - k].numpy(), centres[b][~hit])
                tail = got[b, S - k:].numpy()
                assert len(set(tail.tolist())) == k and not any(t < S and hit[t] for t in tail)
            else:
                assert np.array_equal(got[b].numpy(), centres[b])
    assert {"all_dummy_short": 1, "more_centres_than_points": 1}.get(name, 0) == want_short
    if name == "alternate":
        assert any(xyz[0, t, 0] == 999.0 for s in range(64)
                   for t in rule_numpy(xyz, centres, s, 0, 0)[0][0, 4:]), "a pick may itself be a dummy"


def test_public_op_takes_the_torch_statement_on_a_backend_without_the_kernel(oracle_cpu):
    import tpgan_amd.ops as ops
    xyz, centres = small_cases()["alternate"]
    key = torch.tensor([3, 14], dtype=torch.int64)
    got, short = ops.replace_dummy_centres(torch.from_numpy(xyz), torch.from_numpy(centres), key, 2)
    assert np.array_equal(got.numpy(), rule_numpy(xyz, centres, 3, 14, 2)[0]) and int(short) == 0
    with pytest.raises(RuntimeError, match="draw_key"):
        ops.replace_dummy_centres(torch.from_numpy(xyz), torch.from_numpy(centres), key.int(), 2)
    with pytest.raises(RuntimeError, match="site"):
        ops.replace_dummy_centres(torch.from_numpy(xyz), torch.from_numpy(centres), key, -1)


@pytest.mark.parametrize("sweep", ["n_iter", "seed", "site", "b"])
def test_draws_are_uniform_over_the_pool(sweep):
    """One dummy at slot 3 of 8 in a cloud of 32: the replacement is one of the 31 other indices.  3100 draws per sweep,
    100 expected per index; a binomial(3100, 1/31) count has sd 9.8, so 60..145 is -4.1 / +4.6 sd."""
    import tpgan_amd.ops as ops
    draws = 3100
    nb = draws if sweep == "b" else 1
    one = cloud(1, 32, [[20]])
    centres = np.array([[0, 1, 2, 20, 4, 5, 6, 7]], dtype=np.int32)
    xyz = torch.from_numpy(np.repeat(one, nb, 0))
    cen = torch.from_numpy(np.repeat(centres, nb, 0))
    count = np.zeros(32, dtype=np.int64)
    if sweep == "b":
        out, _ = ops._replace_dummy_centres_torch(xyz, cen, torch.tensor([11, 12], dtype=torch.int64), 1)
        count += np.bincount(out[:, 7].numpy(), minlength=32)
    else:
        for i in range(draws):
            seed, n_iter, site = {"n_iter": (11, i, 1), "seed": (i * 2654435761 + 5, 12, 1), "site": (11, 12, i)}[sweep]
            out, _ = ops._replace_dummy_centres_torch(xyz, cen, torch.tensor([seed, n_iter], dtype=torch.int64), site)
            count[int(out[0, 7])] += 1
    print(sweep, "min", count[count > 0].min(), "max", count.max())
    assert count[3] == 0 and count.sum() == draws
    others = np.delete(count, 3)
    assert others.min() >= 60 and others.max() <= 145, (sweep, others.min(), others.max())


def test_entry_rejects_bad_arguments_before_any_launch(hip_lib):
    """Status codes without a device: malformed calls TPG_ERR_ARG (-1), S beyond the LDS sort TPG_ERR_UNSUPPORTED (-3),
    empty work TPG_OK."""
    buf = (C.c_float * 64)()
    p, q = C.cast(buf, C.c_void_p), C.c_void_p(C.addressof(buf) + 128)

    def call(xyz=p, centres=p, key=p, site=0, B=1, N=32, S=8, out=q, flag=None, short=p):
        return hip_lib.tpg_replace_dummy_centres(xyz, centres, key, site, B, N, S, out, flag, short, None)
    assert call(B=0) == 0 and call(S=0) == 0 and call(B=0, xyz=None) == 0
    assert call(B=-1) == -1 and call(N=-1) == -1 and call(S=-1) == -1 and call(site=-1) == -1
    assert call(N=0) == -1
    for name in ("xyz", "centres", "key", "out", "short"):
        assert call(**{name: None}) == -1, name
    assert call(out=p) == -1                                               # out is centres itself
    big = hip_lib.tpg_patch_select_max_k() + 1
    assert call(N=big, S=big) == -3


def _parser_error(main, argv, capsys):
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_both_trainers_take_graph_and_refuse_what_the_captured_step_lacks(capsys):
    from tpgan_amd import train, train_action
    for mod in (train, train_action):
        assert mod.parse_args([]).graph is False and mod.parse_args(["--graph"]).graph is True
        assert "cuda" in _parser_error(mod.parse_args, ["--graph", "--device", "cpu"], capsys)
        assert "velocities" in _parser_error(mod.parse_args, ["--graph", "--in_node_feats", "6"], capsys)
        assert mod.parse_args(["--in_node_feats", "6", "--device", "cpu"]).graph is False        # fine without --graph
    assert "velocities" in _parser_error(train.parse_args, ["--graph", "--use_vel"], capsys)
    assert train.parse_args(["--graph", "--device", "cuda:1"]).device == "cuda:1"
