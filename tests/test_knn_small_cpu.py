"""Argument checks of the small-cloud kNN entry (csrc/knn_small.hpp) return their status codes before any launch."""
import ctypes as C


def test_knn_small_rejects_bad_arguments_before_any_launch(hip_lib):
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    q = C.c_void_p(p.value + 4)                                       # not 16-byte aligned
    # D in {32, 64}, 2 <= K <= 24, P2 <= 1024
    assert hip_lib.tpg_knn_small_f32(p, p, None, None, 1, 8, 8, 48, 4, p, p, 1, None) == -3
    assert hip_lib.tpg_knn_small_f32(p, p, None, None, 1, 8, 8, 32, 25, p, p, 1, None) == -3
    assert hip_lib.tpg_knn_small_f32(p, p, None, None, 1, 8, 1025, 32, 4, p, p, 1, None) == -3
    assert hip_lib.tpg_knn_small_f32(p, p, None, None, 1, 8, 8, 32, 1, p, p, 1, None) == -1
    assert hip_lib.tpg_knn_small_f32(p, None, None, None, 1, 8, 8, 32, 4, p, p, 1, None) == -1
    assert hip_lib.tpg_knn_small_f32(q, p, None, None, 1, 8, 8, 32, 4, p, p, 1, None) == -1
    assert hip_lib.tpg_knn_small_f32(p, p, None, None, 70000, 8, 8, 32, 4, p, p, 1, None) == -1
    assert hip_lib.tpg_knn_small_f32(p, p, None, None, 0, 8, 8, 32, 4, p, p, 1, None) == 0
