"""The one-sweep matrix-core kNN for small feature-space clouds (csrc/knn_small.hpp) against the query-tiled exhaustive
kernel, kernel alone: hipGraph replay of `reps` launches, both kernels in one process, alternating, `rounds` timings
each; every shape is also checked bit-equal between the two.  See tools/tune_knn.py.

    python tools/tune_knn_small.py build               # here: csrc/variants/knn_small.so, knn_tiled.so
    python tools/tune_knn_small.py run [reps] [rounds] # GPU box

The dispatch bounds TPG_KNN_SMALL_MIN_POINTS / TPG_KNN_SMALL_MAX_POINTS (csrc/knn.hip) go where `small` wins by more than
the spread (max - min) of the repeated timings of either kernel at that shape; profiles/knn_small.txt is this output.
"""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "temporal-pointcloud-upsampling-gan_amd", "csrc")
VDIR = os.path.join(CSRC, "variants")
VARIANTS = {"small": {}, "tiled": {"TPG_KNN_NO_SMALL": 1}}
# (B, P, D, K): the generator's feature-space searches at cfg2 (tools/tune_knn.py) and cfg4, then the sweep
SHAPES = [(24, 512, 64, 12), (24, 512, 64, 4), (24, 512, 32, 20), (24, 512, 32, 9), (8, 512, 64, 12),
          (64, 512, 64, 12), (64, 512, 64, 4), (64, 512, 32, 20), (64, 512, 32, 9)]
SWEEP = [(24, P, D, K) for P in (128, 256, 512, 1024, 1536) for D in (32, 64) for K in (4, 12, 20)]
SMALL_MAX_P = 1024        # KS_MAX_P2: beyond it the kernel's distance matrix does not fit the LDS


def build():
    os.makedirs(VDIR, exist_ok=True)
    for tag, defs in VARIANTS.items():
        out = os.path.join(VDIR, f"knn_{tag}.so")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize",
                               "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include")] +
                              [f"-D{k}={v}" for k, v in defs.items()] + [os.path.join(CSRC, "knn.hip"), "-o", out])
        print("built", out)


def run(reps, rounds):
    import torch
    P_, I, F = C.c_void_p, C.c_int, C.c_float
    dev = torch.device("cuda", 0)
    libs = {}
    for tag in VARIANTS:
        libs[tag] = C.CDLL(os.path.join(VDIR, f"knn_{tag}.so"))
        libs[tag].tpg_knn_f32.argtypes = [P_, P_, P_, P_, I, I, I, I, I, F, P_, P_, P_]
    libs["small"].tpg_knn_small_f32.argtypes = [P_, P_, P_, P_, I, I, I, I, I, P_, P_, I, P_]
    print("us per search: hipGraph replay of %d launches, %d alternating timings each (min .. max)" % (reps, rounds))
    print("%-22s %-26s %-26s %8s %8s %6s" % ("B P D K", "tiled", "small (filter + redo)", "speed-up", "open %", "equal"))
    for (B, P, D, K) in SHAPES + SWEEP:
        x = [torch.randn(B, P, D, device=dev) for _ in range(4)]
        out = {t: (torch.empty(B, P, K, device=dev), torch.empty(B, P, K, device=dev, dtype=torch.int64)) for t in VARIANTS}

        def go(tag, t, st, redo=1):
            dist, idx = out[tag]
            if tag == "small":        # the path itself, whatever the dispatch bounds of this build are
                rc = libs[tag].tpg_knn_small_f32(t.data_ptr(), t.data_ptr(), None, None, B, P, P, D, K, dist.data_ptr(),
                                                 idx.data_ptr(), redo, st)
            else:
                rc = libs[tag].tpg_knn_f32(t.data_ptr(), t.data_ptr(), None, None, B, P, P, D, K, -1.0, dist.data_ptr(),
                                           idx.data_ptr(), st)
            assert rc == 0, (tag, rc)
        tags = ["tiled"] + (["small"] if P <= SMALL_MAX_P else [])
        graphs = {}
        for tag in tags:
            go(tag, x[0], torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                cs = torch.cuda.current_stream().cuda_stream
                for i in range(reps):
                    go(tag, x[i % 4], cs)
            g.replay()
            torch.cuda.synchronize()
            graphs[tag] = g
        times = {tag: [] for tag in tags}
        for _ in range(rounds):
            for tag in tags:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); graphs[tag].replay(); e1.record()
                torch.cuda.synchronize()
                times[tag].append(e0.elapsed_time(e1) * 1e3 / reps)
        cell = {tag: "%7.1f (%6.1f .. %6.1f)" % (sorted(v)[len(v) // 2], min(v), max(v)) for tag, v in times.items()}
        if "small" not in tags:
            print("%-22s %-26s %-26s" % (f"{B} {P} {D} {K}", cell["tiled"], "n/a: above 1024 points"))
            continue
        for tag in tags:
            go(tag, x[0], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        same = torch.equal(out["small"][0], out["tiled"][0]) and torch.equal(out["small"][1], out["tiled"][1])
        go("small", x[0], torch.cuda.current_stream().cuda_stream, redo=0)
        torch.cuda.synchronize()
        open_ = (out["small"][1][:, :, 0] == -2).float().mean().item() * 100
        med = {tag: sorted(v)[len(v) // 2] for tag, v in times.items()}
        print("%-22s %-26s %-26s %7.2fx %8.2f %6s" % (f"{B} {P} {D} {K}", cell["tiled"], cell["small"],
                                                     med["tiled"] / med["small"], open_, same), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        build()
    else:
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 20, int(sys.argv[3]) if len(sys.argv) > 3 else 5)
