"""Milliseconds per step of the fluid step at cfg2 shapes when the generator drops slots, on the GPU box:

    python tools/padded_step_time.py --out profiles/padded_step.txt [--append] [--rounds 6] [--steps 10]

Four legs, interleaved round by round in ONE process (same box, same session), every leg on its own copy of the same
initial networks, alternating odd and even iterations over the same four clips:

    (a) all-keep replay   force_all_keep generator, GraphedFluidStep()             -- what bench.py measures
    (b) padded replay     generator dropping 3 % of the low-resolution points by position (synthetic.force_drop_by_x:
                          unequal counts per sample, so hard masking pads with 999), GraphedFluidStep(padded=True)
    (c) fallback          the same generator and batches through GraphedFluidStep(): the replay, the violation, the
                          state restore and then the eager step -- every line of it the code without the padded regime
    (d) eager             the same generator and batches through gan_step.tempo_gan_step alone

A step is timed by the host clock around the call; every leg's call ends in a host synchronisation (the loss report).
Per leg: the median over the rounds of the round's mean, and the smallest and largest round.  The file also says how many
of (b)'s steps replayed and how many of (c)'s fell back, and the two ratios (b) / (c) and (b) / (a).
"""
import argparse
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True)
    ap.add_argument("--append", action="store_true", help="add this box's block to the file (box-to-box spread)")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10, help="steps per leg and round")
    ap.add_argument("--drop", type=float, default=0.03, help="share of the low-resolution points dropped by position")
    opt = ap.parse_args(argv)

    import torch

    import tpgan_amd  # noqa: F401
    from tpgan_amd import configs
    from tpgan_amd.gan_step import tempo_gan_step
    from tpgan_amd.gan_step_graph import GraphedFluidStep
    from tpgan_amd.synthetic import force_drop_by_x
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    torch.backends.cudnn.enabled = False
    dev = torch.device("cuda", 0)
    amp = torch.bfloat16
    clips = [configs.make_clip("cfg2", seed=1234 + i, device=dev) for i in range(4)]
    thr = float(torch.quantile(clips[0][0][1][0][:, 0], opt.drop))
    kept = [(c[0][1][:, :, 0] > thr).sum(1).tolist() for c in clips]

    def models(drop):
        G, Ds, Dt, opts = configs.build_models("cfg2", dev, seed=1, capturable=True)
        return (force_drop_by_x(G, thr) if drop else G), Ds, Dt, opts

    def stepper(m, padded):
        G, Ds, Dt, opts = m
        return GraphedFluidStep(G, Ds, Dt, opts, configs.FLUID_OPT, clips[0][0], clips[0][1], 1.0, amp, None, padded=padded,
                                draw_seed=1)
    ma, mb, mc, md = models(False), models(True), models(True), models(True)
    sa, sb, sc = stepper(ma, False), stepper(mb, True), stepper(mc, False)

    def eager(low, high, n_iter):
        G, Ds, Dt, (og, ot, os_) = md
        return tempo_gan_step(G, Ds, Dt, low, None, high, None, 1.0, configs.FLUID_OPT, n_iter, og, ot, os_, amp_dtype=amp)
    legs = [("a all-keep replay", sa), ("b padded replay", sb), ("c fallback", sc), ("d eager", eager)]
    times = {name: [] for name, _ in legs}
    gate_open = {name: 0 for name, _ in legs}
    n_iter = 12
    for r in range(opt.rounds + 1):                    # round 0 warms every leg up and is not counted
        for name, fn in legs:
            configs.seed_host_rng(100 + r)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for i in range(opt.steps):
                low, high = clips[(n_iter + i) % len(clips)]
                losses = fn(low, high, n_iter + i)
                gate_open[name] += int(r > 0 and losses["masking_loss"] < 0.1)
            torch.cuda.synchronize(dev)
            if r > 0:
                times[name].append(1e3 * (time.perf_counter() - t0) / opt.steps)
        n_iter += opt.steps
    counted = opt.rounds * opt.steps
    med = {name: statistics.median(v) for name, v in times.items()}
    lines = [f"# box {socket.gethostname()}: {torch.cuda.get_device_name(dev)}, torch {torch.__version__}",
             f"# cfg2 shapes (batch 8, 4096 points, 3 frames, bf16), {opt.rounds} rounds x {opt.steps} steps per leg, legs "
             f"interleaved; {opt.drop:.0%} of the low-resolution points dropped by position",
             f"# kept of 512 per sample, centre frame of the four clips: {kept}",
             "# leg                    ms/step median   min .. max over the rounds   steps with the gate open"]
    for name, _ in legs:
        v = times[name]
        lines.append(f"{name:<24} {med[name]:>14.2f}   {min(v):>6.2f} .. {max(v):<6.2f}   {gate_open[name]:>8d} of {counted}")
    fell_back = counted + opt.steps - sc.replays
    lines += [f"(b) replayed {sb.replays} of {counted + opt.steps} steps (warm-up round included); "
              f"(c) fell back on {fell_back} of {counted + opt.steps}; (a) replayed {sa.replays}",
              f"(b) / (c) = {med['b padded replay'] / med['c fallback']:.3f}    "
              f"(b) / (a) = {med['b padded replay'] / med['a all-keep replay']:.3f}    "
              f"(c) / (d) = {med['c fallback'] / med['d eager']:.3f}", ""]
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "a" if opt.append else "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
