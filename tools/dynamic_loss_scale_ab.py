"""Cost of dynamic loss scaling on the fp16 CIFAR ResNet HIP step: static scale 128 against ``loss_scale="dynamic"``.

    DTF_HALF=1 python tools/dynamic_loss_scale_ab.py [--pops 1,8] [--resnet_size 56] [--batch 128]
                                                     [--steps 40] [--rounds 6]

Both engines live in one process on one GPU with the same members and batches; timed windows of ``--steps``
graph-replayed steps alternate static / dynamic ``--rounds`` times (host clock around work that ends in a device
synchronise), so drift of a shared box hits both alike.  Dynamic mode adds two small launches and one read of the
gradient rows per step.  Prints per-window times, the medians and the spread of each arm; the members start at
scale 2^7 in both arms, so every step is a clean (updating) step."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def hp(bs):
    return {"opt_case": {"optimizer": "Momentum", "lr": 0.01, "momentum": 0.9}, "batch_size": bs,
            "regularizer": "l2_regularizer", "weight_decay": 1e-4, "initializer": "he_init", "decay_steps": 0,
            "decay_rate": 1.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pops", default="1,8")
    ap.add_argument("--resnet_size", type=int, default=56)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=6)
    args = ap.parse_args()
    from distributedtf_amd import ops
    from distributedtf_amd.engine.population import PopulationEngine
    from distributedtf_amd.models.resnet import ResNetArch, cifar_config
    assert torch.cuda.is_available() and ops.half_mode() and ops.build_half(), "needs a GPU and DTF_HALF=1"
    dev = torch.device("cuda")
    arch = ResNetArch(cifar_config(args.resnet_size, 2))
    for pop in [int(p) for p in args.pops.split(",")]:
        g = torch.Generator().manual_seed(1)
        bs = args.batch
        batches = [(torch.randn(bs, 32, 32, 3, generator=g).to(dev), torch.randint(0, 10, (bs,), generator=g).to(dev))
                   for _ in range(pop)]
        slots, hps, lrs = list(range(pop)), [hp(bs)] * pop, [0.01] * pop
        arms = {}
        for name, ls in (("static", 128.0), ("dynamic", "dynamic")):
            e = PopulationEngine(arch, pop, dev, backend="hip", compute_dtype=torch.float16, loss_scale=ls,
                                 initial_loss_scale=128.0, loss_scale_growth_steps=10 ** 9)
            for i in range(pop):
                e.add_member(None, hp(bs), seed=10 + i)
            for _ in range(5):  # eager warm-up, capture, replays
                e.train_step(slots, batches, hps, lrs)
            arms[name] = e
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for r in range(args.rounds):
            for name in (("static", "dynamic") if r % 2 == 0 else ("dynamic", "static")):
                e = arms[name]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    e.train_step(slots, batches, hps, lrs)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
        skipped = arms["dynamic"].lscale[:, 3].cpu().tolist()
        assert not any(skipped), ("a timed step overflowed", skipped)
        assert torch.isfinite(arms["dynamic"].state).all() and torch.isfinite(arms["static"].state).all()
        med = {k: statistics.median(v) for k, v in times.items()}
        print("resnet%d fp16 pop %d batch %d, %d windows x %d steps, ms/step" % (args.resnet_size, pop, bs, args.rounds,
                                                                                 args.steps))
        for k, v in times.items():
            print("  %-8s median %.3f  min %.3f  max %.3f  windows %s" % (k, med[k], min(v), max(v),
                                                                          " ".join("%.3f" % x for x in v)))
        print("  dynamic / static = %.4f (+%.3f ms/step; images/s %.0f -> %.0f)" % (
            med["dynamic"] / med["static"], med["dynamic"] - med["static"], pop * bs / med["static"] * 1e3,
            pop * bs / med["dynamic"] * 1e3))
        del arms
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
