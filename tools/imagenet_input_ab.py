"""Cost of the on-device ImageNet input path: the ResNet-50 HIP step fed the fixed synthetic batch against the same
step fed dataset rows (gather + random-resized crop + resample inside the captured graph, data.hip).

    python tools/imagenet_input_ab.py [--pop 8] [--batch 128] [--image 224] [--side 256] [--steps 10] [--rounds 6]
                                      [--one_step rows|synthetic]

One engine on one GPU holds both plans (the members' weights move, the work per step does not); timed windows of
``--steps`` graph-replayed steps alternate synthetic / rows ``--rounds`` times (host clock around work that ends in a
device synchronise), so drift of a shared box hits both alike.  Prints per-window times, the median and the spread
(min .. max) of each arm.  ``--one_step``: warm up, then run three replays of one arm and exit -- the body of a
kernel-trace run (``rocprofv3 --kernel-trace --stats -- python tools/imagenet_input_ab.py --one_step rows``)."""
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
    ap.add_argument("--pop", type=int, default=8)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--image", type=int, default=224)
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--rows", type=int, default=2048, help="images of the learnable set")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--one_step", default=None, choices=["rows", "synthetic"])
    args = ap.parse_args()
    from distributedtf_amd.data import datasets
    from distributedtf_amd.engine.population import PopulationEngine
    from distributedtf_amd.models.resnet import ResNetArch, imagenet_config
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda")
    pop, bs, H = args.pop, args.batch, args.image
    trx, tr_y, tex, te_y = datasets.learnable_imagenet(n_train=args.rows, n_test=8, side=args.side, num_classes=10)
    ds = datasets.DeviceDataset(trx, tr_y, tex, te_y, dev, augment=datasets.augment_imagenet,
                                eval_transform=datasets.eval_imagenet, out_size=H)
    syn = datasets.SyntheticDataset((H, H, 3), 10, dev, max_batch=bs, n_eval=8)
    e = PopulationEngine(ResNetArch(imagenet_config(50, 2, num_classes=10, image_size=H)), pop, dev, backend="hip")
    for i in range(pop):
        e.add_member(None, hp(bs), seed=i)
    slots, hps, lrs = list(range(pop)), [hp(bs)] * pop, [0.01] * pop
    g = torch.Generator(device=dev).manual_seed(1)

    def step(arm):
        if arm == "rows":
            b = [datasets.IndexBatch(ds, torch.randint(0, ds.num_train, (bs,), device=dev, generator=g))
                 for _ in slots]
        else:
            b = [syn.batch_slice(bs) for _ in slots]
        return e.train_step(slots, b, hps, lrs)

    arms = ("synthetic", "rows")
    for arm in arms if args.one_step is None else (args.one_step,):
        for _ in range(3):  # eager warm-up + capture, then replays
            step(arm)
    torch.cuda.synchronize()
    if args.one_step:
        for _ in range(3):
            loss = step(args.one_step)
        torch.cuda.synchronize()
        print("one_step %s: losses %s" % (args.one_step, [round(float(v), 3) for v in loss.cpu()]))
        return
    times = {a: [] for a in arms}
    for r in range(args.rounds):
        for arm in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss = step(arm)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            times[arm].append(ms)
            print("round %d %-9s %8.3f ms/step" % (r, arm, ms), flush=True)
    assert bool(torch.isfinite(loss).all()), loss
    print("pop %d x %d, image %d, stored side %d, %d steps per window" % (pop, bs, H, args.side, args.steps))
    for arm in arms:
        t = times[arm]
        print("%-9s median %8.3f ms/step  spread %8.3f .. %8.3f" % (arm, statistics.median(t), min(t), max(t)))
    d = statistics.median(times["rows"]) - statistics.median(times["synthetic"])
    print("rows - synthetic: %+.3f ms/step (%+.2f %%)" % (d, 100 * d / statistics.median(times["synthetic"])))


if __name__ == "__main__":
    main()
