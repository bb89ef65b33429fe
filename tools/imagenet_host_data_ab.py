"""Cost of training the ImageNet family from a host-resident set: the ResNet-50 HIP step fed rows of a set that lives
on the device (arm ``device``) against the same step fed the same kind of rows of a set that lives on the host, with
the next step's rows staged while the step runs (arm ``host``) and with every step's rows staged when they are asked
for (arm ``host_sync``, ``HostFeed.prefetch = False``).

    python tools/imagenet_host_data_ab.py [--pop 8] [--batch 128] [--image 224] [--side 256] [--rows 4096]
                                          [--steps 10] [--rounds 6] [--arms device,host,host_sync]

One engine on one GPU holds the plans (the members' weights move, the work per step does not); timed windows of
``--steps`` graph-replayed steps alternate between the arms ``--rounds`` times (host clock around work that ends in a
device synchronise), so drift of a shared box hits all alike.  Prints per-window times, the median and the spread
(min .. max) of each arm, how far the host had run ahead of the device at the end of a window, the host time spent
inside ``HostFeed.begin`` per step, and -- measured on their own, with no step running -- the time to gather one
step's rows into the pinned buffer and the time of its host-to-device copy.  ``--arms device`` runs on a tree without
the host set too (the parent of the change that added it), which is how the two ``device`` lines are compared."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
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
    ap.add_argument("--rows", type=int, default=4096, help="images of the synthetic uint8 set")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--arms", default="device,host,host_sync")
    args = ap.parse_args()
    from distributedtf_amd.data import datasets
    from distributedtf_amd.engine.population import PopulationEngine
    from distributedtf_amd.models.resnet import ResNetArch, imagenet_config
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda")
    pop, bs, H = args.pop, args.batch, args.image
    arms = tuple(args.arms.split(","))
    assert set(arms) <= {"device", "host", "host_sync"}
    rs = np.random.default_rng(0)
    trx = rs.integers(0, 256, (args.rows, args.side, args.side, 3), dtype=np.uint8)
    tr_y = rs.integers(0, 10, (args.rows,), dtype=np.int64)
    sets = {}
    if "device" in arms:
        sets["device"] = datasets.DeviceDataset(trx, tr_y, trx[:8], tr_y[:8], dev, augment=datasets.augment_imagenet,
                                                eval_transform=datasets.eval_imagenet, out_size=H)
    if "host" in arms or "host_sync" in arms:
        sets["host"] = sets["host_sync"] = datasets.HostImageNetDataset(trx, tr_y, trx[:8], tr_y[:8], dev, out_size=H)
    e = PopulationEngine(ResNetArch(imagenet_config(50, 2, num_classes=10, image_size=H)), pop, dev, backend="hip")
    for i in range(pop):
        e.add_member(None, hp(bs), seed=i)
    slots, hps, lrs = list(range(pop)), [hp(bs)] * pop, [0.01] * pop
    g = torch.Generator(device=dev).manual_seed(1)
    gc = torch.Generator().manual_seed(1)
    ahead = {}

    def draw():
        return [torch.randint(0, args.rows, (bs,), generator=gc) for _ in slots]

    def step(arm):
        ds = sets[arm]
        if arm == "device":
            b = [datasets.IndexBatch(ds, torch.randint(0, ds.num_train, (bs,), device=dev, generator=g))
                 for _ in slots]
        else:
            ds.feed.prefetch = arm == "host"
            cur = ahead.pop("rows", None) or draw()
            ahead["rows"] = nxt = draw()  # every step announces the rows of the next one rightly
            b = [datasets.IndexBatch(ds, i, next_rows=n) for i, n in zip(cur, nxt)]
        return e.train_step(slots, b, hps, lrs)

    for arm in arms:
        ahead.clear()
        for _ in range(3):  # eager warm-up + capture, then replays
            step(arm)
    torch.cuda.synchronize()
    times = {a: [] for a in arms}
    drain = {a: [] for a in arms}  # host clock from the last enqueue to the end of the device's work
    begin_s = {a: [] for a in arms}  # host time inside HostFeed.begin per step (staging a step when asked for, waits)
    if "host" in sets:
        feed0 = sets["host"].feed
        inner, spent = feed0.begin, [0.0]

        def timed_begin(rows):
            t = time.perf_counter()
            try:
                return inner(rows)
            finally:
                spent[0] += time.perf_counter() - t

        feed0.begin = timed_begin
    for r in range(args.rounds):
        for arm in arms:
            ahead.clear()
            step(arm)  # the window starts in the arm's steady state (its first step is staged when asked for)
            torch.cuda.synchronize()
            if arm != "device":
                spent[0] = 0.0
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss = step(arm)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            ms = (t2 - t0) * 1e3 / args.steps
            times[arm].append(ms)
            drain[arm].append((t2 - t1) * 1e3)
            if arm != "device":
                begin_s[arm].append(spent[0] * 1e3 / args.steps)
            print("round %d %-9s %8.3f ms/step, device still busy %8.3f ms after the last enqueue"
                  % (r, arm, ms, (t2 - t1) * 1e3), flush=True)
    assert bool(torch.isfinite(loss).all()), loss
    print("pop %d x %d, image %d, stored side %d, set of %d images, %d steps per window, torch threads %d"
          % (pop, bs, H, args.side, args.rows, args.steps, torch.get_num_threads()))
    for arm in arms:
        t = times[arm]
        print("%-9s median %8.3f ms/step  spread %8.3f .. %8.3f" % (arm, statistics.median(t), min(t), max(t)))
    med = {a: statistics.median(times[a]) for a in arms}
    for arm in arms:  # how far the host runs ahead: the device's backlog when the host has enqueued the window
        d = statistics.median(drain[arm])
        line = "%-9s host ahead of the device by %8.3f ms (%.1f steps) at the end of a window" % (arm, d, d / med[arm])
        if begin_s[arm]:
            line += "; %.3f ms/step of host time inside HostFeed.begin" % statistics.median(begin_s[arm])
        print(line)
    if "host" in arms:
        feed = sets["host"].feed
        st = feed.stager
        print("host feed: %d steps served from the prefetched half, %d staged when asked for; staging %.1f MB in %d "
              "gather threads" % (feed.hits, feed.syncs, st.nbytes / 1e6, len(st._threads)))
        gather, copy = [], []
        for i in range(8):  # on their own: nothing else runs
            rows = np.concatenate([t.numpy() for t in draw()])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st.stage(rows, i & 1)
            st.wait_issued(i & 1)
            t1 = time.perf_counter()
            st.copied[i & 1].synchronize()
            t2 = time.perf_counter()
            gather.append((t1 - t0) * 1e3)
            copy.append((t2 - t1) * 1e3)
        mb = pop * bs * args.side * args.side * 3 / 1e6
        print("gather of one step's rows (%.1f MB): median %8.3f ms  spread %8.3f .. %8.3f  (%.1f GB/s)"
              % (mb, statistics.median(gather), min(gather), max(gather), mb / statistics.median(gather)))
        print("host-to-device copy of them:        median %8.3f ms  spread %8.3f .. %8.3f  (%.1f GB/s)"
              % (statistics.median(copy), min(copy), max(copy), mb / statistics.median(copy)))
        if "device" in arms:
            print("host - device: %+.3f ms/step (%+.2f %%)"
                  % (med["host"] - med["device"], 100 * (med["host"] - med["device"]) / med["device"]))
        if "host_sync" in arms:
            print("host_sync - host: %+.3f ms/step (gather + copy %.3f ms, step %.3f ms)"
                  % (med["host_sync"] - med["host"], statistics.median(gather) + statistics.median(copy),
                     med.get("device", med["host"])))
        sets["host"].close()


if __name__ == "__main__":
    main()
