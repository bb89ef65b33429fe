"""A/B of the fp32 row-band weight-gradient kernel (f32wgrad_t3_kernel) against the generic split-K kernel.

    python tools/f32_wgt3_ab.py RESNET_SIZE POP BATCH STEPS_PER_WINDOW ROUNDS OUT_FILE

Builds the fp32 building-block step plan of one engine eight times -- every width of ``_F32_WGT3``, none (the generic
kernel everywhere), one width removed at a time, and every width with the item target at 256 and 1024 instead of 512
-- and times them in alternating windows of graph replays inside one process (each arm's spread is printed next to its
median).  Appends to OUT_FILE; profiles/f32_wgt3_ab.txt is its output for ResNet-18 and 34.
"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributedtf_amd import ops  # noqa: E402
from distributedtf_amd.engine import hip_imagenet_f32 as h32  # noqa: E402
from distributedtf_amd.models.imagenet_model import ImageNetModel  # noqa: E402
from distributedtf_amd.pbt.cluster import sample_population  # noqa: E402

size, pop, batch, steps, rounds = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
out = open(sys.argv[6], "a")


def say(s):
    print(s, flush=True)
    out.write(s + "\n")
    out.flush()


dev = torch.device("cuda")
hps = sample_population(pop, 2024)
for h in hps:
    h["batch_size"] = batch
members = [ImageNetModel(i, hps[i], "/tmp/ab_savedata/model_", seed=2024, resnet_size=size, resnet_version=2, device=dev,
                         backend="hip", dtype="fp32", loss_scale=None, capacity=pop, use_synthetic_data=True,
                         checkpoint_every_round=False) for i in range(pop)]
eng = members[0].engine
be = eng.backend
assert be.__class__.__name__ == "HipImageNetF32Backend"
ds = members[0].dataset()
slots = [m.slot for m in members]
batches = [ds.batch_slice(batch) for _ in members]


def step():
    return eng.train_step(slots, batches, [m.hparams for m in members],
                          [m.learning_rate(eng.host_step[m.slot]) for m in members])


full, target = {56, 28, 14, 7}, h32._F32_WGT3_TARGET
arms = ([("band", full, target), ("generic", set(), target)] + [("no%d" % w, full - {w}, target) for w in (56, 28, 14, 7)]
        + [("t%d" % t, full, t) for t in (256, 1024)])
plans = {}
for name, table, tgt in arms:
    h32._F32_WGT3, h32._F32_WGT3_TARGET = table, tgt
    be._plans.clear()
    step()
    (key, plan), = be._plans.items()
    cnt = {w: [a[2] for fn, a in plan.launches if not isinstance(fn, str)
               and ops.launcher_name(fn) == "dtf_f32_wgrad_t3" and a[1] == w] for w in (56, 28, 14, 7)}
    say("%-8s band launches per width (items of the first): %s" % (
        name, {w: "%d (%d)" % (len(v), v[0]) if v else "0" for w, v in cnt.items()}))
    plans[name] = plan
    for _ in range(2):
        step()
torch.cuda.synchronize()
times = {a[0]: [] for a in arms}
for r in range(rounds):
    for name, _, _ in arms:
        be._plans.clear()
        be._plans[key] = plans[name]
        step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        times[name].append(ms)
        say("round %d %-8s %9.3f ms/step" % (r, name, ms))
say("ResNet-%d v2 224x224 pop %d x %d fp32, %d steps per window" % (size, pop, batch, steps))
for name, _, _ in arms:
    t = times[name]
    say("%-8s median %9.3f ms/step  spread %9.3f .. %9.3f" % (name, statistics.median(t), min(t), max(t)))
g = statistics.median(times["generic"])
for name, _, _ in arms:
    if name != "generic":
        d = statistics.median(times[name]) - g
        say("%s - generic: %+.3f ms/step (%+.2f %%)" % (name, d, 100 * d / g))
say("")
