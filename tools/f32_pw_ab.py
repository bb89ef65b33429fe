"""A/B of the fp32 pointwise kernel (f32conv_pw_kernel) against the generic fp32 conv kernel on the stride-1 1x1 convs.

    python tools/f32_pw_ab.py RESNET_SIZE POP BATCH STEPS_PER_WINDOW ROUNDS OUT_FILE
    python tools/f32_pw_ab.py --trace KERNEL_TRACE_CSV RESNET_SIZE POP BATCH OUT_FILE

First form: builds the fp32 bottleneck step plan of one engine three times -- the plan's routing, every stride-1 1x1
data gradient routed as well (``_F32_PW_DGRAD_MIN_K`` = 0), and ``_F32_PW`` off -- and times them in alternating
windows of graph replays inside one process (each arm's spread is printed next to its median).  Second form: reads the
kernel trace of a run of its own (rocprofv3 --kernel-trace, no counters, of bench.py --model imagenet --dtype fp32 at
the same population and batch, under the DTF_F32_PW of this call), pairs the conv dispatches of its last step with the
plan's launch list in order, and prints per class (launcher, kernel size, stride, direction) its share of the step's
kernel time and, per stride-1 1x1 layer shape, the time per launch with the FLOP/s and HBM bytes/s it implies (FLOP =
2 Ci Co pixels; bytes = operand + output [+ residual, mask source] + weights, each once).  Both append to OUT_FILE;
profiles/f32_pw_ab.txt is their output for ResNet-50.
"""
import collections
import csv
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

argv = sys.argv[1:]
trace = argv[1] if argv[0] == "--trace" else None
if trace:
    argv = argv[2:]
size, pop, batch = int(argv[0]), int(argv[1]), int(argv[2])
out = open(argv[-1], "a")
CONVS = ("dtf_f32_conv", "dtf_f32_conv_pw", "dtf_f32_conv_t3")


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


def conv_launches(plan):
    """(launcher, kh, stride, dgrad, Ci, Co, pixels, epi) of every forward / data-gradient conv launch, in order."""
    rows = []
    for fn, a in plan.launches:
        name = None if isinstance(fn, str) else ops.launcher_name(fn)
        if name in CONVS:
            g = a[0]._obj
            epi, dgrad = (a[3], a[4]) if name == "dtf_f32_conv" else (a[2], a[3])
            rows.append((name, g.kh, g.stride, int(dgrad), g.Ci, g.Co, plan.N * g.Ho * g.Wo, epi))
    return rows


if trace:
    step()
    (key, plan), = be._plans.items()
    rows = conv_launches(plan)
    with open(trace) as f:
        disp = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
    conv_d = [r for r in disp if "f32conv_" in r["Kernel_Name"] and "wgrad" not in r["Kernel_Name"]]
    steps = len(conv_d) / len(rows)
    assert steps >= 1 and steps == int(steps), "the trace holds %d conv dispatches, a step has %d" % (len(conv_d), len(rows))
    last = conv_d[-len(rows):]  # the last step's conv dispatches, in the launch list's order
    assert all(("f32conv_pw" in r["Kernel_Name"]) == (row[0] == "dtf_f32_conv_pw") for row, r in zip(rows, last))
    per_step = sum(us(r) for r in disp) / steps
    say("ResNet-%d v2 224x224 pop %d x %d fp32, _F32_PW=%d: %d dispatches, %d steps, kernel time %.3f ms / step" % (
        size, pop, batch, h32._F32_PW, len(disp), steps, per_step / 1e3))
    cls, lay = collections.defaultdict(list), collections.defaultdict(list)
    for row, r in zip(rows, last):
        cls[row[:4]].append(us(r))
        lay[row].append(us(r))
    for (name, kh, stride, dgrad), t in sorted(cls.items()):
        say("  %-16s %dx%d/%d %-5s x%3d: %9.3f ms  %5.1f %% of the step's kernel time" % (
            name, kh, kh, stride, "dgrad" if dgrad else "fwd", len(t), sum(t) / 1e3, 100 * sum(t) / per_step))
    for (name, kh, stride, dgrad, ci, co, px, epi), t in sorted(lay.items(), key=lambda kv: kv[0][3:]):
        if kh != 1 or stride != 1 or px <= pop * batch:
            continue  # (the dense head is a 1 x 1 "image")
        n_in = 1 + bool(epi & 1) + bool(epi & 2)  # output-sized tensors read next to the one written
        by = 4.0 * (px * ci + px * co * n_in + ci * co)
        fl = 2.0 * ci * co * px
        m = statistics.median(t)
        say("  %-16s %-5s %4d -> %4d px %7d epi %d x%2d: %8.1f us  %6.1f TFLOP/s  %5.2f TB/s  (%5.1f FLOP/B)" % (
            name, "dgrad" if dgrad else "fwd", ci, co, px, epi, len(t), m, fl / m / 1e6, by / m / 1e6, fl / by))
    say("")
    sys.exit(0)

steps, rounds = int(argv[3]), int(argv[4])
kmin = h32._F32_PW_DGRAD_MIN_K  # "pw": the plan's routing; "pw_all": also the short-reduction data gradients
arms = [("pw", True, kmin), ("pw_all", True, 0), ("generic", False, kmin)]
plans = {}
for name, on, k in arms:
    h32._F32_PW, h32._F32_PW_DGRAD_MIN_K = on, k
    be._plans.clear()
    step()
    (key, plan), = be._plans.items()
    rows = conv_launches(plan)
    say("%-8s conv launches: %s" % (name, dict(collections.Counter(r[0] for r in rows))))
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
g = times["generic"]
for name in ("pw", "pw_all"):
    p = times[name]
    d = statistics.median(p) - statistics.median(g)
    say("%s - generic: %+.3f ms/step (%+.2f %%); the two spreads together: %.3f ms" % (
        name, d, 100 * d / statistics.median(g), max(g) - min(g) + max(p) - min(p)))
say("")
