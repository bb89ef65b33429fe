"""A/B of the fp32 stride-2 data-gradient kernel (f32dgrad_s2_kernel) against the generic fp32 conv kernel.

    python tools/f32_ds2_ab.py RESNET_SIZE POP BATCH STEPS_PER_WINDOW ROUNDS OUT_FILE
    python tools/f32_ds2_ab.py --trace KERNEL_TRACE_CSV RESNET_SIZE POP BATCH OUT_FILE

First form: builds the fp32 step plan of one engine twice -- ``_F32_DS2`` on (the plan's routing) and off (the generic
kernel, the routing of before the kernel existed) -- and times them in alternating windows of graph replays inside one
process (each arm's spread is printed next to its median).  Second form: reads the kernel trace of a run of its own
(rocprofv3 --kernel-trace, no counters, of bench.py --model imagenet --dtype fp32 at the same size, population and
batch, under the DTF_F32_DS2 of this call), pairs the conv dispatches of its last step with the plan's launch list in
order, and prints per class (launcher, kernel size, stride, direction) its share of the step's kernel time and, per
stride-2 layer shape, the time per launch of the forward and of the data gradient with the FLOP/s and HBM bytes/s it
implies (FLOP = 2 k^2 Cin Cout x the pixels of the coarse grid, the same for both directions; bytes = operand + output
[+ residual, mask source] + weights, each once).  Both append to OUT_FILE; profiles/f32_ds2_ab.txt is their output.
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
CONVS = ("dtf_f32_conv", "dtf_f32_conv_pw", "dtf_f32_conv_t3", "dtf_f32_dgrad_s2")


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
    """(launcher, kh, stride, dgrad, Ci, Co, pixels of the coarse grid, epi) of every forward / data-gradient conv
    launch, in order (Ci: the reduction's channels, Co: the output's)."""
    rows = []
    for fn, a in plan.launches:
        name = None if isinstance(fn, str) else ops.launcher_name(fn)
        if name in CONVS:
            g = a[0]._obj
            epi, dgrad = (a[3], a[4]) if name == "dtf_f32_conv" else ((a[2], 1) if name == "dtf_f32_dgrad_s2"
                                                                      else (a[2], a[3]))
            px = plan.N * (g.Hi * g.Wi if dgrad else g.Ho * g.Wo)
            rows.append((name, g.kh, g.stride, int(dgrad), g.Ci, g.Co, px, epi))
    return rows


if trace:
    step()
    (key, plan), = be._plans.items()
    rows = conv_launches(plan)
    with open(trace) as f:
        disp = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
    conv_d = [r for r in disp if ("f32conv_" in r["Kernel_Name"] or "f32dgrad_s2" in r["Kernel_Name"])
              and "wgrad" not in r["Kernel_Name"]]
    steps = len(conv_d) / len(rows)
    assert steps >= 1 and steps == int(steps), "the trace holds %d conv dispatches, a step has %d" % (len(conv_d), len(rows))
    last = conv_d[-len(rows):]  # the last step's conv dispatches, in the launch list's order
    assert all(("f32dgrad_s2" in r["Kernel_Name"]) == (row[0] == "dtf_f32_dgrad_s2") for row, r in zip(rows, last))
    per_step = sum(us(r) for r in disp) / steps
    say("ResNet-%d v2 224x224 pop %d x %d fp32, _F32_DS2=%d: %d dispatches, %d steps, kernel time %.3f ms / step" % (
        size, pop, batch, h32._F32_DS2, len(disp), steps, per_step / 1e3))
    cls, lay = collections.defaultdict(list), collections.defaultdict(list)
    for row, r in zip(rows, last):
        cls[row[:4]].append(us(r))
        lay[row].append(us(r))
    for (name, kh, stride, dgrad), t in sorted(cls.items()):
        if stride == 2 and kh in (1, 3):
            say("  %-16s %dx%d/%d %-5s x%3d: %9.3f ms  %5.1f %% of the step's kernel time" % (
                name, kh, kh, stride, "dgrad" if dgrad else "fwd", len(t), sum(t) / 1e3, 100 * sum(t) / per_step))
    for (name, kh, stride, dgrad, ci, co, px, epi), t in sorted(lay.items(), key=lambda kv: (kv[0][6], kv[0][1], kv[0][3])):
        if stride != 2 or kh not in (1, 3):
            continue
        n_in = 1 + bool(epi & 1) + bool(epi & 2)  # output-sized tensors read next to the one written
        px_out = 4 * px if dgrad else px
        px_in = px if dgrad or kh == 1 else 4 * px  # (a 1x1 / 2 forward reads one input pixel in four)
        by = 4.0 * (px_in * ci + px_out * co * n_in + kh * kh * ci * co)
        fl = 2.0 * kh * kh * ci * co * px
        m = statistics.median(t)
        say("  %-16s %dx%d %-5s %4d -> %4d coarse px %7d epi %d x%2d: %8.1f us  %6.1f TFLOP/s  %5.2f TB/s  (%5.1f FLOP/B)" % (
            name, kh, kh, "dgrad" if dgrad else "fwd", ci, co, px, epi, len(t), m, fl / m / 1e6, by / m / 1e6, fl / by))
    say("")
    sys.exit(0)

steps, rounds = int(argv[3]), int(argv[4])
arms = [("ds2", True), ("generic", False)]
plans = {}
for name, on in arms:
    h32._F32_DS2 = on
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
    for name, _ in arms:
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
for name, _ in arms:
    t = times[name]
    say("%-8s median %9.3f ms/step  spread %9.3f .. %9.3f" % (name, statistics.median(t), min(t), max(t)))
g, p = times["generic"], times["ds2"]
d = statistics.median(p) - statistics.median(g)
say("ds2 - generic: %+.3f ms/step (%+.2f %%); the two spreads together: %.3f ms" % (
    d, 100 * d / statistics.median(g), max(g) - min(g) + max(p) - min(p)))
say("")
