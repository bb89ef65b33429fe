"""The host-resident ImageNet set on the GPU: the staged form of the input kernel against the resident form, bit for
bit; the HIP ResNet-50 step fed rows of a HostImageNetDataset against the same step fed the same rows of a
DeviceDataset, with the prefetch protocol observed through the feed's counters; and ``main_manager.py
--imagenet_data host`` end to end in a child process.

Runs in-process on the release, deterministic (DTF_DETERMINISTIC=1) and half (DTF_HALF=1) libraries."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributedtf_amd import ops
from distributedtf_amd.data import datasets

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64  # canary elements before and after every output (a multiple of 16 bytes for every type)
NSET, CAP = 23, 7


class Guarded:
    """An output in the middle of a buffer of canaries: NaN for floating types, a sentinel for integers."""

    def __init__(self, shape, dtype):
        self.fill = float("nan") if dtype.is_floating_point else -77
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), self.fill, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + self.n].view(*shape)

    def check(self, used):
        """The canaries around the output, and everything past its first ``used`` elements, are untouched."""
        rest = torch.cat([self.buf[:GUARD], self.buf[GUARD + used:]])
        assert bool(torch.isnan(rest).all() if self.buf.dtype.is_floating_point else (rest == self.fill).all())


def _outputs(m, H):
    act = ops.act_dtype()
    return dict(out_s2d=Guarded((m, H // 2, H // 2, 16), act), out_pad=Guarded((m, H, H, 8), act),
                out32=Guarded((m, H, H, 3), torch.float32), lab32=Guarded((m,), torch.int32),
                lab64=Guarded((m,), torch.int64), boxes=Guarded((m, 5), torch.int32))


def _bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


@pytest.fixture(scope="module")
def small_sets():
    """23 images at S = 40 and at S = 32, on the host and on the device, with labels."""
    out = {}
    for side in (40, 32):
        g = torch.Generator().manual_seed(side)
        x = torch.randint(0, 256, (NSET, side, side, 3), generator=g, dtype=torch.uint8)
        y = torch.randint(0, 1000, (NSET,), generator=g)
        out[side] = (x, x.cuda(), y.cuda())
    return out


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("side", [40, 32])
def test_staged_kernel_is_bitwise_the_resident_kernel(small_sets, side, half):
    """H = 32 from S = 40 (a resample) and from S = 32; cap = 7, n = 1, 5 and cap; rows with a duplicate, row 0 and
    the last row; both keyings.  Everything the launch must not read holds 0xFF: the staging rows at and beyond n
    and the whole other half.  Every output sits between canaries, with two rows beyond n that stay untouched."""
    H = 32
    xh, xd, y = small_sets[side]
    rows_all = [22, 0, 7, 7, 3, 22, 11]
    state = torch.zeros(4, 10, device="cuda")
    state[:, 6] = torch.tensor([0, 7, 123456, 3], dtype=torch.float32)
    rng = torch.tensor([99173, 41], dtype=torch.int32, device="cuda")
    hw = torch.tensor([half], dtype=torch.int32, device="cuda")
    for n in (1, 5, CAP):
        rows = rows_all[:n]
        idx = torch.tensor(rows, device="cuda")
        stage = torch.full((2, CAP, side, side, 3), 255, dtype=torch.uint8, device="cuda")
        stage[half, :n] = xh[rows].cuda()
        slot = torch.tensor([1, 2, 0, 3, 2, 1, 0][:n], dtype=torch.int32, device="cuda")
        for keys in (None, (slot, state, 10, 6)):
            res, stg = _outputs(n + 2, H), _outputs(n + 2, H)
            ops.augment_imagenet(xd, y, idx, rng, H, True, member_keys=keys, **{k: g.t for k, g in res.items()})
            ops.augment_imagenet_staged(stage, hw, y, idx, rng, H, True, member_keys=keys,
                                        **{k: g.t for k, g in stg.items()})
            torch.cuda.synchronize()
            for k in res:
                per = res[k].n // (n + 2)
                res[k].check(per * n)
                stg[k].check(per * n)
                assert torch.equal(_bits(res[k].t[:n]), _bits(stg[k].t[:n])), (k, n, keys is not None)
            assert torch.equal(stg["lab64"].t[:n], y[idx])
            assert bool(torch.isfinite(stg["out32"].t[:n]).all())
        # the evaluation crop (augment = 0) goes through the same body
        a, b = _outputs(n, H), _outputs(n, H)
        ops.augment_imagenet(xd, y, idx, rng, H, False, out32=a["out32"].t, boxes=a["boxes"].t)
        ops.augment_imagenet_staged(stage, hw, y, idx, rng, H, False, out32=b["out32"].t, boxes=b["boxes"].t)
        assert torch.equal(_bits(a["out32"].t), _bits(b["out32"].t)) and torch.equal(a["boxes"].t, b["boxes"].t)


def test_staged_launch_larger_than_the_halves_is_refused(small_sets):
    """n > cap: the launcher's argument check returns hipErrorInvalidValue and launches nothing."""
    H = 32
    xh, xd, y = small_sets[40]
    stage = torch.full((2, CAP, 40, 40, 3), 255, dtype=torch.uint8, device="cuda")
    idx = torch.arange(CAP + 1, device="cuda")
    rng = torch.tensor([1, 2], dtype=torch.int32, device="cuda")
    hw = torch.zeros(1, dtype=torch.int32, device="cuda")
    o = _outputs(CAP + 1, H)
    with pytest.raises(RuntimeError, match="hipError 1$"):
        ops.augment_imagenet_staged(stage, hw, y, idx, rng, H, True, **{k: g.t for k, g in o.items()})
    torch.cuda.synchronize()
    for g in o.values():
        g.check(0)
    ops.augment_imagenet_staged(stage, hw, y, idx[:CAP], rng, H, True, out32=o["out32"].t)  # n = cap is accepted
    torch.cuda.synchronize()
    o["out32"].check(o["out32"].n // (CAP + 1) * CAP)


# ------------------------------------------------------------------------------------------------- plan level
HP = {"opt_case": {"optimizer": "Momentum", "lr": 0.01, "momentum": 0.9}, "batch_size": 8,
      "regularizer": "l2_regularizer", "weight_decay": 1e-4, "initializer": "he_init"}
IMAGE, SIDE, SIZES = 64, 80, [8, 6, 10]


@pytest.fixture(scope="module")
def learnable():
    trx, tr_y, tex, te_y = datasets.learnable_imagenet(n_train=64, n_test=8, side=SIDE, num_classes=10, seed=3)
    return trx, tr_y


def _engine(members=3):
    from distributedtf_amd.engine.population import PopulationEngine
    from distributedtf_amd.models.resnet import ResNetArch, imagenet_config
    arch = ResNetArch(imagenet_config(50, 2, num_classes=10, image_size=IMAGE))
    kw = dict(compute_dtype=torch.float16, loss_scale=128.0) if ops.half_mode() else {}
    e = PopulationEngine(arch, members, torch.device("cuda"), backend="hip", **kw)
    for i in range(members):
        e.add_member(None, HP, seed=i)
    return e


@pytest.mark.parametrize("s2d", [True, False])
def test_step_fed_host_rows_equals_step_fed_device_rows(learnable, monkeypatch, s2d):
    """ResNet-50 at image 64 from S = 80, members of 8 / 6 / 10 images in one plan, 4 steps (the eager warm-up with
    the capture, then three replays), each fed the same explicit rows through a DeviceDataset plan and through a
    HostImageNetDataset plan.  Every library: ``xin8`` and ``labels`` bitwise equal at every step, losses finite.
    Deterministic library: losses at every step and the full state rows after step 4 bitwise equal.  Steps 1 and 2
    announce the next step's rows rightly, step 3 announces other rows: steps 2 and 3 are served from the prefetched
    half, step 4 is staged when it is asked for, the half alternates, and the graph is captured once."""
    from distributedtf_amd.engine import hip_imagenet
    monkeypatch.setattr(hip_imagenet, "_CG_S2D", s2d)
    trx, tr_y = learnable
    common = dict(out_size=IMAGE, seed=5)
    dev_ds = datasets.DeviceDataset(trx, tr_y, trx[:8], tr_y[:8], "cuda", augment=datasets.augment_imagenet,
                                    eval_transform=datasets.eval_imagenet, **common)
    host_ds = datasets.HostImageNetDataset(trx, tr_y, trx[:8], tr_y[:8], "cuda", **common)
    assert host_ds.hip_augment and host_ds.imagenet and host_ds.train_x is trx
    a, b = _engine(), _engine()
    det = a.backend.det
    for e in (a, b):
        assert e.backend.use_graph and e.backend.s2d == s2d
    slots, lrs = [0, 1, 2], [0.01] * 3
    g = torch.Generator().manual_seed(7)
    steps = [[torch.randint(0, 64, (n,), generator=g) for n in SIZES] for _ in range(4)]
    steps[1][0][:2] = torch.tensor([0, 63])  # row 0 and the last row
    steps[1][1][:2] = steps[1][1][2]  # a row three times over
    announce = [steps[1], steps[2], steps[0], [None] * 3]  # what step k says about step k + 1: right, right, wrong
    feed = host_ds.feed
    halves, counts = [], []
    for k in range(4):
        la = a.train_step(slots, [datasets.IndexBatch(dev_ds, i.cuda()) for i in steps[k]], [HP] * 3, lrs)
        lb = b.train_step(slots, [datasets.IndexBatch(host_ds, i, next_rows=nx)
                                  for i, nx in zip(steps[k], announce[k])], [HP] * 3, lrs)
        (pa,), (pb,) = a.backend._plans.values(), b.backend._plans.values()
        assert pa.src is dev_ds and pb.src is host_ds and pb.host_src and not pa.host_src
        assert [f for f, _ in pa.launches] == [f for f, _ in pb.launches]  # the same list; "augment" runs the staged op
        assert torch.equal(_bits(pa.xin8), _bits(pb.xin8)) and torch.equal(pa.labels, pb.labels)
        assert torch.equal(pb.labels.long().cpu(), torch.from_numpy(tr_y)[torch.cat(steps[k])])
        assert torch.equal(pb.idx.cpu(), torch.cat(steps[k]))
        assert bool(torch.isfinite(la).all() and torch.isfinite(lb).all()), (la, lb)
        if det:
            assert torch.equal(_bits(la), _bits(lb))
        halves.append(int(pb.half_word.item()))
        counts.append((feed.hits, feed.syncs))
    assert counts == [(0, 1), (1, 1), (2, 1), (2, 2)], counts  # steps 2, 3 prefetched; steps 1, 4 staged when asked
    assert halves == [0, 1, 0, 1] and feed.stager.cap == sum(SIZES) and feed.stager.generation == 1
    assert feed.stager.stages == 5  # four steps' rows and the wrong announcement of step 3
    assert pb.graph is not None and b.backend.graphs_captured == 1 and a.backend.graphs_captured == 1
    if det:
        torch.cuda.synchronize()
        assert torch.equal(_bits(a.state[:3]), _bits(b.state[:3])) and bool(torch.isfinite(a.params[:3]).all())
    # the materialising path (the fp32 step, --dp_size, the PyTorch backend): the same rows, seed and counter give
    # bitwise the resident set's batch
    idx = torch.tensor([63, 0, 5, 5, 17])
    dev_ds.rng_counter = host_ds.rng_counter = 100
    hx, hy = host_ds.batch(idx)
    dx, dy = dev_ds.batch(idx.cuda())
    assert torch.equal(_bits(hx), _bits(dx)) and torch.equal(hy, dy)
    host_ds.close()
    assert feed.stager.threads_alive() == 0


def test_main_manager_trains_from_a_host_set(tmp_path):
    """Two short rounds of two members in a child process under a time limit: it exits 0 (so no thread of the stager
    keeps it alive), both members are alive after both rounds, every loss the members report after a round is
    finite, and the step was a captured graph.

    Seed 10 is the first seed whose two sampled members both have a learning rate of at most 1e-3 (RMSProp at 1e-5
    and 1e-4, batch sizes 73 and 172): no member is expected to diverge, so a member that does not come back finite
    was fed wrong data.  The per-member losses are the ``loss`` records the benchmark file logger writes at every
    evaluation (``metrics.jsonl`` holds only accuracies, and drops the NaN ones before it summarises them)."""
    logdir = tmp_path / "bench"
    cmd = [sys.executable, "-u", os.path.join(ROOT, "main_manager.py"), "2", "--model", "imagenet", "--image_size",
           "64", "--imagenet_data", "host", "--use_synthetic_data", "learnable",
           "--max_train_steps", "6", "--rounds", "2", "--backend", "hip", "--seed", "10", "--no_checkpoint",
           "--benchmark_logger_type", "BenchmarkFileLogger", "--benchmark_log_dir", str(logdir),
           "--savedata", str(tmp_path / "savedata"), "--results_file", str(tmp_path / "results.txt")]
    # the child loads the library this process runs on, through the flags that select it
    cmd += (["--dtype", "fp16"] if ops.half_mode() else []) + (["--deterministic"] if ops.deterministic_mode() else [])
    env = {k: v for k, v in os.environ.items() if k not in ("DTF_HALF", "DTF_DETERMINISTIC")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    recs = [json.loads(line) for line in open(tmp_path / "savedata" / "metrics.jsonl")]
    assert len(recs) == 2
    for rec in recs:
        assert rec["population"] == 2 and rec["images"] == 6 * sum(rec["batch_sizes"].values()) > 0, rec
        assert math.isfinite(rec["best_acc"]) and math.isfinite(rec["mean_acc"]), rec
        assert rec["step_graph"] == ["captured"], rec
    metrics = [json.loads(line) for line in open(logdir / "metric.log")]
    losses = [m["value"] for m in metrics if m["name"] == "loss"]
    ids = sorted(int(m["value"]) for m in metrics if m["name"] == "model_id")
    accs = [m["value"] for m in metrics if m["name"] == "accuracy"]
    print("[imagenet_host_data] main_manager losses %s accuracies %s" % (losses, accs))
    assert ids == [0, 0, 1, 1] and len(losses) == 4 and len(accs) == 4, metrics  # each member, after each round
    assert all(math.isfinite(v) and v > 0.0 for v in losses), losses
    assert all(math.isfinite(v) and 0.0 <= v <= 1.0 for v in accs), accs
