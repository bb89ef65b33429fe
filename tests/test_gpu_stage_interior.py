"""Tile staging of the CIFAR stride-1 conv kernels (conv.hip ``Stage``): band interior in two always-active slots,
halo rows in a pass of waves 0 / 1, zero border written once per launch.

The geometry is compile-time, so the small cases are small batches.  To make small batches produce the runs that
matter for the staging -- a workgroup that starts at a band other than 0, one whose run crosses an image boundary
(the halo rows switch between zero and data while the LDS buffers alternate), one that ends mid-image and a
single-iteration one -- the workgroup budget of the plan is capped per member (``_short_plans``); the plan the
engine then builds is inspected and must contain those runs.  The step itself is compared per layer with the fp32
PyTorch oracle by the harness of tests/test_gpu_resnet_step.py (``_compare_step``: 2.5 x the torch-bf16 error,
floor 0.06).
"""
import importlib.util
import os
import subprocess
import sys

import pytest
import torch

from distributedtf_amd import ops
from distributedtf_amd.engine import hip_resnet
from distributedtf_amd.engine.population import PopulationEngine
from distributedtf_amd.models import resnet as R
from distributedtf_amd.models.resnet import ResNetArch, cifar_config

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _hip_engine(arch, n, dev, backend="hip", **kw):
    """The HIP engine of this process's kernel build: fp16 storage with the static loss scale in the half build."""
    if backend == "hip" and ops.half_mode():
        kw.update(compute_dtype=torch.float16, loss_scale=128.0)
    return PopulationEngine(arch, n, dev, backend=backend, **kw)


def _harness():
    """A private copy of tests/test_gpu_resnet_step.py (its _compare_step / _hp), whose HIP engine follows the
    process's kernel build."""
    spec = importlib.util.spec_from_file_location("_resnet_step_harness", os.path.join(HERE, "test_gpu_resnet_step.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.PopulationEngine = _hip_engine
    return mod


def _short_plans(monkeypatch, per):
    """At most ``per`` workgroups per member in every (image, band) work table: runs of several iterations at
    batches of a few images (the default budgets give every workgroup one iteration below ~32 images)."""
    orig = hip_resnet._StepPlan._work_iters

    def capped(self, bands, n_wg, det_per=None):
        return orig(self, bands, min(n_wg, per * len(self.slots)),
                    det_per=min(per, det_per or hip_resnet.DET_WG_PER_MEMBER))

    monkeypatch.setattr(hip_resnet._StepPlan, "_work_iters", capped)


def _plan_runs(hip):
    """(bands, it0, nit) of every non-empty workgroup run of the multi-band work tables of the engine's plans."""
    runs = []
    for p in hip.backend._plans.values():
        for key, w in p._work_cache.items():
            if key[0] == "it" and key[1] > 1:
                runs += [(key[1], it0, nit) for it0, nit, _, _ in w.cpu().tolist() if nit > 0]
    return runs


def _coverage(runs):
    return {"starts_off_band_0": any(it0 % b != 0 for b, it0, n in runs),
            "crosses_image": any(it0 % b + n > b for b, it0, n in runs),
            "ends_mid_image": any((it0 + n) % b != 0 for b, it0, n in runs),
            "single_iteration": any(n == 1 for b, it0, n in runs)}


# (sizes, workgroups per member, runs the plan must hold).  [3, 5] at 4 per member: the 32 x 32 layers (4 bands)
# split 12 / 20 iterations into runs of 3 / 5 (exact plan) or 6 (elastic), the 16 x 16 layers (2 bands) 6 / 10 into
# 2 / 3 with a one-iteration tail.  One image ([1]) cannot cross an image boundary: 4 iterations in runs of 2.
# [2] at 3 per member: 8 iterations in runs of 3, 3, 2.
_ALL = ("starts_off_band_0", "crosses_image", "ends_mid_image", "single_iteration")
_CASES = [
    ("ragged-v2-r8", 8, 2, [3, 5], 4, "0", _ALL),
    ("ragged-v2-r14", 14, 2, [3, 5], 4, "0", _ALL),
    ("ragged-v1-r8", 8, 1, [3, 5], 4, "0", _ALL),
    ("ragged-v1-r14", 14, 1, [3, 5], 4, "0", _ALL),
    ("elastic-v2-r14", 14, 2, [3, 5], 4, "auto", _ALL),
    ("one-v2-r14", 14, 2, [1], 3, "0", ("starts_off_band_0",)),
    ("one-v1-r8", 8, 1, [1], 3, "0", ("starts_off_band_0",)),
    ("two-v2-r8", 8, 2, [2], 3, "0", ("starts_off_band_0", "crosses_image", "ends_mid_image")),
    ("two-v2-r14", 14, 2, [2], 3, "0", ("starts_off_band_0", "crosses_image", "ends_mid_image")),
    ("two-v1-r14", 14, 1, [2], 3, "0", ("starts_off_band_0", "crosses_image", "ends_mid_image")),
]
if ops.half_mode():  # the half build has the ResNet v2 families only
    _CASES = [c for c in _CASES if c[2] == 2]


@pytest.mark.parametrize("size,version,sizes,per,elastic,need", [c[1:] for c in _CASES], ids=[c[0] for c in _CASES])
def test_stage_step_matches_reference(size, version, sizes, per, elastic, need, monkeypatch):
    """Every stride-1 C = 16 / 32 / 64 layer kind of ResNet-8 / 14 (stem, BN input with and without residual, fused
    backward with its three dY modes and xout, dgrad-only and deferred wgrad roles at <= 2 members) on multi-iteration
    runs, per layer against the fp32 oracle; the plan must hold the runs named in ``need``."""
    monkeypatch.setenv("DTF_HIP_GRAPH", "1")
    monkeypatch.setenv("DTF_ELASTIC", elastic)
    _short_plans(monkeypatch, per)
    seen = {}

    def check(hip, plans0):
        seen.update(_coverage(_plan_runs(hip)))

    worst = _harness()._compare_step(ResNetArch(cifar_config(size, version=version)), sizes, check=check)
    print("plan runs:", seen, "worst per-layer relative error %.4f" % worst)
    missing = [k for k in need if not seen.get(k)]
    assert not missing, (missing, seen)


def _relerr(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def test_halo_stays_zero_on_constant_images(monkeypatch):
    """Constant non-zero images and BN shifts > 0: a halo staged as transformed data (a zero input maps to
    relu(shift - mean * scale), non-zero for most channels) or left over from the band that used the LDS buffer before
    (every pixel of a constant image is non-zero) changes the border pixels of the conv output.  The stem output (plain input staging) and the first block's conv_a output (BN + ReLU staging)
    are compared with the fp32 oracle on the border rows / columns and on the interior separately, both with the
    step tests' yardstick (2.5 x the error of the same computation in torch bf16, floor 0.06)."""
    monkeypatch.setenv("DTF_HIP_GRAPH", "0")
    monkeypatch.setenv("DTF_ELASTIC", "0")
    _short_plans(monkeypatch, 4)
    torch.manual_seed(0)
    dev = torch.device("cuda")
    arch = ResNetArch(cifar_config(8, version=2))
    prog = arch.prog
    sizes = [3, 5]
    hp = _harness()._hp
    hip = _hip_engine(arch, len(sizes), dev)
    slots = [hip.add_member(None, hp(bs), seed=20 + i) for i, bs in enumerate(sizes)]
    for b in prog.bns:  # gamma 1, shift 0.5
        hip.state[:len(sizes), b.gamma_off:b.gamma_off + b.c] = 1.0
        hip.state[:len(sizes), b.beta_off:b.beta_off + b.c] = 0.5
    batches = []
    for bs in sizes:
        level = 0.4 + 0.1 * torch.arange(bs, dtype=torch.float32).view(bs, 1, 1, 1)
        x = (level * torch.tensor([1.0, -0.5, 0.75])).expand(bs, 32, 32, 3).contiguous().to(dev)
        batches.append((x, torch.zeros(bs, dtype=torch.long, device=dev)))
    hip.train_step(slots, batches, [hp(bs) for bs in sizes], [0.0] * len(sizes))
    torch.cuda.synchronize()
    cov = _coverage(_plan_runs(hip))
    assert cov["crosses_image"] and cov["starts_off_band_0"], cov
    plan = next(iter(hip.backend._plans.values()))
    blk = prog.blocks[0]
    border = torch.zeros(32, 32, dtype=torch.bool, device=dev)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
    bad = []
    for s, (x, _) in zip(slots, batches):
        params = hip.params[s].clone()
        running = torch.zeros(prog.n_running, device=dev)
        f0 = plan.first[s]
        got = {"stem": plan.xs[0][f0:f0 + x.shape[0]].float().permute(0, 3, 1, 2),
               "conv_a": plan.hs[0][f0:f0 + x.shape[0]].float().permute(0, 3, 1, 2)}
        want = {}
        for dt in (torch.float32, torch.bfloat16):
            x0 = R._conv(prog, params, x.permute(0, 3, 1, 2).to(dt), prog.stem, dt)
            pre = torch.relu(R._bn(prog, params, running, x0, blk.bns[0], True, update_running=False))
            want[dt] = {"stem": x0.float(), "conv_a": R._conv(prog, params, pre, blk.convs[0], dt).float()}
        for name in ("stem", "conv_a"):
            for where, m in (("border", border), ("interior", ~border)):
                ref = want[torch.float32][name][:, :, m]
                tol = max(2.5 * _relerr(want[torch.bfloat16][name][:, :, m], ref), 0.06)
                err = _relerr(got[name][:, :, m], ref)
                print("%s member %d %s: rel %.4f tol %.4f" % (name, s, where, err, tol))
                if not err <= tol:
                    bad.append((name, s, where, err, tol))
    assert not bad, bad


def _det_worker():
    """Two engines in one process (the first one's launches are the first of the process; the second reuses the
    device's LDS after them), each: the same step with lr 0, then with lr 1.  Everything must be bitwise equal."""
    assert ops.deterministic_mode()
    hp = _harness()._hp
    dev = torch.device("cuda")
    arch = ResNetArch(cifar_config(8, version=2))
    sizes = [3, 5]
    g = torch.Generator(device="cpu").manual_seed(3)
    batches = [(torch.randn(bs, 32, 32, 3, generator=g).to(dev), torch.randint(0, 10, (bs,), generator=g).to(dev))
               for bs in sizes]
    out = []
    for _ in range(2):
        eng = _hip_engine(arch, len(sizes), dev)
        slots = [eng.add_member(None, hp(bs), seed=30 + i) for i, bs in enumerate(sizes)]
        hps = [hp(bs) for bs in sizes]
        l0 = eng.train_step(slots, batches, hps, [0.0] * len(sizes)).clone()
        l1 = eng.train_step(slots, batches, hps, [1.0] * len(sizes)).clone()
        torch.cuda.synchronize()
        assert torch.equal(l0, l1), (l0, l1)  # lr 0 left the weights alone: the same forward twice
        assert bool(torch.isfinite(l1).all())
        out.append((l0.cpu(), l1.cpu(), eng.state.clone().cpu(), eng.running.clone().cpu()))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    print("DET_STAGE_OK")


def test_deterministic_build_replays_bitwise(monkeypatch):
    """The deterministic build: losses, weights (and optimizer state) and BN moving statistics of the same step are
    bitwise equal between the first and a later run in one process, on multi-iteration runs.  The kernel library is
    chosen per process, so a release-build session runs the check in a child process."""
    env = dict(os.environ, DTF_DETERMINISTIC="1", DTF_HIP_GRAPH="1", DTF_ELASTIC="0", DTF_STAGE_TEST_PER="4",
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                       timeout=240, cwd=ROOT)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "DET_STAGE_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


if __name__ == "__main__":
    _orig = hip_resnet._StepPlan._work_iters
    _per = int(os.environ.get("DTF_STAGE_TEST_PER", "4"))
    hip_resnet._StepPlan._work_iters = lambda self, bands, n_wg, det_per=None: _orig(
        self, bands, min(n_wg, _per * len(self.slots)), det_per=min(_per, det_per or hip_resnet.DET_WG_PER_MEMBER))
    _det_worker()
