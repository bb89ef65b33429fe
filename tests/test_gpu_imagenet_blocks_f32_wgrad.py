"""Routing of the fp32 building-block plans' stride-1 3x3 weight gradients (engine/hip_imagenet_f32.py): on
f32wgrad_t3_kernel at the widths of ``_F32_WGT3``, on the generic split-K kernel with the table emptied -- which must
still pass the fp64 step rule of tests/test_gpu_imagenet_blocks_f32.py (whose own 224 cases run the row-band kernel).
"""
import pytest
import torch

import test_gpu_imagenet_blocks_f32 as blocks
from distributedtf_amd.engine.population import PopulationEngine
from distributedtf_amd.models.resnet import ResNetArch, imagenet_config

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("size", [18, 34])
def test_plan_routes_3x3_weight_gradients(monkeypatch, size):
    from distributedtf_amd import ops
    from distributedtf_amd.engine import hip_imagenet_f32 as h32
    arch = ResNetArch(imagenet_config(size, 2, num_classes=1001, image_size=224))
    eng = PopulationEngine(arch, 2, torch.device("cuda"), backend="torch", compute_dtype=torch.float32)
    be = h32.HipImageNetF32Backend(eng)
    nb = arch.cfg.block_sizes
    for table in ({56, 28, 14, 7}, set()):
        monkeypatch.setattr(h32, "_F32_WGT3", table)
        plan = be._plan_cls(be, [0, 1], [2, 3])
        got = {w: sum(1 for fn, args in plan.launches if not isinstance(fn, str)
                      and ops.launcher_name(fn) == "dtf_f32_wgrad_t3" and args[1] == w) for w in (56, 28, 14, 7)}
        # every stride-1 3x3 conv: all 2 n of the first stage, 2 n - 1 of the later ones
        want = {w: (2 * nb[i] - (i > 0)) * (w in table) for i, w in enumerate((56, 28, 14, 7))}
        assert got == want, (got, want)
    assert sum(want.values()) == 0  # (the emptied table came last)


def test_generic_weight_gradient_stays_selectable(monkeypatch):
    from distributedtf_amd.engine import hip_imagenet_f32 as h32
    monkeypatch.setattr(h32, "_F32_WGT3", set())
    blocks.test_hip_imagenet_blocks_f32_step_matches_fp64(monkeypatch, 18, 224, "1", True)
