"""Routing of the fp32 ImageNet plans' stride-2 data gradients (engine/hip_imagenet_f32.py): the 3x3 / 2 convs and the
1x1 / 2 projections outside the stem on f32dgrad_s2_kernel with ``_F32_DS2`` on (the step and block tests of
tests/test_gpu_imagenet_f32*.py then run it under their own rules), on the generic kernel with it off -- which must
still pass the step rule.  Eval plans have no data gradient.
"""
import pytest
import torch

import test_gpu_imagenet_f32 as t50
from distributedtf_amd.engine.population import PopulationEngine
from distributedtf_amd.models.resnet import ResNetArch, imagenet_config

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("size,version", [(50, 2), (50, 1), (18, 2)])
def test_plan_routes_stride2_data_gradients(monkeypatch, size, version):
    from distributedtf_amd import ops
    from distributedtf_amd.engine import hip_imagenet_f32 as h32
    arch = ResNetArch(imagenet_config(size, version, num_classes=1001, image_size=64))
    eng = PopulationEngine(arch, 2, torch.device("cuda"), backend="torch", compute_dtype=torch.float32)
    be = h32.HipImageNetF32Backend(eng)
    prog = arch.prog
    s2 = [c for i, c in enumerate(prog.convs) if c.stride == 2 and c.k in (1, 3) and i != prog.stem]
    assert {c.k for c in s2} == {1, 3}  # the strided 3x3 conv and the projection of every downsampling block
    for on in (True, False):
        monkeypatch.setattr(h32, "_F32_DS2", on)
        for ev in (False, True):
            plan = be._plan_cls(be, [0, 1], [2, 3], eval_mode=True) if ev else be._plan_cls(be, [0, 1], [2, 3])
            named = [(ops.launcher_name(fn), args) for fn, args in plan.launches if not isinstance(fn, str)]
            ds2 = [args[0]._obj for name, args in named if name == "dtf_f32_dgrad_s2"]
            assert len(ds2) == len(s2) * on * (not ev), (size, version, on, ev, len(ds2))
            assert sorted((a.kh, a.Co, a.Ci) for a in ds2) == sorted((c.k, c.cin, c.cout) for c in s2) * (on and not ev)
            # ... and no strided data gradient but the stem's is left on the generic kernel
            rest = [args[0]._obj for name, args in named if name == "dtf_f32_conv" and args[4] and args[0]._obj.stride == 2]
            assert all(a.kh == 7 for a in rest) if on else len(rest) >= len(s2) * (not ev)


def test_generic_stride2_data_gradient_stays_selectable(monkeypatch):
    from distributedtf_amd.engine import hip_imagenet_f32 as h32
    monkeypatch.setattr(h32, "_F32_DS2", False)
    t50.test_hip_imagenet_f32_step_matches_fp32_oracle(monkeypatch, 2, "1")
