"""Routing of the fp32 ImageNet plans' stride-1 1x1 convs (engine/hip_imagenet_f32.py): forward and data gradient on
f32conv_pw_kernel with ``_F32_PW`` on (the step and eval tests of tests/test_gpu_imagenet_f32.py then run it under their
own rule), on the generic kernel with it off -- which must still pass that step rule.  The dense head stays on the
generic kernel either way.
"""
import pytest
import torch

import test_gpu_imagenet_f32 as t50
from distributedtf_amd.engine.population import PopulationEngine
from distributedtf_amd.models.resnet import ResNetArch, imagenet_config

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("version", [2, 1])
def test_plan_routes_pointwise_convs(monkeypatch, version):
    from distributedtf_amd import ops
    from distributedtf_amd.engine import hip_imagenet_f32 as h32
    arch = ResNetArch(imagenet_config(50, version, num_classes=1001, image_size=64))
    eng = PopulationEngine(arch, 2, torch.device("cuda"), backend="torch", compute_dtype=torch.float32)
    be = h32.HipImageNetF32Backend(eng)
    prog = arch.prog
    pws = [c for i, c in enumerate(prog.convs) if c.k == 1 and c.stride == 1 and i != prog.stem]
    # every forward; the data gradients but the short-reduction class the plan leaves on the generic kernel
    n, nd = len(pws), sum(1 for c in pws if c.cout >= h32._F32_PW_DGRAD_MIN_K)
    assert n > nd > 0
    for on in (True, False):
        monkeypatch.setattr(h32, "_F32_PW", on)
        for ev in (False, True):
            plan = be._plan_cls(be, [0, 1], [2, 3], eval_mode=True) if ev else be._plan_cls(be, [0, 1], [2, 3])
            named = [(ops.launcher_name(fn), args) for fn, args in plan.launches if not isinstance(fn, str)]
            pw = [args for name, args in named if name == "dtf_f32_conv_pw"]
            got = [sum(1 for args in pw if args[3] == d) for d in (0, 1)]
            assert got == [n * on, nd * on * (not ev)], (version, on, ev, got, n, nd)
            # the dense head (wrows = the class count) keeps the generic kernel: forward [+ data gradient]
            assert all(args[0]._obj.wrows == 0 for args in pw)
            head = [args for name, args in named if name == "dtf_f32_conv" and args[0]._obj.wrows == be.ncls]
            assert len(head) == (1 if ev else 2)


def test_generic_pointwise_stays_selectable(monkeypatch):
    from distributedtf_amd.engine import hip_imagenet_f32 as h32
    monkeypatch.setattr(h32, "_F32_PW", False)
    t50.test_hip_imagenet_f32_step_matches_fp32_oracle(monkeypatch, 2, "1")
