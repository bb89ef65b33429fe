"""The v2 step plan computes every projection shortcut inside conv_a's forward launch and applies block 0's
BN1-backward on the stem weight gradient's dY load: its launch list holds no 1x1 ``dtf_conv_fwd`` and no
``dtf_bn_bwd_apply``, the conv_a launches of the projection blocks carry ``y2``, and the step still matches the fp32
oracle under test_gpu_resnet_step.py's comparison (per-layer gradients, loss, BN running statistics) -- on exact plans
and on one elastic plan with ragged batch sizes."""
import pytest

from distributedtf_amd.models.resnet import ResNetArch, cifar_config

import test_gpu_resnet_step as step

pytestmark = pytest.mark.gpu


def _check_launches(hip, n_proj):
    from distributedtf_amd import ops
    plans = list(hip.backend._plans.values())
    assert plans
    for p in plans:
        names = [ops.launcher_name(fn) for fn, _ in p.launches if not isinstance(fn, str)]
        assert "dtf_bn_bwd_apply" not in names, names
        with_y2 = 0
        for fn, args in p.launches:
            if isinstance(fn, str):
                continue
            name = ops.launcher_name(fn)
            if name == "dtf_conv_fwd":  # (byref(args), cin, cout, stride, k, ...)
                assert args[4] != 1, "a standalone 1x1 projection forward launch"
            if name in ("dtf_conv_fwd", "dtf_conv_fwd_s1"):
                with_y2 += bool(args[0]._obj.y2)
        assert with_y2 == n_proj, (with_y2, n_proj)
        # the stem weight gradient: BN-backward of (dz1, x0) on load
        stem = [args for fn, args in p.launches if not isinstance(fn, str) and ops.launcher_name(fn) == "dtf_conv_wgrad"
                and args[0]._obj.cin_real == 3]
        assert len(stem) == 1 and stem[0][5:7] == (0, 2) and stem[0][0]._obj.dy2, stem


@pytest.mark.parametrize("size,sizes", [(8, [8, 12]), (14, [8, 12])], ids=["r8", "r14"])
def test_proj_plan_matches_reference(size, sizes, monkeypatch):
    monkeypatch.setenv("DTF_HIP_GRAPH", "1")
    arch = ResNetArch(cifar_config(size, version=2))
    n_proj = sum(b.proj is not None for b in arch.prog.blocks)
    assert n_proj == 3
    step._compare_step(arch, sizes, check=lambda hip, plans0: _check_launches(hip, n_proj))


def test_proj_plan_elastic(monkeypatch):
    """Ragged sizes on ONE capacity-keyed plan: warm-up (20, 9), compared replay (12, 17)."""
    monkeypatch.setenv("DTF_HIP_GRAPH", "1")
    monkeypatch.setenv("DTF_ELASTIC", "auto")
    monkeypatch.setenv("DTF_ELASTIC_MAXB", "24")
    arch = ResNetArch(cifar_config(14, version=2))

    def check(hip, plans0):
        plans = hip.backend._plans
        assert len(plans) == 1 and next(iter(plans.values())).elastic
        _check_launches(hip, 3)

    step._compare_step(arch, [12, 17], warm_sizes=[20, 9], check=check)
