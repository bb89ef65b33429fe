"""fp32 HIP step of the ImageNet-shape ResNet-18 / 34 (v2 building blocks, engine/hip_imagenet_f32.py) under the rule
of tests/test_gpu_imagenet_f32.py: one lr = 2^20 gradient step after an lr = 0 warm-up, members of 2 and 3 images;
every gradient tensor against the float64 ``forward_reference`` gradient within max(1e-3, 3 x the PyTorch fp32 step's
error, 3 x the fp64 gradient's movement under 1e-5 input noise), loss within 1e-4 of the fp32 PyTorch step, running
statistics rtol 1e-4 / atol 1e-5.  Image 64: the generic kernel everywhere; image 224: the stride-1 3x3 convs on
f32conv_t3_kernel at 56 / 28 / 14 / 7 (counted on the plan's launch list), or nowhere with ``_F32_T3`` emptied.
"""
import pytest
import torch

from distributedtf_amd.engine.population import PopulationEngine, make_backend
from distributedtf_amd.models.resnet import ResNetArch, forward_reference, imagenet_config
from test_gpu_imagenet_f32 import _hp, _relerr

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("size,image,graph,t3", [(18, 64, "1", True), (18, 64, "0", True), (18, 224, "1", True),
                                                 (34, 224, "1", True), (18, 224, "1", False)])
def test_hip_imagenet_blocks_f32_step_matches_fp64(monkeypatch, size, image, graph, t3):
    from distributedtf_amd import ops
    from distributedtf_amd.engine import hip_imagenet_f32
    monkeypatch.setenv("DTF_HIP_GRAPH", graph)
    if not t3:
        monkeypatch.setattr(hip_imagenet_f32, "_F32_T3", set())
    torch.manual_seed(0)
    arch = ResNetArch(imagenet_config(size, 2, num_classes=1001, image_size=image))
    dev, sizes = torch.device("cuda"), [2, 3]
    ref = PopulationEngine(arch, 2, dev, backend="torch", compute_dtype=torch.float32, optimizer_impl="hip")
    hip = PopulationEngine(arch, 2, dev, backend="hip", compute_dtype=torch.float32)
    assert hip.backend.__class__.__name__ == "HipImageNetF32Backend"
    slots = [e.add_member(None, _hp(bs), seed=3 + i) for i, bs in enumerate(sizes) for e in (ref, hip)][::2]
    g = torch.Generator().manual_seed(1)
    for b in arch.prog.bns:
        ng, nb = 1.0 + 0.2 * torch.randn(2, b.c, generator=g), 0.1 * torch.randn(2, b.c, generator=g)
        for st in (ref.state, hip.state):
            st[:, b.gamma_off:b.gamma_off + b.c] = ng.to(dev)
            st[:, b.beta_off:b.beta_off + b.c] = nb.to(dev)
    batches = [(torch.randn(bs, image, image, 3, generator=g).to(dev),
                torch.randint(0, 1001, (bs,), generator=g).to(dev)) for bs in sizes]
    hps = [_hp(bs) for bs in sizes]
    for e in (ref, hip):
        e.train_step(slots, batches, hps, [0.0, 0.0])
    torch.cuda.synchronize()
    before = hip.params.clone()
    assert torch.equal(before, ref.params)
    plan = next(iter(hip.backend._plans.values()))
    assert (plan.graph is not None) == (graph == "1")
    # stride-1 3x3 convs, forward and data gradient: all 2 n of the first stage, 2 n - 1 of the later ones
    band = {w: sum(1 for fn, args in plan.launches if not isinstance(fn, str)
                   and ops.launcher_name(fn) == "dtf_f32_conv_t3" and args[4] == w) for w in (56, 28, 14, 7)}
    nb = arch.cfg.block_sizes
    want = {w: 2 * (2 * nb[i] - (i > 0)) if image == 224 and t3 else 0 for i, w in enumerate((56, 28, 14, 7))}
    assert band == want, (band, want)
    LR = float(2 ** 20)  # (before - after) / lr recovers the gradient to fp32 rounding
    l_ref = ref.train_step(slots, batches, hps, [LR, LR])
    l_hip = hip.train_step(slots, batches, hps, [LR, LR])
    torch.cuda.synchronize()
    torch.testing.assert_close(l_hip.float(), l_ref.float(), rtol=1e-4, atol=1e-4)
    g_ref, g_hip = (before - ref.params) / LR, (before - hip.params) / LR
    run0 = hip.running.clone()

    def grad64(rel_noise=0.0, seed=0):
        out = torch.zeros_like(before, dtype=torch.float64)
        gn = torch.Generator(device=dev).manual_seed(seed)
        for i, s in enumerate(slots):
            p = before[s].double().clone().requires_grad_(True)
            x, y = batches[i]
            x = x.double() * (1.0 + rel_noise * torch.randn(x.shape, generator=gn, device=dev, dtype=torch.float64))
            logits = forward_reference(arch.prog, p, run0[s].double().clone(), x, training=True,
                                       dtype=torch.float64, update_running=False)
            out[s], = torch.autograd.grad(torch.nn.functional.cross_entropy(logits, y.long()), p)
        return out

    g64, g_pert = grad64(), [grad64(1e-5, seed) for seed in (1, 2)]
    prog = arch.prog
    segs = [("conv%d" % c.idx, c.off, c.off + c.numel) for c in prog.convs]
    for bn in prog.bns:
        segs += [("bn%d.gamma" % bn.idx, bn.gamma_off, bn.gamma_off + bn.c),
                 ("bn%d.beta" % bn.idx, bn.beta_off, bn.beta_off + bn.c)]
    segs.append(("dense", prog.dense_w_off, prog.dense_b_off + arch.cfg.num_classes))
    bad, worst = [], (0.0, 0.0, 0.0, "")
    for s in slots:
        for name, lo, hi in segs:
            err, err32 = _relerr(g_hip[s, lo:hi], g64[s, lo:hi]), _relerr(g_ref[s, lo:hi], g64[s, lo:hi])
            sens = max(_relerr(gp[s, lo:hi], g64[s, lo:hi]) for gp in g_pert)
            worst = max(worst, (err, err32, sens, name))
            if err > max(1e-3, 3.0 * err32, 3.0 * sens):
                bad.append("%s member %d rel %.2e (torch fp32 %.2e, fp64 sensitivity %.2e)" % (name, s, err, err32, sens))
    print("largest gradient error vs fp64: HIP fp32 %.2e (torch fp32 %.2e, fp64 sensitivity %.2e) at %s" % worst)
    assert not bad, "\n".join(bad)
    torch.testing.assert_close(hip.running, ref.running, rtol=1e-4, atol=1e-5)


def test_auto_backend_routes_fp32_building_blocks():
    """--backend auto --dtype fp32: ResNet-18 v2 at ImageNet shape runs the fp32 HIP plan, v1 stays on PyTorch."""
    dev = torch.device("cuda")
    for version, name in ((2, "HipImageNetF32Backend"), (1, "TorchBackend")):
        arch = ResNetArch(imagenet_config(18, version, num_classes=1001, image_size=64))
        eng = PopulationEngine(arch, 1, dev, backend="torch", compute_dtype=torch.float32)
        assert make_backend(eng, "auto").__class__.__name__ == name


def test_hip_imagenet_blocks_f32_eval_matches_oracle(monkeypatch):
    """The ResNet-50 fp32 eval test (logits within 1e-3 relative L2 of the fp32 forward, exact accuracy) on ResNet-18."""
    import test_gpu_imagenet_f32 as t50
    monkeypatch.setattr(t50, "imagenet_config", lambda size, *a, **kw: imagenet_config(18, *a, **kw))
    t50.test_hip_imagenet_f32_eval_matches_oracle()
