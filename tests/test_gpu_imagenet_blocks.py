"""ImageNet-shape ResNet-18 / 34 (v2 building blocks) on the HIP kernels (engine/hip_imagenet.py ``_bb_forward`` /
``_bb_backward``): one training step against the fp32 PyTorch step of the same net, routing, and eval.

The step's bound is the rule of tests/test_gpu_imagenet_step.py: max(floor, 2.5 x the deviation of a bf16 PyTorch run
of the same step from the fp32 reference), floors 3 % (loss), 0.06 (per-parameter relative gradient error) and
rtol 3e-2 / atol 5e-3 (running statistics).  Image 64: stages of 16 / 8 / 4 / 2 pixels, every conv on the generic
kernel.  Image 224: the row-band kernel at 56 / 28 / 14 and packs of whole 7 x 7 images in the last stage -- asserted
on the plan's launch list -- and, with the width-7 entry dropped from ``_CG_T3``, the generic kernel there instead.
"""
import pytest
import torch

from distributedtf_amd.engine.population import PopulationEngine, make_backend
from distributedtf_amd.models.resnet import ResNetArch, imagenet_config

gpu = pytest.mark.gpu


def _hp(bs):
    return {"opt_case": {"optimizer": "gd", "lr": 1.0}, "batch_size": bs, "regularizer": "None",
            "weight_decay": 0.0, "initializer": "he_init"}


def _relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


@gpu
@pytest.mark.parametrize("size,image,graph,t3w7", [(18, 64, "1", True), (18, 64, "0", True), (34, 64, "1", True),
                                                   (18, 224, "1", True), (34, 224, "1", True), (18, 224, "1", False)])
def test_hip_imagenet_blocks_step_matches_reference(monkeypatch, size, image, graph, t3w7):
    """Step 1 (lr 0) captures the graph; the parameter delta of step 2 (lr 1: a graph replay, or a second eager run)
    is the gradient.  Members of 2 and 3 images."""
    from distributedtf_amd import ops
    from distributedtf_amd.engine import hip_imagenet
    monkeypatch.setenv("DTF_HIP_GRAPH", graph)
    if not t3w7:
        monkeypatch.setattr(hip_imagenet, "_CG_T3", {k: v for k, v in hip_imagenet._CG_T3.items() if k != 7})
    torch.manual_seed(0)
    arch = ResNetArch(imagenet_config(size, 2, num_classes=1001, image_size=image))
    dev, sizes = torch.device("cuda"), [2, 3]
    ref = PopulationEngine(arch, 2, dev, backend="torch", compute_dtype=torch.float32, optimizer_impl="hip")
    r16 = PopulationEngine(arch, 2, dev, backend="torch", compute_dtype=torch.bfloat16, optimizer_impl="hip")
    hip = PopulationEngine(arch, 2, dev, backend="hip")
    assert hip.backend.__class__.__name__ == "HipImageNetBackend"
    slots = [e.add_member(None, _hp(bs), seed=3 + i) for i, bs in enumerate(sizes) for e in (ref, r16, hip)][::3]
    g = torch.Generator().manual_seed(1)
    for b in arch.prog.bns:
        ng, nb = 1.0 + 0.2 * torch.randn(2, b.c, generator=g), 0.1 * torch.randn(2, b.c, generator=g)
        for st in (ref.state, hip.state, r16.state):
            st[:, b.gamma_off:b.gamma_off + b.c] = ng.to(dev)
            st[:, b.beta_off:b.beta_off + b.c] = nb.to(dev)
    batches = [(torch.randn(bs, image, image, 3, generator=g).to(dev),
                torch.randint(0, 1001, (bs,), generator=g).to(dev)) for bs in sizes]
    before = hip.params.clone()
    hps = [_hp(bs) for bs in sizes]
    for e in (ref, r16, hip):
        e.train_step(slots, batches, hps, [0.0, 0.0])
    torch.cuda.synchronize()
    assert torch.equal(hip.params, before)
    plan = next(iter(hip.backend._plans.values()))
    assert (plan.graph is not None) == (graph == "1")
    # stride-1 3x3 convs of the last stage (forward and data gradient) as packs of whole 7 x 7 images
    packed = sum(1 for fn, args in plan.launches
                 if not isinstance(fn, str) and ops.launcher_name(fn) == "dtf_convg_t3" and args[4] == 7)
    last = arch.cfg.block_sizes[-1]
    assert packed == (2 * (2 * last - 1) if image == 224 and t3w7 else 0), packed
    l_ref, l16, l_hip = (e.train_step(slots, batches, hps, [1.0, 1.0]).float() for e in (ref, r16, hip))
    torch.cuda.synchronize()
    e_hip, e16 = ((l - l_ref).abs() / l_ref.abs() for l in (l_hip, l16))
    print("loss rel: hip %s, torch bf16 %s" % (e_hip.tolist(), e16.tolist()))
    torch.testing.assert_close(l_hip, l_ref, rtol=max(3e-2, 2.5 * float(e16.max())), atol=3e-2)
    g_ref, g_hip, g16 = before - ref.params, before - hip.params, before - r16.params
    prog = arch.prog
    segs = [("conv%d" % c.idx, c.off, c.off + c.numel) for c in prog.convs]
    for bn in prog.bns:
        segs += [("bn%d.gamma" % bn.idx, bn.gamma_off, bn.gamma_off + bn.c),
                 ("bn%d.beta" % bn.idx, bn.beta_off, bn.beta_off + bn.c)]
    segs.append(("dense", prog.dense_w_off, prog.dense_b_off + arch.cfg.num_classes))
    bad, worst = [], (0.0, 0.0, "")
    for s in slots:
        for name, lo, hi in segs:
            err, e16 = _relerr(g_hip[s, lo:hi], g_ref[s, lo:hi]), _relerr(g16[s, lo:hi], g_ref[s, lo:hi])
            worst = max(worst, (err, e16, name))
            if err > max(2.5 * e16, 0.06):
                bad.append("%s member %d rel %.4f (torch bf16 %.4f)" % (name, s, err, e16))
    print("largest gradient rel: hip %.4f (torch bf16 %.4f) at %s" % worst)
    assert not bad, "\n".join(bad)
    torch.testing.assert_close(hip.running, ref.running, rtol=3e-2, atol=5e-3)


@gpu
def test_auto_backend_routes_building_blocks():
    """--backend auto: ResNet-18 v2 at ImageNet shape runs the HIP plan, the v1 building blocks stay on PyTorch."""
    dev = torch.device("cuda")
    for version, name in ((2, "HipImageNetBackend"), (1, "TorchBackend")):
        arch = ResNetArch(imagenet_config(18, version, num_classes=1001, image_size=64))
        eng = PopulationEngine(arch, 1, dev, backend="torch")
        assert make_backend(eng, "auto").__class__.__name__ == name


@pytest.mark.parametrize("size", [18, 34])
def test_hip_supported_building_blocks(size):
    assert ResNetArch(imagenet_config(size, 2, image_size=224)).hip_supported
    assert not ResNetArch(imagenet_config(size, 1, image_size=224)).hip_supported
    assert not ResNetArch(imagenet_config(size, 2, image_size=200)).hip_supported


@gpu
def test_hip_imagenet_blocks_eval_matches_reference(monkeypatch):
    """Eval-mode logits of ResNet-18 v2 members (64 x 64 input) against the fp32 forward, held to the bound of
    tests/test_gpu_eval.py for ResNet-50: max(0.05, 2.5 x the deviation of the bf16 PyTorch forward)."""
    from test_gpu_eval import _population
    arch = ResNetArch(imagenet_config(18, 2, num_classes=1001, image_size=64))
    eng, g = _population(arch, 2, monkeypatch, seed=9)
    assert eng.backend.__class__.__name__ == "HipImageNetBackend"
    x = torch.randn(12, 64, 64, 3, generator=g).to(eng.state.device)
    for s in range(2):
        ref, r16 = (arch.forward(eng.params[s], eng.running[s].clone(), x, training=False, dtype=dt).float()
                    for dt in (torch.float32, torch.bfloat16))
        err, e16 = _relerr(eng.backend.infer(s, x), ref), _relerr(r16, ref)
        print("member %d: hip rel %.4f, torch bf16 rel %.4f" % (s, err, e16))
        assert err < max(2.5 * e16, 0.05), (s, err, e16)
