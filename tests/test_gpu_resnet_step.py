"""Population-batched HIP ResNet step vs the plain-PyTorch fp32 oracle.

Both engines start from identical member rows; one optimizer step with plain
gradient descent (lr = 1) turns ``params_before - params_after`` into the
gradient, which is compared PER LAYER (localises a wrong kernel), together with
the loss and the BN running statistics.  Members use different batch sizes
(ragged population packing).
"""
import os

import pytest
import torch

from distributedtf_amd.engine.population import PopulationEngine
from distributedtf_amd.models.resnet import ResNetArch, cifar_config

pytestmark = pytest.mark.gpu


def _hp(bs):
    return {"opt_case": {"optimizer": "gd", "lr": 1.0}, "batch_size": bs, "regularizer": "None",
            "weight_decay": 0.0, "initializer": "he_init", "decay_steps": 0, "decay_rate": 1.0}


def _cos(a, b):
    a, b = a.flatten().double(), b.flatten().double()
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))


def _relerr(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _perturb_bn(arch, engines, n, g):
    dev = engines[0].state.device
    for b in arch.prog.bns:
        noise_g = 1.0 + 0.2 * torch.randn(n, b.c, generator=g)
        noise_b = 0.1 * torch.randn(n, b.c, generator=g)
        for e in engines:
            e.state[:n, b.gamma_off:b.gamma_off + b.c] = noise_g.to(dev)
            e.state[:n, b.beta_off:b.beta_off + b.c] = noise_b.to(dev)


def _compare_step(arch, sizes, floor=0.06, seed=0, warm_sizes=None, check=None, active=None):
    """Two optimizer steps on the same batches: step 1 with lr = 0 (the eager warm-up that also captures the HIP
    graph), step 2 with lr = 1 (the first graph REPLAY: device-side step advance, hyper-table refresh, in-graph
    loss gather).  Step 2's parameter delta is its gradient, compared per layer with the fp32 oracle."""
    torch.manual_seed(seed)
    dev = torch.device("cuda")
    n = len(sizes)
    ref = PopulationEngine(arch, n, dev, backend="torch", compute_dtype=torch.float32, optimizer_impl="hip")
    r16 = PopulationEngine(arch, n, dev, backend="torch", compute_dtype=torch.bfloat16, optimizer_impl="hip")
    hip = PopulationEngine(arch, n, dev, backend="hip")
    slots = []
    for i, bs in enumerate(sizes):
        s1 = ref.add_member(None, _hp(bs), seed=10 + i)
        s2 = hip.add_member(None, _hp(bs), seed=10 + i)
        r16.add_member(None, _hp(bs), seed=10 + i)
        assert s1 == s2
        slots.append(s1)
    # perturb BN gammas/betas so the BN paths are exercised away from identity
    g = torch.Generator(device="cpu").manual_seed(1 + seed)
    _perturb_bn(arch, (ref, hip, r16), n, g)
    assert torch.equal(ref.state, hip.state)
    batches = []
    for bs in sizes:
        x = torch.randn(bs, 32, 32, 3, generator=g).to(dev)
        y = torch.randint(0, 10, (bs,), generator=g).to(dev)
        batches.append((x, y))
    hps = [_hp(bs) for bs in sizes]
    if warm_sizes is not None:  # an earlier step with other batch sizes (elastic plans: no new plan / capture)
        warm = [(torch.randn(bs, 32, 32, 3, generator=g).to(dev), torch.randint(0, 10, (bs,), generator=g).to(dev))
                for bs in warm_sizes]
        for e in (ref, r16, hip):
            e.train_step(slots, warm, [_hp(bs) for bs in warm_sizes], [0.0] * n)
            e.train_step(slots, warm, [_hp(bs) for bs in warm_sizes], [0.0] * n)
        plans0 = dict(hip.backend._plans)
    for e in (ref, r16, hip):
        e.train_step(slots, batches, hps, [0.0] * n)
    if check is not None:
        check(hip, plans0 if warm_sizes is not None else None)
    before = hip.params.clone()
    assert torch.equal(before, ref.params)
    full = slots
    if active is not None:  # the compared step trains only these members (an elastic plan's subset replay)
        plans0 = dict(hip.backend._plans)
        state0 = hip.state.clone()
        pos = [slots.index(s) for s in active]
        slots, batches, hps = list(active), [batches[i] for i in pos], [hps[i] for i in pos]
    l_ref = ref.train_step(slots, batches, hps, [1.0] * len(slots))
    r16.train_step(slots, batches, hps, [1.0] * len(slots))
    l_hip = hip.train_step(slots, batches, hps, [1.0] * len(slots))
    torch.cuda.synchronize()
    if active is not None:
        assert dict(hip.backend._plans) == plans0, "a subset step must replay the existing elastic plan"
        for s in full:
            if s not in active:  # idle member: parameters, optimizer slots, BN moving statistics, step counter
                assert torch.equal(hip.state[s], state0[s]), s
        assert hip.host_step == ref.host_step
    torch.testing.assert_close(l_hip.float(), l_ref.float(), rtol=3e-2, atol=3e-2)
    g_ref = before - ref.params
    g_hip = before - hip.params
    g_16 = before - r16.params
    prog = arch.prog
    report = []
    segs = [("conv%d" % c.idx, c.off, c.off + c.numel) for c in prog.convs]
    for bn in prog.bns:
        segs += [("bn%d.gamma" % bn.idx, bn.gamma_off, bn.gamma_off + bn.c),
                 ("bn%d.beta" % bn.idx, bn.beta_off, bn.beta_off + bn.c)]
    segs.append(("dense", prog.dense_w_off, prog.dense_b_off + arch.cfg.num_classes))
    for s in slots:
        for name, lo, hi in segs:
            a, b, c16 = g_hip[s, lo:hi], g_ref[s, lo:hi], g_16[s, lo:hi]
            # tolerance = what a bf16 PyTorch run of the same step deviates from fp32, x2.5
            tol = max(2.5 * _relerr(c16, b), floor)
            report.append((name, s, _cos(a, b), _relerr(a, b), tol))
    bad = [r for r in report if r[3] > r[4]]
    assert not bad, "\n".join("%s member %d cos %.4f rel %.4f tol %.4f" % r for r in bad)
    torch.testing.assert_close(hip.running, ref.running, rtol=2e-2, atol=2e-3)
    torch.testing.assert_close(hip.step_col(), ref.step_col())
    return max(r[3] for r in report)


_STEP_CASES = [(8, "1", 2, [8, 12, 6]), (14, "1", 2, [8, 12, 6]), (14, "0", 2, [8, 12, 6]),
               (14, "1", 2, [8, 12]), (20, "0", 2, [8, 12]), (14, "1", 2, [16]),
               (8, "1", 1, [8, 12]), (14, "0", 1, [8, 12]), (20, "1", 1, [8, 12]),
               (20, "1", 2, [16, 24]), (14, "1", 1, [8, 12])]


def _launch_counts(hip):
    """Launcher symbol -> launches in the training plans of this engine's backend."""
    from distributedtf_amd import ops
    counts = {}
    for p in hip.backend._plans.values():
        for fn, _ in p.launches:
            if not isinstance(fn, str):
                name = ops.launcher_name(fn)
                counts[name] = counts.get(name, 0) + 1
    return counts


@pytest.mark.parametrize("size,graph,version,sizes", _STEP_CASES,
                         ids=["v%d-r%d-g%s-pop%d" % (v, n, g, len(z)) for n, g, v, z in _STEP_CASES])
def test_hip_step_matches_reference(size, graph, version, sizes, monkeypatch):
    """Three members: the fused backward launches (BN1-backward folded into the next conv_b staging, dW slab
    reductions carried by the next launch) next to the dgrad-only launches of the widths whose wgrad is deferred;
    one or two members: every stride-1 layer runs a dgrad-only launch (conv_bwd_dg_kernel) and its wgrad as a
    queued job of the wide launches after the backward (conv_wgrad_all_kernel); v1: fused launches only -- with
    and without graphs, ragged and single-member populations.  The plan's launch list is checked to hold exactly
    those kernels."""
    monkeypatch.setenv("DTF_HIP_GRAPH", graph)

    def check(hip, plans0):
        n = _launch_counts(hip)
        fused, dg, wg_all = (n.get(k, 0) for k in ("dtf_conv_bwd_fused", "dtf_conv_bwd_dg", "dtf_conv_wgrad_all"))
        if version == 1:
            assert fused >= 1 and dg == 0, n
        elif len(sizes) <= 2 and not hip.backend.det:
            assert dg >= 1 and wg_all in (1, 2) and fused == 0, n
        else:  # (also the deterministic build at any size -- tests/test_gpu_eval.py runs a case of this test on
            # it: its plans never switch kernel families with the population, C = 64 alone defers its wgrad)
            assert fused >= 1 and dg >= 1 and wg_all in (1, 2), n

    _compare_step(ResNetArch(cifar_config(size, version=version)), sizes, check=check)


@pytest.mark.parametrize("version", [2, 1])
@pytest.mark.parametrize("elastic", ["auto", "0"])
def test_hip_step_elastic_plan(elastic, version, monkeypatch):
    """Mixed batch sizes run on ONE capacity-keyed plan (DTF_ELASTIC): the work tables are regenerated on the device
    from the per-member sizes each step, so a batch-size change (PBT explore of batch_size) reuses the captured
    graph.  Warm-up with sizes (20, 9, 14), then the compared graph replay with (12, 17, 6) vs the fp32 oracle;
    DTF_ELASTIC=0 (exact plans, one per size tuple) as the control.  v1: the per-image BN kernels (bn_add_relu,
    bn_bwd_reduce) skip each member's capacity padding."""
    monkeypatch.setenv("DTF_HIP_GRAPH", "1")
    monkeypatch.setenv("DTF_ELASTIC", elastic)
    monkeypatch.setenv("DTF_ELASTIC_MAXB", "24")

    def check(hip, plans0):
        plans = hip.backend._plans
        if elastic == "auto":
            assert len(plans) == 1 and list(plans) == list(plans0), list(plans)
            p = next(iter(plans.values()))
            assert p.elastic and p.graph is not None and p.graph is plans0[next(iter(plans0))].graph
        else:
            assert len(plans) == 2 and not any(p.elastic for p in plans.values())

    _compare_step(ResNetArch(cifar_config(14, version=version)), [12, 17, 6], warm_sizes=[20, 9, 14], check=check)


@pytest.mark.parametrize("size,sizes", [(56, [128] * 8), (56, [128]), (110, [128, 128])])
def test_hip_step_benchmark_shapes(size, sizes, monkeypatch):
    """The shapes bench.py times (ResNet-56 v2 at pop 8 x 128 and pop 1 x 128; ResNet-110 at pop 2 x 128): the
    workgroup splits, dW slab budgets and piggyback reductions chosen there (hip_resnet._fused_nwg) and the
    small populations' dgrad-only launches with deferred wgrad jobs (conv_bwd_dg_kernel, conv_wgrad_all_kernel)
    are checked numerically, on the graph-replayed step."""
    monkeypatch.setenv("DTF_HIP_GRAPH", "1")
    worst = _compare_step(ResNetArch(cifar_config(size, version=2)), sizes, floor=0.04)
    print("worst per-layer relative error %.4f" % worst)


def test_hip_step_repeat_and_population_capacity():
    """Several graph replays with members on different optimizers stay finite and learn."""
    arch = ResNetArch(cifar_config(20))
    dev = torch.device("cuda")
    eng = PopulationEngine(arch, 4, dev, backend="hip")
    opts = ["Momentum", "Adam", "RMSProp", "gd"]
    hps = []
    for i, o in enumerate(opts):
        hp = {"opt_case": {"optimizer": o, "lr": {"Adam": 1e-3, "RMSProp": 1e-4}.get(o, 0.05), "momentum": 0.9,
                           "grad_decay": 0.9}, "batch_size": 16, "regularizer": "l2_regularizer",
              "weight_decay": 1e-4, "initializer": "he_init"}
        eng.add_member(None, hp, seed=i)
        hps.append(hp)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(16, 32, 32, 3, generator=g).to(dev)
    y = torch.randint(0, 10, (16,), generator=g).to(dev)
    losses = []
    for it in range(12):
        l = eng.train_step([0, 1, 2, 3], [(x, y)] * 4, hps, [hp["opt_case"]["lr"] for hp in hps])
        losses.append(l.cpu())
    torch.cuda.synchronize()
    L = torch.stack(losses)
    assert torch.isfinite(L).all()
    assert (L[-1] < L[0]).all(), L  # memorising one fixed batch must reduce the loss
    assert eng.host_step[:4] == [12] * 4


def test_hip_step_shrinking_active_set(monkeypatch):
    """Members that finish their epoch drop out of the active set (engine_model._train_cycle): the elastic plan of
    the full set is replayed with zero images for them -- no new plan or capture.  The idle member's parameters,
    optimizer slots, BN moving statistics and step counter stay untouched; the active members' step-2 gradients
    match the fp32 oracle (reference training_worker.py:64-69: members train independently)."""
    monkeypatch.setenv("DTF_HIP_GRAPH", "1")
    _compare_step(ResNetArch(cifar_config(14, version=2)), [20, 9, 14], active=[0, 2])

