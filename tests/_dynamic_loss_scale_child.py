"""Child process of tests/test_gpu_dynamic_loss_scale.py: the kernel library is one per process, chosen at load time
(DTF_HALF / DTF_DETERMINISTIC), so every build runs these checks in a process of its own.

    python tests/_dynamic_loss_scale_child.py kernels      the three new launchers + the head with a scale table
    python tests/_dynamic_loss_scale_child.py step         the whole fp16 step (half builds only), graph and eager

Oracles: engine/optim.py ``loss_scale_update`` (the rule), the static entry points of the same library
(``dtf_fused_optimizer``, the scalar ``loss_scale`` of the head) and, for the whole step of the release fp16 build, a
static-scale engine within 4 x the deviation measured between two runs of that static engine."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from distributedtf_amd import ops  # noqa: E402
from distributedtf_amd.engine import optim as O  # noqa: E402

dev = torch.device("cuda")
INF, NAN = float("inf"), float("nan")


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=dev)


# ---------------------------------------------------------------------------------------- finiteness pass
def check_finite(P):
    cap, slots = 3, [0, 2]
    Pp = (P + 63) // 64 * 64
    g = torch.Generator().manual_seed(5)
    base = torch.randn(cap, Pp, generator=g)
    base[:, P:] = 0.0
    # finite extremes: FLT_MAX, the smallest normal, denormals, -0
    fmax = torch.finfo(torch.float32).max
    for s in range(cap):
        base[s, 1 % P], base[s, 2 % P], base[s, 3 % P] = fmax, -fmax, torch.finfo(torch.float32).tiny
        base[s, 4 % P] = 1e-45
        base[s, P - 2], base[s, P // 2] = -1e-40, -0.0
    canary = torch.tensor([[4.0, 7.0, 0.0, 3.0], [-5.0, -6.0, -7.0, -8.0], [8.0, 1.0, 0.0, 2.0]])

    def case(name, edit, want0, want2, flags0=(0.0, 0.0)):
        gr = base.clone()
        edit(gr)
        gd = gr.to(dev)
        tab = canary.clone()
        tab[0, 2], tab[2, 2] = flags0
        td = tab.to(dev)
        ops.grad_finite_check(gd, Pp, P, i32(slots), td)
        torch.cuda.synchronize()
        got = td.cpu()
        want = tab.clone()
        want[0, 2], want[2, 2] = want0, want2
        assert same(got, want), (name, P, got.tolist(), want.tolist())
        assert same(gd.cpu(), gr), (name, "gradients written")
        print("finite_check P=%d %-28s flags %s ok" % (P, name, [got[0, 2].item(), got[2, 2].item()]))

    def at(s, i, v):
        def f(gr):
            gr[s, i] = v
        return f

    def fill(s, lo, hi, v):
        def f(gr):
            gr[s, lo:hi] = v
        return f

    case("all finite", lambda gr: None, 0.0, 0.0)
    case("all finite, flag kept (OR)", lambda gr: None, 1.0, 0.0, flags0=(1.0, 0.0))
    case("+Inf at 0", at(0, 0, INF), 1.0, 0.0)
    case("NaN at P-1", at(0, P - 1, NAN), 1.0, 0.0)
    case("NaN at P-1 of slot 2", at(2, P - 1, NAN), 0.0, 1.0)
    case("-Inf mid-row, slot 2 only", at(2, P // 2 + 1, -INF), 0.0, 1.0)
    case("NaN in the padding", lambda gr: gr[:, P:].fill_(NAN), 0.0, 0.0)
    case("NaN in idle slot 1", fill(1, 0, Pp, NAN), 0.0, 0.0)
    case("both members", lambda gr: (at(0, P // 3, -NAN)(gr), at(2, 0, INF)(gr)), 1.0, 1.0)


# ------------------------------------------------------------------------------------ optimizer with table
def check_optimizer():
    torch.manual_seed(0)
    P, Pp, n_reg = 1003, 1024, 500
    S = 3 * Pp + 64
    dt = ops.act_dtype()
    opts = list(O.OPT_CODES)
    regs = [None, "l1_regularizer", "l2_regularizer", "l1_l2_regularizer", "l2_regularizer", None]
    G = 14  # 0-5 clean (one optimizer each), 6-11 flagged (one optimizer each), 12 inactive, 13 inactive + flagged
    ks = [7, 15, 3, 0, 24, 10]
    state = torch.randn(G, S)
    state[:, Pp:2 * Pp] = state[:, Pp:2 * Pp].abs() + 0.15
    state[:, 2 * Pp:3 * Pp] = state[:, 2 * Pp:3 * Pp].abs() * 0.1
    for lo in (0, Pp, 2 * Pp):
        state[:, lo + P:lo + Pp] = 0.0  # the rows' padding is zero, as in the engine
    grads = torch.randn(G, Pp)
    grads[:, P:] = 0.0
    hyper = torch.zeros(G, 8)
    lscale = torch.zeros(G, 4)
    for g in range(G):
        o = g % 6
        hp = {"opt_case": {"optimizer": opts[o], "lr": 0.01, "momentum": 0.7, "grad_decay": 0.8},
              "weight_decay": 1e-3, "regularizer": regs[o]}
        hyper[g] = torch.tensor(O.hyper_row(hp, 0.01 * (g + 1), 3 + g, active=g < 12))
        lscale[g] = torch.tensor([2.0 ** ks[o], float(g), 1.0 if (6 <= g < 12 or g == 13) else 0.0, 5.0])
        grads[g, :P] *= 2.0 ** ks[o]  # gradients of scale * loss
        if lscale[g, 2] != 0:
            grads[g, 0], grads[g, P - 1], grads[g, 17], grads[g, P // 2] = INF, NAN, -INF, -NAN
    shadow0 = torch.full((G, Pp), 0.4321).to(dt)
    st, gr, sh, ls, hy = state.to(dev), grads.to(dev), shadow0.to(dev), lscale.to(dev), hyper.to(dev)
    ops.fused_optimizer(st, gr, hy, Pp, P, n_reg, shadow=sh, zero_grads=True, lscale=ls)
    torch.cuda.synchronize()
    assert same(ls.cpu(), lscale) and same(hy.cpu(), hyper), "the optimizer wrote a table"
    st, gr, sh = st.cpu(), gr.cpu(), sh.cpu()
    for g in range(6):  # clean at scale 2^k: bitwise the static launch with gscale = 2^-k
        s2, g2, h2 = state.to(dev), grads.to(dev), shadow0.to(dev)
        ops.fused_optimizer(s2, g2, hy, Pp, P, n_reg, shadow=h2, zero_grads=True, grad_scale=2.0 ** -ks[g])
        torch.cuda.synchronize()
        assert same(st[g], s2[g].cpu()) and same(sh[g], h2[g].cpu()) and same(gr[g], g2[g].cpu()), ("clean", g)
        assert not same(st[g, :P], state[g, :P]) and not gr[g].any()
        assert torch.isfinite(st[g]).all()
    for g in range(6, 12):  # flagged: weights, slots, shadow keep every bit; the gradient row is zeroed
        assert same(st[g], state[g]) and same(sh[g], shadow0[g]), ("flagged", g)
        assert same(gr[g], torch.zeros(Pp)), ("flagged gradients", g)
    for g in (12, 13):  # inactive: untouched, gradients included
        assert same(st[g], state[g]) and same(sh[g], shadow0[g]) and same(gr[g], grads[g]), ("inactive", g)
    # without zero_grads a flagged member's gradients stay too
    s3, g3 = state.to(dev), grads.to(dev)
    ops.fused_optimizer(s3, g3, hy, Pp, P, n_reg, shadow=None, zero_grads=False, lscale=ls)
    torch.cuda.synchronize()
    assert same(s3[6:].cpu(), state[6:]) and same(g3.cpu(), grads)
    print("optimizer with table: 6 clean bitwise == static, 6 flagged skipped + zeroed, 2 inactive untouched ok")


# ------------------------------------------------------------------------------------------- scale update
def check_update():
    cap, slots, interval = 5, [0, 1, 3, 4], 3
    hyper = torch.zeros(cap, 8)
    hyper[:, 7] = torch.tensor([1.0, 1.0, 1.0, 0.0, 1.0])  # member 3 listed but inactive; member 2 not listed
    rows = [[2.0 ** 15, 0, 0, 0], [2.0, 2, 0, 4], [64.0, 1, 1, 1], [32.0, 1, 1, 6], [2.0 ** 23, 0, 0, 0]]
    flags = {0: [0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0], 1: [1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0],
             4: [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0]}
    tab = torch.tensor(rows, dtype=torch.float32).to(dev)
    hy = hyper.to(dev)
    want = [list(map(float, r)) for r in rows]
    seen = set()
    for step in range(12):
        for s, f in flags.items():
            tab[s, 2] = float(f[step])
            want[s][2] = float(f[step])
        ops.loss_scale_update(tab, hy, i32(slots), interval)
        torch.cuda.synchronize()
        for s in flags:
            want[s] = O.loss_scale_update(want[s], interval)
        got = tab.cpu().tolist()
        assert got == want, (step, got, want)  # exact; rows 2 (not listed) and 3 (inactive) keep found_inf too
        assert all(got[s][2] == 0.0 for s in flags)
        seen.update(r[0] for r in got)
    assert 1.0 in seen and 2.0 ** 24 in seen and want[0][3] == 3.0, (seen, want)  # the floor and the cap were reached
    print("scale update: 12 steps x 3 members exact, inactive / unlisted rows unchanged ok ->", want)


# --------------------------------------------------------------------------------- head with a scale table
def check_head():
    import _resnet_aux_exact as rx
    import test_gpu_resnet_aux as tg
    _, hr, _, nrep, det = tg._env()
    k = rx.head_case(32, 10, 1, nrep)
    scales = {0: 2.0 ** 7, 2: 2.0 ** 3}
    n0, n2 = rx.HEAD_SIZES
    nw = len(rx.HEAD_WORK)  # rows of the slabs that _Head allocates
    joint = [[0, n0, 0, 0], [n0, n2, 0, 2]]  # one workgroup per member

    def launch(work, use_slab, scale, tab):
        h = tg._Head(ops, hr, dev, k, 1, scale, use_slab)
        h.a.work, h.nb = h.b.ints(work), len(work)
        if tab is not None:
            h.tab = torch.tensor(tab, dtype=torch.float32, device=dev)
            h.a.scale_tab = h.tab.data_ptr()
        tg.run(ops.lib().dtf_head(ctypes.byref(h.a), h.nb, ops.stream()))
        return h

    live = lambda h, name, shape: tg.live64(getattr(h, name), shape)  # noqa: E731
    tab = [[scales[0], 1.0, 0.0, 0.0], [NAN, NAN, NAN, NAN], [scales[2], 2.0, 0.0, 9.0]]
    for use_slab in ([1] if det else [1, 0]):  # the atomic form is bitwise at one workgroup per member (release build)
        hd = launch(joint, use_slab, 12345.0, tab)  # the scalar is ignored with a table
        assert same(hd.tab.cpu(), torch.tensor(tab)), "the head wrote the table"
        for item, (s, f, e) in enumerate(((0, 0, n0), (2, n0, n0 + n2))):
            alone = [list(w) for w in joint]
            alone[1 - item][1] = 0  # the other member has no image in this launch
            hs = launch(alone, use_slab, scales[s], None)
            assert same(live(hd, "dfeat", (k.n, 64))[f:e], live(hs, "dfeat", (k.n, 64))[f:e]), ("dfeat", s, use_slab)
            assert same(live(hd, "stb", k.stb0.shape)[s], live(hs, "stb", k.stb0.shape)[s]), ("st_b", s, use_slab)
            if use_slab:
                assert same(live(hd, "slab", (nw, k.ncls * 64))[item], live(hs, "slab", (nw, k.ncls * 64))[item])
                assert same(live(hd, "slab_b", (nw, k.ncls))[item], live(hs, "slab_b", (nw, k.ncls))[item])
            assert same(live(hd, "grads", k.grads0.shape)[s], live(hs, "grads", k.grads0.shape)[s]), ("grads", s)
            if not use_slab:
                assert not same(live(hd, "grads", k.grads0.shape)[s], k.grads0[s].double()), "no dense gradient"
            # loss and correct do not see the scale
            assert same(live(hd, "loss", (rx.CAP,))[s], live(hs, "loss", (rx.CAP,))[s])
            assert same(live(hd, "correct", (rx.CAP,))[s], live(hs, "correct", (rx.CAP,))[s])
        # the two members really ran at different scales: member 0 at 2^3 differs from member 0 at 2^7
        h8 = launch(joint, use_slab, 2.0 ** 3, None)
        assert not same(live(hd, "dfeat", (k.n, 64))[:n0], live(h8, "dfeat", (k.n, 64))[:n0])
        assert same(live(hd, "dfeat", (k.n, 64))[n0:], live(h8, "dfeat", (k.n, 64))[n0:])
        assert same(live(hd, "loss", (rx.CAP,)), live(h8, "loss", (rx.CAP,)))
        assert same(live(hd, "correct", (rx.CAP,)), live(h8, "correct", (rx.CAP,)))
        print("head with scale_tab (%s form): dfeat, dense / bias gradients, st_b bitwise == scalar launches ok"
              % ("slab" if use_slab else "atomic"))


# --------------------------------------------------------------------------------------------- whole step
def hp(bs=8):
    return {"opt_case": {"optimizer": "Momentum", "lr": 0.05, "momentum": 0.9}, "batch_size": bs,
            "regularizer": "l2_regularizer", "weight_decay": 1e-4, "initializer": "he_init", "decay_steps": 0,
            "decay_rate": 1.0}


def check_step(use_graph):
    from distributedtf_amd.engine import hip_step
    from distributedtf_amd.engine.population import PopulationEngine
    from distributedtf_amd.models.resnet import ResNetArch, cifar_config
    assert ops.build_half(), "the whole-step check runs on the fp16 builds"
    det = ops.build_deterministic()
    arch = ResNetArch(cifar_config(8, 2))
    n, bs = 3, 8
    mode = "graph" if use_graph else "eager"

    def engine(loss_scale):
        e = PopulationEngine(arch, n, dev, backend="hip", compute_dtype=torch.float16, loss_scale=loss_scale)
        e.backend.use_graph = use_graph
        for i in range(n):
            assert e.add_member(None, hp(bs), seed=10 + i) == i
        return e

    sa, sb, dy = engine(128.0), engine(128.0), engine("dynamic")
    assert same(sa.state, dy.state) and dy.dynamic_loss_scale and not sa.dynamic_loss_scale
    assert dy.lscale.cpu().tolist() == [[2.0 ** 15, 0.0, 0.0, 0.0]] * n
    g = torch.Generator().manual_seed(1)
    batches = [(torch.randn(bs, 32, 32, 3, generator=g).to(dev), torch.randint(0, 10, (bs,), generator=g).to(dev))
               for _ in range(n)]
    slots, hps, lrs = list(range(n)), [hp(bs)] * n, [0.05] * n
    calls = {"check": 0, "update": 0, "dyn": 0}
    real = (ops.grad_finite_check, ops.loss_scale_update, ops.fused_optimizer)

    def counted(key, fn):
        def f(*a, **kw):
            if key != "dyn" or kw.get("lscale") is not None:
                calls[key] += 1
            return fn(*a, **kw)
        return f

    ops.grad_finite_check, ops.loss_scale_update = counted("check", real[0]), counted("update", real[1])
    ops.fused_optimizer = counted("dyn", real[2])
    try:
        def set_scales(v, keep_counts=True):
            rows = dy.lscale.cpu().tolist()
            for s, x in enumerate(v):
                dy.set_loss_scale_row(s, [x, 0.0, 0.0, rows[s][3] if keep_counts else 0.0])

        # step 1 (the eager warm-up that precedes the capture): all members at the static engine's scale
        set_scales([2.0 ** 7] * n)
        for e in (sa, sb):
            e.train_step(slots, batches, hps, lrs)
        assert calls == {"check": 0, "update": 0, "dyn": 0}, ("a static step launched the dynamic kernels", calls)
        dy.train_step(slots, batches, hps, lrs)
        torch.cuda.synchronize()
        first = 2 if use_graph else 1  # graph mode: the eager warm-up, then the same launches recorded by the capture
        assert calls == {"check": first, "update": first, "dyn": first}, calls
        names = lambda e: [fn if isinstance(fn, str) else ops.launcher_name(fn)  # noqa: E731
                           for p in e.backend._plans.values() for fn, _ in p.launches]
        assert names(sa) == names(dy) and "optim" in names(sa), "the launch lists differ outside the optim marker"
        assert dy.lscale.cpu().tolist() == [[2.0 ** 7, 1.0, 0.0, 0.0]] * n
        # step 2 (a graph replay in graph mode): member 1 at 2^40 overflows its fp16 gradient tensors
        set_scales([2.0 ** 7, 2.0 ** 40, 2.0 ** 7])
        before = dy.state.clone()
        for e in (sa, sb, dy):
            loss = e.train_step(slots, batches, hps, lrs)
        torch.cuda.synchronize()
        if use_graph:
            assert hip_step.graph_state(dy.backend) == "captured" and calls["check"] == first, (calls, "not a replay")
        assert torch.isfinite(loss).all(), loss  # the loss does not see the scale
        P, Pp, R = dy.P, dy.Pp, dy.R
        cols = {"params": (0, P), "slot1": (Pp, Pp + P), "slot2": (2 * Pp, 2 * Pp + P), "running": (3 * Pp, 3 * Pp + R)}
        assert same(dy.state[1, :3 * Pp], before[1, :3 * Pp]), "the overflowed member's parameters / slots moved"
        assert dy.lscale[1].cpu().tolist() == [2.0 ** 39, 0.0, 0.0, 1.0], dy.lscale.cpu().tolist()
        assert dy.step_col().cpu().tolist() == [2.0, 2.0, 2.0] and dy.host_step == [2, 2, 2]
        assert dy.hyper[:, O.H_STEP].cpu().tolist() == sa.hyper[:, O.H_STEP].cpu().tolist()
        assert not dy.grads.any(), "gradients survive into the next step"
        assert not same(dy.state[1, 3 * Pp:3 * Pp + R], before[1, 3 * Pp:3 * Pp + R])  # BN moving statistics: forward
        assert torch.isfinite(dy.state).all()
        for m in (0, 2):
            assert not same(dy.state[m, :P], before[m, :P]), "member %d did not update" % m
            assert dy.lscale[m].cpu().tolist() == [2.0 ** 7, 1.0, 0.0, 0.0]
            for name, (lo, hi) in cols.items():
                a, b, d = sa.state[m, lo:hi], sb.state[m, lo:hi], dy.state[m, lo:hi]
                if det:
                    assert same(d, a), "deterministic build: member %d %s differs from the static engine" % (m, name)
                    continue
                ref = float((a.double() - b.double()).abs().max())
                got = float((d.double() - a.double()).abs().max())
                print("DEVIATION %s member %d %-8s static-vs-static %.3e dynamic-vs-static %.3e (allowed %.3e)"
                      % (mode, m, name, ref, got, 4 * ref))
                assert got <= 4 * ref, (mode, m, name, got, ref)
        if det:
            print("DEVIATION %s: deterministic build, members 0 and 2 bitwise == static engine" % mode)
        # step 3: a second replay, member 1 starting from 2^39: the flag of step 2 is gone (cleared on the device)
        dy.train_step(slots, batches, hps, lrs)
        torch.cuda.synchronize()
        row = dy.lscale[1].cpu().tolist()
        assert row in ([2.0 ** 38, 0.0, 0.0, 2.0], [2.0 ** 39, 1.0, 0.0, 1.0]), row
        assert dy.lscale[:, 2].cpu().tolist() == [0.0] * n
        # step 4: back at 2^7 the member updates -- a stale flag would skip it
        set_scales([2.0 ** 7] * n)
        mid = dy.state.clone()
        dy.train_step(slots, batches, hps, lrs)
        torch.cuda.synchronize()
        assert not same(dy.state[1, :P], mid[1, :P]) and torch.isfinite(dy.state).all()
        assert dy.lscale[1].cpu().tolist() == [2.0 ** 7, 1.0, 0.0, row[3]], dy.lscale.cpu().tolist()
        print("whole step (%s, %s): overflowed member skipped bitwise, 2^40 -> 2^39, others updated; row after the "
              "second replay %s; clean step at 2^7 updates ok" % (mode, "det" if det else "release", row))
    finally:
        ops.grad_finite_check, ops.loss_scale_update, ops.fused_optimizer = real


if __name__ == "__main__":
    what = sys.argv[1]
    print("library: half=%s deterministic=%s" % (ops.build_half(), ops.build_deterministic()))
    if what == "kernels":
        check_finite(2 * 512 * 1024 + 3)
        check_finite(5)
        check_optimizer()
        check_update()
        check_head()
    elif what == "step":
        check_step(use_graph=True)
        check_step(use_graph=False)
    else:
        raise SystemExit("unknown check %r" % what)
    print("DLS_OK " + what)
