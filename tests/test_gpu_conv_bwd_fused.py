"""The fused CIFAR backward launch (ops/csrc/conv.hip ``dtf_conv_bwd_fused``: ROLE 0 of ``conv_bwd_body``, 16
instantiations, and its trailing slab-reduction workgroups) launched directly through ctypes and compared BITWISE with
the float64 references of tests/_conv_bwd_exact.py.  One operand set serves both halves of a launch: the dgrad half's
``y``, ``xout`` and sum(dz) statistics row (per replica and summed) and the wgrad half's dW -- through per-workgroup
slabs of exactly n_wg x slab_elems(C) NaN-filled words reduced by ``dtf_dw_slab_reduce``, and through the atomic
flush of ``slab = NULL`` -- into a gradient row that carries a seeded integer pattern before ``g_off``, after the block
and in the idle slot's row.  Every buffer sits inside canary guards; idle rows, the columns past C and every input
must be unchanged.  The sum(dz xhat) row goes through rsqrtf and is held to 4 x the scaled deviation of a float32
evaluation of the same formula (both figures printed).  The conditions that make the bitwise comparison legitimate
are asserted on the reference before every launch (``check_fused``; without a device in
tests/test_conv_bwd_exact_constructions.py).

Members sit in slots 0 and 2 of a capacity-3 population with 3 and 2 images; everything of the idle slot is NaN.
Every instantiation runs with a hand-built work list grouped by member (slot 2 first: a single-iteration item, an item
that crosses an image boundary inside, uneven splits) and with the arithmetic work item (``u_items > 0``, members in
slots 0 and 1) over a poison table.  Identity-mask rows (EPI & 2) without the chain bit get ``st_ep = NULL`` and NaN
epilogue parameter columns and must leave ``st_out`` at its seed; chain rows (EPI & 8) take x-hat from ``x3`` and the
chained BN's statistics.  The trailing workgroups (``nblocks > n_main``) reduce ANOTHER conv's hand-written slabs of
width ``r_c`` into ``r_goff`` while the main part computes its own case.

The float32 evaluation (``bx.fused_xhat``) adds the pixels one at a time in raster order, so its figure is the same
on every host, and ``check_fused`` refuses an operand set whose float32 evaluation lies within 2^-26 of float64
(less than one fp32 rounding of the summed magnitude would be left to the kernel)."""
import ctypes
import time

import pytest
import torch

import _conv_bwd_exact as bx
import _conv_exact as kx
import _convg_aux_exact as ax
import _convg_exact as cx

pytestmark = pytest.mark.gpu

IDS = ["c%d-m%d-e%d" % r for r in bx.FUSED_CASES]


def _env():
    ops, _, dev, _ = cx.gpu_env()
    from distributedtf_amd.engine import hip_resnet as hr
    hr._register()
    assert ops.lib().dtf_conv_args_size() == ctypes.sizeof(hr.ConvArgs)
    return ops, hr, dev, ops.build_nrep()


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _live_ptr(t):
    return None if t is None else t.data_ptr() + kx.PRE * t.element_size()


def _compare_grads(buf, want, what):
    got, exp = buf.cpu().double(), kx.guarded(want, torch.float64)
    if not torch.equal(got, exp):
        bad = (got != exp).nonzero().reshape(-1)
        i = int(bad[0]) - kx.PRE
        pytest.fail("%s: %d gradient words differ; first: slot %d word %d: got %r want %r" % (
            what, bad.numel(), i // want.shape[1], i % want.shape[1], float(got[bad[0]]), float(exp[bad[0]])))


class _Launch:
    """The device buffers of one fused case and its ConvArgs.  ``trail``: a bx.trail_case whose slabs the launch's
    trailing workgroups reduce (the gradient row then holds both convs' blocks)."""

    def __init__(self, c, ops, hr, dev, xout=True, slab=True, trail=None):
        bx.check_fused(c)  # the reference alone, before anything is launched
        dt = ops.act_dtype()
        self.c, self.dt, self.dev, self.inputs, self.trail = c, dt, dev, [], trail
        self.x = self._inp(c.dz, dt)
        self.x2 = self._inp(c.h, dt) if c.mode >= 2 else None
        self.x3 = self._inp(c.x3, dt) if (c.mode == 3 or c.epi & 8) else None
        self.xm = self._inp(c.ep.x, dt)
        self.res = self._inp(c.res, dt) if c.epi & 1 else None
        self.w = self._inp(kx.weight_rows(c), dt)
        self.params = self._inp(bx.param_rows(c), torch.float32)
        self.st_in, self.st_in_b = self._inp(c.st_f, torch.float32), self._inp(c.st_b, torch.float32)
        bn = c.chain if c.epi & 8 else c.ep
        self.st_ep = self._inp(bn.st_in, torch.float32) if bn.st_in is not None else None  # identity mask: NULL
        self.cnt = self._inp(c.ep.cnt, torch.float32)
        self.y = kx.guarded(torch.full_like(c.y, kx.CANARY), dt).to(dev)
        self.xout = kx.guarded(torch.full_like(c.y, kx.CANARY), dt).to(dev) if (xout and c.mode >= 2) else None
        self.st_out = kx.guarded(c.st_seed, torch.float32).to(dev)
        table = kx.poison_work(len(c.items), c.idle) if c.uniform else c.items
        self.work = torch.tensor(table, dtype=torch.int32, device=dev)
        self.red = torch.tensor(c.red, dtype=torch.int32, device=dev)
        self.n_slab = len(c.items) * bx.slab_elems(c.C)  # exactly n_wg x slab_elems(C) words, NaN, inside guards
        self.slab = (kx.guarded(torch.full((self.n_slab,), bx.NAN, dtype=torch.float64), torch.float32).to(dev)
                     if slab else None)
        if trail is None:
            (self.g_off,), self.row = bx.grad_layout([c.C])
            self.seed = bx.grad_seed(self.row, 6100 + c.C + 7 * c.mode + c.epi)
            assert float(self.seed.max()) <= bx.FUSED_SEED_MAX
        else:
            assert trail.C == c.C
            self.g_off, self.row, self.seed = trail.g_off, trail.row, trail.seed
        self.grads = kx.guarded(self.seed, torch.float32).to(dev)
        self.dw = torch.zeros_like(self.seed)  # the launch's own dW in the gradient row layout
        for sl in c.slots:
            self.dw[sl, self.g_off:self.g_off + 9 * c.C * c.C] = c.dw[sl].reshape(-1)
        a = hr.ConvArgs()
        a.x, a.x2, a.x3, a.xm, a.res, a.w = (_live_ptr(t) for t in (self.x, self.x2, self.x3, self.xm, self.res, self.w))
        a.y, a.xout = _live_ptr(self.y), _live_ptr(self.xout)
        a.params, a.st_in, a.st_in_b, a.st_ep, a.st_out, a.cnt = (
            _live_ptr(t) for t in (self.params, self.st_in, self.st_in_b, self.st_ep, self.st_out, self.cnt))
        a.work = self.work.data_ptr()
        a.w_mstride, a.w_off = kx.weight_rows(c).shape[1], kx.W_OFF
        a.p_mstride, a.in_gamma, a.in_beta, a.ep_gamma, a.ep_beta = kx.P_MSTRIDE, bx.IN_GAMMA, 0, bx.EP_GAMMA, bx.EP_BETA
        a.Hi = a.Wi = a.Ho = a.Wo = c.H
        a.rows, a.n_main, a.cin_real = 8, len(c.items), -1
        a.u_items, a.u_chunk, a.u_per = c.u
        a.grads, a.g_mstride, a.g_off = _live_ptr(self.grads), self.row, self.g_off
        a.slab = _live_ptr(self.slab)
        self.n_trail = 0
        if trail is not None:
            _, rc, rslab, red, r_goff = trail.jobs[0]
            self.rslab_host = kx.guarded(rslab, torch.float32)
            self.rslab = self.rslab_host.to(dev)
            self.rtab = torch.tensor(red, dtype=torch.int32, device=dev)
            a.rslab, a.rtab, a.r_c, a.r_goff, a.r_nblk = _live_ptr(self.rslab), self.rtab.data_ptr(), rc, r_goff, trail.nblk
            self.n_trail = trail.nblk * len(red)
        self.a = a

    def _inp(self, t, dt):
        host = kx.guarded(t, dt)
        buf = host.to(self.dev)
        self.inputs.append((host, buf))
        return buf

    def lds(self, ops):
        lib = ops.lib()
        return bx.lds_fused(self.c.C, int(lib.dtf_wpitch(self.c.C)), int(lib.dtf_fused16_wlds()))

    def launch(self, ops, trailing=True):
        c = self.c
        nblocks = len(c.items) + (self.n_trail if trailing else 0)
        rc = ops.lib().dtf_conv_bwd_fused(ctypes.byref(self.a), c.C, c.mode, c.epi, nblocks, self.lds(ops), ops.stream())
        assert rc == 0, rc

    def reduce(self, ops):
        c = self.c
        rc = ops.lib().dtf_dw_slab_reduce(_live_ptr(self.slab), self.red.data_ptr(), len(c.red), _live_ptr(self.grads),
                                          self.row, self.g_off, c.C, ops.stream())
        assert rc == 0, rc

    def check_dgrad(self, what):
        """y, xout, the statistics rows, the slab guards and every input."""
        c = self.c
        torch.cuda.synchronize()
        for name, buf, ref in (("y", self.y, c.y),) + ((("xout", self.xout, c.dy),) if self.xout is not None else ()):
            got, want = buf.cpu().double(), kx.guarded(ref, torch.float64)
            if not torch.equal(got, want):
                bad = (got != want).nonzero().reshape(-1)
                i = int(bad[0]) - kx.PRE  # (negative or past the end: a guard word)
                n, r, col, o = i // (c.H * c.H * c.C), i // (c.H * c.C) % c.H, i // c.C % c.H, i % c.C
                pytest.fail("%s %s: %d words differ; first: image %d row %d column %d channel %d: got %r want %r" % (
                    what, name, bad.numel(), n, r, col, o, float(got[bad[0]]), float(want[bad[0]])))
        st = self.st_out.cpu()
        if not bx.fused_has_stats(c.epi):
            assert torch.equal(_bits(st), _bits(kx.guarded(c.st_seed, torch.float32))), "identity mask: st_out written"
        else:
            assert kx.guards_intact(st, c.st_seed.numel()), "statistics guards"
            st = kx.live(st, c.st_seed.shape)
            seed = c.st_seed.float()
            assert torch.equal(st[c.idle], seed[c.idle]), "idle slot's statistics rows touched"
            assert torch.equal(st[..., c.C:], seed[..., c.C:]), "statistics columns past C touched"
            delta = (st.double() - c.st_seed).sum(1)[:, 0]  # over the replicas: sum(dz) per member and channel
            if not torch.equal(delta, c.st):
                bad = (delta != c.st).nonzero()
                s, ch = (int(v) for v in bad[0])
                pytest.fail("%s: %d sum(dz) words differ; first: slot %d channel %d: got %r want %r" % (
                    what, bad.shape[0], s, ch, float(delta[s, ch]), float(c.st[s, ch])))
            assert torch.equal(st.double()[:, :, 0], bx.dg_replica_rows(c)), "a workgroup's sum(dz) went to the wrong replica"
            (r64, mag), (r32, _) = bx.fused_xhat(c, torch.float64), bx.fused_xhat(c, torch.float32)
            kd, yd = ax.deviation(st.double()[:, :, 1].sum(1), r64, mag), ax.deviation(r32, r64, mag)
            print("%s: sum(dz xhat) kernel %.3e float32 %.3e (allowed %.3e), ratio %.3f" % (
                what, kd, yd, bx.FACTOR_RSQRT * yd, kd / yd if yd > 0 else 0.0))
            assert kd <= bx.FACTOR_RSQRT * yd, (kd, yd)
        if self.slab is not None:
            assert kx.guards_intact(self.slab.cpu(), self.n_slab), "a word past the n_wg slabs was written"
        for host, buf in self.inputs:  # the inputs are as they were
            assert torch.equal(_bits(buf.cpu()), _bits(host)), "an input buffer was written"

    def untouched(self):
        torch.cuda.synchronize()
        assert torch.equal(self.y.cpu().double(), torch.full_like(self.y.cpu().double(), kx.CANARY))
        assert torch.equal(self.st_out.cpu(), kx.guarded(self.c.st_seed, torch.float32))
        assert torch.equal(_bits(self.grads.cpu()), _bits(kx.guarded(self.seed, torch.float32)))
        if self.xout is not None:
            assert torch.equal(self.xout.cpu().double(), torch.full_like(self.xout.cpu().double(), kx.CANARY))
        if self.slab is not None:
            assert bool(torch.isnan(kx.live(self.slab.cpu(), (self.n_slab,))).all())


def _timed(what, t0):
    print("%s: %.2f s" % (what, time.perf_counter() - t0))


@pytest.mark.parametrize("work", ["list", "uniform"])
@pytest.mark.parametrize("row", bx.FUSED_CASES, ids=IDS)
def test_conv_bwd_fused_is_exact(row, work):
    """conv_bwd_fused_kernel<C, MODE_DY, EPI> into dW slabs, then dtf_dw_slab_reduce: y, xout, the statistics rows
    and the gradient row, bit for bit."""
    t0 = time.perf_counter()
    ops, hr, dev, nrep = _env()
    c = bx.fused_case(*row, uniform=work == "uniform", nrep=nrep)
    what = "fused c%d-m%d-e%d-%s" % (row + (work,))
    L = _Launch(c, ops, hr, dev)
    L.launch(ops)
    L.check_dgrad(what)
    _compare_grads(L.grads, L.seed, what + " (before the reduction: slabs only)")
    slab = kx.live(L.slab.cpu(), (len(c.items), bx.slab_elems(c.C)))
    valid, _ = bx.slab_index(c.C)
    assert not bool(torch.isnan(slab[:, valid]).any()), "a workgroup left part of its slab unwritten"
    L.reduce(ops)
    torch.cuda.synchronize()
    _compare_grads(L.grads, L.seed + L.dw, what)
    assert kx.guards_intact(L.slab.cpu(), L.n_slab)
    _timed(what, t0)


@pytest.mark.parametrize("row", bx.FUSED_CASES, ids=IDS)
def test_conv_bwd_fused_atomic_flush_is_exact(row):
    """slab = NULL: the accumulators are flushed into the seeded gradient row with atomics; the same dW."""
    t0 = time.perf_counter()
    ops, hr, dev, nrep = _env()
    c = bx.fused_case(*row, uniform=False, nrep=nrep)
    what = "fused c%d-m%d-e%d-noslab" % row
    L = _Launch(c, ops, hr, dev, slab=False)
    assert L.a.slab is None
    L.launch(ops)
    L.check_dgrad(what)
    _compare_grads(L.grads, L.seed + L.dw, what)
    _timed(what, t0)


@pytest.mark.parametrize("row", bx.FUSED_NULL_XOUT, ids=["c%d-m%d-e%d" % r for r in bx.FUSED_NULL_XOUT])
def test_conv_bwd_fused_without_xout(row):
    """xout = NULL: the same y, statistics and dW, nothing else written."""
    ops, hr, dev, nrep = _env()
    c = bx.fused_case(*row, uniform=False, nrep=nrep)
    what = "fused c%d-m%d-e%d-noxout" % row
    L = _Launch(c, ops, hr, dev, xout=False)
    assert L.a.xout is None
    L.launch(ops)
    L.check_dgrad(what)
    L.reduce(ops)
    torch.cuda.synchronize()
    _compare_grads(L.grads, L.seed + L.dw, what)


def _trail(tr, full=False):
    cc, rc, members, nblk = tr
    return bx.trail_case(cc, rc, tuple(members), nblk, full)


@pytest.mark.parametrize("tr", bx.FUSED_TRAIL, ids=["c%d-rc%d-nblk%d" % (t[0], t[1], t[3]) for t in bx.FUSED_TRAIL])
def test_conv_bwd_fused_trailing_reduction(tr):
    """nblocks = n_main + r_nblk x rows: the trailing workgroups add ANOTHER conv's slabs (width r_c, at r_goff) to
    the gradient row while the main part computes its own case; with nblocks = n_main that block keeps its seed."""
    t0 = time.perf_counter()
    ops, hr, dev, nrep = _env()
    k = _trail(tr)
    bx.check_reduce_case(k)
    c = bx.fused_case(k.C, 0, 0, uniform=False, nrep=nrep)
    what = "fused trail c%d-rc%d-nblk%d" % (k.C, k.rc, k.nblk)
    E32 = bx.slab_elems(k.rc) // 32
    assert (E32 % k.nblk == 0) == (k.nblk == E32)
    ctl = _Launch(c, ops, hr, dev, trail=k)  # control: no trailing workgroups
    ctl.launch(ops, trailing=False)
    ctl.check_dgrad(what + " control")
    _compare_grads(ctl.grads, k.seed, what + " control")
    L = _Launch(c, ops, hr, dev, trail=k)
    assert L.n_trail == k.nblk * len(k.red) > 0
    L.launch(ops)
    L.check_dgrad(what)
    _compare_grads(L.grads, k.want, what)  # the other conv's block; the launch's own dW is still in its slabs
    assert torch.equal(_bits(L.rslab.cpu()), _bits(L.rslab_host)), "the reduced slabs were written"
    L.reduce(ops)
    torch.cuda.synchronize()
    _compare_grads(L.grads, k.want + L.dw, what + " + own slabs")
    _timed(what, t0)


def test_conv_bwd_fused_trailing_reduction_full_mantissa():
    """Full-mantissa fp32 slab words through the trailing workgroups: inside (n + 8) 2^-24 sum |x_i| of float64 per
    element, and bitwise the same on a second launch (the summation order is fixed)."""
    ops, hr, dev, nrep = _env()
    k = _trail(bx.FUSED_TRAIL_FULL, True)
    bx.check_reduce_case(k)
    c = bx.fused_case(k.C, 0, 0, uniform=False, nrep=nrep)
    out = []
    for i in range(2):
        L = _Launch(c, ops, hr, dev, trail=k)
        L.launch(ops)
        L.check_dgrad("fused trail full mantissa %d" % i)
        out.append(L.grads.cpu())
    assert torch.equal(_bits(out[0]), _bits(out[1])), "two launches over the same slabs differ"
    assert kx.guards_intact(out[0], k.seed.numel())
    got = kx.live(out[0], k.seed.shape).double()
    bound = (k.nslab + 8) * 2.0 ** -24 * k.mag
    err = (got - k.want).abs()
    print("fused trail full mantissa: largest error / bound %.3f" % float((err / bound).max()))
    assert bool((err <= bound).all()), float((err / bound).max())
    assert bool((err > 0).any()), "the case is not exact: the bound is what is tested"
    untouched = k.nslab == 0
    assert torch.equal(got[untouched], k.seed[untouched]), "words outside the reduced block changed"


@pytest.mark.parametrize("cc,mode,epi", bx.FUSED_REJECTS, ids=["c64-m2-e1", "c16-m3-e1", "c32-m0-e3", "c48"])
def test_conv_bwd_fused_rejects_unsupported(cc, mode, epi):
    """No instantiation: -1 and nothing launched (every output keeps its pre-fill)."""
    ops, hr, dev, nrep = _env()
    c = bx.fused_case(64 if cc == 48 else cc, mode, 0, uniform=False, nrep=nrep)
    L = _Launch(c, ops, hr, dev)
    rc = ops.lib().dtf_conv_bwd_fused(ctypes.byref(L.a), cc, mode, epi, len(c.items), L.lds(ops), ops.stream())
    assert rc == -1, rc
    L.untouched()
