"""The dgrad role of the deferred CIFAR backward (ops/csrc/conv.hip ``dtf_conv_bwd_dg``: 13 instantiations) launched
directly through ctypes and compared BITWISE with the float64 references of tests/_conv_bwd_exact.py: the whole ``y``
buffer, the whole ``xout`` buffer (the transformed dY of MODE_DY 2 / 3) and the sum(dz) statistics row, per replica (workgroup b adds to
replica b % NREP of its member) and summed over them, inside canary guards, idle member rows and the columns past C included, and every input unchanged.  The sum(dz xhat) row goes
through rsqrtf and is held to 4 x the scaled deviation of a float32 evaluation of the same formula (both figures
printed).  The conditions that make the bitwise comparison legitimate are asserted on the reference before every
launch (``check_dg``; without a device in tests/test_conv_bwd_exact_constructions.py).

Members sit in slots 0 and 2 of a capacity-3 population with 3 and 2 images; everything of the idle slot is NaN.
Every instantiation runs with a hand-built work list (a single-iteration item, an item that crosses an image boundary
inside, uneven splits, the members' items interleaved) and with the arithmetic work item (``u_items > 0``, members in
slots 0 and 1, a chunk that does not divide the member's iterations) while ``work`` points at a poison table."""
import ctypes

import pytest
import torch

import _conv_bwd_exact as bx
import _conv_exact as kx
import _convg_aux_exact as ax
import _convg_exact as cx

pytestmark = pytest.mark.gpu

DG_IDS = ["c%d-m%d-e%d-rows%d" % r for r in bx.DG_CASES]


def _env():
    ops, _, dev, _ = cx.gpu_env()
    from distributedtf_amd.engine import hip_resnet as hr
    hr._register()
    assert ops.lib().dtf_conv_args_size() == ctypes.sizeof(hr.ConvArgs)
    return ops, hr, dev, ops.build_nrep()


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


class _Launch:
    """The device buffers of one dgrad case and its ConvArgs."""

    def __init__(self, c, ops, hr, dev, xout=True):
        bx.check_dg(c)  # the reference alone, before anything is launched
        dt = ops.act_dtype()
        self.c, self.dt, self.dev, self.inputs = c, dt, dev, []
        self.x = self._inp(c.dz, dt)
        self.x2 = self._inp(c.h, dt) if c.mode >= 2 else None
        self.x3 = self._inp(c.x3, dt) if c.mode == 3 else None
        self.xm = self._inp(c.ep.x, dt)
        self.res = self._inp(c.res, dt) if c.epi & 1 else None
        self.w = self._inp(kx.weight_rows(c), dt)
        self.params = self._inp(bx.param_rows(c), torch.float32)
        self.st_in, self.st_in_b = self._inp(c.st_f, torch.float32), self._inp(c.st_b, torch.float32)
        self.st_ep = self._inp(c.ep.st_in, torch.float32)
        self.cnt = self._inp(c.ep.cnt, torch.float32)
        self.y = kx.guarded(torch.full_like(c.y, kx.CANARY), dt).to(dev)
        self.xout = kx.guarded(torch.full_like(c.y, kx.CANARY), dt).to(dev) if (xout and c.mode >= 2) else None
        self.st_out = kx.guarded(c.st_seed, torch.float32).to(dev)
        table = kx.poison_work(len(c.items), c.idle) if c.uniform else c.items
        self.work = torch.tensor(table, dtype=torch.int32, device=dev)
        a = hr.ConvArgs()

        def p(t, esz):
            return None if t is None else t.data_ptr() + kx.PRE * esz

        a.x, a.x2, a.x3, a.xm, a.res, a.w = (p(t, 2) for t in (self.x, self.x2, self.x3, self.xm, self.res, self.w))
        a.y, a.xout = p(self.y, 2), p(self.xout, 2)
        a.params, a.st_in, a.st_in_b, a.st_ep, a.st_out, a.cnt = (
            p(t, 4) for t in (self.params, self.st_in, self.st_in_b, self.st_ep, self.st_out, self.cnt))
        a.work = self.work.data_ptr()
        a.w_mstride, a.w_off = kx.weight_rows(c).shape[1], kx.W_OFF
        a.p_mstride, a.in_gamma, a.in_beta, a.ep_gamma, a.ep_beta = kx.P_MSTRIDE, bx.IN_GAMMA, 0, bx.EP_GAMMA, bx.EP_BETA
        a.Hi = a.Wi = a.Ho = a.Wo = c.H
        a.rows, a.n_main = c.rows, len(c.items)
        a.u_items, a.u_chunk, a.u_per = c.u
        self.a = a

    def _inp(self, t, dt):
        host = kx.guarded(t, dt)
        buf = host.to(self.dev)
        self.inputs.append((host, buf))
        return buf

    def launch(self, ops):
        c = self.c
        lds = bx.lds_dg(c.C, c.rows, int(ops.lib().dtf_wpitch(c.C)))
        rc = ops.lib().dtf_conv_bwd_dg(ctypes.byref(self.a), c.C, c.mode, c.epi, c.rows, len(c.items), lds, ops.stream())
        assert rc == 0, rc

    def check(self, what):
        c = self.c
        torch.cuda.synchronize()
        for name, buf, ref in (("y", self.y, c.y),) + ((("xout", self.xout, c.dy),) if self.xout is not None else ()):
            got, want = buf.cpu().double(), kx.guarded(ref, torch.float64)
            if not torch.equal(got, want):
                bad = (got != want).nonzero().reshape(-1)
                i = int(bad[0]) - kx.PRE  # (negative or past the end: a guard word)
                n, r, col, o = i // (c.H * c.H * c.C), i // (c.H * c.C) % c.H, i // c.C % c.H, i % c.C
                pytest.fail("%s: %d words differ; first: image %d row %d column %d channel %d: got %r want %r" % (
                    name, bad.numel(), n, r, col, o, float(got[bad[0]]), float(want[bad[0]])))
        st = self.st_out.cpu()
        assert kx.guards_intact(st, c.st_seed.numel()), "statistics guards"
        st = kx.live(st, c.st_seed.shape)
        seed = c.st_seed.float()
        assert torch.equal(st[c.idle], seed[c.idle]), "idle slot's statistics rows touched"
        assert torch.equal(st[..., c.C:], seed[..., c.C:]), "statistics columns past C touched"
        delta = (st.double() - c.st_seed).sum(1)[:, 0]  # over the replicas: sum(dz) per member and channel
        if not torch.equal(delta, c.st):
            bad = (delta != c.st).nonzero()
            s, ch = (int(v) for v in bad[0])
            pytest.fail("%d sum(dz) words differ; first: slot %d channel %d: got %r want %r" % (
                bad.shape[0], s, ch, float(delta[s, ch]), float(c.st[s, ch])))
        assert torch.equal(st.double()[:, :, 0], bx.dg_replica_rows(c)), "a workgroup's sum(dz) went to the wrong replica"
        (r64, mag), (r32, _) = bx.dg_xhat(c, torch.float64), bx.dg_xhat(c, torch.float32)
        kd, yd = ax.deviation(st.double()[:, :, 1].sum(1), r64, mag), ax.deviation(r32, r64, mag)
        print("%s: sum(dz xhat) kernel %.3e float32 %.3e (allowed %.3e), ratio %.3f" % (
            what, kd, yd, bx.FACTOR_RSQRT * yd, kd / yd if yd > 0 else 0.0))
        assert kd <= bx.FACTOR_RSQRT * yd, (kd, yd)
        for host, buf in self.inputs:  # the inputs are as they were
            assert torch.equal(_bits(buf.cpu()), _bits(host)), "an input buffer was written"

    def untouched(self):
        torch.cuda.synchronize()
        assert torch.equal(self.y.cpu().double(), torch.full_like(self.y.cpu().double(), kx.CANARY))
        assert torch.equal(self.st_out.cpu(), kx.guarded(self.c.st_seed, torch.float32))


@pytest.mark.parametrize("work", ["list", "uniform"])
@pytest.mark.parametrize("row", bx.DG_CASES, ids=DG_IDS)
def test_conv_bwd_dg_is_exact(row, work):
    """conv_bwd_dg_kernel<C, MODE_DY, EPI, ROWS>: y, xout, the sum(dz) row of both members, untouched idle rows."""
    ops, hr, dev, nrep = _env()
    c = bx.dg_case(*row, uniform=work == "uniform", nrep=nrep)
    L = _Launch(c, ops, hr, dev)
    L.launch(ops)
    L.check("dg c%d-m%d-e%d-rows%d-%s" % (row + (work,)))


@pytest.mark.parametrize("row", bx.DG_NULL_XOUT, ids=["c%d-m%d-e%d-rows%d" % r for r in bx.DG_NULL_XOUT])
def test_conv_bwd_dg_without_xout(row):
    """xout = NULL: the same y and statistics, nothing else written."""
    ops, hr, dev, nrep = _env()
    c = bx.dg_case(*row, uniform=False, nrep=nrep)
    L = _Launch(c, ops, hr, dev, xout=False)
    assert L.a.xout is None
    L.launch(ops)
    L.check("dg c%d-m%d-e%d-rows%d-noxout" % row)


@pytest.mark.parametrize("cc,mode,epi,rows", bx.DG_REJECTS, ids=["rows4-c32", "epi2", "c48"])
def test_conv_bwd_dg_rejects_unsupported(cc, mode, epi, rows):
    """No instantiation: -1 and nothing launched (y and the statistics keep their pre-fill)."""
    ops, hr, dev, nrep = _env()
    c = bx.dg_case(64 if cc == 48 else cc, mode, 0, 8, uniform=False, nrep=nrep)
    L = _Launch(c, ops, hr, dev)
    L.a.rows = rows
    rc = ops.lib().dtf_conv_bwd_dg(ctypes.byref(L.a), cc, mode, epi, rows, len(c.items), 65536, ops.stream())
    assert rc == -1, rc
    L.untouched()
