"""The generic ImageNet conv / data-gradient kernel (ops/csrc/convg.hip convg_fwd_kernel) launched directly through
``dtf_convg_fwd`` and compared **bitwise** with a float64 CPU reference on small-integer operands
(tests/_convg_fwd_exact.py; its conditions are asserted without a device by test_convg_fwd_exact_constructions.py).

Every one of the 23 (MODE, EPI, TRANS, AKM) dispatch rows runs at tc 64 and tc 128 in every legal tile variant (base,
BK 64, 256-pixel tiles, 32x32 MFMA tiles): all 146 instantiations, none untested.  One pytest case is one row x tc;
it loops over its variants and conv shapes (1x1, 3x3 stride 1, 3x3 stride 2 forward and transposed, 1x1 stride 2
transposed with its K = 0 parity classes, the compact 1x1 data gradient, the compact residual of EPI 15, the 7x7 / 2
and 4x4 / 1 stems, Ci = 256) on non-square 13 x 11 (14 x 12 / 7 x 6) images with Co = 72 / 136: a full channel tile
and an 8-channel one.  Members in slots 0 and 2 of capacity 3 with 2 and 1 images; an image between them that belongs
to nobody, the idle slot's weights and coefficient rows and the table columns past the channel count are NaN; outputs
are pre-filled with a non-integer canary between guards, statistics rows are pre-seeded with integers.

Not covered: the register-direct epilogue behind CG_EPI_REGS (compiled out at its default 0).
"""
import ctypes
import functools

import pytest
import torch

import _convg_exact as cx
import _convg_fwd_exact as fx

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _env():
    return cx.gpu_env()


def _first_diff(got, want, what):
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    i, r, col, o = (int(v) for v in bad[0])
    pytest.fail("%s: %d elements differ; first: image %d row %d column %d channel %d: got %r want %r" % (
        what, bad.shape[0], i, r, col, o, float(got[i, r, col, o]), float(want[i, r, col, o])))


class Launch:
    """The device buffers of one case (inputs uploaded once per case and activation type)."""

    def __init__(self, c):
        ops, hi, dev, det = _env()
        self.c, self.dt, self.dev, self.det = c, ops.act_dtype(), dev, det
        up = lambda t: None if t is None else t.to(self.dt).to(dev)  # noqa: E731
        self.x, self.x2, self.x3, self.res, self.xm = up(c.x), up(c.x2), up(c.x3), up(c.res), up(c.xm)
        self.w = up(fx.weight_rows(c))
        self.c_in, self.c_ep = c.c_in.float().to(dev), c.c_ep.float().to(dev)
        self.fx = cx.FX_GRAD if c.epi & 2 else cx.FX_STAT

    def run(self, variant, items, has3=True, label="", only=None):
        ops, hi, dev, det = _env()
        c, dt = self.c, self.dt
        what = "%s variant %d %s Ci %d%s" % (str(c.row), variant, c.shape, c.ci, label)
        tp = fx.tile_pixels(variant)
        fx.check_items(items, c, tp, only)  # the promised coverage, on the list that is launched
        work = torch.tensor(items, dtype=torch.int32, device=dev)
        ybuf, y = fx.guarded((fx.N_IMG, c.ho, c.wo, c.co), cx.Y_CANARY, dt, dev)
        xbuf, xout = fx.guarded((fx.N_IMG, c.hi, c.wi, c.ci), fx.NAN, dt, dev)
        xbuf0 = xbuf.clone()
        st = cx.acc_upload(c.seed_st, self.fx, det, dev)
        st0 = st.clone()
        p = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
        a = hi.CgArgs()
        a.x, a.x2, a.w, a.y, a.res, a.xm = p(self.x), p(self.x2), p(self.w), y.data_ptr(), p(self.res), p(self.xm)
        a.w_mstride, a.w_off = self.w.shape[1], fx.W_OFF
        a.c_in, a.c_ep, a.st_out, a.work = p(self.c_in), p(self.c_ep), st.data_ptr(), work.data_ptr()
        a.Hi, a.Wi, a.Ci, a.Ho, a.Wo, a.Co = c.hi, c.wi, c.ci, c.ho, c.wo, c.co
        a.kh = a.kw = c.k
        a.stride, a.pad, a.cmax, a.log2ci = c.kstride, c.pad, cx.CMAX, c.ci.bit_length() - 1
        if c.mode == 3:
            a.x3, a.xout = (p(self.x3) if has3 else 0), xout.data_ptr()
        rc = ops.lib().dtf_convg_fwd(ctypes.byref(a), c.tc, c.mode, c.epi, fx.trans_arg(c.row, variant), len(items),
                                     ops.stream())
        assert rc == 0, (what, rc)
        torch.cuda.synchronize()
        yref, stref, _, xref = c.out[has3]
        if only is not None:
            yref, stref = fx.class_expected(c, only)
        _first_diff(y.cpu().double(), yref, what + " y")
        g = fx.GUARD
        assert bool((ybuf[:g] == cx.Y_CANARY).all()) and bool((ybuf[-g:] == cx.Y_CANARY).all()), what + " y guards"
        if c.epi & 4:
            # both members' rows, the idle slot's untouched row and columns [Co, CMAX) in one comparison
            got = cx.acc_download(st, self.fx, det)
            if not torch.equal(got, stref.float()):
                bad = (got != stref.float()).nonzero()
                s, r, o = (int(v) for v in bad[0])
                pytest.fail("%s statistics: %d differ; first: slot %d row %d channel %d: got %r want %r" % (
                    what, bad.shape[0], s, r, o, float(got[s, r, o]), float(stref[s, r, o])))
        else:
            assert torch.equal(st, st0), what + ": st_out written by a row without the statistics bit"
        if c.mode == 3:
            # the launched pixels by value (no NaN among them), nobody's image by the bits of its NaN pre-fill
            gx = xout.cpu()
            member = [i for _, f, e in fx.RANGES for i in range(f, e)]
            _first_diff(gx[member].double(), xref[member], what + " xout (member images 0, 1, 3)")
            assert torch.equal(fx.bits(gx[fx.IDLE_IMG]), fx.bits(xbuf0[:gx[0].numel()].cpu()).view(gx[0].shape)), \
                what + ": xout of the idle image written"
            assert torch.equal(fx.bits(xbuf[:g].cpu()), fx.bits(xbuf0[:g].cpu()))
            assert torch.equal(fx.bits(xbuf[-g:].cpu()), fx.bits(xbuf0[-g:].cpu())), what + " xout guards"
        else:
            assert torch.equal(fx.bits(xbuf.cpu()), fx.bits(xbuf0.cpu()))
        return fx.bits(y.cpu()).clone(), (fx.bits(xout.cpu()).clone() if c.mode == 3 else None)


@pytest.mark.parametrize("tc", fx.TCS)
@pytest.mark.parametrize("row", fx.ROWS, ids=lambda r: "m%d-e%d-t%d-a%d" % r)
def test_convg_fwd_is_exact(row, tc):
    """Output, statistics rows of both members, the idle slot's row, columns [Co, CMAX) and (MODE 3) xout equal the
    float64 reference bit for bit, in every tile variant and conv shape of the row."""
    ops = _env()[0]
    cache = {}
    for variant, shape, ci in fx.launches(row, tc):
        c = fx.fwd_case(row, tc, shape, ci)
        if (shape, ci) not in cache:
            fx.check_case(c, ops.act_dtype())
            cache[(shape, ci)] = Launch(c)
        ln = cache[(shape, ci)]
        tp = fx.tile_pixels(variant)
        ybits, xbits = ln.run(variant, fx.work_items(c, tp))
        if c.mode == 3:
            # the co-tile order reversed: still only the o0 == 0 workgroups write xout, to the same bits
            yr, xr = ln.run(variant, fx.work_items(c, tp, reverse_tiles=True), label=" (co tiles reversed)")
            assert torch.equal(yr, ybits) and torch.equal(xr, xbits)
            ln.run(variant, fx.work_items(c, tp), has3=False, label=" (x3 = NULL)")
        if c.trans and variant == fx.V_BASE:
            # all four classes over the same pixels cannot tell py from px: class 1 (py 0, px 1) alone, then 2 and 3
            for only in ((1,), (2, 3)):
                ln.run(variant, fx.work_items(c, tp, only=only), label=" (classes %s only)" % (only,), only=only)


def test_convg_fwd_rejections():
    """Return codes of launches the dispatcher must refuse; nothing is launched, so nothing is written."""
    ops, hi, dev, det = _env()
    dt = ops.act_dtype()
    buf = torch.full((4096,), cx.Y_CANARY, dtype=dt, device=dev)
    work = torch.tensor([[0, 0, 1, 0]], dtype=torch.int32, device=dev)

    def call(tc, mode, epi, trans, ci=32, co=72, nwork=1):
        a = hi.CgArgs()
        a.x = a.x2 = a.w = a.y = a.res = a.xm = a.x3 = a.xout = buf.data_ptr()
        a.work = work.data_ptr()
        a.Hi = a.Wi = a.Ho = a.Wo = a.kh = a.kw = a.stride = 1
        a.Ci, a.Co, a.cmax, a.log2ci = ci, co, cx.CMAX, max(ci, 1).bit_length() - 1
        return ops.lib().dtf_convg_fwd(ctypes.byref(a), tc, mode, epi, trans, nwork, ops.stream())

    assert call(64, 0, 0, 0, ci=48) == -2, "Ci not a power of two"
    assert call(64, 0, 0, 0, ci=4) == -2, "Ci < 8"
    assert call(64, 0, 0, 0, co=68) == -2, "Co % 8 != 0"
    assert call(64, 0, 0, 2, ci=16) == -2, "AKM with Ci < BK 32"
    assert call(64, 0, 0, 2 | 4, ci=32) == -2, "AKM with Ci < BK 64"
    assert call(64, 0, 0, 3, ci=16) == -2 and call(64, 0, 0, 3 | 4, ci=32) == -2, "TRANS with Ci < BK"
    assert call(128, 0, 0, 2 | 8 | 16, co=136) == -2, "M32 with AKM"
    assert call(64, 0, 0, 8 | 16) == -2, "M32 with tc 64"
    assert call(128, 0, 0, 16, co=136) == -2, "M32 without 256-pixel tiles"
    assert call(64, 0, 0, 8 | 4) == -2, "256-pixel tiles with BK 64"
    assert call(64, 3, 0, 2) == -1 and call(64, 1, 4, 2) == -1 and call(64, 0, 2, 0) == -1, "unlisted (mode, epi)"
    assert call(96, 0, 0, 0) == -1, "unlisted tc"
    assert call(64, 0, 0, 0, nwork=0) == 0 and call(64, 3, 0, 2, nwork=0) == 0, "nwork = 0"
    torch.cuda.synchronize()
    assert bool((buf == cx.Y_CANARY).all())
