"""f32dgrad_s2_kernel behind ``dtf_f32_dgrad_s2`` (ops/csrc/f32conv.hip), bit for bit against float64
``conv_transpose2d(stride=2, padding=(k - 1) // 2, output_padding=1)`` on small-integer operands (the argument of
tests/_convg_exact.py: every sum stays an integer below 2^24, exact in fp32 in any order and in the deterministic
build's fixed point), for k in 1 / 3 and every instantiated epilogue.  dy 9 x 11 (odd width, not square: the +1 taps fall
off the bottom and right edge inside a tile) -> dx 18 x 22, 48 dy channels (three chunks), 144 dx channels (a full
channel tile and a 16-row partial one); members in slots 0 and 2 of capacity 3 with 3 and 1 images around a NaN image
that is nobody's: 297 class pixels give full items, one of them starting inside an image and crossing into the next,
and a ragged tail; 99 a member shorter than a tile.  NaN weights and coefficients and a pre-seeded statistics row in the
idle slot; guards around every buffer.  The launch is repeated with the classes in the reverse order.

Share of non-zero outputs asserted on the reference: a dense integer output is non-zero at least half of the time, a
quarter with the ReLU mask (the bounds of tests/test_gpu_f32_conv_pw.py); at k = 1 without a residual only class 0, a
quarter of the pixels, carries a sum at all, so the bound is a quarter of that.
"""
import ctypes
import functools
import types

import pytest
import torch
import torch.nn.functional as F

import _convg_exact as cx
from test_gpu_f32_conv_t3 import GUARD, NAN, guarded

pytestmark = pytest.mark.gpu
HI, WI, CI, CO = 9, 11, 48, 144
SIDE = 3  # _pix_work takes the side of a square grid: a 9 x 11 image is eleven 3 x 3 ones to it
FX_LIMIT = 2.0 ** (54 - cx.FX_GRAD)  # common.h DTF_FX_LIMIT at the gradient scale, for a wave's partial (tp / 2 pixels)


@functools.lru_cache(maxsize=None)
def case(k, epi):
    """Operands, float64 outputs ``y`` (canary where nobody writes) and statistics rows ``st`` of one launch."""
    c = types.SimpleNamespace()
    c.ranges = [(s, f + i, e + i) for i, (s, f, e) in enumerate(cx.member_ranges((3, 1)))]
    n, c.idle = c.ranges[-1][2], c.ranges[0][2]
    g = torch.Generator().manual_seed(10 * k + epi)
    c.x = cx._ints(g, (n, HI, WI, CI), -2, 2)
    c.xm, c.res = (cx._ints(g, (n, 2 * HI, 2 * WI, CO), -2, 2) for _ in range(2))
    c.w = cx._ints(g, (cx.CAP, CI, k, k, CO), -1, 1)  # OHWI of the forward conv
    c.c_ep = cx._coefs(g, CO)  # mask BN: integer scale, shift; integer mean in [-1, 1], inverse deviation in {1, 2}
    c.c_ep[:, 2, :CO], c.c_ep[:, 3, :CO] = cx._ints(g, (cx.CAP, CO), -1, 1), cx._ints(g, (cx.CAP, CO), 1, 2)
    c.seed_st = cx._ints(g, (cx.CAP, 2, cx.CMAX), -3, 3)
    c.y = torch.full((n, 2 * HI, 2 * WI, CO), cx.Y_CANARY, dtype=torch.float64)
    c.st, c.ab, c.big = c.seed_st.clone(), c.seed_st.abs(), 0.0
    for s, f, e in c.ranges:
        xn, wn, ep = c.x[f:e].permute(0, 3, 1, 2), c.w[s].permute(0, 3, 1, 2), c.c_ep[s, :, :CO]
        y = F.conv_transpose2d(xn, wn, stride=2, padding=(k - 1) // 2, output_padding=1).permute(0, 2, 3, 1)
        y = y + c.res[f:e] if epi & 1 else y
        if epi & 2:
            y = torch.where(c.xm[f:e] * ep[0] + ep[1] > 0, y, torch.zeros_like(y))
        q = y * (c.xm[f:e] - ep[2]) * ep[3] if epi & 2 else y * y
        c.big = max(c.big, float(q.abs().max())) if epi & 2 else 0.0
        c.y[f:e] = y + 0.0  # (no negative zero: the kernel's sums start from +0)
        if epi & 4:
            c.st[s, :, :CO] += torch.stack([y.sum((0, 1, 2)), q.sum((0, 1, 2))])
            c.ab[s, :, :CO] += torch.stack([y.abs().sum((0, 1, 2)), q.abs().sum((0, 1, 2))])
    c.x[c.idle], c.xm[c.idle], c.res[c.idle], c.w[1], c.c_ep[1] = NAN, NAN, NAN, NAN, NAN
    return c


@pytest.mark.parametrize("epi", [0, 6, 7])
@pytest.mark.parametrize("k", [1, 3])
def test_f32_dgrad_s2_is_exact(k, epi):
    from distributedtf_amd.engine import hip_imagenet_f32 as h32
    ops, hi, dev, det = cx.gpu_env()
    h32._register()
    L, c = ops.lib(), case(k, epi)
    members = [i for _, f, e in c.ranges for i in range(f, e)]
    assert bool((c.y[members] == c.y[members].round()).all()) and c.ab.max() < cx.EXACT
    dense = 1.0 if k == 3 or epi & 1 else 0.25  # share of the dx pixels that carry a sum or a residual
    assert float((c.y[members] != 0).double().mean()) >= (0.25 if epi & 2 else 0.5) * dense
    assert torch.equal(c.st[1], c.seed_st[1]) and bool((c.y[c.idle] == cx.Y_CANARY).all())
    x, w, res, xm, c_ep = (guarded(t, NAN, dev)[1] for t in (c.x, c.w, c.res, c.xm, c.c_ep))
    seed = cx.acc_upload(c.seed_st, cx.FX_GRAD, det, dev)
    tc = L.dtf_f32_dgrad_s2_tc(0)
    tp = L.dtf_f32_dgrad_s2_tp(tc)
    assert tc > 0 and tp > 0 and L.dtf_f32_dgrad_s2_tp(32) == 0 and c.big * (tp // 2) < FX_LIMIT
    # the plan's own items over this case's members
    per = HI * WI // (SIDE * SIDE)
    plan = types.SimpleNamespace(slots=[s for s, _, _ in c.ranges], sizes=[(e - f) * per for _, f, e in c.ranges],
                                 first={s: f * per for s, f, _ in c.ranges}, _xcd_order=hi._ImageNetPlan._xcd_order,
                                 _hold=lambda t: t, be=types.SimpleNamespace(dev=dev))
    classes = h32._F32_DS2_CLASSES[k]
    work = hi._ImageNetPlan._pix_work(plan, SIDE, CO, tc, classes=classes, tp=tp)
    assert CO % tc == 16 and CI // 16 == 3
    for cls in range(4):
        rows = [r for r in work.tolist() if r[3] >> 16 == cls]
        assert {r[3] & 0xffff for r in rows} == set(range(0, CO, tc))  # a 16-row partial last channel tile
        assert any(b - a == tp for _, a, b, _ in rows) and any((b - a) % 16 for _, a, b, _ in rows)
        # starts inside an image and crosses into the next; a member shorter than a tile
        assert any(a % (HI * WI) and a // (HI * WI) != (b - 1) // (HI * WI) for _, a, b, _ in rows)
        assert any(s == c.ranges[1][0] and (a, b) == (c.ranges[1][1] * HI * WI, c.ranges[1][2] * HI * WI) and b - a < tp
                   for s, a, b, _ in rows)
    by_class = [work[(work[:, 3] >> 16) == cls] for cls in classes]
    reverse = torch.cat(by_class[::-1]).contiguous()

    def launch(wk, y, st, ci=CI, stride=2, ho=2 * HI, tc_=tc):
        a = h32.F32Args()
        a.x, a.y, a.w, a.work, a.st_out = (t.data_ptr() for t in (x, y, w, wk, st))
        a.res, a.xm, a.c_ep = res.data_ptr(), xm.data_ptr(), c_ep.data_ptr()
        a.w_mstride, a.w_off, a.Ci, a.wci, a.Co, a.cmax = w[0].numel(), 0, ci, ci, CO, cx.CMAX
        a.Hi, a.Wi, a.Ho, a.Wo = HI, WI, ho, 2 * WI
        a.kh, a.kw, a.stride, a.pad = k, k, stride, (k - 1) // 2
        rc = L.dtf_f32_dgrad_s2(ctypes.byref(a), tc_, epi, wk.shape[0], ops.stream())
        torch.cuda.synchronize()
        return rc

    for wk in (work, reverse):
        ybuf, y = guarded(torch.full_like(c.y, cx.Y_CANARY), cx.Y_CANARY, dev)
        stbuf, st = guarded(seed, 7, dev, seed.dtype)
        # a stride-1 conv; a dx grid that is not twice dy's; Ci no multiple of 16; no such channel tile
        assert (launch(wk, y, st, stride=1), launch(wk, y, st, ho=2 * HI - 1), launch(wk, y, st, ci=24),
                launch(wk, y, st, tc_=32)) == (-2, -2, -2, -1)
        assert bool((ybuf == cx.Y_CANARY).all()) and torch.equal(st, seed)
        assert launch(wk, y, st) == 0
        diff = (y.cpu().view(torch.int32) != c.y.float().view(torch.int32)).nonzero()
        assert not len(diff), "%d outputs differ; first at [image, row, column, channel] %s" % (len(diff), diff[0].tolist())
        diff = (cx.acc_download(st, cx.FX_GRAD, det) != c.st.float()).nonzero()
        assert not len(diff), "%d statistics differ; first at [slot, row, channel] %s" % (len(diff), diff[0].tolist())
        for buf, fill in ((ybuf, cx.Y_CANARY), (stbuf, 7)):
            assert bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())
