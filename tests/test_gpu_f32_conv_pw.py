"""f32conv_pw_kernel behind ``dtf_f32_conv_pw`` (ops/csrc/f32conv.hip), bit for bit against float64 ``conv2d`` /
``conv_transpose2d`` on small-integer operands (the argument of tests/_convg_exact.py: every sum stays an integer below
2^24, exact in fp32 in any order and in the deterministic build's fixed point), for every instantiated (epilogue,
direction) and every channel tile of the library.  13 x 13 images, Ci = 48 (three chunks: the prefetch with an odd chunk
count), Co = 144 (full channel tiles and a 16-row partial one); members in slots 0 and 2 of capacity 3 with 2 and 1
images around a NaN image that is nobody's: 338 pixels give full items, one that starts inside an image and crosses
into the next, and a ragged tail; 169 pixels a member shorter than two tiles.  NaN weights and coefficients and a
pre-seeded statistics row in the idle slot; guards around every buffer.
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
HW, CI, CO = 13, 48, 144
FX_LIMIT = 2.0 ** (54 - cx.FX_GRAD)  # common.h DTF_FX_LIMIT at the gradient scale, for a wave's partial (tp / 2 pixels)


@functools.lru_cache(maxsize=None)
def case(epi, dgrad):
    """Operands, float64 outputs ``y`` (canary where nobody writes) and statistics rows ``st`` of one launch."""
    c = types.SimpleNamespace()
    c.ranges = [(s, f + i, e + i) for i, (s, f, e) in enumerate(cx.member_ranges((2, 1)))]
    n, c.idle = c.ranges[-1][2], c.ranges[0][2]
    g = torch.Generator().manual_seed(100 * epi + dgrad)
    c.x, c.xm, c.res = (cx._ints(g, (n, HW, HW, ch), -2, 2) for ch in (CI, CO, CO))
    c.w = cx._ints(g, (cx.CAP, CI, 1, 1, CO) if dgrad else (cx.CAP, CO, 1, 1, CI), -1, 1)  # OHWI of the forward conv
    c.c_ep = cx._coefs(g, CO)  # mask BN: integer scale, shift; integer mean in [-1, 1], inverse deviation in {1, 2}
    c.c_ep[:, 2, :CO], c.c_ep[:, 3, :CO] = cx._ints(g, (cx.CAP, CO), -1, 1), cx._ints(g, (cx.CAP, CO), 1, 2)
    c.seed_st = cx._ints(g, (cx.CAP, 2, cx.CMAX), -3, 3)
    c.y = torch.full((n, HW, HW, CO), cx.Y_CANARY, dtype=torch.float64)
    c.st, c.ab, c.big = c.seed_st.clone(), c.seed_st.abs(), 0.0
    for s, f, e in c.ranges:
        xn, wn, ep = c.x[f:e].permute(0, 3, 1, 2), c.w[s].permute(0, 3, 1, 2), c.c_ep[s, :, :CO]
        y = (F.conv_transpose2d(xn, wn) if dgrad else F.conv2d(xn, wn)).permute(0, 2, 3, 1)
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


@pytest.mark.parametrize("epi,dgrad", [(0, 0), (4, 0), (5, 0), (0, 1), (3, 1), (6, 1), (7, 1)])
def test_f32_conv_pw_is_exact(epi, dgrad):
    from distributedtf_amd.engine import hip_imagenet_f32 as h32
    ops, hi, dev, det = cx.gpu_env()
    h32._register()
    L, k = ops.lib(), case(epi, dgrad)
    members = [i for _, f, e in k.ranges for i in range(f, e)]
    assert bool((k.y[members] == k.y[members].round()).all()) and k.ab.max() < cx.EXACT
    assert float((k.y[members] != 0).double().mean()) >= (0.25 if epi & 2 else 0.5)
    assert torch.equal(k.st[1], k.seed_st[1]) and bool((k.y[k.idle] == cx.Y_CANARY).all())
    shift = cx.FX_GRAD if epi & 2 else cx.FX_STAT
    x, w, res, xm, c_ep = (guarded(t, NAN, dev)[1] for t in (k.x, k.w, k.res, k.xm, k.c_ep))
    seed = cx.acc_upload(k.seed_st, shift, det, dev)
    plan = types.SimpleNamespace(slots=[s for s, _, _ in k.ranges], sizes=[e - f for _, f, e in k.ranges],
                                 first={s: f for s, f, _ in k.ranges}, _xcd_order=hi._ImageNetPlan._xcd_order,
                                 _hold=lambda t: t, be=types.SimpleNamespace(dev=dev))
    tcs = [L.dtf_f32_conv_pw_tc(i) for i in range(8) if L.dtf_f32_conv_pw_tc(i) > 0]
    assert tcs and 32 not in tcs
    for tc in tcs:
        tp = L.dtf_f32_conv_pw_tp(tc)
        assert k.big * (tp // 2) < FX_LIMIT
        ybuf, y = guarded(torch.full_like(k.y, cx.Y_CANARY), cx.Y_CANARY, dev)
        stbuf, st = guarded(seed, 7, dev, seed.dtype)
        work = h32._ImageNetF32Plan._pw_work(plan, HW * HW, CO, tc, tp)  # the plan's own items over this case's members
        rows = work.tolist()
        assert any(b - a == tp for _, a, b, _ in rows) and any((b - a) % 16 for _, a, b, _ in rows)
        assert any(a % (HW * HW) for _, a, _, _ in rows)  # starts inside an image; crosses into the next image
        assert any(a // (HW * HW) != (b - 1) // (HW * HW) for _, a, b, _ in rows)
        assert CO % tc == 16 and {r[3] for r in rows} == set(range(0, CO, tc))  # a 16-row partial last channel tile

        def launch(ci, stride, tc_):
            a = h32.F32Args()
            a.x, a.y, a.w, a.work, a.st_out = (t.data_ptr() for t in (x, y, w, work, st))
            a.res, a.xm, a.c_ep = res.data_ptr(), xm.data_ptr(), c_ep.data_ptr()
            a.w_mstride, a.w_off, a.Ci, a.wci, a.Co, a.cmax = w[0].numel(), 0, ci, ci, CO, cx.CMAX
            a.Hi = a.Wi = a.Ho = a.Wo = HW
            a.kh, a.kw, a.stride, a.pad = 1, 1, stride, 0
            rc = L.dtf_f32_conv_pw(ctypes.byref(a), tc_, epi, dgrad, work.shape[0], ops.stream())
            torch.cuda.synchronize()
            return rc

        # Ci no multiple of 16; a strided conv; no such channel tile
        assert (launch(24, 1, tc), launch(CI, 2, tc), launch(CI, 1, 32)) == (-2, -2, -1)
        assert bool((ybuf == cx.Y_CANARY).all()) and torch.equal(st, seed)
        assert launch(CI, 1, tc) == 0
        diff = (y.cpu().view(torch.int32) != k.y.float().view(torch.int32)).nonzero()
        assert not len(diff), "tile %d: %d outputs differ; first at [image, row, column, channel] %s" % (
            tc, len(diff), diff[0].tolist())
        diff = (cx.acc_download(st, shift, det) != k.st.float()).nonzero()
        assert not len(diff), "tile %d: %d statistics differ; first at [slot, row, channel] %s" % (
            tc, len(diff), diff[0].tolist())
        for buf, fill in ((ybuf, cx.Y_CANARY), (stbuf, 7)):
            assert bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())
