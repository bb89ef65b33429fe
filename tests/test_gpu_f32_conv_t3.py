"""f32conv_t3_kernel behind ``dtf_f32_conv_t3`` (ops/csrc/f32conv.hip), bit for bit against float64 ``conv2d`` /
``conv_transpose2d`` on small-integer operands (the argument of tests/_convg_exact.py: every sum stays an integer below
2^24, exact in fp32 in any order and in the deterministic build's fixed point).  Ci = 32 (two chunks: the chunk loop
and its prefetch), Co = 80 (full channel tiles and a partial one); members in slots 0 and 2 of capacity 3 with 2 and 1
images (width 7: 5 -- a full and a ragged one-image pack -- and 1) around a NaN image that is nobody's; NaN weights and
coefficients and a pre-seeded statistics row in the idle slot; guards around every buffer.
"""
import ctypes
import functools
import types

import pytest
import torch
import torch.nn.functional as F

import _convg_exact as cx

pytestmark = pytest.mark.gpu
CI, CO, GUARD, NAN = 32, 80, 4096, float("nan")
FX_LIMIT = 2.0 ** (54 - cx.FX_GRAD)  # common.h DTF_FX_LIMIT at the gradient scale, for a wave's partial (112 pixels)


@functools.lru_cache(maxsize=None)
def case(hw, epi):
    """Operands, float64 outputs ``y`` (canary where nobody writes) and statistics rows ``st`` of one launch."""
    c, dgrad = types.SimpleNamespace(), epi >= 6
    c.ranges = [(s, f + i, e + i) for i, (s, f, e) in enumerate(cx.member_ranges((5, 1) if hw == 7 else (2, 1)))]
    n, c.idle = c.ranges[-1][2], c.ranges[0][2]
    g = torch.Generator().manual_seed(1000 * hw + epi)
    c.x, c.xm, c.res = (cx._ints(g, (n, hw, hw, ch), -2, 2) for ch in (CI, CO, CO))
    c.w = cx._ints(g, (cx.CAP, CI, 3, 3, CO) if dgrad else (cx.CAP, CO, 3, 3, CI), -1, 1)  # OHWI of the forward conv
    c.c_ep = cx._coefs(g, CO)  # mask BN: integer scale, shift; integer mean in [-1, 1], inverse deviation in {1, 2}
    c.c_ep[:, 2, :CO], c.c_ep[:, 3, :CO] = cx._ints(g, (cx.CAP, CO), -1, 1), cx._ints(g, (cx.CAP, CO), 1, 2)
    c.seed_st = cx._ints(g, (cx.CAP, 2, cx.CMAX), -3, 3)
    c.y = torch.full((n, hw, hw, CO), cx.Y_CANARY, dtype=torch.float64)
    c.st, c.ab, c.big = c.seed_st.clone(), c.seed_st.abs(), 0.0
    for s, f, e in c.ranges:
        xn, wn, ep = c.x[f:e].permute(0, 3, 1, 2), c.w[s].permute(0, 3, 1, 2), c.c_ep[s, :, :CO]
        y = (F.conv_transpose2d(xn, wn, padding=1) if dgrad else F.conv2d(xn, wn, padding=1)).permute(0, 2, 3, 1)
        y = y + c.res[f:e] if epi & 1 else y
        if dgrad:
            y = torch.where(c.xm[f:e] * ep[0] + ep[1] > 0, y, torch.zeros_like(y))
        q = y * (c.xm[f:e] - ep[2]) * ep[3] if dgrad else y * y
        c.big = max(c.big, float(q.abs().max())) if dgrad else 0.0
        c.y[f:e] = y + 0.0  # (no negative zero: the kernel's sums start from +0)
        c.st[s, :, :CO] += torch.stack([y.sum((0, 1, 2)), q.sum((0, 1, 2))])
        c.ab[s, :, :CO] += torch.stack([y.abs().sum((0, 1, 2)), q.abs().sum((0, 1, 2))])
    c.x[c.idle], c.xm[c.idle], c.res[c.idle], c.w[1], c.c_ep[1] = NAN, NAN, NAN, NAN, NAN
    return c


def guarded(t, fill, dev, dtype=torch.float32):
    """``t`` on the device inside a buffer with GUARD words of ``fill`` on either side: (buffer, view)."""
    buf = torch.full((t.numel() + 2 * GUARD,), fill, dtype=dtype, device=dev)
    buf[GUARD:-GUARD] = t.to(dtype).reshape(-1)
    return buf, buf[GUARD:-GUARD].view(t.shape)


@pytest.mark.parametrize("epi", [4, 5, 6, 7])
@pytest.mark.parametrize("hw", [56, 28, 14, 7])
def test_f32_conv_t3_is_exact(hw, epi):
    from distributedtf_amd.engine import hip_imagenet_f32 as h32
    ops, hi, dev, det = cx.gpu_env()
    h32._register()
    L, k, dgrad = ops.lib(), case(hw, epi), epi >= 6
    members = [i for _, f, e in k.ranges for i in range(f, e)]
    assert bool((k.y[members] == k.y[members].round()).all()) and k.ab.max() < cx.EXACT and k.big * 112 < FX_LIMIT
    assert float((k.y[members] != 0).double().mean()) >= (0.25 if dgrad else 0.5)
    assert torch.equal(k.st[1], k.seed_st[1]) and bool((k.y[k.idle] == cx.Y_CANARY).all())
    shift = cx.FX_GRAD if dgrad else cx.FX_STAT
    x, w, res, xm, c_ep = (guarded(t, NAN, dev)[1] for t in (k.x, k.w, k.res, k.xm, k.c_ep))
    ybuf, y = guarded(torch.full_like(k.y, cx.Y_CANARY), cx.Y_CANARY, dev)
    seed = cx.acc_upload(k.seed_st, shift, det, dev)
    stbuf, st = guarded(seed, 7, dev, seed.dtype)
    # items by the plan's own rule (_ImageNetPlan._band_work) over this case's members
    plan = types.SimpleNamespace(slots=[s for s, _, _ in k.ranges], sizes=[e - f for _, f, e in k.ranges],
                                 first={s: f for s, f, _ in k.ranges}, _xcd_order=hi._ImageNetPlan._xcd_order,
                                 _hold=lambda t: t, be=types.SimpleNamespace(dev=dev))
    tc, pack = L.dtf_f32_conv_t3_tc(), L.dtf_f32_conv_t3_pack() if hw == 7 else 1
    rows = L.dtf_f32_conv_t3_rows(hw)  # (width 7: a full pack, the ragged one-image pack, the one-image member)
    work = hi._ImageNetPlan._band_work(plan, hw, rows, CO, tc, pack=pack)
    assert {b - a for _, a, b, _ in work.tolist()} == ({49, 49 * pack} if hw == 7 else {rows * hw})
    assert CO % tc != 0 and {r[3] for r in work.tolist()} == set(range(0, CO, tc))  # a partial last channel tile

    def launch(ci, tc_):
        a = h32.F32Args()
        a.x, a.y, a.w, a.work, a.st_out = (t.data_ptr() for t in (x, y, w, work, st))
        a.res, a.xm, a.c_ep = res.data_ptr(), xm.data_ptr(), c_ep.data_ptr()
        a.w_mstride, a.w_off, a.Ci, a.wci, a.Co, a.cmax = w[0].numel(), 0, ci, ci, CO, cx.CMAX
        a.Hi = a.Wi = a.Ho = a.Wo = hw
        a.kh, a.kw, a.stride, a.pad = 3, 3, 1, 1
        rc = L.dtf_f32_conv_t3(ctypes.byref(a), tc_, epi, int(dgrad), hw, work.shape[0], ops.stream())
        torch.cuda.synchronize()
        return rc

    assert launch(24, tc) == -2 and launch(CI, 2 * tc) == -1  # Ci no multiple of 16; no such channel tile
    assert bool((ybuf == cx.Y_CANARY).all()) and torch.equal(st, seed)
    assert launch(CI, tc) == 0
    diff = (y.cpu().view(torch.int32) != k.y.float().view(torch.int32)).nonzero()
    assert not len(diff), "%d outputs differ; first at [image, row, column, channel] %s" % (len(diff), diff[0].tolist())
    diff = (cx.acc_download(st, shift, det) != k.st.float()).nonzero()
    assert not len(diff), "%d statistics differ; first at [slot, row, channel] %s" % (len(diff), diff[0].tolist())
    for buf, fill in ((ybuf, cx.Y_CANARY), (stbuf, 7)):
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())
