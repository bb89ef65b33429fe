"""convg_t3n_kernel behind ``dtf_convg_t3`` (ops/csrc/convg.hip), bit for bit against float64 ``conv2d`` /
``conv_transpose2d`` on small-integer operands (the argument of tests/_convg_fwd_exact.py).

Packs of whole 7 x 7 images, EPI 4 / 5 / 6: Ci = 64 (two channel chunks), Co = 136 (a full and a ragged channel tile);
slot 0 owns PACK + 1 images (a full and a one-image pack), the next image is nobody's (NaN everywhere), slot 2 owns one
image; the idle slot's weights and coefficients are NaN, its pre-seeded statistics row keeps its words; canary guards
around the output; a bad geometry returns -2 and a missing instantiation -1 with every pre-fill intact.
EPI 5 at 56 / 28 / 14: ``t3_case`` plus an integer residual.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import _convg_exact as cx
import _convg_fwd_exact as fx

pytestmark = pytest.mark.gpu

CI, CO = 64, 136


@functools.lru_cache(maxsize=None)
def pack_case(epi, pack):
    """Like fx.t3_case, for Ci != Co and members (slot, first image, end image) around a NaN image."""
    c, dgrad = fx.Case(), epi == 6
    c.ranges, c.idle, n = [(0, 0, pack + 1), (2, pack + 2, pack + 3)], pack + 1, pack + 3
    g = torch.Generator().manual_seed(fx._seed("t3pack", epi, pack))
    c.x, c.xm, c.res = (cx._ints(g, (n, 7, 7, ch), -2, 2) for ch in (CI, CO, CO))
    wshape = (cx.CAP, CI, 3, 3, CO) if dgrad else (cx.CAP, CO, 3, 3, CI)  # forward layout [o][ky][kx][i]
    c.w = (2 * cx._ints(g, wshape, 0, 1) - 1) * (torch.randint(0, 16, wshape, generator=g) == 0)
    c.c_ep, c.seed_st = fx.ep_coefs(g, CO), cx._ints(g, (cx.CAP, 2, cx.CMAX), -3, 3)
    c.y = torch.full((n, 7, 7, CO), cx.Y_CANARY, dtype=torch.float64)
    c.st, c.ab, c.big, c.u = c.seed_st.clone(), c.seed_st.abs(), 0.0, torch.ones(n, 7, 7, CO)
    for s, f, e in c.ranges:
        xn, wn = c.x[f:e].permute(0, 3, 1, 2), c.w[s].permute(0, 3, 1, 2)
        if dgrad:
            c.u[f:e] = c.xm[f:e] * c.c_ep[s, 0, :CO] + c.c_ep[s, 1, :CO]
            y = F.conv_transpose2d(xn, wn, padding=1).permute(0, 2, 3, 1)
            y = torch.where(c.u[f:e] > 0, y, torch.zeros_like(y))
            q = y * (c.xm[f:e] - c.c_ep[s, 2, :CO]) * c.c_ep[s, 3, :CO]
            c.big = max(c.big, float(q.abs().max()))
        else:
            y = F.conv2d(xn, wn, padding=1).permute(0, 2, 3, 1) + (c.res[f:e] if epi == 5 else 0)
            q = y * y
        c.y[f:e] = y
        c.st[s, :, :CO] += torch.stack([y.sum((0, 1, 2)), q.sum((0, 1, 2))])
        c.ab[s, :, :CO] += torch.stack([y.abs().sum((0, 1, 2)), q.abs().sum((0, 1, 2))])
    for t in (c.x, c.xm, c.res, c.u):
        t[c.idle] = fx.NAN
    c.w[fx.IDLE_SLOT] = fx.NAN
    return c


def check(y, ab, u, big, dt):
    """The conditions of fx.check_t3: integer outputs the 16-bit format holds, half of the unmasked ones non-zero,
    sums below 2^24; masked: a wave's partial (112 pixels) below the deterministic build's limit, ties present."""
    assert bool((y == y.round()).all()) and y.abs().max() <= min(cx.INT_EXACT[torch.bfloat16], cx.INT_EXACT[dt])
    assert ab.max() < cx.EXACT and big * 112 < fx.FX_LIMIT
    assert big == 0 or (int((u == 0).sum()) >= 8 and 0.25 <= float((u > 0).double().mean()) <= 0.75)
    assert float((y[u > 0] != 0).double().mean()) >= 0.5


def launch(hw, ci, co, tc, epi, flags, items, x, w, y, st, res=None, xm=None, c_ep=None):
    ops, hi, dev, _ = cx.gpu_env()
    work = torch.tensor(items, dtype=torch.int32, device=dev)
    a = hi.CgArgs()
    a.x, a.y, a.w, a.work, a.st_out = x.data_ptr(), y.data_ptr(), w.data_ptr(), work.data_ptr(), st.data_ptr()
    a.res, a.xm, a.c_ep = (t.data_ptr() if t is not None else None for t in (res, xm, c_ep))
    a.w_mstride, a.w_off = w[0].numel(), 0
    a.Hi = a.Wi = a.Ho = a.Wo = hw
    a.Ci, a.Co = ci, co
    a.kh = a.kw = 3
    a.stride, a.pad, a.cmax, a.log2ci, a.flags = 1, 1, cx.CMAX, ci.bit_length() - 1, flags
    rc = ops.lib().dtf_convg_t3(ctypes.byref(a), tc, epi, int(epi == 6), hw, work.shape[0], 0, ops.stream())
    torch.cuda.synchronize()
    return rc


def assert_same(ybuf, y, want, st, want_st, shift, det):
    dt, g = y.dtype, fx.GUARD
    diff = (fx.bits(y.cpu()) != fx.bits(want.to(dt))).nonzero()
    assert not len(diff), "%d outputs differ; first at [image, row, column, channel] %s" % (len(diff), diff[0].tolist())
    assert bool((ybuf[:g] == cx.Y_CANARY).all()) and bool((ybuf[-g:] == cx.Y_CANARY).all())
    diff = (cx.acc_download(st, shift, det) != want_st.float()).nonzero()
    assert not len(diff), "%d statistics differ; first at [slot, row, channel] %s" % (len(diff), diff[0].tolist())


@pytest.mark.parametrize("epi,flags", [(4, 1), (4, 0), (5, 1), (5, 0), (6, 1)])  # flags 1: staged A, 0: direct A
def test_convg_t3_pack_is_exact(epi, flags):
    ops, hi, dev, det = cx.gpu_env()
    pack, dt = ops.lib().dtf_convg_t3_pack(), ops.act_dtype()
    k = pack_case(epi, pack)
    members = [i for _, f, e in k.ranges for i in range(f, e)]
    check(k.y[members], k.ab, k.u[members], k.big, dt)
    assert torch.equal(k.st[fx.IDLE_SLOT], k.seed_st[fx.IDLE_SLOT]) and bool((k.y[k.idle] == cx.Y_CANARY).all())
    x, w, res, xm = (t.to(dt).to(dev) for t in (k.x, k.w, k.res, k.xm))
    ybuf, y = fx.guarded(tuple(k.y.shape), cx.Y_CANARY, dt, dev)
    shift = cx.FX_GRAD if epi == 6 else cx.FX_STAT
    st = cx.acc_upload(k.seed_st, shift, det, dev)
    items = [[s, i * 49, min(i + pack, e) * 49, o0] for s, f, e in k.ranges for i in range(f, e, pack)
             for o0 in range(0, CO, 128)]
    assert sorted({(b - a) // 49 for _, a, b, _ in items}) == [1, pack]  # full, ragged and one-image packs
    kw = dict(res=res if epi == 5 else None, xm=xm if epi == 6 else None,
              c_ep=k.c_ep.float().to(dev) if epi == 6 else None)
    assert launch(7, 48, CO, 128, epi, flags, items, x, w, y, st, **kw) == -2  # Ci no multiple of 32
    assert launch(7, CI, CO, 64, epi, flags, items, x, w, y, st, **kw) == -1  # no 64-channel tiles at width 7
    assert bool((ybuf == cx.Y_CANARY).all()) and torch.equal(cx.acc_download(st, shift, det), k.seed_st.float())
    assert launch(7, CI, CO, 128, epi, flags, items, x, w, y, st, **kw) == 0
    assert_same(ybuf, y, k.y, st, k.st, shift, det)


@pytest.mark.parametrize("hw,c", fx.T3_GEO)
@pytest.mark.parametrize("flags", [1, 0])
def test_convg_t3_residual_is_exact(hw, c, flags):
    """EPI 5 at the row-band widths: y = conv(x) + res, statistics sum y and sum y^2 of the sum."""
    ops, hi, dev, det = cx.gpu_env()
    k, dt = fx.t3_case(hw, c, False), ops.act_dtype()
    res = cx._ints(torch.Generator().manual_seed(fx._seed("t3res", hw)), tuple(k.y.shape), -2, 2)
    want, st, ab = k.y + res, k.seed_st.clone(), k.seed_st.abs()
    for s, f, e in fx.T3_RANGES:
        v = want[f:e]
        st[s, :, :c] += torch.stack([v.sum((0, 1, 2)), (v * v).sum((0, 1, 2))])
        ab[s, :, :c] += torch.stack([v.abs().sum((0, 1, 2)), (v * v).sum((0, 1, 2))])
    check(want, ab, torch.ones_like(want), 0.0, dt)
    ybuf, y = fx.guarded(tuple(k.y.shape), cx.Y_CANARY, dt, dev)
    acc = cx.acc_upload(k.seed_st, cx.FX_STAT, det, dev)
    rows, tc = hi._CG_T3[hw], 64 if hw == 56 else 128
    items = [[s, (img * hw + y0) * hw, (img * hw + y0 + rows) * hw, o0] for s, f, e in fx.T3_RANGES
             for img in range(f, e) for y0 in range(0, hw, rows) for o0 in range(0, c, tc)]
    xd, wd, rd = (t.to(dt).to(dev) for t in (k.x, k.w, res))
    assert launch(hw, c, c, tc, 5, flags, items, xd, wd, y, acc, res=rd) == 0
    assert_same(ybuf, y, want, acc, st, cx.FX_STAT, det)
