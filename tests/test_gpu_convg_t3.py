"""Stride-1 3x3 conv kernel with LDS-resident input rows (ops/csrc/convg.hip convg_t3_kernel) vs fp32 PyTorch.

Forward (statistics epilogue) and data gradient (A operand from the forward weight layout, ReLU mask by BN(xm),
BN-backward statistics) at every instantiated geometry: 56 x 56 x 64 (8-row tiles of 448 pixels), 28 x 28 x 128
(8-row tiles) and 14 x 14 x 256 (whole images in 224-pixel tiles); two members with their own weight rows.

The folded forward (``dtf_convg_t3`` mode 1, convg_t3_kernel XF: relu(x * scale + shift) applied while the input rows
are staged, padding left zero) at the same geometries is compared bitwise with a float64 reference on small-integer
operands (tests/_convg_exact.py ``t3_fold_case``: |y| <= 256 and sum(y^2) < 2^24 are asserted on the reference first).
So are the plain (mode 0) forward and the data gradient (EPI 6, akm = 1) with both statistics rows
(tests/_convg_fwd_exact.py ``t3_case``); ``test_convg_t3_matches_torch`` keeps the full-mantissa comparison.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CMAX = 512


def _relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("hw,c", [(56, 64), (28, 128), (14, 256)])
@pytest.mark.parametrize("dgrad", [False, True])
@pytest.mark.parametrize("flags", [1, 0])  # 1: staged A (product default, hip_imagenet.T3_FLAGS); 0: direct A
def test_convg_t3_matches_torch(hw, c, dgrad, flags):
    from distributedtf_amd import ops
    from distributedtf_amd.engine import hip_imagenet as hi
    hi._register()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(hw + int(dgrad))
    slots = [0, 0, 1]  # image -> member
    n = len(slots)
    x = torch.randn(n, hw, hw, c, generator=g).bfloat16()
    w = (torch.randn(2, c, 3, 3, c, generator=g) / (3 * c ** 0.5)).bfloat16()  # [member][o][ky][kx][i]
    xm = torch.randn(n, hw, hw, c, generator=g).bfloat16()
    ep = torch.zeros(2, 4, CMAX)
    ep[:, 0, :c] = 1.0 + 0.1 * torch.randn(2, c, generator=g)
    ep[:, 1, :c] = 0.1 * torch.randn(2, c, generator=g)
    ep[:, 2, :c] = 0.1 * torch.randn(2, c, generator=g)
    ep[:, 3, :c] = 1.0 + 0.1 * torch.rand(2, c, generator=g)
    xd, wd, xmd, epd = x.to(dev), w.to(dev), xm.to(dev), ep.to(dev)
    y = torch.zeros(n, hw, hw, c, dtype=torch.bfloat16, device=dev)
    st = torch.zeros(2, 2, CMAX, device=dev)
    rows = hi._CG_T3[hw]
    tc = 64 if hw == 56 else 128
    items = []
    for img, s in enumerate(slots):
        for y0 in range(0, hw, rows):
            p0 = (img * hw + y0) * hw
            for o0 in range(0, c, tc):
                items.append([s, p0, p0 + rows * hw, o0])
    work = torch.tensor(items, dtype=torch.int32, device=dev)
    a = hi.CgArgs()
    a.x, a.y, a.w, a.work, a.st_out = xd.data_ptr(), y.data_ptr(), wd.data_ptr(), work.data_ptr(), st.data_ptr()
    a.w_mstride, a.w_off = c * 9 * c, 0
    a.Hi = a.Wi = a.Ho = a.Wo = hw
    a.Ci = a.Co = c
    a.kh = a.kw = 3
    a.stride, a.pad = 1, 1
    a.cmax = CMAX
    a.log2ci = c.bit_length() - 1
    a.flags = flags
    if dgrad:
        a.xm, a.c_ep = xmd.data_ptr(), epd.data_ptr()
    rc = ops.lib().dtf_convg_t3(ctypes.byref(a), tc, 6 if dgrad else 4, int(dgrad), hw, work.shape[0], 0,
                                ops.stream())  # mode 0: plain operand (no folded BN)
    assert rc == 0, rc
    torch.cuda.synchronize()
    yh, sth = y.float().cpu(), st.cpu()
    xf = x.float().permute(0, 3, 1, 2)
    for s in (0, 1):
        sel = [i for i, t in enumerate(slots) if t == s]
        wo = w[s].float().permute(0, 3, 1, 2)  # [o][i][ky][kx]
        if dgrad:
            ref = F.conv_transpose2d(xf[sel], wo, padding=1).permute(0, 2, 3, 1)
            xms = xm[sel].float()
            keep = xms * ep[s, 0, :c] + ep[s, 1, :c] > 0
            ref = torch.where(keep, ref, torch.zeros_like(ref))
            xhat = (xms - ep[s, 2, :c]) * ep[s, 3, :c]
            out = yh[sel]
            s0, s1 = out.sum((0, 1, 2)), (out * xhat).sum((0, 1, 2))
        else:
            ref = F.conv2d(xf[sel], wo, padding=1).permute(0, 2, 3, 1)
            out = yh[sel]
            s0, s1 = out.sum((0, 1, 2)), (out * out).sum((0, 1, 2))
        assert _relerr(out, ref) < 1e-2, (s, _relerr(out, ref))
        assert _relerr(sth[s, 0, :c], s0) < 1e-3 and _relerr(sth[s, 1, :c], s1) < 1e-3


@pytest.mark.parametrize("hw,c", [(56, 64), (28, 128), (14, 256)])
@pytest.mark.parametrize("flags", [1, 0])
def test_convg_t3_folded_forward_is_exact(hw, c, flags):
    """mode 1 (XF), forward: output and both statistics rows of members in slots 0 and 2 (capacity 3) equal the
    float64 reference bit for bit; the statistics row of the unused slot stays zero."""
    import _convg_exact as cx
    ops, hi, dev, det = cx.gpu_env()
    k = cx.t3_fold_case(hw, c)
    dt = ops.act_dtype()
    cx.check_t3_fold(k, dt)  # the reference alone
    n = k.x.shape[0]
    xd, wd, cd = k.x.to(dt).to(dev), k.w.to(dt).to(dev), k.coef.float().to(dev)
    y = torch.full((n, hw, hw, c), cx.Y_CANARY, dtype=dt, device=dev)
    st = torch.zeros(cx.CAP, 2, cx.CMAX, dtype=torch.int64 if det else torch.float32, device=dev)
    rows = hi._CG_T3[hw]
    tc = 64 if hw == 56 else 128
    items = [[s, (img * hw + y0) * hw, (img * hw + y0 + rows) * hw, o0] for s, f, e in cx.member_ranges(k.sizes)
             for img in range(f, e) for y0 in range(0, hw, rows) for o0 in range(0, c, tc)]
    work = torch.tensor(items, dtype=torch.int32, device=dev)
    a = hi.CgArgs()
    a.x, a.y, a.w, a.work, a.st_out, a.c_in = (xd.data_ptr(), y.data_ptr(), wd.data_ptr(), work.data_ptr(),
                                               st.data_ptr(), cd.data_ptr())
    a.w_mstride, a.w_off = c * 9 * c, 0
    a.Hi = a.Wi = a.Ho = a.Wo = hw
    a.Ci = a.Co = c
    a.kh = a.kw = 3
    a.stride, a.pad, a.cmax, a.log2ci, a.flags = 1, 1, cx.CMAX, c.bit_length() - 1, flags
    rc = ops.lib().dtf_convg_t3(ctypes.byref(a), tc, 4, 0, hw, work.shape[0], 1, ops.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = y.cpu().double()
    if not torch.equal(got, k.y):
        bad = (got != k.y).nonzero()
        i, r, col, o = (int(v) for v in bad[0])
        pytest.fail("%d outputs differ; first: image %d row %d column %d channel %d: got %r want %r" % (
            bad.shape[0], i, r, col, o, float(got[i, r, col, o]), float(k.y[i, r, col, o])))
    assert torch.equal(cx.acc_download(st, cx.FX_STAT, det), k.st.float())


@pytest.mark.parametrize("hw,c", [(56, 64), (28, 128), (14, 256)])
@pytest.mark.parametrize("dgrad", [False, True])
@pytest.mark.parametrize("flags", [1, 0])
def test_convg_t3_plain_is_exact(hw, c, dgrad, flags):
    """mode 0: the forward (EPI 4) and the data gradient (EPI 6, akm = 1: taps flipped over the forward weight layout,
    mask by BN(xm) > 0, sums dz and dz xhat) of members in slots 0 and 2 (capacity 3) equal the float64 reference bit
    for bit (tests/_convg_fwd_exact.py ``t3_case``); the statistics rows are pre-seeded with integers, the idle
    slot's row and the columns past the channel count stay as seeded, the idle slot's weights and coefficients are
    NaN and the output sits between canary guards."""
    import _convg_exact as cx
    import _convg_fwd_exact as fx
    ops, hi, dev, det = cx.gpu_env()
    k = fx.t3_case(hw, c, dgrad)
    dt = ops.act_dtype()
    fx.check_t3(k, dt)  # the reference alone
    n = k.x.shape[0]
    xd, wd, xmd, epd = k.x.to(dt).to(dev), k.w.to(dt).to(dev), k.xm.to(dt).to(dev), k.c_ep.float().to(dev)
    ybuf, y = fx.guarded((n, hw, hw, c), cx.Y_CANARY, dt, dev)
    shift = cx.FX_GRAD if dgrad else cx.FX_STAT
    st = cx.acc_upload(k.seed_st, shift, det, dev)
    rows = hi._CG_T3[hw]
    tc = 64 if hw == 56 else 128
    items = [[s, (img * hw + y0) * hw, (img * hw + y0 + rows) * hw, o0] for s, f, e in fx.T3_RANGES
             for img in range(f, e) for y0 in range(0, hw, rows) for o0 in range(0, c, tc)]
    work = torch.tensor(items, dtype=torch.int32, device=dev)
    a = hi.CgArgs()
    a.x, a.y, a.w, a.work, a.st_out = xd.data_ptr(), y.data_ptr(), wd.data_ptr(), work.data_ptr(), st.data_ptr()
    a.w_mstride, a.w_off = c * 9 * c, 0
    a.Hi = a.Wi = a.Ho = a.Wo = hw
    a.Ci = a.Co = c
    a.kh = a.kw = 3
    a.stride, a.pad, a.cmax, a.log2ci, a.flags = 1, 1, cx.CMAX, c.bit_length() - 1, flags
    if dgrad:
        a.xm, a.c_ep = xmd.data_ptr(), epd.data_ptr()
    rc = ops.lib().dtf_convg_t3(ctypes.byref(a), tc, 6 if dgrad else 4, int(dgrad), hw, work.shape[0], 0, ops.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = y.cpu().double()
    if not torch.equal(got, k.y):
        bad = (got != k.y).nonzero()
        i, r, col, o = (int(v) for v in bad[0])
        pytest.fail("%d outputs differ; first: image %d row %d column %d channel %d: got %r want %r" % (
            bad.shape[0], i, r, col, o, float(got[i, r, col, o]), float(k.y[i, r, col, o])))
    g = fx.GUARD
    assert bool((ybuf[:g] == cx.Y_CANARY).all()) and bool((ybuf[-g:] == cx.Y_CANARY).all())
    gs = cx.acc_download(st, shift, det)
    if not torch.equal(gs, k.st.float()):
        bad = (gs != k.st.float()).nonzero()
        s, r, o = (int(v) for v in bad[0])
        pytest.fail("%d statistics differ; first: slot %d row %d channel %d: got %r want %r" % (
            bad.shape[0], s, r, o, float(gs[s, r, o]), float(k.st[s, r, o])))
