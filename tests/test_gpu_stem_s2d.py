"""The space-to-depth stem forward from row bands (ops/csrc/convg.hip convg_stem_s2d_kernel<112, 2, 0 | 4>: swizzled
LDS output staging, statistics epilogue) against the ORIGINAL operation, the 7x7 stride-2 pad-3 convolution of the
3-channel 224 x 224 image, in float64 on the CPU -- bitwise (tests/_convg_exact.py: image values in [-1, 1], sparse
weights in {-1, 0, 1}; |y| <= 256 and sum(y^2) < 2^24 per member and channel are asserted on the reference first).

The device operands come from the project's own rearrangement kernels, cg_prep_input_s2d and cg_weight_prep (table
row with t[7] = 1, as the backend's conv_table), which are thereby compared exactly with their host mirror too.
Members in slots 0 and 2; band items with a mid-image start, an image crossing, and the bottom band of an image on
its own (the "1 after" padding rows); the last 18 bands of the last image are left out of the launch and must keep the
output canary; statistic rows of slots outside the work list stay zero."""
import ctypes

import pytest
import torch

import _convg_exact as cx

pytestmark = pytest.mark.gpu


def _device_weights(c, ops, dev):
    """[CAP][64 * 256] stem rows written by cg_weight_prep for slots 0 and 2 from the fp32 state rows."""
    wtot = cx.STEM_CO * 256
    state = c.state.float().to(dev)
    table = torch.tensor([[cx.STEM_W_OFF, cx.STEM_CO, 3, 7, 16, 0, -1, 1]], dtype=torch.int32, device=dev)
    slots = torch.tensor(cx.SLOTS, dtype=torch.int32, device=dev)
    wf = torch.full((cx.CAP, wtot), 3.0, dtype=ops.act_dtype(), device=dev)
    rc = ops.lib().dtf_cg_weight_prep(state.data_ptr(), cx.STEM_S, table.data_ptr(), 1, slots.data_ptr(), len(cx.SLOTS),
                                      wf.data_ptr(), wf.data_ptr(), wtot, ops.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = wf.cpu().double().view(cx.CAP, cx.STEM_CO, 4, 4, 16)
    for s in cx.SLOTS:
        assert torch.equal(got[s], cx.s2d_weight(c.w[s]))
    assert bool((got[1] == 3.0).all())  # the slot that was not asked for
    return wf, wtot


@pytest.mark.parametrize("epi", [0, 4])
def test_stem_s2d_forward_is_exact(epi):
    ops, hi, dev, det = cx.gpu_env()
    c = cx.stem_case()
    dt = ops.act_dtype()
    cx.check_stem_fwd(c, dt)  # the reference alone
    items = cx.stem_items(cx.STEM_CUTS_FWD)
    cov = cx.band_coverage(items, cx.STEM_SIZES, cx.STEM_BPI)
    assert all(cov[k] for k in ("starts_off_first_band", "crosses_image", "single_band", "ends_mid_image")), cov
    assert [0, 55, 56, 0] in items  # the bottom band of an image as an item of its own
    yexp, stexp = cx.stem_fwd_expected(c, items)
    assert stexp[:, 1].max() < cx.EXACT

    xs = cx.s2d_device_input(c.img, ops, dev)
    wf, wtot = _device_weights(c, ops, dev)
    n = c.img.shape[0]
    y = torch.full((n, 112, 112, cx.STEM_CO), cx.Y_CANARY, dtype=dt, device=dev)
    st = torch.zeros(cx.CAP, 2, cx.CMAX, dtype=torch.int64 if det else torch.float32, device=dev)
    work = torch.tensor(items, dtype=torch.int32, device=dev)
    a = hi.CgArgs()
    a.x, a.y, a.w, a.work, a.st_out = xs.data_ptr(), y.data_ptr(), wf.data_ptr(), work.data_ptr(), st.data_ptr()
    a.w_mstride, a.w_off = wtot, 0
    a.Hi = a.Wi = a.Ho = a.Wo = 112
    a.Ci, a.Co, a.kh, a.kw, a.stride, a.pad, a.log2ci, a.cmax = 16, cx.STEM_CO, 4, 4, 1, 2, 4, cx.CMAX
    rc = ops.lib().dtf_convg_stem_s2d(ctypes.byref(a), 112, 2, epi, len(items), ops.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = y.cpu().double()
    if not torch.equal(got, yexp):
        bad = (got != yexp).nonzero()
        i, r, col, o = (int(v) for v in bad[0])
        pytest.fail("%d outputs differ; first: image %d row %d column %d channel %d: got %r want %r" % (
            bad.shape[0], i, r, col, o, float(got[i, r, col, o]), float(yexp[i, r, col, o])))
    gst = cx.acc_download(st, cx.FX_STAT, det)
    want = stexp.float() if epi == 4 else torch.zeros_like(gst)  # both rows of both members; other slots stay zero
    assert torch.equal(gst, want), (gst - want).abs().max()
