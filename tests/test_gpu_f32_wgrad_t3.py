"""f32wgrad_t3_kernel behind ``dtf_f32_wgrad_t3`` (ops/csrc/f32conv.hip), bit for bit against the float64 weight gradient
on small-integer operands (the argument of tests/_convg_exact.py: every sum is an integer below 2^24, exact in fp32 in
any order and in the deterministic build's fixed point).  Ci = 48 (three input chunks), Co = 80 (a full 64-row tile and
a partial one); members in slots 0 and 2 of capacity 3 with 2 and 1 images (width 7: 5 and 1, a run with full packs
and a ragged one, and a one-image run); two partitions of the bands against the one reference.  The whole gradient
buffer is compared: the words before and after a member's block and the idle slot's row are canaries, and NaN guards
surround the buffer and both operands.
"""
import ctypes

import pytest
import torch

import _convg_exact as cx
from test_gpu_f32_conv_t3 import GUARD, NAN, guarded

pytestmark = pytest.mark.gpu
CI, CO = 48, 80
FX_LIMIT = 2.0 ** (54 - cx.FX_GRAD)  # common.h DTF_FX_LIMIT at the gradient scale: bounds every item's partial


@pytest.mark.parametrize("kind", ["ragged", "even"])
@pytest.mark.parametrize("hw", [56, 28, 14, 7])
def test_f32_wgrad_t3_is_exact(hw, kind):
    from distributedtf_amd.engine import hip_imagenet_f32 as h32
    ops, _, dev, det = cx.gpu_env()
    h32._register()
    L = ops.lib()
    sizes = (5, 1) if hw == 7 else (2, 1)
    c = cx.wgrad_case(hw, CI, CO, 3, 1, sizes, 0)
    cx.check_wgrad(c)
    assert c.absref.max() < FX_LIMIT
    bpi, pack, to, ti = hw // L.dtf_f32_wgrad_t3_rows(hw), L.dtf_f32_wgrad_t3_pack(), L.dtf_f32_wgrad_t3_to(), \
        L.dtf_f32_wgrad_t3_ti()
    tiles = [o0 | (cc << 16) for o0 in range(0, CO, to) for cc in range(CI // ti)]
    assert CO % to != 0 and CI // ti > 1
    items = cx.band_items(sizes, bpi, tiles, kind)
    cx.assert_partition(items, [(s, f * bpi, e * bpi) for s, f, e in cx.member_ranges(sizes)], tiles)
    cov = cx.band_coverage(items, sizes, bpi)
    assert all(cov[k] for k in cx.band_need(bpi, kind)), cov
    if hw == 7:  # a run of full packs that ends in a ragged one
        assert any(b1 - b0 > pack and (b1 - b0) % pack for _, b0, b1, _ in items)
    x, dy = (guarded(t, NAN, dev)[1] for t in (c.x, c.dy))
    seed = cx.acc_upload(c.prefill, cx.FX_GRAD, det, dev)
    fill = 7 if det else NAN
    gbuf, grads = guarded(seed, fill, dev, seed.dtype)
    work = torch.tensor(items, dtype=torch.int32, device=dev)

    def launch(ci, w):
        a = h32.F32Args()
        a.x, a.dy, a.grads, a.work = x.data_ptr(), dy.data_ptr(), grads.data_ptr(), work.data_ptr()
        a.g_mstride, a.g_off, a.Ci, a.wci, a.Co, a.cmax = c.g_mstride, cx.G_OFF, ci, ci, CO, cx.CMAX
        a.Hi = a.Wi = a.Ho = a.Wo = w
        a.kh, a.kw, a.stride, a.pad = 3, 3, 1, 1
        rc = L.dtf_f32_wgrad_t3(ctypes.byref(a), w, work.shape[0], ops.stream())
        torch.cuda.synchronize()
        return rc

    assert launch(24, hw) == -2 and launch(CI, 32) == -1  # Ci no multiple of 16; a width without an instantiation
    assert torch.equal(grads, seed)
    assert launch(CI, hw) == 0
    got, want = cx.acc_download(grads, cx.FX_GRAD, det), c.ref.float()
    diff = (got.view(torch.int32) != want.view(torch.int32)).nonzero()
    assert not len(diff), "%d words differ; first at slot %d word %d (block starts at %d, row length %d): %r, not %r" % (
        len(diff), diff[0][0], diff[0][1], cx.G_OFF, c.kr, float(got[tuple(diff[0])]), float(want[tuple(diff[0])]))
    for g in (gbuf[:GUARD], gbuf[-GUARD:]):
        assert bool((g == fill).all() if det else g.isnan().all())
