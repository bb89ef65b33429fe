"""ImageNet weight-gradient kernels of ops/csrc/convg.hip, launched directly with hand-built work lists and compared
BITWISE with a float64 CPU reference (tests/_convg_exact.py: small-integer operands, every sum exact below 2^24; the
conditions are asserted on the reference before the kernel output is looked at, and in the CPU suite by
tests/test_convg_exact_constructions.py).

* convg_wgrad_t3_kernel<56, 4>, <28, 7>, <14, 14>, plain and with relu(BN(x)) applied while the halo is staged
  (MX = 1), Ci = 64 (both 32-channel chunks), Co = 64 and once Co = 72 (a second 64-row tile with 8 live rows); two
  partitions of the same bands must give the same dW;
* the same kernel as the space-to-depth stem's weight gradient <112, 2, 4, 16, 2> (cin_real = -3): against the
  7x7 / 2 convolution's gradient over the 3-channel image, input rearranged by the project's own cg_prep_input_s2d;
* convg_wgrad_wide_kernel 64 / 128 x 288 and x 256 (table form and P1 form), MX 0 / 1;
* convg_wgrad_kernel (generic split-K) 128-row, 64-row and P1 forms.

Every launch accumulates into a pre-filled [capacity 3][g_mstride] buffer of which the WHOLE content is compared:
the words before and after a member's [Co][Kr] block and the row of the unused slot are canaries.  Members sit in
slots 0 and 2; the work lists hold items that start mid-image / mid-row, cross image boundaries, have one band / one
pixel or a ragged last k-step (asserted on the list that is launched).
"""
import ctypes

import pytest
import torch

import _convg_exact as cx

pytestmark = pytest.mark.gpu


def _run_wgrad(c, items, launch, x_dev=None, geom=None):
    """Launch one weight-gradient kernel over ``items`` into a fresh pre-filled buffer; the decoded buffer (fp32)."""
    ops, hi, dev, det = cx.gpu_env()
    cx.check_wgrad(c)  # the reference alone
    dt = ops.act_dtype()
    x = x_dev if x_dev is not None else c.x.to(dt).to(dev)
    dy, coef = c.dy.to(dt).to(dev), c.coef.float().to(dev)
    grads = cx.acc_upload(c.prefill, cx.FX_GRAD, det, dev)
    work = torch.tensor(items, dtype=torch.int32, device=dev)
    a = hi.CgArgs()
    a.x, a.dy, a.c_in, a.grads, a.work = x.data_ptr(), dy.data_ptr(), coef.data_ptr(), grads.data_ptr(), work.data_ptr()
    a.g_mstride, a.g_off, a.cmax = c.g_mstride, cx.G_OFF, cx.CMAX
    if geom is None:
        a.Hi = a.Wi = c.hw
        a.Ho = a.Wo = c.ho
        a.Ci, a.Co, a.kh, a.kw, a.stride, a.pad = c.ci, c.co, c.k, c.k, c.stride, c.pad
        a.log2ci, a.cin_real = c.ci.bit_length() - 1, c.ci
    else:
        geom(a)
    rc = launch(ops.lib(), ctypes.byref(a), len(items), ops.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return cx.acc_download(grads, cx.FX_GRAD, det)


def _assert_rows(got, c):
    want = c.ref.float()
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        s, i = (int(v) for v in bad[0])
        j = i - cx.G_OFF
        pytest.fail("%d words differ; first: slot %d word %d (o %d, column %d of %d): got %r want %r" % (
            bad.shape[0], s, i, j // c.kr, j % c.kr, c.kr, float(got[s, i]), float(want[s, i])))


# ------------------------------------------------------------------------------------------- 1. row-band 3x3
_T3 = [(w, r, mx, kind, 64) for w, r in cx.T3_GEO for mx in (0, 1) for kind in ("ragged", "even")]
_T3.append((56, 4, 1, "ragged", 72))


@pytest.mark.parametrize("w,r,mode_x,kind,co", _T3, ids=["w%d-mx%d-%s-co%d" % (t[0], t[2], t[3], t[4]) for t in _T3])
def test_wgrad_t3_is_exact(w, r, mode_x, kind, co):
    sizes, bpi = cx.t3_sizes(w, r), w // r
    c = cx.wgrad_case(w, 64, co, 3, 1, sizes, mode_x)
    tiles = cx.t3_tiles(64, co)
    items = cx.band_items(sizes, bpi, tiles, kind)
    cx.assert_partition(items, [(s, f * bpi, e * bpi) for s, f, e in cx.member_ranges(sizes)], tiles)
    cov = cx.band_coverage(items, sizes, bpi)
    assert all(cov[k] for k in cx.band_need(bpi, kind)), cov
    got = _run_wgrad(c, items, lambda L, a, n, st: L.dtf_convg_wgrad_t3(a, w, r, n, mode_x, st))
    _assert_rows(got, c)  # both partitions against the one reference: the same dW


# ---------------------------------------------------------------------------------- 2. space-to-depth stem form
def test_wgrad_t3_stem_s2d_is_exact():
    ops, hi, dev, det = cx.gpu_env()
    c = cx.stem_wgrad_case()
    items = cx.stem_items(cx.STEM_CUTS_WGRAD)
    cx.assert_partition(items, [(s, f * 56, e * 56) for s, f, e in cx.member_ranges(c.sizes)], [0])
    cov = cx.band_coverage(items, c.sizes, cx.STEM_BPI)
    assert cov["starts_off_first_band"] and cov["crosses_image"] and cov["single_band"], cov

    def geom(a):
        a.Hi = a.Wi = a.Ho = a.Wo = 112
        a.Ci, a.Co, a.kh, a.kw, a.stride, a.pad, a.log2ci, a.cin_real = 16, 64, 4, 4, 1, 2, 4, -3

    got = _run_wgrad(c, items, lambda L, a, n, st: L.dtf_convg_wgrad_t3(a, 112, 2, n, 0, st),
                     x_dev=cx.s2d_device_input(c.x, ops, dev), geom=geom)
    # all 64 x 147 entries; the 64 x (256 - 147) discarded columns wrote nothing: the words around the block
    # (and the unused slot's row) are the pre-fill
    _assert_rows(got, c)


# ------------------------------------------------------------------------------------------- 4. wide split-K
def _pixel_list(c, wo, wt):
    hwo = c.ho * c.ho
    tiles = cx.gemm_tiles(c.co, c.k * c.k * c.ci, wo, wt)
    items = cx.pixel_items(c.sizes, hwo, tiles)
    cx.assert_partition(items, [(s, f * hwo, e * hwo) for s, f, e in cx.member_ranges(c.sizes)], tiles)
    cov = cx.pixel_coverage(items, c.sizes, hwo, c.ho)
    assert all(cov[k] for k in cx.PIXEL_NEED), cov
    return items


@pytest.mark.parametrize("mode_x", [0, 1])
@pytest.mark.parametrize("sub", cx.WIDE_SUB, ids=[s[0] for s in cx.WIDE_SUB])
@pytest.mark.parametrize("wo", [128, 64])
def test_wgrad_wide_is_exact(wo, sub, mode_x):
    _, k, stride, ci, wt = sub
    c = cx.wgrad_case(14, ci, wo, k, stride, cx.WIDE_SIZES, mode_x)
    items = _pixel_list(c, wo, wt)
    got = _run_wgrad(c, items, lambda L, a, n, st: L.dtf_convg_wgrad_wide(a, wo, wt, n, mode_x, st))
    _assert_rows(got, c)


# ---------------------------------------------------------------------------------------- 5. generic split-K
@pytest.mark.parametrize("sub", cx.GENERIC_SUB, ids=[s[0] for s in cx.GENERIC_SUB])
def test_wgrad_generic_is_exact(sub):
    _, k, stride, ci, co, flags = sub
    c = cx.wgrad_case(14, ci, co, k, stride, cx.WIDE_SIZES, 0)
    items = _pixel_list(c, 64 if flags & 8 else 128, 128)
    got = _run_wgrad(c, items, lambda L, a, n, st: L.dtf_convg_wgrad(a, 0, flags, n, st))
    _assert_rows(got, c)
