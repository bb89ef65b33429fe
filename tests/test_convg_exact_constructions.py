"""The integer constructions of tests/_convg_exact.py, without a device: every case the exact GPU tests launch
(tests/test_gpu_convg_wgrad.py, test_gpu_stem_s2d.py, the folded case of test_gpu_convg_t3.py) satisfies the
conditions that make a bitwise comparison legitimate, the hand-built work lists have the edges they are meant to
have, and the host mirror of the space-to-depth rearrangement composes to the 7x7 / 2 convolution exactly -- so a
GPU mismatch cannot be blamed on the reference."""
import pytest
import torch
import torch.nn.functional as F

import _convg_exact as cx


def test_wgrad_constructions_are_exact():
    """sum |dy| |x'| + |prefill| < 2^24 for every gradient element of every weight-gradient case; operand ranges;
    scale / shift sets (relu(x * scale + shift) <= 6)."""
    cases = cx.all_wgrad_cases()
    assert len(cases) == 28
    for c in cases:
        cx.check_wgrad(c)
        assert c.absref.max() <= 4 * 6 * 3 * 112 * 112 + 3  # the crude bound: |dy| |x'| pixels of the largest member


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_stem_and_folded_forward_constructions_are_exact(dtype):
    """Stem |y| inside the dtype's exact-integer range and sum(y^2) < 2^24 per (member, channel); the same for the
    folded 3x3 forward; every operand survives the round trip through the 16-bit type."""
    s = cx.stem_case()
    cx.check_stem_fwd(s, dtype)
    yexp, st = cx.stem_fwd_expected(s, cx.stem_items(cx.STEM_CUTS_FWD))
    assert st[:, 1].max() < cx.EXACT and bool((st[1] == 0).all())
    assert int((yexp == cx.Y_CANARY).all(-1).sum()) == 18 * 2 * 112  # the bands of image 2 left out of the launch
    for hw, ch in cx.T3_FOLD_GEO:
        c = cx.t3_fold_case(hw, ch)
        cx.check_t3_fold(c, dtype)
        for t in (c.x, c.w, c.y):
            assert torch.equal(t.to(dtype).double(), t)
    for t in (s.img, s.w, s.y, s.dy, cx.wgrad_case(14, 64, 64, 3, 1, (1, 2), 1).x):
        assert torch.equal(t.to(dtype).double(), t)
    assert torch.equal(torch.tensor([cx.Y_CANARY]).to(dtype).double(), torch.tensor([cx.Y_CANARY]).double())


def test_work_lists_have_their_edges():
    for w, r in cx.T3_GEO:
        bpi, sizes = w // r, cx.t3_sizes(w, r)
        ranges = [(s, f * bpi, e * bpi) for s, f, e in cx.member_ranges(sizes)]
        seen = {}
        for kind in ("ragged", "even"):
            for co in (64, 72):
                tiles = cx.t3_tiles(64, co)
                assert len(tiles) == 2 * -(-co // 64)  # both 32-channel chunks of every 64-row tile
                items = cx.band_items(sizes, bpi, tiles, kind)
                cx.assert_partition(items, ranges, tiles)
                cov = cx.band_coverage(items, sizes, bpi)
                assert all(cov[k] for k in cx.band_need(bpi, kind)), (w, kind, cov)
                seen = {k: seen.get(k, False) or v for k, v in cov.items()}
        if bpi > 1:
            assert all(seen.values()), (w, seen)
    for cuts, need in ((cx.STEM_CUTS_WGRAD, ("starts_off_first_band", "crosses_image", "single_band")),
                       (cx.STEM_CUTS_FWD, ("starts_off_first_band", "crosses_image", "single_band", "ends_mid_image"))):
        items = cx.stem_items(cuts)
        cov = cx.band_coverage(items, cx.STEM_SIZES, cx.STEM_BPI)
        assert all(cov[k] for k in need), cov
    assert [0, 55, 56, 0] in cx.stem_items(cx.STEM_CUTS_FWD)  # the bottom band of image 0 on its own
    ranges = [(s, f * 56, e * 56) for s, f, e in cx.member_ranges(cx.STEM_SIZES)]
    cx.assert_partition(cx.stem_items(cx.STEM_CUTS_WGRAD), ranges, [0])
    for hwo, wo_ in ((196, 14), (49, 7)):
        tiles = cx.gemm_tiles(128, 576, 64, 288)
        items = cx.pixel_items(cx.WIDE_SIZES, hwo, tiles)
        cx.assert_partition(items, [(s, f * hwo, e * hwo) for s, f, e in cx.member_ranges(cx.WIDE_SIZES)], tiles)
        cov = cx.pixel_coverage(items, cx.WIDE_SIZES, hwo, wo_)
        assert all(cov[k] for k in cx.PIXEL_NEED), cov


def test_s2d_host_mirror_composes_to_the_7x7_stride_2_convolution():
    """Input blocks and W'[co][a][b][(2 dy + dx) * 3 + c] = W[co][2a + dy - 1][2b + dx - 1][c], as a 4x4 convolution
    padded 2 before / 1 after, equal the 7x7 / 2 pad-3 convolution exactly; the 4x4 weight gradient mapped back
    through the same table equals the 7x7 one (each 7x7x3 weight is reached from exactly one column)."""
    s = cx.stem_case()
    xs = cx.s2d_input(s.img).permute(0, 3, 1, 2)
    xp = F.pad(xs, (2, 1, 2, 1))
    for slot, f, e in cx.member_ranges(cx.STEM_SIZES):
        w4 = cx.s2d_weight(s.w[slot])
        y4 = F.conv2d(xp[f:e], w4.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
        assert torch.equal(y4, s.y[f:e])
        assert torch.equal(cx.s2d_weight_inverse(w4), s.w[slot])
        assert int((w4 != 0).sum()) == int((s.w[slot] != 0).sum())  # the 256 - 147 other columns are zero
    g = cx.stem_wgrad_case()
    for slot, f, e in cx.member_ranges(cx.STEM_SIZES):
        dn = s.dy[f:e].permute(0, 3, 1, 2).contiguous()
        dw4 = torch.nn.grad.conv2d_weight(xp[f:e].contiguous(), (64, 16, 4, 4), dn).permute(0, 2, 3, 1)
        want = g.ref[slot, cx.G_OFF:cx.G_OFF + 64 * 147] - g.prefill[slot, cx.G_OFF:cx.G_OFF + 64 * 147]
        assert torch.equal(cx.s2d_weight_inverse(dw4).reshape(-1), want)
    # rows of the members outside the [Co][147] block, and the unused slot, are the untouched pre-fill
    assert torch.equal(g.ref[1], g.prefill[1]) and torch.equal(g.ref[:, :cx.G_OFF], g.prefill[:, :cx.G_OFF])
    assert torch.equal(g.ref[:, cx.G_OFF + 64 * 147:], g.prefill[:, cx.G_OFF + 64 * 147:])
