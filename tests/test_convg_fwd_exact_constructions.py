"""The conditions behind the exact tests of ``dtf_convg_fwd`` and of the plain ``dtf_convg_t3`` forward / data gradient
(tests/_convg_fwd_exact.py), asserted on the float64 references alone -- no device -- and the sync of the case table
with the dispatch table of convg.hip.  These are conditions, not measurements: if one does not hold the bitwise
comparison on the GPU proves nothing, so the density of a case is lowered and the bounds stay."""
import pytest
import torch
import torch.nn.functional as F

import _convg_fwd_exact as fx


def test_case_table_equals_the_dispatch_table():
    """Every CG_ALL_TC line of convg.hip has a case and the other way round: no instantiation untested."""
    src = fx.source_rows()
    assert len(src) == 23 and len(set(src)) == 23
    assert src == fx.ROWS
    inst = fx.instantiations()
    # 23 rows x 2 channel tiles x (base, BK 64, 256-pixel tiles) + the 32x32 MFMA form of the 8 plain-A rows at tc 128
    assert len(inst) == len(set(inst)) == 23 * 2 * 3 + 8 == 146
    launched = {(row, tc, v) for row in fx.ROWS for tc in fx.TCS for v, _, _ in fx.launches(row, tc)}
    assert launched == set(inst)


def test_every_shape_of_the_issue_is_launched():
    shapes = {sh for row in fx.ROWS for sh in fx.row_shapes(row)}
    assert shapes == set(fx.SHAPES)
    for row in fx.ROWS:
        mode, epi, trans, akm = row
        for tc in fx.TCS:
            for v, sh, ci in fx.launches(row, tc):
                assert ci & (ci - 1) == 0 and ci >= 8
                if akm or trans:  # the launcher's own rule for the one-tap-per-k-step gather
                    assert ci >= (64 if v == fx.V_BK64 else 32)
    assert set(fx.row_shapes((0, 4, 0, 0))) >= {"stem7", "s2dfb"} <= set(fx.row_shapes((0, 0, 0, 0)))
    # ragged last k-step of the 7x7 stem for BK 32 and BK 64
    assert (7 * 7 * 8) % 32 != 0 and (7 * 7 * 8) % 64 != 0


@pytest.mark.parametrize("tc", fx.TCS)
@pytest.mark.parametrize("row", fx.ROWS, ids=lambda r: "m%d-e%d-t%d-a%d" % r)
def test_conditions_and_work_lists(row, tc):
    seen = set()
    for v, sh, ci in fx.launches(row, tc):
        c = fx.fwd_case(row, tc, sh, ci)
        if (sh, ci) not in seen:
            seen.add((sh, ci))
            fx.check_case(c)
            assert c.co % tc == 8 and c.co > tc
        tp = fx.tile_pixels(v)
        items = fx.work_items(c, tp)
        fx.check_items(items, c, tp)
        rev = fx.work_items(c, tp, reverse_tiles=True)
        fx.check_items(rev, c, tp)
        assert sorted(items) == sorted(rev) and items != rev
        if c.trans and v == fx.V_BASE:
            # single parity classes: the class word's py * 2 + px contract (the classes' references add up)
            parts = [fx.class_expected(c, (cls,)) for cls in (0, 1, 2, 3)]
            for only in ((1,), (2, 3)):
                fx.check_items(fx.work_items(c, tp, only=only), c, tp, only)
            y, st = fx.class_expected(c, (0, 1, 2, 3))
            assert torch.equal(y, c.out[True][0]) and torch.equal(st, c.out[True][1])
            assert torch.equal(sum(p[1] - c.seed_st for p in parts) + c.seed_st, st)
            assert not torch.equal(parts[1][0], parts[2][0])


def test_member_0_is_a_full_256_pixel_tile_and_a_ragged_one():
    c = fx.fwd_case((0, 4, 0, 0), 64, "1x1s1", 32)
    last = [(a, b) for s, a, b, w in fx.work_items(c, 256) if s == 0 and w == 64]
    assert last == [(0, 256), (256, 286)]


@pytest.mark.parametrize("shape", ["d3x3s1", "t3x3s2", "t1x1s2"])
def test_data_gradient_reference_equals_autograd(shape):
    """conv_transpose2d over the forward-layout weights is the gradient of the float64 forward conv."""
    row = (0, 0, 1, 1) if shape.startswith("t") else (0, 0, 0, 1)
    c = fx.fwd_case(row, 64, shape, 32)
    for s, f, e in fx.RANGES:
        dy = c.x[f:e].permute(0, 3, 1, 2)
        xin = torch.zeros(e - f, c.co, c.ho, c.wo, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(xin, c.w[s].permute(0, 3, 1, 2), stride=c.stride, padding=c.padf)
        assert y.shape == dy.shape
        (gx,) = torch.autograd.grad(y, xin, dy)
        assert torch.equal(gx.permute(0, 2, 3, 1), c.out[True][0][f:e])
    if shape == "t1x1s2":
        y = c.out[True][0]
        live = fx.live_outputs(c)
        member = [i for _, f, e in fx.RANGES for i in range(f, e)]
        assert bool((y[member][~live[member]] == 0).all()), "the K = 0 parity classes store zeros"


@pytest.mark.parametrize("hw,ch", fx.T3_GEO)
@pytest.mark.parametrize("dgrad", [False, True])
def test_t3_conditions(hw, ch, dgrad):
    fx.check_t3(fx.t3_case(hw, ch, dgrad))
