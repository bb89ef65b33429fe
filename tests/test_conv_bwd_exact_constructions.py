"""The constructions of tests/_conv_bwd_exact.py, checked without a device: every exactness and snap condition of every
case the GPU tests launch (both statistic-replica counts), the float64 references against torch.autograd on float64,
the work lists, the slab map, and the agreement of the hand-built launches with the engine's own arithmetic."""
import pytest
import torch
import torch.nn.functional as F

import _conv_bwd_exact as bx
import _conv_exact as kx

DG_IDS = ["c%d-m%d-e%d-rows%d" % r for r in bx.DG_CASES]
WG_JOBS = [(cc, m) for cc in bx.WIDTHS for m in (0, 2)]


def test_case_tables_cover_every_instantiation():
    want = {(cc, m, 0, 8) for cc in (16, 32, 64) for m in (0, 2, 3)} | {(16, 2, 1, 8)} | {(64, m, 0, 4) for m in (0, 2, 3)}
    assert set(bx.DG_CASES) == want and len(bx.DG_CASES) == 13 and bx.DG_UNTESTED == []
    assert sorted(j for jobs in bx.WG_SETS.values() for j in jobs) == sorted(WG_JOBS)
    assert {m for r in bx.DG_NULL_XOUT for m in (r[1],)} == {2, 3} and all(r in bx.DG_CASES for r in bx.DG_NULL_XOUT)


@pytest.mark.parametrize("nrep", [8, 64])
@pytest.mark.parametrize("uniform", [False, True], ids=["list", "uniform"])
@pytest.mark.parametrize("row", bx.DG_CASES, ids=DG_IDS)
def test_dg_case_conditions(row, uniform, nrep):
    c = bx.dg_case(*row, uniform=uniform, nrep=nrep)
    bx.check_dg(c)
    rep = bx.dg_replica_rows(c)
    assert torch.equal((rep - c.st_seed[:, :, 0]).sum(1), c.st)
    if nrep == 8 and len(c.items) > 1:
        assert bool(((rep - c.st_seed[:, :, 0])[:, 1:] != 0).any()), "some workgroup adds to a replica other than 0"


@pytest.mark.parametrize("nrep", [8, 64])
@pytest.mark.parametrize("uniform", [False, True], ids=["list", "uniform"])
@pytest.mark.parametrize("cc,mode", WG_JOBS)
def test_wg_job_conditions(cc, mode, uniform, nrep):
    bx.check_wg(bx.wg_job(cc, mode, uniform, nrep), 9.0)


@pytest.mark.parametrize("row", [(16, 0, 0, 8), (32, 3, 0, 8), (16, 2, 1, 8), (64, 2, 0, 4)],
                         ids=["c16-m0", "c32-m3", "c16-m2-e1", "c64-m2-rows4"])
def test_dg_reference_matches_autograd(row):
    """dx of the reference = the gradient of sum(conv(x, w) dy) w.r.t. x, w[co][ci][ky][kx] = W_ihwo[ci][ky][kx][co]."""
    c = bx.dg_case(*row)
    for sl, f, e in kx.ranges(c.slots, c.sizes):
        x = torch.zeros(e - f, c.C, c.H, c.H, dtype=torch.float64, requires_grad=True)
        w = c.w[sl].permute(3, 0, 1, 2).contiguous()
        (F.conv2d(x, w, padding=1) * c.dy[f:e].permute(0, 3, 1, 2)).sum().backward()
        dx = x.grad.permute(0, 2, 3, 1)
        if c.epi & 1:
            dx = dx + c.res[f:e]
        assert torch.equal(torch.where(c.ep.snap[f:e] > 0, dx, torch.zeros_like(dx)), c.y[f:e])


@pytest.mark.parametrize("cc,mode", WG_JOBS)
def test_wg_reference_matches_autograd(cc, mode):
    c = bx.wg_job(cc, mode)
    for sl, f, e in kx.ranges(c.slots, c.sizes):
        w = torch.zeros(cc, cc, 3, 3, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(c.ep.xin[f:e].permute(0, 3, 1, 2), w, padding=1)
        (y * c.dy[f:e].permute(0, 3, 1, 2)).sum().backward()
        assert torch.equal(w.grad.permute(0, 2, 3, 1), c.dw[sl])  # [co][ci][ky][kx] -> [co][ky][kx][ci]


@pytest.mark.parametrize("cc", bx.WIDTHS)
def test_slab_map_is_a_bijection(cc):
    valid, idx = bx.slab_index(cc)
    assert valid.numel() == bx.slab_elems(cc)
    assert sorted(idx[valid].tolist()) == list(range(9 * cc * cc))
    ntn = 9 * cc // 16
    assert int((~valid).sum()) == ((ntn + 3) // 4 * 4 - ntn) * (cc // 16) * 64 * 4


def test_reduce_cases():
    k = bx.reduce_case(tuple((c, tuple(m)) for c, m in bx.RED_ALL_CONV), tuple((c, tuple(m)) for c, m in bx.RED_ALL_DENSE))
    bx.check_reduce_case(k)
    counts = sorted(n for _, ms in bx.RED_ALL_CONV for _, n in ms)
    assert counts == [0, 1, 3, 4, 5, 13, 16, 17, 29] and {c for c, _ in bx.RED_ALL_CONV} == {16, 32, 64}
    assert sorted(n for _, ms in bx.RED_ALL_DENSE for _, n in ms) == [1, 8, 9, 25, 32, 33, 57]
    chunks = [bx.slab_elems(c) // 256 for c, _ in bx.RED_ALL_CONV]
    assert min(chunks) < bx.RED_ALL_MAX_BLOCKS < max(chunks)
    assert any(len(ms) < bx.RED_ALL_MAX_MEMBERS for _, ms in bx.RED_ALL_CONV)
    assert max(-(-kel // 32) for kel, _ in bx.RED_ALL_DENSE) > bx.RED_ALL_MAX_BLOCKS
    # the row without slabs keeps its seed
    (cc, ms), job = bx.RED_ALL_CONV[3], k.jobs[3]
    assert ms[1] == (0, 0)
    off = job[4]
    assert torch.equal(k.want[0, off:off + 9 * cc * cc], k.seed[0, off:off + 9 * cc * cc])
    assert torch.equal(k.want[1], k.seed[1])
    assert sorted(n for _, ms in bx.DW_REDUCE for _, n in ms) == [1, 8, 9, 16, 17, 24]
    for cc, ms in bx.DW_REDUCE:
        bx.check_reduce_case(bx.reduce_case(((cc, tuple(ms)),), ()))
    bx.check_reduce_case(bx.reduce_case((), tuple((c, tuple(m)) for c, m in bx.RED_ALL_DENSE)))
    bx.check_reduce_case(bx.reduce_case(((32, ((2, 24), (0, 9))),), ((650, ((0, 9), (2, 25))),), True))


def test_launch_sizes_agree_with_the_engine():
    """The LDS sizes and slab extents of the hand-built launches are the engine's (never smaller)."""
    from distributedtf_amd.engine import hip_resnet as hr
    wp = {16: 34, 32: 18, 64: 10}  # conv.hip wpitch<C>() (DTF_WP64 = 10); the GPU tests read it from the library
    for cc in bx.WIDTHS:
        assert bx.slab_elems(cc) == hr._StepPlan._slab_elems(cc)
        for rows in (8, 4):
            tsz = ((rows + 2) * wp[cc] * hr._cpad(cc) + 8 + 63) // 64 * 64
            assert bx.lds_dg(cc, rows, wp[cc]) == 2304 + 2 * tsz * 2
        tsz = (10 * wp[cc] * hr._cpad(cc) + 8 + 63) // 64 * 64
        assert bx.lds_wg(cc, wp[cc]) == 2304 + 4 * tsz * 2 <= 160 * 1024
