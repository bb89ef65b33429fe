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


# ------------------------------------------------------------------------------------------- the fused launch
FUSED_IDS = ["c%d-m%d-e%d" % r for r in bx.FUSED_CASES]


def test_fused_table_is_the_launchers():
    """FUSED_CASES = the FUSED_CASE(...) lines of dtf_conv_bwd_fused, in order; nothing untested without a reason."""
    import os
    import re
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "distributedtf_amd", "ops", "csrc", "conv.hip")
    with open(src) as f:
        rows = [tuple(int(v) for v in m) for m in re.findall(r"^\s*FUSED_CASE\((\d+), (\d+), (\d+)\)", f.read(), re.M)]
    assert len(rows) == 16 and bx.FUSED_CASES == rows
    assert {r for r, _ in bx.FUSED_UNTESTED} <= set(rows) and all(reason for _, reason in bx.FUSED_UNTESTED)
    assert bx.FUSED_UNTESTED == []
    assert {r[1] for r in bx.FUSED_NULL_XOUT} == {2, 3} and all(r in rows for r in bx.FUSED_NULL_XOUT)
    assert not any(r in rows for r in bx.FUSED_REJECTS)


@pytest.mark.parametrize("nrep", [8, 64])
@pytest.mark.parametrize("uniform", [False, True], ids=["list", "uniform"])
@pytest.mark.parametrize("row", bx.FUSED_CASES, ids=FUSED_IDS)
def test_fused_case_conditions(row, uniform, nrep):
    c = bx.fused_case(*row, uniform=uniform, nrep=nrep)
    bx.check_fused(c)
    rep = bx.dg_replica_rows(c)
    assert torch.equal((rep - c.st_seed[:, :, 0]).sum(1), c.st)
    if nrep == 8:
        assert bool(((rep - c.st_seed[:, :, 0])[:, 1:] != 0).any()), "some workgroup adds to a replica other than 0"
    if c.epi & 2:
        assert c.ep.st_in is None and bool(torch.isnan(bx.param_rows(c)[:, bx.EP_GAMMA:bx.EP_GAMMA + c.C]).all()) == (
            not c.epi & 8)
    # the hand-listed slab table: a member's workgroups are contiguous, slot 2 first
    if not uniform:
        assert [r[3] for r in c.red] == [2, 0] and c.red[0][0] == 0 and c.red[1][0] == c.red[0][1]


@pytest.mark.parametrize("key", sorted(bx.FUSED_SALT), ids=lambda k: "c%d-m%d-e%d-%s" % (k[:3] + ("uniform" if k[3] else "list",)))
def test_fused_seed_offsets_are_the_first_that_pass(key, monkeypatch):
    """FUSED_SALT's rule: a listed set has statistics, and every smaller offset fails check_fused at one of the replica
    counts (the listed offset itself is checked by test_fused_case_conditions)."""
    cc, mode, epi, uniform = key
    assert (cc, mode, epi) in bx.FUSED_CASES and bx.fused_has_stats(epi) and bx.FUSED_SALT[key] > 0
    for k in range(bx.FUSED_SALT[key]):
        monkeypatch.setitem(bx.FUSED_SALT, key, k)
        ok = True
        for nrep in (8, 64):
            try:
                bx.check_fused(bx.fused_case.__wrapped__(cc, mode, epi, uniform=uniform, nrep=nrep))
            except AssertionError:
                ok = False
                break
        assert not ok, "offset %d already meets every condition" % k


@pytest.mark.parametrize("row", bx.FUSED_CASES, ids=FUSED_IDS)
def test_fused_references_match_autograd(row):
    """y and dW of one operand set = the gradients of sum(conv2d(xin, W) T(dy)) w.r.t. xin (masked, + res) and W, with
    xin = relu(BN_x(x)) or relu(x) and W[co][ci][ky][kx] = W_ihwo[ci][ky][kx][co]."""
    c = bx.fused_case(*row)
    for sl, f, e in kx.ranges(c.slots, c.sizes):
        x = c.ep.xin[f:e].permute(0, 3, 1, 2).clone().requires_grad_(True)
        w = c.w[sl].permute(3, 0, 1, 2).clone().requires_grad_(True)
        (F.conv2d(x, w, padding=1) * c.dy[f:e].permute(0, 3, 1, 2)).sum().backward()
        dx = x.grad.permute(0, 2, 3, 1)
        if c.epi & 1:
            dx = dx + c.res[f:e]
        mask = (c.ep.x[f:e] > 0) if c.epi & 2 else (c.ep.snap[f:e] > 0)
        assert torch.equal(torch.where(mask, dx, torch.zeros_like(dx)), c.y[f:e])
        assert torch.equal(w.grad.permute(0, 2, 3, 1), c.dw[sl])  # [co][ci][ky][kx] -> [co][ky][kx][ci]


@pytest.mark.parametrize("cc", bx.WIDTHS)
def test_fused_chain_xhat_row_matches_direct_evaluation(cc):
    """EPI & 8: row 1 = sum(dz (x3 inv - mean inv)) with the chained BN's statistics, all replicas and seeds summed."""
    c = bx.fused_case(cc, 2, 11)
    val, mag = bx.fused_xhat(c, torch.float64)
    assert c.x3 is c.chain.x
    for s, f, e in kx.ranges(c.slots, c.sizes):
        n = (e - f) * c.H * c.H
        w = c.chain.st_in[s].double()[:, :, :cc].sum(0)
        mean = w[0] / n
        var = (w[1] / n - mean * mean).clamp(min=0.0)
        assert bool((w[1] / n - mean * mean < 0).any()), "the clamp runs"
        inv = 1.0 / torch.sqrt(var + float(torch.tensor(kx.BN_EPS, dtype=torch.float32)))
        direct = (c.y[f:e] * (c.x3[f:e] - mean) * inv).sum((0, 1, 2)) + c.st_seed[s, :, 1, :cc].sum(0)
        assert bool(((direct - val[s, :cc]).abs() <= 1e-12 * mag[s, :cc]).all())
        assert bool((direct != c.st_seed[s, :, 1, :cc].sum(0)).any())
    # and it is not the mask input's x-hat
    assert not torch.equal(c.chain.st_in[c.slots[0]], torch.zeros_like(c.chain.st_in[c.slots[0]]))


def test_fused_trailing_tables():
    counts = sorted(n for _, _, ms, _ in bx.FUSED_TRAIL for _, n in ms)
    assert set(counts) == {0, 1, 8, 9, 16, 17, 24, 25}
    pairs = {(cc, rc) for cc, rc, _, _ in bx.FUSED_TRAIL}
    assert {(16, 16), (32, 16), (16, 32)} <= pairs and any(rc == 64 for _, rc in pairs)
    plan = [nb == bx.slab_elems(rc) // 32 for _, rc, _, nb in bx.FUSED_TRAIL]
    assert any(plan) and not all(plan)
    for cc, rc, ms, nb in bx.FUSED_TRAIL + [bx.FUSED_TRAIL_FULL]:
        assert (bx.slab_elems(rc) // 32) % nb != 0 or nb == bx.slab_elems(rc) // 32
        k = bx.trail_case(cc, rc, tuple(ms), nb, (cc, rc, ms, nb) == bx.FUSED_TRAIL_FULL)
        bx.check_reduce_case(k)
        assert k.r_goff != k.g_off and k.r_goff + 9 * rc * rc + bx.G_GAP == k.row
        blk = slice(k.g_off, k.g_off + 9 * cc * cc)
        assert torch.equal(k.want[:, blk], k.seed[:, blk]), "the launch's own block is not the trailing reduction's"
        assert torch.equal(k.want[1], k.seed[1])
        for _, n, _, slot in k.red:
            if n == 0:
                assert torch.equal(k.want[slot], k.seed[slot])


def test_fused_launch_sizes_agree_with_the_engine():
    from distributedtf_amd.engine import hip_resnet as hr
    wp = {16: 34, 32: 18, 64: 10}  # conv.hip wpitch<C>(); the GPU tests read it from the library
    for cc in bx.WIDTHS:
        tsz = (10 * wp[cc] * hr._cpad(cc) + 8 + 63) // 64 * 64
        want = 2304 + (4 * tsz + (2 * 8 * (512 // cc) * hr._cpad(cc) if cc >= 64 else 0)) * 2
        assert bx.lds_fused(cc, wp[cc], 0) == want <= 160 * 1024
        assert bx.lds_fused(cc, wp[cc], 1) == want + (16 * (32 * 5 + 8) * 2 if cc == 16 else 0) <= 160 * 1024
