"""The constructions of tests/_conv_exact.py, without a device: every case tests/test_gpu_conv_fwd.py launches
satisfies the exactness and snap conditions that make a bitwise comparison legitimate (for the 8 statistic replicas
of the release and half builds and the 64 of the deterministic one), the work lists have the edges they are meant to
have, the host mirror of the arithmetic work item tiles every iteration once, and the float64 reference is the plain
convolution -- so a GPU mismatch cannot be blamed on the reference."""
import pytest
import torch
import torch.nn.functional as F

import _conv_exact as kx

S1_IDS = ["c%d-m%d-r%d-rows%d-%s" % (r + (u,)) for r in kx.S1_CASES for u in ("list", "uniform")]
GEN_IDS = ["%d-%d-s%d-k%d-m%d-r%d-st%d-%dx%d-rows%d" % r for r in kx.GEN_CASES + kx.GEN_EXTRA]


@pytest.mark.parametrize("nrep", [8, 64])
@pytest.mark.parametrize("row,uniform", [(r, u) for r in kx.S1_CASES for u in (False, True)], ids=S1_IDS)
def test_s1_case_conditions(row, uniform, nrep):
    c = kx.s1_case(*row, uniform=uniform, nrep=nrep)
    kx.check_case(c)
    assert c.bands == (512 // row[0]) // row[3] and c.hi == c.wi == 512 // row[0]


@pytest.mark.parametrize("nrep", [8, 64])
@pytest.mark.parametrize("row", kx.GEN_CASES + kx.GEN_EXTRA, ids=GEN_IDS)
def test_generic_case_conditions(row, nrep):
    c, stats = kx.gen_case(row, nrep)
    kx.check_case(c)
    assert kx.generic_fits(c), "outside the launch limits hip_resnet._conv_fwd keeps"


def test_case_tables_cover_the_instantiations():
    assert len(kx.S1_CASES) == 11 and len(set(kx.S1_CASES)) == 11
    assert len(kx.GEN_CASES) == 19 and len({r[:7] for r in kx.GEN_CASES}) == 19
    assert {c.bands for c in (kx.s1_case(*r, uniform=False) for r in kx.S1_CASES)} == {1, 2, 4}
    assert kx.GEN_REJECT not in {r[:7] for r in kx.GEN_CASES}
    for r in kx.GEN_EXTRA:
        assert r[:7] in {g[:7] for g in kx.GEN_CASES} and r[9] != 8
    assert any(r[7] != r[8] for r in kx.GEN_EXTRA if r[:4] == (16, 32, 2, 3))
    assert any(r[7] != r[8] for r in kx.GEN_EXTRA if r[:4] == (16, 16, 1, 3))
    assert any(r[7] == r[8] == 16 for r in kx.GEN_EXTRA if r[:4] == (16, 32, 2, 3))
    assert any(r[7] == r[8] == 16 for r in kx.GEN_EXTRA if r[:4] == (16, 16, 1, 3))


def test_uniform_work_item_mirror_tiles_every_iteration_once():
    """work_item_at (u_items > 0): for every per-member total and every chunk, the items of n packed members cover
    iterations 0 .. n * per - 1 exactly once, never cross a member, and the last item of a member is the short one."""
    for per in range(1, 30):
        for chunk in range(1, per + 2):
            ui, uc, up = kx.uniform_geo(per, chunk)
            for n in (1, 2, 3):
                items = [kx.work_item_at(b, ui, uc, up) for b in range(ui * n)]
                seen = []
                for it0, nit, z, m in items:
                    assert nit >= 1 and z == 0 and m * per <= it0 and it0 + nit <= (m + 1) * per
                    seen += list(range(it0, it0 + nit))
                assert seen == list(range(n * per))
                assert items[ui - 1][1] == per - (ui - 1) * chunk
    for r in kx.S1_CASES:
        c = kx.s1_case(*r, uniform=True)
        assert c.items[c.u[0] - 1][1] < c.u[1], "the last item of a member is short"
        assert kx.poison_work(len(c.items), c.idle)[0] == [0, 1, 0, c.idle] and c.idle == 2


def test_listed_work_lists_have_their_edges():
    for bands in (1, 2, 4, 8):
        items = kx.listed_items(*kx.LISTED, bands)
        kx.assert_tiling(items, *kx.LISTED, bands)
        cov = kx.items_coverage(items, bands)
        assert all(cov[k] for k in kx.ITEMS_NEED), (bands, cov)
        if bands > 1:  # the crossing item starts and ends inside an image
            assert any(it0 % bands and (it0 + nit) % bands and it0 // bands != (it0 + nit - 1) // bands
                       for it0, nit, _, _ in items)


def _plain_conv(c):
    """The convolution written out: loops over image, output pixel and tap, the weight row indexed as the kernel
    flattens it (k = (ky * K + kx) * Ci + ci), zero padding by the bounds test."""
    y = torch.zeros_like(c.y)
    for sl, f, e in kx.ranges(c.slots, c.sizes):
        wrow = c.w[sl].reshape(c.cout, c.k * c.k * c.cin)
        for n in range(f, e):
            for oy in range(c.ho):
                for ox in range(c.wo):
                    acc = torch.zeros(c.cout, dtype=torch.float64)
                    for ky in range(c.k):
                        for kx_ in range(c.k):
                            iy, ix = oy * c.s - c.pad + ky, ox * c.s - c.pad + kx_
                            if 0 <= iy < c.hi and 0 <= ix < c.wi:
                                k0 = (ky * c.k + kx_) * c.cin
                                acc += wrow[:, k0:k0 + c.cin] @ c.xin[n, iy, ix]
                    y[n, oy, ox] = acc + (c.res[n, oy, ox] if c.resid else 0)
    return y


@pytest.mark.parametrize("row", [(16, 32, 2, 3, 1, 0, 1, 32, 16, 4), (16, 16, 1, 3, 1, 1, 1, 16, 16, 4)], ids=GEN_IDS[-3:-1])
def test_reference_is_the_plain_convolution(row):
    c, _ = kx.gen_case(row)
    assert row in kx.GEN_EXTRA
    assert torch.equal(_plain_conv(c), c.y)
    # and F.conv2d on the whole packed batch with one member's weights agrees on that member's images
    for sl, f, e in kx.ranges(c.slots, c.sizes):
        y = F.conv2d(c.xin.permute(0, 3, 1, 2), c.w[sl].permute(0, 3, 1, 2), stride=c.s, padding=c.pad).permute(0, 2, 3, 1)
        assert torch.equal(y[f:e] + (c.res[f:e] if c.resid else 0), c.y[f:e])
        assert torch.equal(c.st[sl, 0, :c.cout], c.y[f:e].sum((0, 1, 2)))
        assert torch.equal(c.st[sl, 1, :c.cout], (c.y[f:e] ** 2).sum((0, 1, 2)))
    assert bool((c.st[c.idle] == 0).all()) and bool((c.st[:, :, c.cout:] == 0).all())


def test_buffer_layouts():
    c, _ = kx.gen_case(kx.GEN_CASES[7])
    w = kx.weight_rows(c)
    n = c.cout * c.k * c.k * c.cin
    assert w.shape == (kx.CAP, kx.W_OFF + n + kx.W_TAIL) and w.shape[1] % 8 == 0 and kx.W_OFF % 8 == 0
    assert bool(torch.isnan(w[:, :kx.W_OFF]).all()) and bool(torch.isnan(w[:, kx.W_OFF + n:]).all())
    assert bool(torch.isnan(w[c.idle]).all()) and torch.equal(w[0, kx.W_OFF:kx.W_OFF + n], c.w[0].reshape(-1))
    p = kx.param_rows(c)
    assert kx.IN_GAMMA > 0 and kx.IN_BETA >= kx.IN_GAMMA + 64 and kx.P_MSTRIDE >= kx.IN_BETA + 64
    assert torch.equal(p[2, kx.IN_BETA:kx.IN_BETA + c.cin], c.beta[2]) and int(torch.isnan(p[0]).sum()) == 400 - 2 * c.cin
    g = kx.guarded(c.y, torch.bfloat16)
    assert g.numel() == c.y.numel() + 2 * kx.PRE and kx.guards_intact(g, c.y.numel())
    assert torch.equal(kx.live(g, c.y.shape).double(), c.y)
    assert not bool((c.y == kx.CANARY).any()) and (kx.PRE * 2) % 16 == 0
    for dt in (torch.bfloat16, torch.float16):
        assert float(torch.tensor(kx.CANARY).to(dt)) == kx.CANARY
