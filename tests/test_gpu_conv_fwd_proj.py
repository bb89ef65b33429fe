"""The projection shortcut computed inside conv_a's forward launch (ops/csrc/conv.hip: ``ConvArgs.y2`` / ``w2_off``, the
PROJ instantiations of ``conv_fwd_s1_kernel<16, 1, false, 8>`` and ``conv_fwd_kernel<16, 32, 2, 3, 1, false, true>`` /
``<32, 64, ...>``), launched directly through ctypes and compared BITWISE with float64 references: conv_a's output
and statistics against tests/_conv_exact.py's reference (the launch of tests/test_gpu_conv_fwd.py, with a second
weight block in the row), the projection output against a float64 1x1 conv of the same staged input
(tests/_conv_fwd_proj_exact.py).  Every buffer sits inside guard words, ``y2`` included; the idle slot is NaN.

Controls: the same launch with ``y2 = null`` leaves the y2 buffer's pre-fill alone and gives the same output and
statistics words; ``y2`` on a shape without a PROJ instantiation returns -1 and launches nothing.

The exactness conditions of the second output are asserted on the reference alone, without a device
(``test_proj_constructions``)."""
import ctypes

import pytest
import torch

import _conv_exact as kx
import _conv_fwd_proj_exact as px
import test_gpu_conv_fwd as base

gpu = pytest.mark.gpu


class _ProjLaunch(base._Launch):
    """The launch of test_gpu_conv_fwd with both weight blocks in the member rows and a guarded y2 buffer."""

    def __init__(self, p, ops, hr, dev, with_y2=True):
        px.check_proj(p)  # the reference alone, before anything is launched
        super().__init__(p.c, ops, hr, dev)
        self.p = p
        rows = px.weight_rows(p)
        self.w = kx.guarded(rows, self.dt).to(dev)
        self.y2 = kx.guarded(torch.full_like(p.y2, kx.CANARY), self.dt).to(dev)
        self.a.w = self.w.data_ptr() + kx.PRE * 2
        self.a.w_mstride = rows.shape[1]
        self.a.w2_off = p.w2_off
        self.a.y2 = self.y2.data_ptr() + kx.PRE * 2 if with_y2 else None

    def check_y2(self, written=True):
        p = self.p
        torch.cuda.synchronize()
        got = self.y2.cpu().double()
        want = kx.guarded(p.y2 if written else torch.full_like(p.y2, kx.CANARY), torch.float64)
        if not torch.equal(got, want):
            c = p.c
            bad = (got != want).nonzero().reshape(-1)
            i = int(bad[0]) - kx.PRE  # (negative or past the end: a guard word)
            n, r, col, o = i // (c.ho * c.wo * c.cout), i // (c.wo * c.cout) % c.ho, i // c.cout % c.wo, i % c.cout
            pytest.fail("%d projection words differ; first: image %d row %d column %d channel %d: got %r want %r" % (
                bad.numel(), n, r, col, o, float(got[bad[0]]), float(want[bad[0]])))


def _s1(L, lib, ops):
    c = L.c
    lds = kx.lds_s1(c, int(lib.dtf_wpitch(c.cin)), int(lib.dtf_cpad_fwd(c.cin)))
    return lib.dtf_conv_fwd_s1(ctypes.byref(L.a), c.cin, 1, 0, c.rows, len(c.items), lds, ops.stream())


def _gen(L, lib, ops, hr):
    c = L.c
    assert kx.generic_fits(c)
    lds = kx.lds_generic(c, max(hr._cpad(c.cin), hr._cpad_fwd(c.cin)))
    return lib.dtf_conv_fwd(ctypes.byref(L.a), c.cin, c.cout, c.s, 3, 1, 0, 1, len(c.items), lds, ops.stream())


def test_proj_constructions():
    """No device: the conv_a cases pass _conv_exact's conditions at the new geometries, the projection references pass
    theirs, and the generic geometry is the band rule's own."""
    for ci, co, hi, rows in px.GEN_PROJ:
        assert px.band_rule_rows(hi, 2, 3, ci) == rows
        assert px.band_rule_rows(hi // 2, 2, 3, ci) is None  # nothing smaller: Ho = 2 has no whole 16-pixel tile
    for nrep in (8, 64):
        for p in px.all_cases(nrep):
            kx.check_case(p.c)
            px.check_proj(p)
            if p.c.s == 2:
                assert kx.generic_fits(p.c)


@gpu
@pytest.mark.parametrize("cc,uniform", px.S1_PROJ, ids=["list", "uniform"])
@pytest.mark.parametrize("with_y2", [True, False], ids=["y2", "null"])
def test_conv_fwd_s1_proj_is_exact(cc, uniform, with_y2):
    """conv_fwd_s1_kernel<16, 1, false, 8, PROJ>: h, its statistics and the projection output; y2 = null: the
    non-PROJ instantiation, the y2 buffer untouched."""
    ops, hr, dev, nrep = base._env()
    L = _ProjLaunch(px.proj_case(cc, cc, 1, 512 // cc, 8, uniform, nrep), ops, hr, dev, with_y2)
    rc = _s1(L, ops.lib(), ops)
    assert rc == 0, rc
    L.check()
    L.check_y2(written=with_y2)


@gpu
@pytest.mark.parametrize("ci,co,hi,rows", px.GEN_PROJ, ids=["16-32", "32-64"])
@pytest.mark.parametrize("with_y2", [True, False], ids=["y2", "null"])
def test_conv_fwd_generic_proj_is_exact(ci, co, hi, rows, with_y2):
    """conv_fwd_kernel<Ci, Co, 2, 3, 1, false, true, PROJ> at the smallest geometry of the band rule."""
    ops, hr, dev, nrep = base._env()
    L = _ProjLaunch(px.proj_case(ci, co, 2, hi, rows, False, nrep), ops, hr, dev, with_y2)
    rc = _gen(L, ops.lib(), ops, hr)
    assert rc == 0, rc
    L.check()
    L.check_y2(written=with_y2)


def _untouched(L):
    torch.cuda.synchronize()
    assert torch.equal(L.y.cpu().double(), torch.full_like(L.y.cpu().double(), kx.CANARY))
    assert torch.equal(L.st_out.cpu(), kx.guarded(L.c.st_seed, torch.float32))
    L.check_y2(written=False)


@gpu
def test_conv_fwd_proj_rejects_unsupported():
    """y2 on a shape without a PROJ instantiation: -1 from both launchers, nothing launched."""
    ops, hr, dev, nrep = base._env()
    lib = ops.lib()
    cc, mode, resid, rows = px.S1_REJECT
    L = _ProjLaunch(px.proj_case(cc, cc, 1, 512 // cc, rows, False, nrep), ops, hr, dev)
    lds = kx.lds_s1(L.c, int(lib.dtf_wpitch(cc)), int(lib.dtf_cpad_fwd(cc)))
    rc = lib.dtf_conv_fwd_s1(ctypes.byref(L.a), cc, mode, resid, rows, len(L.c.items), lds, ops.stream())
    assert rc == -1, rc
    _untouched(L)
    cin, cout, s, k, mode, resid, stats = px.GEN_REJECT
    L = _ProjLaunch(px.proj_case(cin, cout, s, 512 // cin, 8, False, nrep), ops, hr, dev)
    lds = kx.lds_generic(L.c, max(hr._cpad(cin), hr._cpad_fwd(cin)))
    rc = lib.dtf_conv_fwd(ctypes.byref(L.a), cin, cout, s, k, mode, resid, stats, len(L.c.items), lds, ops.stream())
    assert rc == -1, rc
    _untouched(L)
