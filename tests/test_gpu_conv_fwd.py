"""The CIFAR forward convolution kernels (ops/csrc/conv.hip ``dtf_conv_fwd_s1``: 11 instantiations, ``dtf_conv_fwd``:
19) launched directly through ctypes and compared BITWISE with the float64 references of tests/_conv_exact.py: the
whole output buffer and the whole statistics buffer inside canary guards, idle member rows included.  No tolerance
anywhere; the conditions that make that legitimate are asserted on the reference before every launch
(``check_case``; without a device in tests/test_conv_exact_constructions.py).

Members sit in slots 0 and 2 of a capacity-3 population with 3 and 2 images; the idle slot's weights, params,
statistics and image count are NaN.  Work lists are hand-built: a single-iteration item, an item that crosses an image
boundary inside, uneven splits, the members' items interleaved.  ``dtf_conv_fwd_s1`` also runs with the arithmetic
work item (``u_items > 0``, members in slots 0 and 1, a chunk that does not divide the member's iterations) while
``work`` points at a table of idle-slot items it must not read."""
import ctypes

import pytest
import torch

import _conv_exact as kx
import _convg_exact as cx

pytestmark = pytest.mark.gpu

S1_IDS = ["c%d-m%d-r%d-rows%d" % r for r in kx.S1_CASES]
GEN_IDS = ["%d-%d-s%d-k%d-m%d-r%d-st%d-%dx%d-rows%d" % r for r in kx.GEN_CASES + kx.GEN_EXTRA]


def _env():
    """(ops, hip_resnet with its launchers registered, device, statistic replicas of the loaded library)."""
    ops, _, dev, _ = cx.gpu_env()
    from distributedtf_amd.engine import hip_resnet as hr
    hr._register()
    assert ops.lib().dtf_conv_args_size() == ctypes.sizeof(hr.ConvArgs)
    return ops, hr, dev, ops.build_nrep()


class _Launch:
    """The device buffers of one case and its ConvArgs."""

    def __init__(self, c, ops, hr, dev, stats=1):
        kx.check_case(c)  # the reference alone, before anything is launched
        dt = ops.act_dtype()
        self.c, self.dt, self.stats = c, dt, stats
        esz = 2
        self.x = kx.guarded(c.x, dt).to(dev)
        self.w = kx.guarded(kx.weight_rows(c), dt).to(dev)
        self.y = kx.guarded(torch.full_like(c.y, kx.CANARY), dt).to(dev)
        self.res = kx.guarded(c.res, dt).to(dev) if c.resid else None
        self.params = kx.guarded(kx.param_rows(c), torch.float32).to(dev)
        self.st_in = kx.guarded(c.st_in, torch.float32).to(dev)
        self.st_out = kx.guarded(c.st_seed, torch.float32).to(dev)
        self.cnt = kx.guarded(c.cnt, torch.float32).to(dev)
        table = kx.poison_work(len(c.items), c.idle) if c.uniform else c.items
        self.work = torch.tensor(table, dtype=torch.int32, device=dev)
        a = hr.ConvArgs()
        a.x, a.y, a.w = (t.data_ptr() + kx.PRE * esz for t in (self.x, self.y, self.w))
        a.res = self.res.data_ptr() + kx.PRE * esz if c.resid else None
        a.params, a.st_in, a.st_out, a.cnt = (t.data_ptr() + kx.PRE * 4 for t in (self.params, self.st_in, self.st_out,
                                                                                  self.cnt))
        a.work = self.work.data_ptr()
        a.w_mstride, a.w_off = kx.weight_rows(c).shape[1], kx.W_OFF
        a.p_mstride, a.in_gamma, a.in_beta = kx.P_MSTRIDE, kx.IN_GAMMA, kx.IN_BETA
        a.Hi, a.Wi, a.Ho, a.Wo, a.rows = c.hi, c.wi, c.ho, c.wo, c.rows
        a.u_items, a.u_chunk, a.u_per = c.u
        self.a = a

    def check(self):
        c = self.c
        torch.cuda.synchronize()
        got = self.y.cpu().double()
        want = kx.guarded(c.y, torch.float64)
        if not torch.equal(got, want):
            bad = (got != want).nonzero().reshape(-1)
            i = int(bad[0]) - kx.PRE  # (negative or past the end: a guard word)
            n, r, col, o = i // (c.ho * c.wo * c.cout), i // (c.wo * c.cout) % c.ho, i // c.cout % c.wo, i % c.cout
            pytest.fail("%d output words differ; first: image %d row %d column %d channel %d: got %r want %r" % (
                bad.numel(), n, r, col, o, float(got[bad[0]]), float(want[bad[0]])))
        shape = c.st_seed.shape
        st = self.st_out.cpu()
        assert kx.guards_intact(st, c.st_seed.numel()), "statistics guards"
        st = kx.live(st, shape)
        seed = c.st_seed.float()
        if not self.stats:
            assert torch.equal(st, seed), "stats = 0: the statistics buffer must stay as it was"
        else:
            assert torch.equal(st[c.idle], seed[c.idle]), "idle slot's statistics row touched"
            assert torch.equal(st[..., c.cout:], seed[..., c.cout:]), "statistics columns past Co touched"
            delta = (st.double() - c.st_seed).sum(1)  # over the replicas: sum, sum of squares per member and channel
            if not torch.equal(delta, c.st):
                bad = (delta != c.st).nonzero()
                s, wh, ch = (int(v) for v in bad[0])
                pytest.fail("%d statistics differ; first: slot %d %s channel %d: got %r want %r" % (
                    bad.shape[0], s, ("sum", "sumsq")[wh], ch, float(delta[s, wh, ch]), float(c.st[s, wh, ch])))
        # the inputs are as they were
        assert torch.equal(self.x.cpu().double(), kx.guarded(c.x, torch.float64))


@pytest.mark.parametrize("work", ["list", "uniform"])
@pytest.mark.parametrize("row", kx.S1_CASES, ids=S1_IDS)
def test_conv_fwd_s1_is_exact(row, work):
    """conv_fwd_s1_kernel<C, mode, resid, rows>: output, both statistics rows of both members, untouched idle rows."""
    ops, hr, dev, nrep = _env()
    cc, mode, resid, rows = row
    c = kx.s1_case(cc, mode, resid, rows, work == "uniform", nrep)
    L = _Launch(c, ops, hr, dev)
    lib = ops.lib()
    lds = kx.lds_s1(c, int(lib.dtf_wpitch(cc)), int(lib.dtf_cpad_fwd(cc)))
    rc = lib.dtf_conv_fwd_s1(ctypes.byref(L.a), cc, mode, resid, rows, len(c.items), lds, ops.stream())
    assert rc == 0, rc
    L.check()


@pytest.mark.parametrize("cc,mode,resid,rows", kx.S1_REJECTS, ids=["rows4-c32", "rows4-mode0", "c48"])
def test_conv_fwd_s1_rejects_unsupported(cc, mode, resid, rows):
    """No instantiation: -1 and nothing launched (output and statistics keep their pre-fill)."""
    ops, hr, dev, nrep = _env()
    c = kx.s1_case(64 if cc == 48 else cc, mode, resid, 8, False, nrep)
    L = _Launch(c, ops, hr, dev)
    L.a.rows = rows
    rc = ops.lib().dtf_conv_fwd_s1(ctypes.byref(L.a), cc, mode, resid, rows, len(c.items), 65536, ops.stream())
    assert rc == -1, rc
    torch.cuda.synchronize()
    assert torch.equal(L.y.cpu().double(), torch.full_like(L.y.cpu().double(), kx.CANARY))
    assert torch.equal(L.st_out.cpu(), kx.guarded(c.st_seed, torch.float32))


@pytest.mark.parametrize("row", kx.GEN_CASES + kx.GEN_EXTRA, ids=GEN_IDS)
def test_conv_fwd_generic_is_exact(row):
    """conv_fwd_kernel<Ci, Co, S, K, mode, resid, stats>: every FWD_CASE row at its production geometry, plus smaller
    and non-square geometries of the 16 -> 32 3x3 / 2 and the 16 -> 16 3x3 rows; stats = 0 leaves st_out alone."""
    ops, hr, dev, nrep = _env()
    c, stats = kx.gen_case(row, nrep)
    assert kx.generic_fits(c)
    L = _Launch(c, ops, hr, dev, stats)
    lds = kx.lds_generic(c, max(hr._cpad(c.cin), hr._cpad_fwd(c.cin)))
    rc = ops.lib().dtf_conv_fwd(ctypes.byref(L.a), c.cin, c.cout, c.s, c.k, c.mode, c.resid, stats, len(c.items), lds,
                                ops.stream())
    assert rc == 0, rc
    L.check()


def test_conv_fwd_generic_rejects_unsupported():
    ops, hr, dev, nrep = _env()
    c, stats = kx.gen_case(kx.GEN_CASES[7], nrep)
    L = _Launch(c, ops, hr, dev)
    cin, cout, s, k, mode, resid, stats = kx.GEN_REJECT
    rc = ops.lib().dtf_conv_fwd(ctypes.byref(L.a), cin, cout, s, k, mode, resid, stats, len(c.items), 65536,
                                ops.stream())
    assert rc == -1, rc
    torch.cuda.synchronize()
    assert torch.equal(L.y.cpu().double(), torch.full_like(L.y.cpu().double(), kx.CANARY))
    assert torch.equal(L.st_out.cpu(), kx.guarded(c.st_seed, torch.float32))
