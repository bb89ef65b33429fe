"""The deferred weight gradients of the CIFAR backward (ops/csrc/conv.hip): ``dtf_conv_wgrad_all`` (the wgrad role
of every deferred layer in one launch per width set) into per-workgroup dW slabs, the one-launch reduction
``dtf_slab_reduce_all`` (conv and dense slab jobs) and ``dtf_dw_slab_reduce``, launched directly through ctypes and
compared BITWISE with the float64 references of tests/_conv_bwd_exact.py: the whole gradient buffer inside canary
guards -- the words before ``g_off``, the words after each layer's block and the idle slot's row carry a seeded
integer pattern and must keep it.  The exactness conditions are asserted on the reference before every launch
(``check_wg``, ``check_reduce_case``; without a device in tests/test_conv_bwd_exact_constructions.py).

The wgrad launches put the jobs of both widths and both dY modes in one launch with interleaved ``map`` rows, each
job with its own work list (hand-listed, or the arithmetic ``u_items`` form over a poison table), its own NaN-filled
slab of exactly n_wg x slab_elems(C) words, a BN+ReLU ``x`` operand and, in mode 2, a BN-backward dY.  The slab
reductions also run on hand-written integer slabs (NaN in the duplicate tiles nt >= NTN) with member slab counts on
both sides of every unrolled-loop boundary, and on full-mantissa slabs inside the summation bound
(n + 8) 2^-24 sum |x_i|, twice with bitwise equal results."""
import ctypes

import pytest
import torch

import _conv_bwd_exact as bx
import _conv_exact as kx
import _convg_exact as cx

pytestmark = pytest.mark.gpu


def _env():
    ops, _, dev, _ = cx.gpu_env()
    from distributedtf_amd.engine import hip_resnet as hr
    hr._register()
    assert ops.lib().dtf_conv_args_size() == ctypes.sizeof(hr.ConvArgs)
    assert ops.lib().dtf_slab_job_size() == ctypes.sizeof(hr.SlabJob)
    assert ops.lib().dtf_dense_job_size() == ctypes.sizeof(hr.DenseJob)
    return ops, hr, dev, ops.build_nrep()


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _struct_array(arr, dev):
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)


def _live_ptr(t):
    return t.data_ptr() + kx.PRE * t.element_size()


def _compare_grads(buf, want, offs_note=""):
    got, exp = buf.cpu().double(), kx.guarded(want, torch.float64)
    if not torch.equal(got, exp):
        bad = (got != exp).nonzero().reshape(-1)
        i = int(bad[0]) - kx.PRE
        pytest.fail("%d gradient words differ; first: slot %d word %d%s: got %r want %r" % (
            bad.numel(), i // want.shape[1], i % want.shape[1], offs_note, float(got[bad[0]]), float(exp[bad[0]])))


class _WgradLaunch:
    """One dtf_conv_wgrad_all launch: the jobs' device buffers, their ConvArgs array, the interleaved map, the
    seeded gradient rows and the expected result."""

    def __init__(self, jobs, ops, hr, dev, slabs=True):
        dt = ops.act_dtype()
        self.jobs, self.dev, self.inputs, self.hold = jobs, dev, [], []
        offs, row = bx.grad_layout([j.C for j in jobs])
        self.offs, self.row = offs, row
        self.seed = bx.grad_seed(row, 5100 + 3 * len(jobs) + jobs[0].C)
        for j in jobs:
            bx.check_wg(j, float(self.seed.max()))  # the reference alone, before anything is launched
        self.want = self.seed.clone()
        for j, off in zip(jobs, offs):
            for sl in j.slots:
                self.want[sl, off:off + 9 * j.C * j.C] += j.dw[sl].reshape(-1)
        self.grads = kx.guarded(self.seed, torch.float32).to(dev)
        args, self.slabs, self.reds = [], [], []
        for j, off in zip(jobs, offs):
            a = hr.ConvArgs()
            x, xm = self._inp(j.dz, dt), self._inp(j.ep.x, dt)
            a.x, a.xm = _live_ptr(x), _live_ptr(xm)
            if j.mode == 2:
                a.x2 = _live_ptr(self._inp(j.h, dt))
            a.params = _live_ptr(self._inp(bx.param_rows(j), torch.float32))
            a.st_in, a.st_in_b = _live_ptr(self._inp(j.st_f, torch.float32)), _live_ptr(self._inp(j.st_b, torch.float32))
            a.st_ep = _live_ptr(self._inp(j.ep.st_in, torch.float32))
            a.cnt = _live_ptr(self._inp(j.ep.cnt, torch.float32))
            table = kx.poison_work(len(j.items), j.idle) if j.uniform else j.items
            work = torch.tensor(table, dtype=torch.int32, device=dev)
            self.hold.append(work)
            a.work = work.data_ptr()
            a.p_mstride, a.in_gamma, a.in_beta, a.ep_gamma, a.ep_beta = kx.P_MSTRIDE, bx.IN_GAMMA, 0, bx.EP_GAMMA, bx.EP_BETA
            a.Hi = a.Wi = a.Ho = a.Wo = j.H
            a.rows, a.n_main, a.cin_real = 8, len(j.items), -1
            a.u_items, a.u_chunk, a.u_per = j.u
            a.grads, a.g_mstride, a.g_off = _live_ptr(self.grads), row, off
            if slabs:
                n = len(j.items) * bx.slab_elems(j.C)  # exactly n_wg x slab_elems(C) words, NaN, inside guards
                slab = kx.guarded(torch.full((n,), bx.NAN, dtype=torch.float64), torch.float32).to(dev)
                self.slabs.append(slab)
                a.slab = _live_ptr(slab)
                self.reds.append(torch.tensor(j.red, dtype=torch.int32, device=dev))
            args.append(a)
        self.args = args
        self.jt = _struct_array((hr.ConvArgs * len(args))(*args), dev)
        self.map = bx.interleaved_map(jobs)
        assert len({(m[0], m[2]) for m in self.map[:len(jobs)]}) == len(jobs), "neighbouring workgroups: different jobs"
        self.mt = torch.tensor(self.map, dtype=torch.int32, device=dev)

    def _inp(self, t, dt):
        host = kx.guarded(t, dt)
        buf = host.to(self.dev)
        self.inputs.append((host, buf))
        return buf

    def launch(self, ops, cset):
        lib = ops.lib()
        lds = max(bx.lds_wg(j.C, int(lib.dtf_wpitch(j.C))) for j in self.jobs)
        rc = lib.dtf_conv_wgrad_all(self.jt.data_ptr(), self.mt.data_ptr(), len(self.map), cset, lds, ops.stream())
        assert rc == 0, rc

    def reduce(self, ops, hr):
        sj = (hr.SlabJob * len(self.jobs))()
        for i, (j, off) in enumerate(zip(self.jobs, self.offs)):
            sj[i] = hr.SlabJob(_live_ptr(self.slabs[i]), self.reds[i].data_ptr(), off, len(j.red), j.C)
        st = _struct_array(sj, self.dev)
        self.hold.append(st)
        nb = max(bx.slab_elems(j.C) // 256 for j in self.jobs)
        rc = ops.lib().dtf_slab_reduce_all(st.data_ptr(), len(self.jobs), None, 0, max(len(j.red) for j in self.jobs),
                                           nb, _live_ptr(self.grads), self.row, ops.stream())
        assert rc == 0, rc

    def check(self):
        torch.cuda.synchronize()
        _compare_grads(self.grads, self.want)
        for slab, j in zip(self.slabs, self.jobs):
            assert kx.guards_intact(slab.cpu(), len(j.items) * bx.slab_elems(j.C)), "slab guards"
        for host, buf in self.inputs:
            assert torch.equal(_bits(buf.cpu()), _bits(host)), "an input buffer was written"


@pytest.mark.parametrize("work", ["list", "uniform"])
@pytest.mark.parametrize("cset", [0, 1])
def test_wgrad_all_slabs_reduce_to_exact_dw(cset, work):
    """conv_wgrad_all_kernel<64, 32> / <16, 16>: every job of the set in one launch, then one slab_reduce_all."""
    ops, hr, dev, nrep = _env()
    jobs = [bx.wg_job(cc, mode, work == "uniform", nrep) for cc, mode in bx.WG_SETS[cset]]
    L = _WgradLaunch(jobs, ops, hr, dev)
    L.launch(ops, cset)
    torch.cuda.synchronize()
    _compare_grads(L.grads, L.seed)  # the wgrad launch itself writes slabs only
    L.reduce(ops, hr)
    L.check()


@pytest.mark.parametrize("cc", bx.WIDTHS)
def test_wgrad_all_atomic_flush_is_exact(cc):
    """slab = NULL: the accumulators are flushed into the gradient rows with atomics; the same dW."""
    ops, hr, dev, nrep = _env()
    jobs = [bx.wg_job(cc, mode, False, nrep) for mode in (2, 0)]
    L = _WgradLaunch(jobs, ops, hr, dev, slabs=False)
    L.launch(ops, 1 if cc == 16 else 0)
    L.check()


# ------------------------------------------------------------------------------------ the reductions on their own
class _Reduce:
    """Device buffers of a bx.reduce_case."""

    def __init__(self, k, hr, dev):
        bx.check_reduce_case(k)
        self.k, self.dev, self.hr = k, dev, hr
        self.slabs = [kx.guarded(slab, torch.float32).to(dev) for _, _, slab, _, _ in k.jobs]
        self.reds = [torch.tensor(red, dtype=torch.int32, device=dev) for _, _, _, red, _ in k.jobs]
        conv = [i for i, j in enumerate(k.jobs) if j[0] == "conv"]
        dense = [i for i, j in enumerate(k.jobs) if j[0] == "dense"]
        hr_ = hr
        sj, dj = (hr_.SlabJob * max(1, len(conv)))(), (hr_.DenseJob * max(1, len(dense)))()
        for n, i in enumerate(conv):
            _, cc, _, red, off = k.jobs[i]
            sj[n] = hr_.SlabJob(_live_ptr(self.slabs[i]), self.reds[i].data_ptr(), off, len(red), cc)
        for n, i in enumerate(dense):
            _, kel, _, red, off = k.jobs[i]
            dj[n] = hr_.DenseJob(_live_ptr(self.slabs[i]), self.reds[i].data_ptr(), off, kel, len(red))
        self.nsj, self.ndj = len(conv), len(dense)
        self.st, self.dt = _struct_array(sj, dev), _struct_array(dj, dev)

    def fresh_grads(self):
        return kx.guarded(self.k.seed, torch.float32).to(self.dev)

    def reduce_all(self, ops, grads, max_members, max_blocks):
        rc = ops.lib().dtf_slab_reduce_all(self.st.data_ptr() if self.nsj else None, self.nsj,
                                           self.dt.data_ptr() if self.ndj else None, self.ndj, max_members, max_blocks,
                                           _live_ptr(grads), self.k.row, ops.stream())
        assert rc == 0, rc

    def dw_reduce(self, ops, grads, c=None):
        _, cc, _, red, off = self.k.jobs[0]
        return ops.lib().dtf_dw_slab_reduce(_live_ptr(self.slabs[0]), self.reds[0].data_ptr(), len(red),
                                            _live_ptr(grads), self.k.row, off, c or cc, ops.stream())

    def inputs_intact(self):
        for buf, (_, _, slab, _, _) in zip(self.slabs, self.k.jobs):
            assert torch.equal(_bits(buf.cpu()), _bits(kx.guarded(slab, torch.float32))), "a slab was written"


def _t(cases):
    return tuple((c, tuple(m)) for c, m in cases)


def test_slab_reduce_all_conv_and_dense_jobs():
    """Widths 16, 32, 64 and the dense jobs in one launch: slab counts around every unrolled-loop bound, a row without
    slabs, a job with fewer rows than max_members, max_blocks between the narrowest and the widest chunk count."""
    ops, hr, dev, _ = _env()
    k = bx.reduce_case(_t(bx.RED_ALL_CONV), _t(bx.RED_ALL_DENSE))
    R = _Reduce(k, hr, dev)
    g = R.fresh_grads()
    R.reduce_all(ops, g, bx.RED_ALL_MAX_MEMBERS, bx.RED_ALL_MAX_BLOCKS)
    torch.cuda.synchronize()
    _compare_grads(g, k.want)
    R.inputs_intact()


def test_slab_reduce_all_dense_jobs_only():
    """nsj = 0: every z is a dense job."""
    ops, hr, dev, _ = _env()
    k = bx.reduce_case((), _t(bx.RED_ALL_DENSE))
    R = _Reduce(k, hr, dev)
    g = R.fresh_grads()
    R.reduce_all(ops, g, bx.RED_ALL_MAX_MEMBERS, bx.RED_ALL_MAX_BLOCKS)
    torch.cuda.synchronize()
    _compare_grads(g, k.want)
    R.inputs_intact()


@pytest.mark.parametrize("cc,members", bx.DW_REDUCE, ids=["c16", "c32", "c64"])
def test_dw_slab_reduce_is_exact(cc, members):
    ops, hr, dev, _ = _env()
    k = bx.reduce_case(((cc, tuple(members)),), ())
    R = _Reduce(k, hr, dev)
    g = R.fresh_grads()
    assert R.dw_reduce(ops, g) == 0
    torch.cuda.synchronize()
    _compare_grads(g, k.want)
    R.inputs_intact()


def test_dw_slab_reduce_rejects_c48():
    ops, hr, dev, _ = _env()
    k = bx.reduce_case(((32, tuple(bx.DW_REDUCE[1][1])),), ())
    R = _Reduce(k, hr, dev)
    g = R.fresh_grads()
    assert R.dw_reduce(ops, g, c=48) == -1
    torch.cuda.synchronize()
    _compare_grads(g, k.seed)


@pytest.mark.parametrize("kernel", ["slab_reduce_all", "dw_slab_reduce"])
def test_slab_reductions_full_mantissa(kernel):
    """Full-mantissa fp32 slab words: inside (n + 8) 2^-24 sum |x_i| of float64 per element (n slabs, the seed and the
    partial sums' adds), and bitwise the same when repeated into a fresh buffer (the summation order is fixed)."""
    ops, hr, dev, _ = _env()
    conv, dense = ((32, ((2, 24), (0, 9))),), ((650, ((0, 9), (2, 25))),)
    k = bx.reduce_case(conv, dense if kernel == "slab_reduce_all" else (), True)
    R = _Reduce(k, hr, dev)
    out = []
    for _ in range(2):
        g = R.fresh_grads()
        if kernel == "slab_reduce_all":
            R.reduce_all(ops, g, 2, 16)
        else:
            assert R.dw_reduce(ops, g) == 0
        torch.cuda.synchronize()
        out.append(g.cpu())
    assert torch.equal(_bits(out[0]), _bits(out[1])), "two launches over the same slabs differ"
    assert kx.guards_intact(out[0], k.seed.numel())
    got = kx.live(out[0], k.seed.shape).double()
    bound = (k.nslab + 8) * 2.0 ** -24 * k.mag
    err = (got - k.want).abs()
    print("%s full mantissa: largest error / bound %.3f" % (kernel, float((err / bound).max())))
    assert bool((err <= bound).all()), float((err / bound).max())
    assert bool((err > 0).any()), "the case is not exact: the bound is what is tested"
    R.inputs_intact()
