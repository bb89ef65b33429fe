"""Kernel-level tests of the CIFAR auxiliary kernels (ops/csrc/resnet_aux.hip): every launcher called directly
through ctypes and compared with the float64 references of tests/_resnet_aux_exact.py.

Bitwise: prep_input, weight_prep (both layouts, the folded zeroing), work_gen (whole int4 tables and ``red``),
bn_eval_stats, the gradient half of bn_running_update / bn_step_end, the sum(d) rows of bn_bwd_reduce (and the
per-image slab row 0 on the deterministic build), the head's ``correct`` counts, its v1 logits, every buffer a mode
does not write, and the v1 form of head_bwd_apply.  Against float64 within 4 x (rsqrtf kernels) / 8 x (the head:
__expf / __logf) the scaled deviation of a float32 CPU evaluation of the same formula, both figures printed:
bn_bwd_apply, bn_add_relu, the xhat rows of bn_bwd_reduce, the moving statistics, the head and head_bwd_apply.

Members sit in slots 0 and 2 of a capacity-3 population with ragged image counts; the idle slot's params,
statistics and ``cnt`` are NaN; every output lies inside canary guards and is compared whole; inputs are checked
unchanged; the conditions behind every comparison are asserted on the reference before the launch."""
import ctypes

import pytest
import torch

import _convg_exact as cx
import _resnet_aux_exact as rx

pytestmark = pytest.mark.gpu
PRE = rx.PRE
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _env():
    """(ops, hip_resnet with its launchers registered, device, statistic replicas, deterministic build?); the four
    argument-struct sizes are asserted before anything is launched."""
    ops, _, dev, _ = cx.gpu_env()
    from distributedtf_amd.engine import hip_resnet as hr
    hr._register()
    L = ops.lib()
    assert L.dtf_bnbwd_args_size() == ctypes.sizeof(hr.BnBwdArgs)
    assert L.dtf_bnew_args_size() == ctypes.sizeof(hr.BnEwArgs)
    assert L.dtf_head_args_size() == ctypes.sizeof(hr.HeadArgs)
    assert L.dtf_workgen_desc_size() == ctypes.sizeof(hr.WorkGenDesc)
    return ops, hr, dev, ops.build_nrep(), ops.build_deterministic()


def test_argument_struct_sizes():
    ops, hr, dev, nrep, det = _env()
    assert nrep == (64 if det else 8)


def bits(t):
    return t.contiguous().view(_BITS[t.element_size()])


def same(a, b):
    """Bitwise equality (NaN words included)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


class Bufs:
    """Device buffers of one launch: inputs (checked unchanged afterwards) and outputs, all inside guards."""

    def __init__(self, dev):
        self.dev, self.ins = dev, []

    def inp(self, t, dt):
        if t is None:
            return None
        h = rx.guarded(t, dt)
        d = h.to(self.dev)
        self.ins.append((h, d))
        return d.data_ptr() + PRE * h.element_size()

    def ints(self, v):
        return self.inp(torch.tensor(v, dtype=torch.int32), torch.int32)

    def out(self, init, dt):
        """(device buffer, pointer to its live region, host copy of the initial buffer)."""
        h = rx.guarded(init, dt)
        d = h.to(self.dev)
        return d, d.data_ptr() + PRE * h.element_size(), h

    def blank(self, shape, dt):
        return self.out(torch.full(tuple(shape), rx.CANARY, dtype=torch.float64), dt)

    def unchanged(self):
        torch.cuda.synchronize()
        for h, d in self.ins:
            assert same(d.cpu(), h), "an input buffer was written"


def run(rc):
    assert rc == 0, rc
    torch.cuda.synchronize()


def whole(buf, want, dt, what):
    """The whole buffer, guards included, equals ``want`` inside canaries, bit for bit."""
    got, exp = buf.cpu(), rx.guarded(want, dt)
    if not same(got, exp):
        bad = (bits(got) != bits(exp)).nonzero().reshape(-1)
        i = int(bad[0])
        pytest.fail("%s: %d words differ; first at %d (live region starts at %d, %d long): got %r want %r" % (
            what, bad.numel(), i - PRE, 0, want.numel(), float(got[i]), float(exp[i])))


def live64(buf, shape):
    assert rx.guards_intact(buf.cpu(), int(torch.tensor(shape).prod())), "guard words written"
    return rx.live(buf.cpu(), shape).double()


class Report:
    """Collects (name, kernel deviation, float32 yardstick deviation); asserts kernel <= factor x yardstick."""

    def __init__(self, what, factor):
        self.what, self.factor, self.rows = what, factor, []

    def add(self, name, kd, d):
        self.rows.append((name, kd, d))

    def f32(self, name, got, r64, r32):
        self.add(name, rx.deviation(got, r64[0], r64[1]), rx.deviation(r32[0], r64[0], r64[1]))

    def b16(self, name, got, ref, mag, ref32, dt, relu=False):
        """A 16-bit output: got must lie between the roundings of ref - tol and ref + tol (after the ReLU)."""
        d = rx.deviation(ref32, ref, mag)
        tol = self.factor * d * mag
        lo, hi = ref - tol, ref + tol
        if relu:
            lo, hi, ref = torch.relu(lo), torch.relu(hi), torch.relu(ref)
        lo, hi = lo.to(dt).double(), hi.to(dt).double()
        ok = (got >= lo) & (got <= hi)
        self.add(name, rx.excess16(got, ref, mag, dt), d)
        self.bad16 = int((~ok).sum())
        self.msg16 = "" if self.bad16 == 0 else "%s: %d elements outside [round(ref - tol), round(ref + tol)]" % (
            name, self.bad16)

    def finish(self):
        line = "%s: " % self.what + "; ".join("%s kernel %.3e float32 %.3e (allowed %.3e)" % (n, kd, d, self.factor * d)
                                             for n, kd, d in self.rows)
        print(line)
        assert not getattr(self, "msg16", ""), self.msg16 + " | " + line
        assert all(kd <= self.factor * d for _, kd, d in self.rows), line


# ---------------------------------------------------------------------------------------------- prep_input
@pytest.mark.parametrize("c_in,npix", rx.PREP_CASES)
def test_prep_input_is_bitwise(c_in, npix):
    """prep_input_kernel: fp32 NHWC -> 16-bit, channels zero-padded to 16; 300 pixels (a ragged last workgroup) and
    4096 x 256 + 300 (the grid-stride loop's second trip)."""
    ops, hr, dev, nrep, det = _env()
    dt = ops.act_dtype()
    x = rx.prep_input_case(c_in, npix)
    b = Bufs(dev)
    xp = b.inp(x, torch.float32)
    y, yp, _ = b.blank((npix, 16), dt)
    run(ops.lib().dtf_prep_input(xp, yp, npix, c_in, ops.stream()))
    want = rx.guarded(rx.prep_input_ref(x, dt), dt).to(dev)
    assert bool((bits(y) == bits(want)).all()), int((bits(y) != bits(want)).sum())
    b.unchanged()


# --------------------------------------------------------------------------------------------- weight_prep
@pytest.mark.parametrize("zn", rx.WP_ZN)
def test_weight_prep_is_bitwise(zn):
    """weight_prep_kernel: the float4 row, the padded stem row, the scalar row, the LDS-transposed and the gathered
    IHWO copies (none for dgr_off < 0), and exactly [0, zn) of the non-zero zbuf zeroed."""
    ops, hr, dev, nrep, det = _env()
    dt = ops.act_dtype()
    rx.check_weight_prep_table()
    state = rx.weight_prep_state()
    wf_want, wd_want = rx.weight_prep_expected(state, dt)
    b = Bufs(dev)
    sp, tp, slp = b.inp(state, torch.float32), b.ints(rx.WP_TABLE), b.ints(list(rx.SLOTS))
    wf, wfp, _ = b.blank((rx.CAP, rx.WP_W), dt)
    wd, wdp, _ = b.blank((rx.CAP, rx.WP_W), dt)
    zlen = max(rx.WP_ZN) + 5
    z0 = torch.arange(1, zlen + 1, dtype=torch.float64)
    z, zp, _ = b.out(z0, torch.float32)
    run(ops.lib().dtf_weight_prep(sp, rx.WP_S, tp, len(rx.WP_TABLE), slp, len(rx.SLOTS), wfp, wdp, rx.WP_W, zp, zn,
                                  ops.stream()))
    whole(wf, wf_want, dt, "forward (OHWI) shadow")
    whole(wd, wd_want, dt, "dgrad (IHWO) shadow")
    zw = z0.clone()
    zw[:zn] = 0
    whole(z, zw, torch.float32, "zbuf")
    b.unchanged()


# ------------------------------------------------------------------------------------------------ work_gen
def test_work_gen_tables_are_bitwise():
    """work_gen_kernel: six descriptors in one launch (prop 0 / 1, split 0 / 1, red NULL / set, bands 1 / 4, min_chunk
    above / below the computed chunk, per = 1, a 297-row tail) for members of 5, 0 and 131 images.  cnt of the listed
    slots is read, so the member without images has cnt 0; the unlisted slot's cnt is NaN."""
    ops, hr, dev, nrep, det = _env()
    M = len(rx.WG_SLOTS)
    cnt = torch.full((rx.CAP4,), rx.NAN, dtype=torch.float64)
    for s, v in rx.WG_CNT.items():
        cnt[s] = v
    b = Bufs(dev)
    slp, fp, cp = b.ints(list(rx.WG_SLOTS)), b.ints(list(rx.WG_FIRST)), b.inp(cnt, torch.float32)
    descs = (hr.WorkGenDesc * len(rx.WG_DESCS))()
    tabs, reds, want = [], [], []
    for i, d in enumerate(rx.WG_DESCS):
        per, bands, min_chunk, split, prop, red = d
        table, redt = rx.work_gen_ref(d, hr.elastic_rows)
        rx.check_work_table(d, table, redt)
        t = torch.full((2 * PRE + 4 * len(table),), rx.ICANARY, dtype=torch.int32, device=dev)
        r = torch.full((2 * PRE + 4 * M,), rx.ICANARY, dtype=torch.int32, device=dev)
        tabs.append(t)
        reds.append(r)
        want.append((table, redt))
        descs[i].dst = t.data_ptr() + 4 * PRE
        descs[i].red = r.data_ptr() + 4 * PRE if red else None
        descs[i].per, descs[i].bands, descs[i].min_chunk, descs[i].split, descs[i].prop = per, bands, min_chunk, split, prop
    dd = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
    run(ops.lib().dtf_work_gen(dd.data_ptr(), len(rx.WG_DESCS), slp, fp, M, cp, ops.stream()))
    for i, d in enumerate(rx.WG_DESCS):
        table, redt = want[i]
        exp = torch.full_like(tabs[i].cpu(), rx.ICANARY)
        exp[PRE:PRE + 4 * len(table)] = torch.tensor(table, dtype=torch.int32).reshape(-1)
        got = tabs[i].cpu()
        assert torch.equal(got, exp), (i, d, (got != exp).nonzero().reshape(-1)[:8].tolist())
        rx.check_work_table(d, got[PRE:PRE + 4 * len(table)].reshape(-1, 4).tolist(), redt)  # the contract, on the output
        expr = torch.full_like(reds[i].cpu(), rx.ICANARY)
        if d[5]:
            expr[PRE:PRE + 4 * M] = torch.tensor(redt, dtype=torch.int32).reshape(-1)
        assert torch.equal(reds[i].cpu(), expr), (i, d)
    b.unchanged()


# ------------------------------------------------------------------------------------------ per-BN kernels
def test_bn_eval_stats_is_bitwise():
    """bn_eval_stats_kernel: replica 0 = (n mean, n (var + mean^2)), replicas 1.. zero, columns >= C and the idle slot
    untouched, two table rows whose statistics index is not their row number."""
    ops, hr, dev, nrep, det = _env()
    k = rx.bn_eval_case(nrep)
    rx.check_bn_eval(k)
    b = Bufs(dev)
    sp, tp, slp, cp = b.inp(k.state, torch.float32), b.ints(rx.BN_TABLE), b.ints(list(rx.SLOTS)), b.inp(k.cnt, torch.float32)
    st, stp, _ = b.out(k.stats0, torch.float32)
    run(ops.lib().dtf_bn_eval_stats(sp, rx.BN_S, rx.BN_RUN_BASE, tp, len(rx.BN_TABLE), stp, rx.CAP * nrep * 128, slp,
                                    len(rx.SLOTS), cp, ops.stream()))
    whole(st, k.stats, torch.float32, "statistics")
    b.unchanged()


@pytest.mark.parametrize("n1", [False, True], ids=["n>1", "n=1"])
@pytest.mark.parametrize("mode", ["grads", "running", "step_end"])
def test_bn_running_update_and_step_end(mode, n1):
    """bn_running_update_kernel.  grads != NULL (and z = 0 of bn_step_end): g[gamma_off + c] += sum q, g[beta_off + c]
    += sum s from integer replica words onto an integer seed, bitwise.  grads == NULL (and z = 1): moving mean and
    unbiased variance (n = 1: the biased one) within 4 x the float32 yardstick.  One bn_step_end launch gives both.  The
    listed member with cnt == 0 (its cnt is read; statistics NaN) and the unlisted slot (cnt NaN) keep every word."""
    ops, hr, dev, nrep, det = _env()
    L = ops.lib()
    k = rx.bn_end_case(nrep, n1)
    rx.check_bn_end(k)
    b = Bufs(dev)
    tp, slp, cp = b.ints(k.table), b.ints(list(rx.SLOTS4)), b.inp(k.cnt, torch.float32)
    fp, bp = b.inp(k.stf, torch.float32), b.inp(k.stb, torch.float32)
    st, sp, st_h = b.out(k.state0, torch.float32)
    gr, gp, _ = b.out(k.grads0, torch.float32)
    stride, nb, ns = rx.CAP4 * nrep * 128, len(k.table), len(rx.SLOTS4)
    if mode == "grads":
        run(L.dtf_bn_running_update(sp, rx.BN_S, rx.BN_RUN_BASE, tp, nb, bp, stride, slp, ns, cp, gp, rx.BN_G, ops.stream()))
    elif mode == "running":
        run(L.dtf_bn_running_update(sp, rx.BN_S, rx.BN_RUN_BASE, tp, nb, fp, stride, slp, ns, cp, None, rx.BN_G,
                                    ops.stream()))
    else:
        run(L.dtf_bn_step_end(sp, rx.BN_S, rx.BN_RUN_BASE, tp, nb, fp, bp, stride, slp, ns, cp, gp, rx.BN_G, ops.stream()))
    whole(gr, k.grads0 if mode == "running" else k.grads, torch.float32, "gradient rows")
    got = st.cpu()
    if mode == "grads":
        assert same(got, st_h), "state written by the gradient half"
    else:
        r64, r32 = rx.bn_running_eval(k, torch.float64), rx.bn_running_eval(k, torch.float32)
        rep = Report("bn running %s n1=%d" % (mode, n1), rx.FACTOR_RSQRT)
        keep = torch.ones(rx.CAP4, rx.BN_S, dtype=torch.bool)
        g2 = rx.live(got, (rx.CAP4, rx.BN_S)).double()
        for (row, s), (m, mm, v, vm) in r64.items():
            run_off, c = k.table[row][0], k.table[row][1]
            o = rx.BN_RUN_BASE + run_off
            keep[s, o:o + 2 * c] = False
            rep.f32("mean[%d,%d]" % (row, s), g2[s, o:o + c], (m, mm), r32[(row, s)][0:2])
            rep.f32("var[%d,%d]" % (row, s), g2[s, o + c:o + 2 * c], (v, vm), r32[(row, s)][2:4])
        h2 = rx.live(st_h, (rx.CAP4, rx.BN_S))
        assert same(rx.live(got, (rx.CAP4, rx.BN_S))[keep], h2[keep]) and rx.guards_intact(got, rx.CAP4 * rx.BN_S)
        assert bool(torch.isfinite(g2[list(rx.SLOTS)]).all())
        rep.finish()
    b.unchanged()


# ---------------------------------------------------------------------------------------------- bn_bwd_apply
def _stats_ptrs(b, *sts):
    return [b.inp(s, torch.float32) for s in sts]


@pytest.mark.parametrize("c,hw,add", rx.BWD_APPLY_CASES)
def test_bn_bwd_apply_matches_float64(c, hw, add):
    """bn_bwd_apply_kernel: g = A dz + B x + C (+ add) with the coefficients of bwd_coef from fp32 replica words spread
    unevenly; split 1 with idle threads, split 2 and 4, wrapping c0, one channel of variance exactly 0."""
    ops, hr, dev, nrep, det = _env()
    dt = ops.act_dtype()
    k = rx.bwd_apply_case(c, hw, add, nrep)
    rx.check_bwd_apply(k)
    b = Bufs(dev)
    a = hr.BnBwdArgs()
    a.dz, a.x, a.add = b.inp(k.dz, dt), b.inp(k.x, dt), b.inp(k.add, dt)
    out, a.out, _ = b.blank(k.x.shape, dt)
    a.img_slot, a.params, a.p_mstride, a.gamma_off = b.ints(rx.img_slots()), b.inp(k.params, torch.float32), \
        k.params.shape[1], k.gamma_off
    a.st_f, a.st_b = _stats_ptrs(b, k.stf, k.stb)
    a.cnt, a.hw, a.C, a.nimg = b.inp(k.cnt, torch.float32), hw, c, k.n
    run(ops.lib().dtf_bn_bwd_apply(ctypes.byref(a), ops.stream()))
    (r64, mag), (r32, _) = rx.bwd_apply_eval(k, torch.float64), rx.bwd_apply_eval(k, torch.float32)
    rep = Report("bn_bwd_apply C%d hw%d add%d" % (c, hw, add), rx.FACTOR_RSQRT)
    rep.b16("out", live64(out, k.x.shape), r64, mag, r32, dt)
    rep.finish()
    b.unchanged()


# ----------------------------------------------------------------------------------------------- bn_add_relu
def _ew_args(hr, b, k, dt, with_h2, with_add):
    a = hr.BnEwArgs()
    a.h1 = b.inp(k.h1, dt)
    a.h2 = b.inp(k.h2, dt) if with_h2 else None
    a.add = b.inp(k.h2, dt) if with_add else None
    a.img_slot, a.params, a.p_mstride = b.ints(k.slot), b.inp(k.params, torch.float32), k.params.shape[1]
    (a.g1, a.b1), (a.g2, a.b2) = k.offs
    a.st1, a.st2 = _stats_ptrs(b, k.st1, k.st2)
    a.cnt, a.hw, a.C, a.nimg = b.inp(k.cnt, torch.float32), k.hw, k.c, len(k.slot)
    return a


@pytest.mark.parametrize("cap", [rx.ELASTIC_CAP, 0], ids=["elastic", "cap0"])
@pytest.mark.parametrize("c,hw,form", rx.ADD_RELU_CASES)
def test_bn_add_relu_matches_float64(c, hw, form, cap):
    """bn_add_relu_kernel: relu(BN1(h1) + [0 | add | BN2(h2)]).  Elastic form: the padded images hold NaN and their
    outputs keep the canary; cap = 0 on the same data gives the same real outputs and writes the padded ones."""
    ops, hr, dev, nrep, det = _env()
    dt = ops.act_dtype()
    k = rx.add_relu_case(c, hw, form, nrep)
    rx.check_add_relu(k)
    b = Bufs(dev)
    a = _ew_args(hr, b, k, dt, form == 2, form == 1)
    out, a.out, _ = b.blank(k.h1.shape, dt)
    a.cap = cap
    run(ops.lib().dtf_bn_add_relu(ctypes.byref(a), ops.stream()))
    (v64, mag), (v32, _) = rx.add_relu_eval(k, torch.float64), rx.add_relu_eval(k, torch.float32)
    got, r = live64(out, k.h1.shape), k.real
    rep = Report("bn_add_relu C%d hw%d form%d cap%d" % (c, hw, form, cap), rx.FACTOR_RSQRT)
    rep.b16("out", got[r], v64[r], mag[r], v32[r], dt, relu=True)
    if cap:
        assert bool((got[~r] == rx.CANARY).all()), "a padded image was written"
    else:
        assert bool((got[~r] != rx.CANARY).all())  # without cap the kernel cannot tell them apart
    rep.finish()
    b.unchanged()


# ---------------------------------------------------------------------------------------------- bn_bwd_reduce
@pytest.mark.parametrize("c,hw,two,sizes,elastic", rx.REDUCE_CASES)
def test_bn_bwd_reduce_matches_float64(c, hw, two, sizes, elastic):
    """bn_bwd_reduce_kernel (+ bn_bwd_reduce_finish_kernel on the deterministic build, which returns -1 and writes
    nothing elsewhere): the sum(d) rows of both accumulators bitwise (integer d), the xhat rows within 4 x the float32
    yardstick, as replica sums onto a non-zero seed; NaN padded images of the elastic form add nothing; the idle
    slot's rows and the columns >= C keep their words.  Deterministic build: one slab row per image, row 0 exact,
    only replica 0 written, ``first`` from the ragged (or capacity) layout."""
    ops, hr, dev, nrep, det = _env()
    L, dt = ops.lib(), ops.act_dtype()
    k = rx.reduce_case(c, hw, two, sizes, elastic, nrep)
    rx.check_reduce(k)
    b = Bufs(dev)
    a = _ew_args(hr, b, k, dt, bool(two), False)
    a.d = b.inp(k.d, dt)
    a.cap = rx.ELASTIC_CAP if elastic else 0
    sb1, a.sb1, _ = b.out(k.seed1, torch.float32)
    sb2, a.sb2, _ = b.out(k.seed2, torch.float32)
    n = len(k.slot)
    slab, slab_p, _ = b.blank((n, 3, 64), torch.float32)
    a.slab = slab_p if det else None
    run(L.dtf_bn_bwd_reduce(ctypes.byref(a), ops.stream()))
    rc = L.dtf_bn_bwd_reduce_finish(ctypes.byref(a), b.ints(k.first), b.ints(list(rx.SLOTS)), len(rx.SLOTS), ops.stream())
    torch.cuda.synchronize()
    r64, r32 = rx.reduce_eval(k, torch.float64), rx.reduce_eval(k, torch.float32)
    g1, g2 = live64(sb1, k.seed1.shape), live64(sb2, k.seed2.shape)
    gs = live64(slab, (n, 3, 64))
    if det:
        assert rc == 0
        assert torch.equal(g1[:, 1:], k.seed1[:, 1:]) and torch.equal(g2[:, 1:], k.seed2[:, 1:])  # replica 0 only
        assert torch.equal(gs[k.real][:, 0, :c], r64["img_sd"][k.real]), "per-image sum(d) rows"
        assert bool((gs[~k.real] == rx.CANARY).all()) and bool((gs[:, :, c:] == rx.CANARY).all())
    else:
        assert rc == -1 and bool((gs == rx.CANARY).all())
    for got, seed in ((g1, k.seed1), (g2, k.seed2)):
        assert torch.equal(got[rx.IDLE], seed[rx.IDLE]) and torch.equal(got[..., c:], seed[..., c:])
    assert torch.equal(g1[:, :, 0].sum(1), r64["sd"][0]), "sum(d) of BN1"
    rep = Report("bn_bwd_reduce C%d hw%d h2=%d n=%d elastic%d" % (c, hw, two, n, elastic), rx.FACTOR_RSQRT)
    rep.f32("xhat1", g1[:, :, 1].sum(1), r64["x1"], r32["x1"])
    if two:
        assert torch.equal(g2[:, :, 0].sum(1), r64["sd2"]), "sum(d) of BN2"
        rep.f32("xhat2", g2[:, :, 1].sum(1), r64["x2"], r32["x2"])
    else:
        assert torch.equal(g2, k.seed2), "the second accumulator was written without h2"
    rep.finish()
    b.unchanged()


# ------------------------------------------------------------------------------------------------------ head
class _Head:
    def __init__(self, ops, hr, dev, k, train, loss_scale, use_slab, **over):
        dt = ops.act_dtype()
        self.b = b = Bufs(dev)
        self.k, self.nb = k, len(rx.HEAD_WORK)
        a = hr.HeadArgs()
        a.x, a.labels = b.inp(k.x, dt), b.ints(k.labels.tolist())
        a.work, a.params, a.p_mstride = b.ints(rx.HEAD_WORK), b.inp(k.params, torch.float32), rx.HEAD_P
        a.gamma_off, a.beta_off, a.dw_off, a.db_off = (rx.HEAD_GAMMA if k.v2 else -1), rx.HEAD_BETA, rx.HEAD_DW, rx.HEAD_DB
        self.grads, a.grads, _ = b.out(k.grads0, torch.float32)
        a.g_mstride = rx.HEAD_P
        a.st_f = b.inp(k.stf, torch.float32)
        self.stb, a.st_b, _ = b.out(k.stb0, torch.float32)
        a.cnt = b.inp(k.cnt, torch.float32)
        self.dfeat, a.dfeat, _ = b.blank((k.n, 64), torch.float32)
        self.loss, a.loss, _ = b.out(k.loss0, torch.float32)
        self.correct, a.correct, _ = b.out(k.correct0, torch.float32)
        self.logits, a.logits_out, _ = b.blank((k.n, k.ncls), torch.float32)
        a.hw, a.C, a.ncls, a.train, a.loss_scale = k.hw, 64, k.ncls, train, loss_scale
        self.slab, sp, _ = b.blank((self.nb, k.ncls * 64), torch.float32)
        self.slab_b, sbp, _ = b.blank((self.nb, k.ncls), torch.float32)
        a.slab, a.slab_b = (sp, sbp) if use_slab else (None, None)
        for name, v in over.items():
            setattr(a, name, v)
        self.a = a

    def untouched(self, names):
        k = self.k
        init = {"grads": k.grads0, "stb": k.stb0, "loss": k.loss0, "correct": k.correct0}
        for name in names:
            buf = getattr(self, name)
            if name in init:
                whole(buf, init[name], torch.float32, name)
            else:
                assert bool((buf.cpu() == rx.CANARY).all()), "%s was written" % name


@pytest.mark.parametrize("hw,ncls,v2,train,loss_scale,use_slab", rx.HEAD_CASES)
def test_head_matches_float64(hw, ncls, v2, train, loss_scale, use_slab):
    """head_kernel.  Bitwise: the ``correct`` counts (argmax gaps are 128 x the tolerance; image 1 is labelled with its
    runner-up), the logits of the v1 form (integer operands), the statistics of the v1 form and every buffer the mode
    does not write (train = 0: dfeat, st_b, gradients, slabs; slab form: the gradient rows; atomic form: the slabs).
    Within 8 x the float32 yardstick: loss, logits, dfeat, dense dw / db (per workgroup in the slab form, as gradient
    rows in the atomic form) and the st_b replica sums.  Deterministic build: each workgroup's loss partial is
    rounded to 2^-16, so the loss must lie between the sums of the partials' roundings at ref -+ tol."""
    ops, hr, dev, nrep, det = _env()
    k = rx.head_case(hw, ncls, v2, nrep)
    rx.check_head(k)
    h = _Head(ops, hr, dev, k, train, loss_scale, use_slab)
    run(ops.lib().dtf_head(ctypes.byref(h.a), h.nb, ops.stream()))
    r64, r32 = rx.head_eval(k, loss_scale, torch.float64), rx.head_eval(k, loss_scale, torch.float32)
    t64, t32 = rx.head_totals(k, r64, nrep), rx.head_totals(k, r32, nrep)
    rep = Report("head hw%d ncls%d v%d train%d x%g slab%d" % (hw, ncls, 2 if v2 else 1, train, loss_scale, use_slab),
                 rx.FACTOR_EXP)
    whole(h.correct, rx.head_correct(k), torch.float32, "correct")
    glog = live64(h.logits, (k.n, ncls))
    if v2:
        rep.f32("logits", glog, r64["logits"], r32["logits"])
    else:
        whole(h.logits, r64["logits"][0], torch.float32, "v1 logits")
    gl = live64(h.loss, (rx.CAP,))
    assert gl[rx.IDLE] == k.loss0[rx.IDLE]
    d_loss = rx.deviation(r32["item_loss"][0], *r64["item_loss"])
    if det:  # the partials' roundings at ref -+ tol bound the sum
        ref, mag = rx.head_eval(k, loss_scale, torch.float64)["item_loss"]
        tol = rx.FACTOR_EXP * d_loss * mag
        lo, hi = k.loss0.clone(), k.loss0.clone()
        for i, (_, _, _, s) in enumerate(rx.HEAD_WORK):
            lo[s] += torch.round((ref[i] - tol[i]) * 65536) / 65536
            hi[s] += torch.round((ref[i] + tol[i]) * 65536) / 65536
        sl = list(rx.SLOTS)
        assert bool((gl[sl] >= lo[sl]).all()) and bool((gl[sl] <= hi[sl]).all()), (gl, lo, hi)
        assert bool(((gl - k.loss0) * 65536 == ((gl - k.loss0) * 65536).round()).all())
        print("head loss (deterministic build): kernel deviation %.3e, float32 %.3e before the 2^-16 rounding" % (
            rx.deviation(gl, *t64["loss"]), d_loss))
    else:
        rep.f32("loss", gl, t64["loss"], t32["loss"])
    if train:
        rep.f32("dfeat", live64(h.dfeat, (k.n, 64)), r64["dfeat"], r32["dfeat"])
        gst = live64(h.stb, k.stb0.shape)
        if v2:
            assert torch.equal(gst[rx.IDLE], k.stb0[rx.IDLE])
            rep.f32("st_b", gst.sum(1), t64["st_b"], t32["st_b"])
        else:
            h.untouched(["stb"])
        if use_slab:
            rep.f32("slab dw", live64(h.slab, (h.nb, ncls, 64)), r64["dw"], r32["dw"])
            rep.f32("slab db", live64(h.slab_b, (h.nb, ncls)), r64["db"], r32["db"])
            h.untouched(["grads"])
        else:
            gg = live64(h.grads, k.grads0.shape)
            keep = torch.ones_like(k.grads0, dtype=torch.bool)
            keep[list(rx.SLOTS), rx.HEAD_DW:rx.HEAD_DW + ncls * 64] = False
            keep[list(rx.SLOTS), rx.HEAD_DB:rx.HEAD_DB + ncls] = False
            assert torch.equal(gg[keep], k.grads0[keep]), "gradient words outside dw / db"
            rep.f32("grads dw/db", gg, t64["grads"], t32["grads"])
            h.untouched(["slab", "slab_b"])
    else:
        h.untouched(["dfeat", "stb", "grads", "slab", "slab_b"])
    rep.finish()
    h.b.unchanged()


@pytest.mark.parametrize("over", rx.HEAD_REJECTS, ids=lambda o: "%s=%d" % next(iter(o.items())))
def test_head_rejects_geometries_it_cannot_run(over):
    """dtf_head returns -22 for C != 64, hw % 32 != 0, hw > 128, ncls > 16 and ncls < 1, and writes nothing."""
    ops, hr, dev, nrep, det = _env()
    k = rx.head_case(32, 10, 0, nrep)
    h = _Head(ops, hr, dev, k, 1, 1.0, True, **over)
    rc = ops.lib().dtf_head(ctypes.byref(h.a), h.nb, ops.stream())
    torch.cuda.synchronize()
    assert rc == -22, rc
    h.untouched(["grads", "stb", "loss", "correct", "dfeat", "logits", "slab", "slab_b"])
    h.b.unchanged()


# --------------------------------------------------------------------------------------------- head_bwd_apply
@pytest.mark.parametrize("hw,v2", rx.HEAD_BWD_CASES)
def test_head_bwd_apply_matches_float64(hw, v2):
    """head_bwd_apply_kernel from constructed dfeat and statistics.  v1 (gamma_off < 0): dfeat * [x > 0], bitwise.  v2:
    A dz + B x + C with dz = dfeat * [x s + t > 0] (mask margins asserted), within 4 x the float32 yardstick."""
    ops, hr, dev, nrep, det = _env()
    dt = ops.act_dtype()
    k = rx.head_bwd_case(hw, v2, nrep)
    rx.check_head_bwd(k)
    b = Bufs(dev)
    out, outp, _ = b.blank(k.x.shape, dt)
    go, bo = k.offs[0]
    run(ops.lib().dtf_head_bwd_apply(b.inp(k.x, dt), b.inp(k.dfeat, torch.float32), outp, b.ints(rx.img_slots()),
                                     b.inp(k.params, torch.float32), k.params.shape[1], go if v2 else -1, bo,
                                     b.inp(k.stf, torch.float32), b.inp(k.stb, torch.float32),
                                     b.inp(k.cnt, torch.float32), hw, 64, k.n, ops.stream()))
    r64, mag, _, _ = rx.head_bwd_eval(k, torch.float64)
    if v2:
        rep = Report("head_bwd_apply hw%d v2" % hw, rx.FACTOR_RSQRT)
        rep.b16("out", live64(out, k.x.shape), r64, mag, rx.head_bwd_eval(k, torch.float32)[0], dt)
        rep.finish()
    else:
        assert torch.equal(r64.to(dt).double(), r64)
        whole(out, r64, dt, "v1 out")
    b.unchanged()
