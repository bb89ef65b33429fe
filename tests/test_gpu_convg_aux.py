"""Kernel-level tests of the ImageNet auxiliary kernels (ops/csrc/convg_aux.hip, and the fp32 pool of f32net.hip):
direct launches against the float64 references of tests/_convg_aux_exact.py, bitwise wherever the integer design
allows (max-pool and its argmax bytes, the three BN apply passes on both their kernel forms, channel statistics,
BN-backward sums, GAP at hw 1 / 4 / 16, the input / weight / dense preparation), and against float64 with a tolerance
taken from a float32 CPU evaluation of the same formulas for BN finalize (x 4) and softmax cross-entropy (x 8), whose
figures are printed.  Members in slots 0 and 2 of capacity 3, ragged image counts, outputs inside canary guards and
compared whole, argument-struct sizes asserted before the first launch."""
import ctypes

import pytest
import torch

import _convg_aux_exact as ax
import _convg_exact as cx

pytestmark = pytest.mark.gpu

PRE = 64  # guard elements before and after every output (keeps 16-byte alignment for every element size)


def guarded(init, dt, dev, canary=ax.CANARY):
    """(device buffer [PRE canaries | init | PRE canaries], address of the live region)."""
    n = init.numel()
    flat = torch.full((n + 2 * PRE,), canary, dtype=dt)
    flat[PRE:PRE + n] = init.reshape(-1).to(dt)
    b = flat.to(dev)
    return b, b.data_ptr() + PRE * b.element_size()


def out_buf(shape, dt, dev, canary=ax.CANARY):
    return guarded(torch.full(tuple(shape), canary, dtype=torch.float64), dt, dev, canary)


def assert_whole(buf, want, what, canary=ax.CANARY):
    """The whole buffer, guards included, equals ``want`` inside canaries."""
    got = buf.cpu().double()
    exp = torch.full_like(got, float(canary))
    exp[PRE:PRE + want.numel()] = want.reshape(-1).double()
    if not torch.equal(got, exp):
        bad = (got != exp).nonzero()
        i = int(bad[0])
        pytest.fail("%s: %d words differ; first at %d (live region starts at %d, %d long): got %r want %r" % (
            what, bad.shape[0], i, PRE, want.numel(), float(got[i]), float(exp[i])))


def acc64(t, shift, det):
    """Accumulator words as float64 (the fixed-point words decode without a rounding)."""
    return t.cpu().double() * 2.0 ** -shift if det else t.cpu().double()


def i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def run(rc):
    assert rc == 0, rc
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- max-pool
def _pool(ops, fn, k, dt, dev, fwd=True, bwd=True, am_from_kernel=False):
    n = ax.POOL_N
    am_t = k.am.to(torch.uint8).to(dev)
    if fwd:
        x = k.x.to(dt).to(dev)
        y, yp = out_buf(k.y.shape, dt, dev)
        am, amp = out_buf(k.am.shape, torch.uint8, dev, ax.AM_CANARY)
        run(fn(x.data_ptr(), yp, amp, None, None, n, k.h, k.w, k.ho, k.wo, k.c, 0, ops.stream()))
        assert_whole(y, k.y, "y")
        assert_whole(am, k.am, "argmax", ax.AM_CANARY)
        if am_from_kernel:
            am_t = am[PRE:PRE + k.am.numel()].clone()
    if bwd:
        g = k.g.to(dt).to(dev)
        dx, dxp = out_buf(k.dx.shape, dt, dev)
        run(fn(None, None, am_t.data_ptr(), g.data_ptr(), dxp, n, k.h, k.w, k.ho, k.wo, k.c, 1, ops.stream()))
        assert_whole(dx, k.dx, "dx")


@pytest.mark.parametrize("c", ax.POOL_C)
@pytest.mark.parametrize("h,w", ax.POOL_GEO)
def test_maxpool_forward_is_exact(h, w, c):
    """cg_maxpool_fwd_kernel: values and argmax bytes (first tap wins a tie, clipped last window, -inf padding)."""
    ops, hi, dev, det = cx.gpu_env()
    k = ax.pool_case(h, w, c)
    ax.check_pool(k)
    _pool(ops, ops.lib().dtf_cg_maxpool, k, ops.act_dtype(), dev, bwd=False)


@pytest.mark.parametrize("c", ax.POOL_C)
@pytest.mark.parametrize("h,w", ax.POOL_GEO)
def test_maxpool_backward_is_exact(h, w, c):
    """cg_maxpool_bwd2_kernel at the even geometries, cg_maxpool_bwd_kernel at (7, 5), from the reference's argmax."""
    ops, hi, dev, det = cx.gpu_env()
    k = ax.pool_case(h, w, c)
    ax.check_pool(k)
    assert (h == 2 * k.ho and w == 2 * k.wo) == (h % 2 == 0)  # the launcher's choice of kernel
    _pool(ops, ops.lib().dtf_cg_maxpool, k, ops.act_dtype(), dev, fwd=False)


@pytest.mark.parametrize("h,w,c", [(6, 10, 8), (7, 5, 24)])
def test_maxpool_forward_feeds_backward(h, w, c):
    ops, hi, dev, det = cx.gpu_env()
    k = ax.pool_case(h, w, c)
    ax.check_pool(k)
    _pool(ops, ops.lib().dtf_cg_maxpool, k, ops.act_dtype(), dev, am_from_kernel=True)


@pytest.mark.parametrize("c", ax.POOL_C_F32)
@pytest.mark.parametrize("h,w", ax.POOL_GEO_F32)
def test_f32_maxpool_is_exact(h, w, c):
    """f32_maxpool_fwd_kernel / f32_maxpool_bwd_kernel: the same contract at fp32, forward feeding backward."""
    ops, hi, dev, det = cx.gpu_env()
    from distributedtf_amd.engine import hip_imagenet_f32
    hip_imagenet_f32._register()
    k = ax.pool_case(h, w, c)
    ax.check_pool(k)
    _pool(ops, ops.lib().dtf_f32_maxpool, k, torch.float32, dev, am_from_kernel=True)
    _pool(ops, ops.lib().dtf_f32_maxpool, k, torch.float32, dev, fwd=False)


# ------------------------------------------------------------------------------------------ BN apply passes
def _apply_params(kind):
    return [pytest.param(g, v, id="%s-v%d" % (g[0], v)) for g in ax.apply_geos(kind)
            for v in ax.apply_variants(kind, g[5])]


def _run_apply(kind, geo, v):
    name, c, hw, sizes, kernel, multi = geo
    ops, hi, dev, det = cx.gpu_env()
    L, dt = ops.lib(), ops.act_dtype()
    k = ax.apply_case(kind, c, hw, sizes, v)
    ax.check_apply(k)
    assert k.bound <= ax.INT_EXACT[dt]
    p = ax.apply_path(c, hw, k.n)
    assert (p["kernel"], p["multi"]) == (kernel, multi) and (p["mid"] or not multi), p
    slot = i32(ax.img_slots(sizes), dev)
    coef = k.coef.float().to(dev)
    h = k.h.to(dt).to(dev)
    out, outp = out_buf(k.out.shape, dt, dev)
    keep = []
    if kind == "add":
        a = hi.BnAddArgs()
        assert ctypes.sizeof(a) == L.dtf_bnadd_args_size()
        s = k.s.to(dt).to(dev)
        a.h, a.s, a.out, a.coef_h, a.img_slot = h.data_ptr(), s.data_ptr(), outp, coef.data_ptr(), slot.data_ptr()
        if v:
            keep.append(k.coef_s.float().to(dev))
            a.coef_s = keep[-1].data_ptr()
        fn = L.dtf_cg_bn_add_relu
    else:
        a = hi.EwArgs()
        assert ctypes.sizeof(a) == L.dtf_ew_args_size()
        a.h, a.out, a.coef, a.img_slot = h.data_ptr(), outp, coef.data_ptr(), slot.data_ptr()
        if kind == "bwd":
            keep.append(k.dz.to(dt).to(dev))
            a.dz = keep[-1].data_ptr()
            if v:
                keep.append(k.add.to(dt).to(dev))
                a.add = keep[-1].data_ptr()
        fn = L.dtf_cg_bn_relu_apply if kind == "relu" else L.dtf_cg_bn_bwd_apply
    a.hw, a.C, a.cmax, a.nimg = hw, c, ax.ACMAX, k.n
    run(fn(ctypes.byref(a), ops.stream()))
    assert_whole(out, k.out, "%s %s" % (kind, name))
    assert torch.equal(coef.cpu().double(), k.coef)


@pytest.mark.parametrize("geo,v", _apply_params("relu"))
def test_bn_relu_apply_is_exact(geo, v):
    """cg_ew_apply_cf_kernel<true> (cf-*) and cg_bn_relu_apply_kernel (walk-*: chan8's modulo branch)."""
    _run_apply("relu", geo, v)


@pytest.mark.parametrize("geo,v", _apply_params("bwd"))
def test_bn_bwd_apply_is_exact(geo, v):
    """cg_ew_apply_cf_kernel<false> and cg_bn_bwd_apply_kernel, without (v0) and with (v1) the added gradient."""
    _run_apply("bwd", geo, v)


@pytest.mark.parametrize("geo,v", _apply_params("add"))
def test_bn_add_relu_is_exact(geo, v):
    """cg_bn_add_relu_cf_kernel and cg_bn_add_relu_kernel, identity (v0) and projection-BN (v1) shortcut."""
    _run_apply("add", geo, v)


# -------------------------------------------------------------------------- channel statistics, BN-bwd sums
@pytest.mark.parametrize("hw", ax.STAT_HW)
@pytest.mark.parametrize("c", ax.STAT_C)
def test_chan_stats_is_exact(c, hw):
    ops, hi, dev, det = cx.gpu_env()
    k = ax.stats_case(c, hw)
    ax.check_stats(k)
    x = k.x.to(ops.act_dtype()).to(dev)
    slot = i32(ax.img_slots(k.sizes), dev)
    sums = cx.acc_upload(k.prefill, cx.FX_STAT, det, dev)
    run(ops.lib().dtf_cg_chan_stats(x.data_ptr(), slot.data_ptr(), sums.data_ptr(), x.shape[0], hw, c, ax.ACMAX,
                                    ops.stream()))
    got = acc64(sums, cx.FX_STAT, det)
    assert torch.equal(got, k.ref), (got - k.ref).abs().max()


def _bnsum_launch(ops, hi, dev, det, k, c):
    L, dt = ops.lib(), ops.act_dtype()
    a = hi.BnSumArgs()
    assert ctypes.sizeof(a) == L.dtf_bnsum_args_size()
    t = [k.dz.to(dt).to(dev), k.h.to(dt).to(dev), k.fc.float().to(dev), i32(ax.img_slots(k.sizes), dev)]
    sums = cx.acc_upload(k.prefill, cx.FX_GRAD, det, dev)
    sums2 = cx.acc_upload(k.prefill2, cx.FX_GRAD, det, dev)
    a.dz, a.h, a.fc, a.img_slot, a.sums, a.sums2 = (t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                                                    sums.data_ptr(), sums2.data_ptr())
    if k.two:
        t += [k.h2.to(dt).to(dev), k.fc2.float().to(dev)]
        a.h2, a.fc2 = t[-2].data_ptr(), t[-1].data_ptr()
    a.hw, a.C, a.cmax = k.hw, c, ax.ACMAX
    rc = L.dtf_cg_bn_bwd_sums(ctypes.byref(a), k.dz.shape[0], ops.stream())
    torch.cuda.synchronize()
    return rc, acc64(sums, cx.FX_GRAD, det), acc64(sums2, cx.FX_GRAD, det)


@pytest.mark.parametrize("two", [0, 1])
@pytest.mark.parametrize("hw", ax.STAT_HW)
@pytest.mark.parametrize("c", ax.STAT_C)
def test_bn_bwd_sums_is_exact(c, hw, two):
    ops, hi, dev, det = cx.gpu_env()
    k = ax.bnsum_case(c, hw, two)
    ax.check_bnsum(k)
    rc, got, got2 = _bnsum_launch(ops, hi, dev, det, k, c)
    assert rc == 0, rc
    assert torch.equal(got, k.ref), (got - k.ref).abs().max()
    assert torch.equal(got2, k.ref2), (got2 - k.ref2).abs().max()  # one BN: the second table is untouched


@pytest.mark.parametrize("c", ax.STAT_REJECT)
def test_statistics_launchers_reject_widths_they_cannot_split(c):
    """C = 24 (2048 % C != 0: the fixed-channel walk would not hold) and C = 4096 (LDS rows are 2048 wide): -2 and
    untouched tables, never a silent kernel that adds nothing."""
    ops, hi, dev, det = cx.gpu_env()
    assert ax.stats_split(c) is None
    k = ax.bnsum_case(8, 1, 1)  # any tensors: the launchers must return before a launch
    x = torch.ones(5 * c, dtype=ops.act_dtype(), device=dev)
    slot = i32(ax.img_slots(ax.SIZES), dev)
    sums = cx.acc_upload(k.prefill, cx.FX_STAT, det, dev)
    rc = ops.lib().dtf_cg_chan_stats(x.data_ptr(), slot.data_ptr(), sums.data_ptr(), 5, 1, c, ax.ACMAX, ops.stream())
    torch.cuda.synchronize()
    assert rc == -2 and torch.equal(acc64(sums, cx.FX_STAT, det), k.prefill)
    rc, got, got2 = _bnsum_launch(ops, hi, dev, det, k, c)
    assert rc == -2 and torch.equal(got, k.prefill) and torch.equal(got2, k.prefill2)


# ----------------------------------------------------------------------------------------------------- GAP
def _gap_launch(ops, hi, dev, det, k, which, dt):
    """Launch dtf_cg_gap ``which`` on case k; returns (feat buffer, sums as float64, out buffer)."""
    L = ops.lib()
    a = hi.GapArgs()
    assert ctypes.sizeof(a) == L.dtf_gap_args_size()
    n = k.x.shape[0]
    t = [k.x.to(dt).to(dev), i32(ax.img_slots(k.sizes), dev), k.dfeat.float().to(dev)]
    a.x, a.img_slot, a.dfeat = t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr()
    if k.v2:
        t += [k.coef.float().to(dev), k.bcoef.float().to(dev)]
        a.coef, a.bcoef = t[-2].data_ptr(), t[-1].data_ptr()
    feat, a.feat = out_buf((n, k.c), dt, dev)
    out, a.out = out_buf(k.x.shape, dt, dev)
    sums = cx.acc_upload(k.prefill if k.v2 else torch.zeros(ax.CAP, 2, ax.ACMAX, dtype=torch.float64), cx.FX_GRAD,
                         det, dev)
    a.sums = sums.data_ptr()
    a.hw, a.C, a.cmax = k.hw, k.c, ax.ACMAX
    run(L.dtf_cg_gap(ctypes.byref(a), which, n, ops.stream()))
    return feat, acc64(sums, cx.FX_GRAD, det), out


@pytest.mark.parametrize("v2", [1, 0])
@pytest.mark.parametrize("hw", ax.GAP_HW)
@pytest.mark.parametrize("c", ax.GAP_C)
def test_gap_is_exact(c, hw, v2):
    """cg_gap_kernel, cg_gap_bwd_reduce_kernel (v2 only: it needs the final BN) and cg_gap_bwd_apply_kernel, with the
    final BN's coefficients (v2) and with coef == NULL (v1); each launch leaves the other outputs' canaries."""
    ops, hi, dev, det = cx.gpu_env()
    dt = ops.act_dtype()
    k = ax.gap_case(c, hw, v2)
    ax.check_gap(k)
    blank_f, blank_o = torch.full_like(k.feat, ax.CANARY), torch.full_like(k.out, ax.CANARY)
    before = k.prefill if v2 else torch.zeros(ax.CAP, 2, ax.ACMAX, dtype=torch.float64)
    for which in ((0, 1, 2) if v2 else (0, 2)):
        feat, sums, out = _gap_launch(ops, hi, dev, det, k, which, dt)
        assert_whole(feat, k.feat if which == 0 else blank_f, "feat (which %d)" % which)
        assert_whole(out, k.out if which == 2 else blank_o, "out (which %d)" % which)
        want = k.ref if which == 1 else before
        assert torch.equal(sums, want), (which, (sums - want).abs().max())


def test_gap_at_49_pixels():
    """hw = 49: 1 / hw is rounded, so feat and out may differ from the float64 result rounded to the activation type by
    one unit in the last place of that type, and the sums get BN finalize's tolerance: 4 x the scaled deviation of a
    float32 CPU evaluation (printed with the kernel's own)."""
    ops, hi, dev, det = cx.gpu_env()
    dt = ops.act_dtype()
    k = ax.gap_case(64, 49, 1)
    ax.check_gap(k, exact=False)
    r64, r32 = ax.gap_reduce_eval(k, torch.float64), ax.gap_reduce_eval(k, torch.float32)
    d = ax.deviation(r32["sums"][0], *r64["sums"])
    for which, want in ((0, k.feat), (2, k.out)):
        feat, sums, out = _gap_launch(ops, hi, dev, det, k, which, dt)
        got = (feat if which == 0 else out)[PRE:PRE + want.numel()].cpu().double().view(want.shape)
        err = (got - want.to(dt).double()).abs()
        assert bool((err <= ax.ulp16(want, dt)).all()), (which, float(err.max()))
    feat, sums, out = _gap_launch(ops, hi, dev, det, k, 1, dt)
    kd = ax.deviation(sums, *r64["sums"])
    print("gap hw=49 sums: float32 CPU deviation %.3e, kernel %.3e (allowed %.3e)" % (d, kd, 4 * d))
    assert kd <= 4 * d, (kd, d)


# ----------------------------------------------------------------------------- layout + rounding (prep kernels)
@pytest.mark.parametrize("c_in", [1, 3])
def test_prep_input_is_bitwise(c_in):
    ops, hi, dev, det = cx.gpu_env()
    dt = ops.act_dtype()
    g = torch.Generator().manual_seed(16000 + c_in)
    x = torch.randn(5 * 7 * 5, c_in, generator=g)
    want = torch.zeros(x.shape[0], 8, dtype=torch.float64)
    want[:, :c_in] = x.to(dt).double()
    xd = x.to(dev)
    y, yp = out_buf(want.shape, dt, dev)
    run(ops.lib().dtf_cg_prep_input(xd.data_ptr(), yp, x.shape[0], c_in, ops.stream()))
    assert_whole(y, want, "prep_input")


@pytest.mark.parametrize("c_in,h,w", [(1, 4, 6), (4, 4, 6), (3, 6, 10)])
def test_prep_input_s2d_is_bitwise(c_in, h, w):
    """c_in 3: the 8-byte-load branch; c_in 1 and 4: the generic one.  Odd H is refused."""
    ops, hi, dev, det = cx.gpu_env()
    dt = ops.act_dtype()
    g = torch.Generator().manual_seed(16100 + c_in)
    x = torch.randn(3, h, w, c_in, generator=g)
    want = ax.s2d_blocks(x.to(dt).double())
    xd = x.to(dev)
    y, yp = out_buf(want.shape, dt, dev)
    run(ops.lib().dtf_cg_prep_input_s2d(xd.data_ptr(), yp, 3, h, w, c_in, ops.stream()))
    assert_whole(y, want, "prep_input_s2d")
    y2, yp2 = out_buf(want.shape, dt, dev)
    rc = ops.lib().dtf_cg_prep_input_s2d(xd.data_ptr(), yp2, 3, h - 1, w, c_in, ops.stream())
    torch.cuda.synchronize()
    assert rc == -2
    assert_whole(y2, torch.full_like(want, ax.CANARY), "refused launch")


def test_weight_prep_is_bitwise():
    """cg_weight_prep_kernel: the float4 row, the padded row (cin 3 -> 8), the unpadded scalar row, and the flipped /
    transposed data-gradient copy d[ci][tap][co] = W[co][kk - 1 - tap][ci]; the row with dgr_off < 0 writes none."""
    ops, hi, dev, det = cx.gpu_env()
    dt = ops.act_dtype()
    ax.check_weight_prep_table()
    g = torch.Generator().manual_seed(16200)
    state = torch.randn(ax.CAP, ax.WP_S, generator=g)
    wf_want, wd_want = ax.weight_prep_expected(state, dt)
    sd, table, slots = state.to(dev), i32(ax.WP_TABLE, dev), i32(ax.SLOTS, dev)
    wf, wfp = out_buf((ax.CAP, ax.WP_W), dt, dev)
    wd, wdp = out_buf((ax.CAP, ax.WP_W), dt, dev)
    run(ops.lib().dtf_cg_weight_prep(sd.data_ptr(), ax.WP_S, table.data_ptr(), len(ax.WP_TABLE), slots.data_ptr(),
                                     len(ax.SLOTS), wfp, wdp, ax.WP_W, ops.stream()))
    assert_whole(wf, wf_want, "forward shadow")
    assert_whole(wd, wd_want, "data-gradient shadow")
    assert torch.equal(sd.cpu(), state)


def test_dense_prep_is_bitwise():
    ops, hi, dev, det = cx.gpu_env()
    dt = ops.act_dtype()
    ncls, npad, c, w_off, s_stride, o_stride = 10, 16, 64, 12, 12 + 10 * 64 + 20, 16 * 64 + 32
    g = torch.Generator().manual_seed(16300)
    state = torch.randn(ax.CAP, s_stride, generator=g)
    want = torch.full((ax.CAP, o_stride), ax.CANARY, dtype=torch.float64)
    for s in ax.SLOTS:
        want[s, :npad * c] = 0
        want[s, :ncls * c] = state[s, w_off:w_off + ncls * c].to(dt).double()
    sd, slots = state.to(dev), i32(ax.SLOTS, dev)
    out, outp = out_buf(want.shape, dt, dev)
    run(ops.lib().dtf_cg_dense_prep(sd.data_ptr(), s_stride, w_off, ncls, npad, c, slots.data_ptr(), len(ax.SLOTS),
                                    outp, o_stride, ops.stream()))
    assert_whole(out, want, "dense shadow")


# ------------------------------------------------------------------------------------------------ BN finalize
def _untouched(got, before, live):
    mask = torch.ones_like(before, dtype=torch.bool)
    for idx in live:
        mask[idx] = False
    return torch.equal(got[mask], before[mask])


@pytest.mark.parametrize("hw", [4, 1])
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["forward", "backward", "eval"])
def test_bn_final_matches_float64(mode, hw):
    """cg_bn_fwd_final_kernel / cg_bn_bwd_final_kernel / cg_bn_eval_final_kernel: every coefficient row, the running
    statistics, the += into the gradient words; hw 4 with a constant channel (variance clamps to 0, inv = rsqrt(eps)),
    hw 1 with one image per member (n == 1: the unbiased variance is the biased one).  Tolerance 4 d, d the largest
    scaled deviation of the float32 CPU evaluation of the same formulas from float64."""
    ops, hi, dev, det = cx.gpu_env()
    L = ops.lib()
    k = ax.bnfin_case(hw)
    ax.check_bnfin(k)
    c, sl = k.c, list(ax.SLOTS)
    a = hi.BnFinArgs()
    assert ctypes.sizeof(a) == L.dtf_bnfin_args_size()
    state, coef, fcoef, grads = (t.float().to(dev) for t in (k.state, k.coef0, k.fcoef, k.grads0))
    sums = cx.acc_upload(k.bsums, cx.FX_GRAD, det, dev) if mode == 1 else cx.acc_upload(k.sums, cx.FX_STAT, det, dev)
    slots, cnt = i32(sl, dev), k.cnt.float().to(dev)
    a.state, a.s_mstride, a.sums, a.coef, a.fcoef = state.data_ptr(), ax.BNF_S, sums.data_ptr(), coef.data_ptr(), \
        fcoef.data_ptr()
    a.grads, a.g_mstride, a.slots, a.cnt = grads.data_ptr(), ax.BNF_S, slots.data_ptr(), cnt.data_ptr()
    a.gamma_off, a.beta_off, a.run_off, a.C, a.hw, a.cmax = ax.BNF_GAMMA, ax.BNF_BETA, ax.BNF_RUN, c, hw, ax.ACMAX
    run(L.dtf_cg_bn_final(ctypes.byref(a), mode, len(sl), ops.stream()))
    r64, r32 = ax.bnfin_eval(k, mode, torch.float64), ax.bnfin_eval(k, mode, torch.float32)
    d = max(ax.deviation(r32[n][0], r64[n][0], r64[n][1]) for n in r64)
    gc, gs, gg = coef.cpu().double(), state.cpu().double(), grads.cpu().double()
    where = {"c0": (gc, (sl, 0, slice(0, c))), "c1": (gc, (sl, 1, slice(0, c))), "c2": (gc, (sl, 2, slice(0, c))),
             "c3": (gc, (sl, 3, slice(0, c))),
             "run_mean": (gs, (sl, slice(ax.BNF_RUN, ax.BNF_RUN + c))),
             "run_var": (gs, (sl, slice(ax.BNF_RUN + c, ax.BNF_RUN + 2 * c))),
             "dgamma": (gg, (sl, slice(ax.BNF_GAMMA, ax.BNF_GAMMA + c))),
             "dbeta": (gg, (sl, slice(ax.BNF_BETA, ax.BNF_BETA + c)))}
    live = {id(gc): [], id(gs): [], id(gg): []}
    kd = {}
    for name, (ref, mag) in r64.items():
        t, idx = where[name]
        live[id(t)].append(idx)
        kd[name] = ax.deviation(t[idx], ref, mag)
    print("bn_final mode %d hw %d: float32 CPU deviation %.3e, allowed %.3e, kernel %s" % (
        mode, hw, d, 4 * d, " ".join("%s=%.3e" % kv for kv in sorted(kd.items()))))
    # everything the launch does not own is bit-identical: the unused slot, columns >= C, row 3 in the backward,
    # the state row around the running statistics, the gradient row around the gamma / beta words
    assert _untouched(gc, k.coef0, live[id(gc)]) and _untouched(gs, k.state, live[id(gs)])
    assert _untouched(gg, k.grads0, live[id(gg)])
    assert bool(torch.isfinite(gc).all()) and bool(torch.isfinite(gs).all())
    assert max(kd.values()) <= 4 * d, (kd, d)


# --------------------------------------------------------------------------------------- softmax cross-entropy
@pytest.mark.parametrize("form,loss_scale", [("train", 1.0), ("train", 128.0), ("eval", 1.0)])
@pytest.mark.parametrize("ncls,ld", ax.SM_SHAPES)
def test_softmax_ce_matches_float64(ncls, ld, form, loss_scale):
    """cg_softmax_ce_kernel.  Exact: the per-slot correct counts (ties: the lowest index wins), dl's padding columns,
    every word outside the bias gradient, and in the eval form (grads == dl == NULL) everything but loss and correct.
    Loss, dbias and dl: within 8 d of float64, d the largest scaled deviation of a float32 CPU log_softmax evaluation
    of the same outputs (the kernel uses __expf / __logf); dl, rounded to 16 bits, one more unit in its last place."""
    ops, hi, dev, det = cx.gpu_env()
    L, dt = ops.lib(), ops.act_dtype()
    k = ax.softmax_case(ncls, ld)
    ax.check_softmax(k)
    train = form == "train"
    logits, labels, slot = k.logits.float().to(dev), i32(k.labels.tolist(), dev), i32(ax.img_slots(k.sizes), dev)
    state, cnt, correct = k.state.float().to(dev), k.cnt.float().to(dev), k.correct0.float().to(dev)
    grads = cx.acc_upload(k.grads0, cx.FX_GRAD, det, dev)
    loss = cx.acc_upload(k.loss0, cx.FX_GRAD, det, dev)
    dl, dlp = out_buf((k.n, ld), dt, dev)
    run(L.dtf_cg_softmax_ce(logits.data_ptr(), ld, ncls, labels.data_ptr(), slot.data_ptr(), state.data_ptr(),
                            k.s_stride, ax.SM_B_OFF, grads.data_ptr() if train else None, k.s_stride, cnt.data_ptr(),
                            loss.data_ptr(), correct.data_ptr(), dlp if train else None, k.n, loss_scale,
                            ops.stream()))
    r64, r32 = ax.softmax_eval(k, loss_scale, torch.float64), ax.softmax_eval(k, loss_scale, torch.float32)
    d = max(ax.deviation(r32[n][0], r64[n][0], r64[n][1]) for n in r64)
    assert torch.equal(correct.cpu().double(), k.correct), (correct.cpu(), k.correct)
    gl, gg = acc64(loss, cx.FX_GRAD, det), acc64(grads, cx.FX_GRAD, det)
    assert bool(torch.isfinite(gl).all()) and gl[1] == k.loss0[1]
    kd = {"loss": ax.deviation(gl, *r64["loss"])}
    if train:
        b0, b1 = ax.SM_B_OFF, ax.SM_B_OFF + ncls
        assert torch.equal(gg[1], k.grads0[1]) and torch.equal(gg[:, :b0], k.grads0[:, :b0])
        assert torch.equal(gg[:, b1:], k.grads0[:, b1:])
        kd["dbias"] = ax.deviation(gg, *r64["dbias"])
        gd = dl[PRE:PRE + k.n * ld].cpu().double().view(k.n, ld)
        ref, mag = r64["dl"]
        assert bool((gd[:, ncls:] == 0).all())
        excess = ((gd - ref).abs() - ax.ulp16(ref, dt)).clamp(min=0)[:, :ncls] / mag[:, :ncls]
        kd["dl"] = float(excess.max())
        guard = dl.cpu().double()
        assert bool((guard[:PRE] == ax.CANARY).all()) and bool((guard[PRE + k.n * ld:] == ax.CANARY).all())
    else:
        assert torch.equal(gg, k.grads0)
        assert_whole(dl, torch.full((k.n, ld), ax.CANARY, dtype=torch.float64), "dl (eval form)")
    print("softmax %d/%d %s x%g: float32 CPU deviation %.3e, allowed %.3e, kernel %s" % (
        ncls, ld, form, loss_scale, d, 8 * d, " ".join("%s=%.3e" % kv for kv in sorted(kd.items()))))
    assert max(kd.values()) <= 8 * d, (kd, d)
