"""Fused population optimizer kernel vs the PyTorch fp32 reference (engine/optim.py)."""
import pytest
import torch

from distributedtf_amd.engine import optim as O

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("opt", list(O.OPT_CODES))
@pytest.mark.parametrize("reg", [None, "l1_regularizer", "l2_regularizer", "l1_l2_regularizer"])
def test_fused_optimizer_matches_reference(opt, reg):
    from distributedtf_amd import ops
    torch.manual_seed(0)
    G, P, n_reg = 3, 1000, 700
    Pp = 1024
    S = 3 * Pp + 64
    dev = "cuda"
    state = torch.randn(G, S, device=dev)
    s1i, s2i = O.slot_init_values(opt)
    state[:, Pp:2 * Pp] = state[:, Pp:2 * Pp].abs() + s1i + 0.05  # keep second-moment slots positive
    state[:, 2 * Pp:3 * Pp] = state[:, 2 * Pp:3 * Pp].abs() * 0.1 + s2i
    grads = torch.randn(G, Pp, device=dev)
    hp = {"opt_case": {"optimizer": opt, "lr": 0.01, "momentum": 0.7, "grad_decay": 0.8},
          "weight_decay": 1e-3, "regularizer": reg}
    hyper = torch.tensor([O.hyper_row(hp, 0.01 * (g + 1), 3 + g, active=(g != 1)) for g in range(G)],
                         device=dev, dtype=torch.float32)
    ref = state.clone()
    O.apply_reference(ref[:, :P], grads[:, :P], ref[:, Pp:Pp + P], ref[:, 2 * Pp:2 * Pp + P], hyper, n_reg)
    shadow = torch.zeros(G, Pp, dtype=torch.bfloat16, device=dev)
    g2 = grads.clone()
    ops.fused_optimizer(state, g2, hyper, Pp, P, n_reg, shadow=shadow, zero_grads=True)
    torch.cuda.synchronize()
    for g in range(G):
        for a, b in [(0, P), (Pp, Pp + P), (2 * Pp, 2 * Pp + P)]:
            torch.testing.assert_close(state[g, a:b], ref[g, a:b], rtol=2e-5, atol=2e-6)
    act = [0, 2]
    torch.testing.assert_close(shadow[act, :P].float(), state[act, :P].bfloat16().float())
    assert float(g2[act, :P].abs().sum()) == 0.0
    assert torch.equal(g2[1], grads[1])  # inactive member untouched


# ----------------------------------------------------------------------------------------------------------------
# Kernel-level tests against the float64 references of tests/_resnet_aux_exact.py: one launch with a different
# optimizer per member, whole guarded state / shadow / gradient buffers, the step counters, the loss ring and the
# shadow refresh.
import ctypes  # noqa: E402

import _resnet_aux_exact as rx  # noqa: E402

_PRE = rx.PRE


def _guarded(t, dt, dev):
    """(flat device buffer inside guards, its live region viewed with t's shape, host copy of the flat buffer)."""
    h = rx.guarded(t, dt)
    d = h.to(dev)
    return d, d[_PRE:_PRE + t.numel()].view(t.shape), h


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _opt_launch(k, gscale, with_shadow, zero_grads):
    from distributedtf_amd import ops
    dev, dt = "cuda", ops.act_dtype()
    sbuf, state, _ = _guarded(k.state, torch.float32, dev)
    gbuf, grads, gh = _guarded(k.grads, torch.float32, dev)
    hbuf, hyper, hh = _guarded(k.hyper, torch.float32, dev)
    shbuf, shadow, _ = _guarded(torch.full((rx.OPT_G, k.Pp), rx.CANARY, dtype=torch.float64), dt, dev)
    ops.fused_optimizer(state, grads, hyper, k.Pp, k.P, k.n_reg, shadow=shadow if with_shadow else None,
                        zero_grads=zero_grads, grad_scale=gscale)
    torch.cuda.synchronize()
    assert torch.equal(_bits(hbuf.cpu()), _bits(hh)), "hyper table written"
    for buf, n in ((sbuf, k.state.numel()), (gbuf, k.grads.numel()), (shbuf, rx.OPT_G * k.Pp)):
        assert rx.guards_intact(buf.cpu(), n), "guard words written"
    got = state.cpu()
    act = [s for s in range(rx.OPT_G) if k.hyper[s, 7] != 0]
    # the shadow is the 16-bit rounding of the kernel's own fp32 weights over [0, ceil4(P)) of the active rows
    sh_want = torch.full((rx.OPT_G, k.Pp), rx.CANARY, dtype=torch.float32).to(dt)
    if with_shadow:
        sh_want[act, :k.p4] = got[act, :k.p4].to(dt)
    assert torch.equal(_bits(shadow.cpu()), _bits(sh_want)), "shadow"
    g_want = k.grads.float()
    if zero_grads:
        g_want[act, :k.p4] = 0.0
    assert torch.equal(_bits(grads.cpu()), _bits(g_want)), "gradients"
    return got.double(), act


OPT_LAUNCHES = [(1002, 701, 1.0, True, True), (512 * 1024 + 1002, 300001, 1 / 128, True, True), (530, 305, 1.0, True, True),
                (1002, 0, 1.0, True, True), (1002, 1002, 1 / 128, True, True), (1002, 701, 1.0, False, True),
                (1002, 701, 1 / 128, True, False)]


@pytest.mark.parametrize("P,n_reg,gscale,with_shadow,zero_grads", OPT_LAUNCHES)
def test_fused_optimizer_mixed_population(P, n_reg, gscale, with_shadow, zero_grads):
    """One launch of G = 7: codes 0 .. 5 on six scattered members, each with its own lr / momentum / decay / wd /
    regularizer / step (Adam at t = 1), and one inactive member; P % 4 == 2 and n_reg % 4 == 1 (the regularizer boundary
    and the end of the row fall inside a float4), P above 512 x 1024 (a second grid-stride trip) and below 1024.
    Reference: float64, written out per optimizer; yardstick: the same at float32; the kernel may deviate 4 x as much
    (8 x for the Adam member: powf).  Bitwise (deviation() demands equality where no term stands behind a word): the
    columns [P, Pp) of every region -- the lanes of the last float4 past P keep their words, which the engine leaves
    zero (Adagrad's 0 * rsqrt(0) there would be NaN) --, the slot regions the optimizer does not own, the tail
    [3 Pp, S), the inactive member's state, shadow and gradients, shadow == 16-bit(new w), zeroed / kept gradients."""
    k = rx.opt_case(P, n_reg)
    rx.check_opt(k)
    assert P % 4 == 2 and n_reg % 4 in ((1,) if 0 < n_reg < P else (0, 1, 2))
    got, act = _opt_launch(k, gscale, with_shadow, zero_grads)
    st64, mag = rx.opt_eval(k, gscale, torch.float64)
    st32, _ = rx.opt_eval(k, gscale, torch.float32)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got[rx.OPT_INACTIVE], k.state[rx.OPT_INACTIVE])
    lines, ok = [], True
    for s in act:
        code = int(k.hyper[s, 0])
        factor = rx.FACTOR_EXP if code == 2 else rx.FACTOR_RSQRT
        kd, d = rx.deviation(got[s], st64[s], mag[s]), rx.deviation(st32[s], st64[s], mag[s])
        lines.append("code %d kernel %.3e float32 %.3e (allowed %.3e)" % (code, kd, d, factor * d))
        ok = ok and kd <= factor * d
    print("fused_optimizer P=%d n_reg=%d gscale=%g: %s" % (P, n_reg, gscale, "; ".join(lines)))
    assert ok, lines


@pytest.mark.parametrize("n_reg", [701, 0])
def test_fused_optimizer_gd_and_momentum_are_bitwise(n_reg):
    """Codes 0 and 1 with l1_l2 / l1 on dyadic w, g, lr, momentum, wd and gradient scale (zeros among the weights:
    sign(0) = 0): every product and sum is exact at fp32, so the whole state rows equal the float64 reference."""
    k = rx.opt_case(1002, n_reg, dyadic=True)
    rx.check_opt(k)
    got, act = _opt_launch(k, 0.5, True, True)
    st64, _ = rx.opt_eval(k, 0.5, torch.float64)
    assert torch.equal(got, st64), int((got != st64).sum())


def _step_bufs(k, dev):
    return (_guarded(k.state, torch.float32, dev), _guarded(k.hyper, torch.float32, dev),
            torch.tensor(k.slots, dtype=torch.int32, device=dev), _guarded(k.loss, torch.float32, dev))


def _whole(buf, want, dt, what):
    assert torch.equal(_bits(buf.cpu()), _bits(rx.guarded(want, dt))), what


@pytest.mark.parametrize("n", [2, 70])
def test_step_advance_and_step_end(n):
    """step_advance_kernel: the state counter column and the hyper step column advance for active listed members only
    (slot list [2, 0] of capacity 3, member 0 inactive; n = 70: two waves in the ring form's single block); loss_sel in
    slot-list order; ring_rows 3 and four calls write rows 0, 1, 2, 0 and leave ring_idx at 4."""
    from distributedtf_amd import ops
    L, dev = ops.lib(), "cuda"
    k = rx.step_case(n)
    (sb, st, _), (hb, hy, _), slots, (lb, loss, _) = _step_bufs(k, dev)
    assert L.dtf_step_advance(st.data_ptr(), k.S, k.col, hy.data_ptr(), k.h_step, slots.data_ptr(), n, ops.stream()) == 0
    torch.cuda.synchronize()
    st1, hy1, sel = rx.step_expected(k, 1)
    _whole(sb, st1, torch.float32, "state after step_advance")
    _whole(hb, hy1, torch.float32, "hyper after step_advance")
    # step_end without a ring: the gather only
    selb, sel_d, _ = _guarded(torch.full((n,), rx.CANARY, dtype=torch.float64), torch.float32, dev)
    assert L.dtf_step_end(st.data_ptr(), k.S, k.col, hy.data_ptr(), k.h_step, slots.data_ptr(), n, loss.data_ptr(),
                          sel_d.data_ptr(), None, None, 1, ops.stream()) == 0
    torch.cuda.synchronize()
    st2, hy2, _ = rx.step_expected(k, 2)
    _whole(sb, st2, torch.float32, "state after step_end")
    _whole(selb, sel, torch.float32, "loss_sel")
    # four ring calls, the losses scaled by the call number
    ringb, ring, _ = _guarded(torch.full((3, n), rx.CANARY, dtype=torch.float64), torch.float32, dev)
    idx = torch.zeros(1 + 2 * _PRE, dtype=torch.int32, device=dev)
    want = torch.full((3, n), rx.CANARY, dtype=torch.float64)
    for call in range(4):
        loss.copy_((k.loss * (call + 1)).float())
        assert L.dtf_step_end(st.data_ptr(), k.S, k.col, hy.data_ptr(), k.h_step, slots.data_ptr(), n, loss.data_ptr(),
                              sel_d.data_ptr(), ring.data_ptr(), idx.data_ptr() + 4 * _PRE, 3, ops.stream()) == 0
        torch.cuda.synchronize()
        want[call % 3] = sel * (call + 1)
        _whole(ringb, want, torch.float32, "ring after call %d" % call)
        _whole(selb, sel * (call + 1), torch.float32, "loss_sel after call %d" % call)
    exp_idx = torch.zeros_like(idx.cpu())
    exp_idx[_PRE] = 4
    assert torch.equal(idx.cpu(), exp_idx)
    st6, hy6, _ = rx.step_expected(k, 6)
    _whole(sb, st6, torch.float32, "state after six calls")
    _whole(hb, hy6, torch.float32, "hyper after six calls")
    # refused ring launches write nothing
    for nn, ip, rows in ((1025, idx.data_ptr() + 4 * _PRE, 3), (n, None, 3), (n, idx.data_ptr() + 4 * _PRE, 0)):
        rc = L.dtf_step_end(st.data_ptr(), k.S, k.col, hy.data_ptr(), k.h_step, slots.data_ptr(), nn, loss.data_ptr(),
                            sel_d.data_ptr(), ring.data_ptr(), ip, rows, ops.stream())
        torch.cuda.synchronize()
        assert rc == -2, rc
    _whole(sb, st6, torch.float32, "state after refused launches")
    _whole(ringb, want, torch.float32, "ring after refused launches")
    assert torch.equal(idx.cpu(), exp_idx)


def test_shadow_refresh_is_bitwise():
    """shadow_refresh_kernel over rows [2, 0] of 3 with P above 512 x 1024 (second grid-stride trip): every second
    value is a round-to-nearest-even tie of the 16-bit type; the unlisted row keeps its canaries."""
    from distributedtf_amd import ops
    dev, dt = "cuda", ops.act_dtype()
    P = rx.SHADOW_P
    Pp, S = P + 64, P + 64 + 8
    state = torch.full((3, S), rx.NAN, dtype=torch.float32)
    for s in (0, 2):
        state[s, :P] = rx.shadow_values(P, dt, 30 + s)
    sbuf, sd, sh = _guarded(state, torch.float32, dev)
    shb, shadow, _ = _guarded(torch.full((3, Pp), rx.CANARY, dtype=torch.float64), dt, dev)
    ops.shadow_refresh(sd, shadow, [2, 0], Pp, P)
    torch.cuda.synchronize()
    want = torch.full((3, Pp), rx.CANARY, dtype=torch.float32).to(dt)
    want[[0, 2], :P] = state[[0, 2], :P].to(dt)
    assert torch.equal(_bits(shb.cpu()), _bits(rx.guarded(want, dt))), "shadow"
    assert torch.equal(_bits(sbuf.cpu()), _bits(sh)), "state written"
