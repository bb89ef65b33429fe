"""The constructions of tests/_resnet_aux_exact.py, without a device: every bitwise case's reference satisfies its
exactness conditions (integrality, sums below 2^24, the exact-integer range of bfloat16 AND float16), every tolerant
case its ReLU / argmax margins with no element excluded, the mirrored launcher arithmetic puts each case on the path
it claims, and each reference agrees with a written-out loop over one small case -- so a GPU mismatch cannot be
blamed on the reference."""
import math

import pytest
import torch

import _resnet_aux_exact as rx

NREPS = (8, 64)


def test_prep_input_reference():
    for c_in, npix in rx.PREP_CASES[:2]:
        x = rx.prep_input_case(c_in, npix)
        assert npix % 256 != 0 and x.shape == (npix, c_in)
        for dt in rx.DTYPES:
            want = rx.prep_input_ref(x, dt)
            for p in (0, 7, npix - 1):
                for c in range(16):
                    assert float(want[p, c]) == (float(x[p, c].to(dt)) if c < c_in else 0.0)
            assert bool((want.float()[:, :c_in] != x).any())  # roundings occur
    assert rx.PREP_CASES[2][1] > 4096 * 256 and {c for c, _ in rx.PREP_CASES} == {1, 3}


def test_weight_prep_table_and_reference():
    rx.check_weight_prep_table()
    st = rx.weight_prep_state()
    assert bool(torch.isnan(st[rx.IDLE]).all())
    for dt in rx.DTYPES:
        wf, wd = rx.weight_prep_expected(st, dt)
        assert bool((wf[rx.IDLE] == rx.CANARY).all()) and bool((wd[rx.IDLE] == rx.CANARY).all())
        s = 2
        for w_off, cout, cin, k, cin_pad, fwd_off, dgr_off, _ in rx.WP_TABLE:
            kk = k * k
            for co in (0, cout - 1):
                for tap in (0, kk - 1):
                    for ci in (0, cin - 1, cin_pad - 1):
                        src = float(st[s, w_off + (co * kk + tap) * cin + ci].to(dt)) if ci < cin else 0.0
                        assert float(wf[s, fwd_off + (co * kk + tap) * cin_pad + ci]) == src
                        if dgr_off >= 0 and ci < cin:
                            assert float(wd[s, dgr_off + (ci * kk + tap) * cout + co]) == src
        # nothing is written to wd for the row without a dgrad copy: wd's written words are exactly the other rows'
        n_d = sum(r[1] * r[2] * r[3] ** 2 for r in rx.WP_TABLE if r[6] >= 0)
        assert int((wd[s] != rx.CANARY).sum()) <= n_d and int((wd[s] != rx.CANARY).sum()) > n_d - 8


def test_work_gen_reference_meets_the_contract():
    from distributedtf_amd.engine import hip_resnet as hr
    seen = set()
    for d in rx.WG_DESCS:
        per, bands, min_chunk, split, prop, red = d
        table, redt = rx.work_gen_ref(d, hr.elastic_rows)
        rx.check_work_table(d, table, redt)
        assert all(w != rx.ICANARY for row in table for w in row)  # the members' rows cover the table
        totals = [int(rx.WG_CNT[s]) * bands for s in rx.WG_SLOTS]
        rows = hr.elastic_rows(totals, per, min_chunk, prop)
        R, M = per * len(totals), len(totals)
        fixed = not (prop and R > M)
        if not fixed:
            computed = -(-sum(totals) // (R - M))
            seen.add("min_above" if min_chunk > computed else "min_below")
            if rows[-1][1] > 256:
                seen.add("thread_loop")
        elif prop:
            seen.add("per1_fallback")
        seen.add(("prop", prop))
        seen.add(("split", split))
        seen.add(("red", red))
        seen.add(("bands", bands))
        assert any(nit == 0 for _, nit, _, _ in table)  # the member without images has only empty rows
    need = {"min_above", "min_below", "thread_loop", "per1_fallback"} | {(k, v) for k in ("prop", "split", "red")
                                                                        for v in (0, 1)} | {("bands", 1), ("bands", 4)}
    assert need <= seen, need - seen
    # written out: 5 images x 1 band over 2 rows of chunk 4 (descriptor 4): rows (0, 4) and (4, 1)
    table, redt = rx.work_gen_ref(rx.WG_DESCS[4], hr.elastic_rows)
    assert table[0] == [0, 4, 0, 0] and table[1] == [4, 1, 0, 0] and table[2] == [160, 0, 0, 3]
    assert table[3] == [320, 4, 0, 2] and table[3 + 32] == [320 + 128, 3, 0, 2] and table[3 + 33] == [320, 0, 0, 2]
    assert redt == [[0, 2, 0, 0], [2, 1, 0, 3], [3, 297, 0, 2]]


@pytest.mark.parametrize("nrep", NREPS)
def test_bn_eval_and_step_end_constructions(nrep):
    k = rx.bn_eval_case(nrep)
    rx.check_bn_eval(k)
    run_off, c, hw, si, _, _, _, _ = rx.BN_TABLE[0]
    o = rx.BN_RUN_BASE + run_off
    for ch in (0, c - 1):
        m, v = float(k.state[2, o + ch]), float(k.state[2, o + c + ch])
        assert float(k.stats[si, 2, 0, 0, ch]) == 2 * hw * m and float(k.stats[si, 2, 0, 1, ch]) == 2 * hw * (v + m * m)
    for n1 in (False, True):
        e = rx.bn_end_case(nrep, n1)
        rx.check_bn_end(e)
        run_off, c, hw, si, go, bo, _, _ = e.table[1]
        s, ch = 0, 7
        assert float(e.grads[s, go + ch]) == float(e.grads0[s, go + ch]) + sum(float(e.stb[si, s, r, 1, ch]) for r in range(nrep))
        assert float(e.grads[s, bo + ch]) == float(e.grads0[s, bo + ch]) + sum(float(e.stb[si, s, r, 0, ch]) for r in range(nrep))
        r64, r32 = rx.bn_running_eval(e, torch.float64), rx.bn_running_eval(e, torch.float32)
        n = float(e.cnt[s]) * hw
        sm = sum(float(e.stf[si, s, r, 0, ch]) for r in range(nrep))
        q = sum(float(e.stf[si, s, r, 1, ch]) for r in range(nrep))
        mean = sm / n
        var = max(q / n - mean * mean, 0.0)
        unb = var * n / (n - 1) if n > 1 else var
        o = rx.BN_RUN_BASE + run_off
        assert math.isclose(float(r64[(1, s)][0][ch]), rx.BN_MOM * float(e.state0[s, o + ch]) + rx.BN_ONE_M * mean, rel_tol=1e-13)
        assert math.isclose(float(r64[(1, s)][2][ch]), rx.BN_MOM * float(e.state0[s, o + c + ch]) + rx.BN_ONE_M * unb,
                            rel_tol=1e-13)
        d = max(max(rx.deviation(r32[key][0], r64[key][0], r64[key][1]), rx.deviation(r32[key][2], r64[key][2], r64[key][3]))
                for key in r64)
        assert d < 1e-5, d
        if not n1:
            assert bool((r64[(0, 0)][2] != rx.bn_running_eval(_biased(e), torch.float64)[(0, 0)][2]).any())


def _biased(e):
    """The same case with every count doubled: a reference that used another n gives other values (the yardstick
    cannot hide an n for n - 1 slip)."""
    k = rx.Case()
    k.__dict__.update(e.__dict__)
    k.cnt = e.cnt * 2
    return k


def test_elementwise_launch_mirrors():
    n = sum(rx.SIZES)
    geo = {(c, hw): (rx.ew_split(hw, c, n), rx.ew_chunks(hw, c, n), rx.ew_wraps(hw, c, n)) for c, hw, _ in rx.BWD_APPLY_CASES}
    assert geo[(16, 64)][0] == 1 and 0 in geo[(16, 64)][1] and geo[(16, 64)][2]  # threads without a chunk, c0 wraps
    assert geo[(16, 256)][0] == 2 and geo[(32, 256)][0] == 4 and geo[(64, 64)][0] == 2 and geo[(16, 256)][2]
    assert all(max(ch) == 1 for _, ch, _ in geo.values())
    assert {c for c, _, _ in rx.BWD_APPLY_CASES} == {16, 32, 64} and {a for _, _, a in rx.BWD_APPLY_CASES} == {0, 1}
    # bn_bwd_reduce: trips of the two-chunk loop on the atomic builds; one workgroup per image on the slab form
    trips = {}
    for c, hw, two, sizes, el in rx.REDUCE_CASES:
        nimg = 2 * rx.ELASTIC_CAP if el else sum(sizes)
        trips[(c, hw, nimg)] = (rx.ew_split(hw, c, nimg), rx.ew_chunks(hw, c, nimg, pair=True))
        assert rx.ew_split(hw, c, nimg, det_slab=True) == 1
    assert trips[(16, 64, 5)][0] == 1 and [] in trips[(16, 64, 5)][1]
    assert trips[(16, 256, 5)][0] == 2
    sp, tr = trips[(32, 192, 2048)]
    assert sp == 1 and all(t == [2, 1] for t in tr) and 32 * 192 // 8 == 768
    assert {(c, two) for c, _, two, _, _ in rx.REDUCE_CASES} >= {(16, 0), (16, 1), (32, 1), (64, 0), (64, 1)}
    assert any(el for *_, el in rx.REDUCE_CASES)
    big = 2048 * 192 * 32 * 2
    assert big < 32 * 2 ** 20  # tens of MB per tensor


@pytest.mark.parametrize("nrep", NREPS)
def test_bn_bwd_apply_constructions(nrep):
    for c, hw, add in rx.BWD_APPLY_CASES:
        k = rx.bwd_apply_case(c, hw, add, nrep)
        rx.check_bwd_apply(k)
        o64, mag = rx.bwd_apply_eval(k, torch.float64)
        o32, _ = rx.bwd_apply_eval(k, torch.float32)
        assert rx.deviation(o32, o64, mag) < 1e-5
    # written out for one element
    k = rx.bwd_apply_case(16, 64, 1, nrep)
    o64, _ = rx.bwd_apply_eval(k, torch.float64)
    img, p, ch, s = 4, 9, 6, 2
    n = 2.0 * 64
    sm, q, sd, sdx = (sum(float(t[s, r, row, ch]) for r in range(nrep)) for t, row in ((k.stf, 0), (k.stf, 1), (k.stb, 0), (k.stb, 1)))
    mean = sm / n
    inv = 1 / math.sqrt(max(q / n - mean * mean, 0.0) + rx.BN_EPS)
    scale = float(k.params[s, k.gamma_off + ch]) * inv
    want = scale * float(k.dz[img, p, ch]) - scale * inv * (sdx / n) * float(k.x[img, p, ch]) - scale * (sd / n) + \
        scale * inv * mean * (sdx / n) + float(k.add[img, p, ch])
    assert math.isclose(float(o64[img, p, ch]), want, rel_tol=1e-12, abs_tol=1e-12)


@pytest.mark.parametrize("nrep", NREPS)
def test_bn_add_relu_constructions(nrep):
    for c, hw, form in rx.ADD_RELU_CASES:
        k = rx.add_relu_case(c, hw, form, nrep)
        d = rx.check_add_relu(k)
        assert d < 1e-5
        assert int(k.real.sum()) == sum(rx.SIZES) and len(k.slot) == 2 * rx.ELASTIC_CAP
    assert {f for _, _, f in rx.ADD_RELU_CASES} == {0, 1, 2} and {c for c, _, _ in rx.ADD_RELU_CASES} == {16, 64}
    k = rx.add_relu_case(16, 64, 2, nrep)
    v64, _ = rx.add_relu_eval(k, torch.float64)
    img, p, ch, s = 5, 3, 9, 2  # member 1's second image
    n = 2.0 * 64
    val = 0.0
    for st, pair, h in ((k.st1, 0, k.h1), (k.st2, 1, k.h2)):
        sm, q = (sum(float(st[s, r, row, ch]) for r in range(nrep)) for row in (0, 1))
        mean = sm / n
        inv = 1 / math.sqrt(max(q / n - mean * mean, 0.0) + rx.BN_EPS)
        go, bo = k.offs[pair]
        scale = float(k.params[s, go + ch]) * inv
        val += float(h[img, p, ch]) * scale + float(k.params[s, bo + ch]) - mean * scale
    assert math.isclose(float(v64[img, p, ch]), val, rel_tol=1e-12, abs_tol=1e-12)


@pytest.mark.parametrize("nrep", NREPS)
def test_bn_bwd_reduce_constructions(nrep):
    for c, hw, two, sizes, el in rx.REDUCE_CASES[:-1]:
        k = rx.reduce_case(c, hw, two, sizes, el, nrep)
        rx.check_reduce(k)
        r64, r32 = rx.reduce_eval(k, torch.float64), rx.reduce_eval(k, torch.float32)
        assert torch.equal(r32["sd"][0].double(), r64["sd"][0]) and torch.equal(r32["img_sd"].double(), r64["img_sd"])
        assert rx.ax.is_int(r64["sd"][0]) and rx.deviation(r32["x1"][0], *r64["x1"]) < 1e-5
        assert torch.equal(r64["sd"][0][rx.IDLE], k.seed1[rx.IDLE, :, 0].sum(0))
        if not two:
            assert torch.equal(r64["x2"][0], k.seed2[:, :, 1].sum(1)) and torch.equal(r64["sd2"], k.seed2[:, :, 0].sum(1))
    k = rx.reduce_case(16, 64, 0, rx.SIZES, 0, nrep)
    r64 = rx.reduce_eval(k, torch.float64)
    s, ch = 2, 11
    n = 2.0 * 64
    sm, q = (sum(float(k.st1[s, r, row, ch]) for r in range(nrep)) for row in (0, 1))
    mean = sm / n
    inv = 1 / math.sqrt(max(q / n - mean * mean, 0.0) + rx.BN_EPS)
    sd = float(k.seed1[s, :, 0, ch].sum())
    sx = float(k.seed1[s, :, 1, ch].sum())
    for img in (3, 4):
        for p in range(64):
            sd += float(k.d[img, p, ch])
            sx += float(k.d[img, p, ch]) * (float(k.h1[img, p, ch]) * inv - mean * inv)
    assert float(r64["sd"][0][s, ch]) == sd and math.isclose(float(r64["x1"][0][s, ch]), sx, rel_tol=1e-11, abs_tol=1e-11)


@pytest.mark.parametrize("nrep", NREPS)
def test_head_constructions(nrep):
    for hw, ncls, v2 in sorted({(h, n, v) for h, n, v, *_ in rx.HEAD_CASES}):
        k = rx.head_case(hw, ncls, v2, nrep)
        rx.check_head(k)
        for ls in (1.0, 128.0):
            r64, r32 = rx.head_eval(k, ls, torch.float64), rx.head_eval(k, ls, torch.float32)
            t64, t32 = rx.head_totals(k, r64, nrep), rx.head_totals(k, r32, nrep)
            for name in t64:
                assert rx.deviation(t32[name][0], *t64[name]) < 1e-4, name
    assert {h for h, *_ in rx.HEAD_CASES} == {32, 64, 128} and {c[1] for c in rx.HEAD_CASES} == {10, 16}
    assert {(c[2], c[3]) for c in rx.HEAD_CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(c[4], c[5]) for c in rx.HEAD_CASES if c[3]} == {(1.0, 0), (1.0, 1), (128.0, 0), (128.0, 1)}
    # written out: image 7 of the v1 case (slot 2)
    k = rx.head_case(32, 16, 0, nrep)
    r = rx.head_eval(k, 1.0, torch.float64)
    img, s = 7, 2
    feat = [sum(max(float(k.x[img, p, c]), 0.0) for p in range(32)) / 32 for c in range(64)]
    lg = [sum(float(k.params[s, rx.HEAD_DW + j * 64 + c]) * feat[c] for c in range(64)) + float(k.params[s, rx.HEAD_DB + j])
          for j in range(16)]
    assert [float(v) for v in r["logits"][0][img]] == lg
    lse = math.log(sum(math.exp(v - max(lg)) for v in lg)) + max(lg)
    assert math.isclose(float(r["li"][img]), lse - lg[int(k.labels[img])], rel_tol=1e-12)
    j, c = 3, 17
    dfe = sum((math.exp(lg[jj] - lse) - (jj == int(k.labels[img]))) / 4.0 * float(k.params[s, rx.HEAD_DW + jj * 64 + c])
              for jj in range(16)) / 32
    assert math.isclose(float(r["dfeat"][0][img, c]), dfe, rel_tol=1e-11, abs_tol=1e-14)
    item = 3  # (7, 1, 0, 2)
    assert math.isclose(float(r["dw"][0][item][j, c]), (math.exp(lg[j] - lse) - (j == int(k.labels[img]))) / 4.0 * feat[c],
                        rel_tol=1e-11, abs_tol=1e-14)
    assert math.isclose(float(r["sdz"][0][item][c]), dfe * sum(float(k.x[img, p, c]) > 0 for p in range(32)), rel_tol=1e-11,
                        abs_tol=1e-14)


@pytest.mark.parametrize("nrep", NREPS)
def test_head_bwd_apply_constructions(nrep):
    for hw, v2 in rx.HEAD_BWD_CASES:
        k = rx.head_bwd_case(hw, v2, nrep)
        rx.check_head_bwd(k)
    assert {h for h, _ in rx.HEAD_BWD_CASES} == {32, 64} and {v for _, v in rx.HEAD_BWD_CASES} == {0, 1}
    k = rx.head_bwd_case(32, 0, nrep)
    o = rx.head_bwd_eval(k, torch.float64)[0]
    assert float(o[4, 5, 6]) == (float(k.dfeat[4, 6]) if float(k.x[4, 5, 6]) > 0 else 0.0)


def test_step_and_shadow_constructions():
    for n in (2, 70):
        k = rx.step_case(n)
        assert k.hyper[0, 7] == 0 and 0 in k.slots and 1 not in k.slots and k.slots[0] == k.cap - 1
        st, hy, sel = rx.step_expected(k, 4)
        assert float(st[0, k.col]) == float(k.state[0, k.col]) and float(st[2, k.col]) == float(k.state[2, k.col]) + 4
        assert float(hy[2, k.h_step]) == float(k.hyper[2, k.h_step]) + 4 and torch.equal(st[1], k.state[1])
        assert sel.tolist() == [float(k.loss[s]) for s in k.slots] and rx.ax.is_int(k.loss * 8)
    assert rx.step_case(2).slots == [2, 0] and rx.step_case(70).cap > 64
    assert rx.SHADOW_P % 4 == 0 and rx.SHADOW_P > 512 * 1024
    for dt in rx.DTYPES:
        v = rx.shadow_values(4096, dt, 5)
        r = v.to(dt).float()
        ties = (v - r).abs().double() == rx.ax.ulp16(v.double(), dt) / 2
        assert int(ties.sum()) >= 1024 and bool((r != v).any()) and bool(torch.isfinite(r).all())
        up = v.double().abs() + rx.ax.ulp16(v.double(), dt) / 2  # a tie rounds to the even neighbour, up or down
        assert bool((r.abs().double()[ties] == up[ties]).any()) and bool((r.abs().double()[ties] != up[ties]).any())


def test_optimizer_constructions():
    for P, n_reg in ((1002, 701), (1002, 0), (1002, 1002), (530, 305)):
        k = rx.opt_case(P, n_reg)
        rx.check_opt(k)
        assert P % 4 == 2 and k.Pp % 64 == 0 and k.Pp - k.p4 >= 64 and k.S > 3 * k.Pp
    assert 701 % 4 == 1 and 305 % 4 == 1 and 530 < 1024
    kd = rx.opt_case(1002, 701, dyadic=True)
    rx.check_opt(kd)
    # written out per optimizer for one regularised element of each member
    k = rx.opt_case(1002, 701)
    st, _ = rx.opt_eval(k, 1 / 128, torch.float64)
    f = rx.F32
    for s in rx.OPT_MEMBERS:
        code, lr, mom, dec, wd, reg, t, _ = k.hyper[s].tolist()
        i = 3
        assert k.state[s, i] != 0
        w, a, b = float(k.state[s, i]), float(k.state[s, k.Pp + i]), float(k.state[s, 2 * k.Pp + i])
        g = float(k.grads[s, i]) / 128
        if reg in (2, 3):
            g += wd * w
        if reg in (1, 3):
            g += wd * math.copysign(1.0, w)
        if code == 0:
            w -= lr * g
        elif code == 1:
            a = mom * a + g
            w -= lr * a
        elif code == 2:
            lr_t = lr * math.sqrt(1 - f(0.999) ** t) / (1 - f(0.9) ** t)
            a, b = f(0.9) * a + f(0.1) * g, f(0.999) * b + f(0.001) * g * g
            w -= lr_t * a / (math.sqrt(b) + f(1e-8))
        elif code == 3:
            a += g * g
            w -= lr * g / math.sqrt(a)
        elif code == 4:
            a = f(0.95) * a + f(0.05) * g * g
            u = math.sqrt(b + f(1e-8)) / math.sqrt(a + f(1e-8)) * g
            b = f(0.95) * b + f(0.05) * u * u
            w -= lr * u
        else:
            a = dec * a + (1 - dec) * g * g
            b = mom * b + lr * g / math.sqrt(a + f(1e-10))
            w -= b
        own = rx.OWNS[int(code)]
        assert math.isclose(float(st[s, i]), w, rel_tol=1e-12)
        assert math.isclose(float(st[s, k.Pp + i]), a if own[0] else float(k.state[s, k.Pp + i]), rel_tol=1e-12)
        assert math.isclose(float(st[s, 2 * k.Pp + i]), b if own[1] else float(k.state[s, 2 * k.Pp + i]), rel_tol=1e-12)
    # an unregularised element (past n_reg) and the inactive row
    assert torch.equal(st[rx.OPT_INACTIVE], k.state[rx.OPT_INACTIVE])
    s = 5
    assert math.isclose(float(st[s, 900]), float(k.state[s, 900]) - float(k.hyper[s, 1]) * float(k.grads[s, 900]) / 128, rel_tol=1e-12)
