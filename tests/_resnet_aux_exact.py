"""Constructions and float64 CPU references for the kernel-level tests of the CIFAR auxiliary kernels
(ops/csrc/resnet_aux.hip) and of ops/csrc/optim.hip, built without a device.  Used by tests/test_gpu_resnet_aux.py,
tests/test_gpu_optimizer.py and, for the conditions themselves, tests/test_resnet_aux_constructions.py.

The pattern is that of tests/_conv_exact.py and tests/_convg_aux_exact.py, whose helpers are reused.  Members sit in
slots 0 and 2 of a capacity-3 population (capacity 4 where a listed member without images is needed: the kernel then
reads that slot's ``cnt``), images packed ragged (3 + 2); the idle slot's params, statistics and ``cnt`` are NaN.

Bitwise cases use integer or dyadic operands whose partial sums stay below 2^24 and inside the exact-integer range
of bf16 and fp16, so the result does not depend on the order of summation or on FMA contraction.  The kernels that
use rsqrtf / __expf / __logf / division are evaluated by one formula at float64 (the reference) and at float32 (the
yardstick): ``deviation`` scales every error by the summed magnitude of the terms behind the element, and the
kernel may deviate by FACTOR_RSQRT = 4 (FACTOR_EXP = 8 where __expf / __logf / powf enter) times the yardstick's
deviation.  A 16-bit output is accepted iff it lies between the 16-bit roundings of ref - tol and ref + tol.
Statistics are [CAP][nrep][2][64] fp32 words (row 0: sums, row 1: sums of squares / xhat sums); the references read
the same fp32 words the kernel reads, and the float32 yardstick adds the replicas in the kernel's order.
"""
import functools

import torch

import _conv_exact as kx
import _convg_aux_exact as ax
from _conv_exact import guarded, guards_intact, live, PRE  # noqa: F401 (re-exported)
from _convg_aux_exact import deviation  # noqa: F401
from _convg_exact import EXACT, INT_EXACT, _ints, member_ranges  # noqa: F401

CAP, SLOTS, SIZES = 3, (0, 2), (3, 2)
IDLE = 1
CAP4, SLOTS4, IDLE4, EMPTY4 = 4, (0, 2, 3), 1, 3  # slot 3 is listed with cnt == 0, slot 1 is not listed
CANARY = kx.CANARY
ICANARY = -77  # int tables
FACTOR_RSQRT, FACTOR_EXP, MARGIN = 4.0, 8.0, 64.0
BN_EPS, BN_MOM, BN_ONE_M = ax.BN_EPS, ax.BN_MOM, ax.BN_ONE_M
NAN = float("nan")
DTYPES = (torch.bfloat16, torch.float16)


class Case:
    pass


def gen(seed):
    return torch.Generator().manual_seed(seed)


def img_slots(sizes=SIZES, slots=SLOTS):
    return [s for s, n in zip(slots, sizes) for _ in range(n)]


def half_ulp16(v, dt):
    return ax.ulp16(v, dt) / 2


def bounds16(ref, tol, dt):
    """The 16-bit roundings of ref - tol and ref + tol (float64)."""
    return (ref - tol).to(dt).double(), (ref + tol).to(dt).double()


def excess16(got, ref, mag, dt):
    """Scaled distance from ref to the nearest value that rounds to ``got`` (0: got is a rounding of ref itself)."""
    d = ((got - ref).abs() - half_ulp16(got, dt)).clamp(min=0)
    d = torch.where(torch.isfinite(got), d, torch.zeros_like(d))  # an overflow of fp16 the bounds agree with
    nz = mag > 0
    return float((d[nz] / mag[nz]).max()) if bool(nz.any()) else 0.0


# ------------------------------------------------------------------------------------------- replica statistics
def spread_int(g, total, nrep):
    """[..., C] integers -> [nrep, ..., C] integer shares, uneven, some negative, that add up to ``total``."""
    sh = _ints(g, (nrep,) + tuple(total.shape), -4, 4)
    sh[nrep - 1] = total - sh[:nrep - 1].sum(0)
    return sh


def spread_pos(g, total, nrep):
    """fp32 words [nrep, ...]: uneven positive shares of ``total`` (each rounded to fp32 on its own)."""
    w = 1.0 + _ints(g, (nrep,) + tuple(total.shape), 0, 6)
    return (w / w.sum(0, keepdim=True) * total).float().double()


def rep_sum(words, dtype):
    """The kernel's stats_sum: replicas added in order at ``dtype``.  words [nrep, ...] (fp32 values as float64)."""
    w = words.to(dtype)
    s = torch.zeros_like(w[0])
    for r in range(w.shape[0]):
        s = s + w[r]
    return s


def fwd_stats(g, slots, ns, nrep, c, cap=CAP, const_ch=None):
    """Forward statistics [cap][nrep][2][64] fp32 words of a BN with mean in [-1, 1] and variance in [0.5, 4],
    channel ``const_ch`` constant 1 / 4 (integer shares: q / n - mean^2 is exactly 0 at fp32 and at float64).  Idle slots
    and columns >= c: NaN."""
    st = torch.full((cap, nrep, 2, 64), NAN, dtype=torch.float64)
    for s, n in zip(slots, ns):
        mean = _ints(g, (c,), -8, 8) / 8
        var = _ints(g, (c,), 4, 32) / 8
        st[s, :, 0, :c] = spread_pos(g, mean.abs() * n, nrep) * torch.sign(mean)
        st[s, :, 1, :c] = spread_pos(g, (var + mean * mean) * n, nrep)
        if const_ch is not None:
            base = torch.tensor([float(n // nrep + (r < n % nrep)) for r in range(nrep)], dtype=torch.float64)
            st[s, :, 0, const_ch] = base / 4
            st[s, :, 1, const_ch] = base / 16
    return st


def fwd_coef(st, n, gamma, beta, dtype):
    """fwd_coef2 of resnet_aux.hip at ``dtype`` from the fp32 words st [nrep][2][64]: (scale, shift, mean, inv)."""
    c = gamma.shape[0]
    sq = rep_sum(st[:, :, :c], dtype)
    n = torch.tensor(float(n), dtype=dtype)
    mean = sq[0] / n
    var = torch.clamp(sq[1] / n - mean * mean, min=0)
    inv = 1 / torch.sqrt(var + torch.tensor(BN_EPS, dtype=dtype))
    scale = gamma.to(dtype) * inv
    return scale, beta.to(dtype) - mean * scale, mean, inv


def bwd_coef(stf, stb, n, gamma, dtype):
    """bwd_coef of resnet_aux.hip at ``dtype``: A, B, the two terms of C."""
    c = gamma.shape[0]
    scale, _, mean, inv = fwd_coef(stf, n, gamma, torch.zeros_like(gamma), dtype)
    sb = rep_sum(stb[:, :, :c], dtype)
    n = torch.tensor(float(n), dtype=dtype)
    mdz, mdzx = sb[0] / n, sb[1] / n
    return scale, -scale * inv * mdzx, -scale * mdz, scale * inv * mean * mdzx


def param_rows(g, c, cap, live_slots, n_pairs=2, stride=400):
    """[cap][stride] params: n_pairs (gamma, beta) blocks at odd offsets; gamma in +-[0.5, 1.5], beta in [-1, 1]
    (multiples of 1/8).  Everything else, the idle slots' rows included, NaN."""
    rows = torch.full((cap, stride), NAN, dtype=torch.float64)
    offs = [(37 + 150 * i, 37 + 150 * i + 71) for i in range(n_pairs)]
    for s in live_slots:
        for go, bo in offs:
            rows[s, go:go + c] = _ints(g, (c,), 4, 12) / 8 * (2 * _ints(g, (c,), 0, 1) - 1)
            rows[s, bo:bo + c] = _ints(g, (c,), -8, 8) / 8
        rows[s, offs[0][1] + 3] = 4.0 - 8.0 * (s == 0)  # the constant channel of the first BN: x scale + shift == beta
    return rows, offs


# ----------------------------------------------------------------------------------------------- prep_input
PREP_CASES = [(3, 300), (1, 300), (3, 4096 * 256 + 300)]  # the last: the grid-stride loop's second trip


def prep_input_case(c_in, npix):
    g = gen(21000 + c_in + npix % 1000)
    x = (torch.randint(-2 ** 15, 2 ** 15, (npix, c_in), generator=g).float() / 1024)  # 16 significant bits: ties occur
    return x


def prep_input_ref(x, dt):
    want = torch.zeros(x.shape[0], 16, dtype=dt)
    want[:, :x.shape[1]] = x.to(dt)
    return want


# ---------------------------------------------------------------------------------------------- weight_prep
# {w_off, cout, cin, k, cin_pad, fwd_off, dgr_off, 0}: float4 row + LDS transpose with cout != cin; the padded stem
# row (cin 3 -> 16) without a dgrad copy; a scalar row forced by w_off % 4 != 0 (1 x 1: LDS transpose, one tap); a
# row with cout > 64: float4 forward, gather dgrad
WP_S, WP_W = 8000, 9000
WP_TABLE = [[8, 32, 16, 3, 16, 16, 24, 0], [4700, 16, 3, 3, 16, 4700, -1, 0], [5141, 16, 16, 1, 16, 7100, 4701, 0],
            [5400, 72, 8, 1, 8, 7400, 5001, 0]]
WP_ZN = (1027, 0)


def wp_row_path(row):
    w_off, cout, cin, k, cin_pad, fwd_off, dgr_off, _ = row
    nf = cout * k * k * cin_pad
    fwd = "float4" if cin_pad == cin and nf % 4 == 0 and w_off % 4 == 0 else "scalar"
    dgr = None if dgr_off < 0 else ("lds" if cout <= 64 and cin <= 64 else "gather")
    return fwd, dgr


def weight_prep_expected(state, dt):
    wf = torch.full((CAP, WP_W), CANARY, dtype=torch.float64)
    wd = torch.full((CAP, WP_W), CANARY, dtype=torch.float64)
    for s in SLOTS:
        for w_off, cout, cin, k, cin_pad, fwd_off, dgr_off, _ in WP_TABLE:
            kk = k * k
            w = state[s, w_off:w_off + cout * kk * cin].to(dt).double().view(cout, kk, cin)
            f = torch.zeros(cout, kk, cin_pad, dtype=torch.float64)
            f[:, :, :cin] = w
            wf[s, fwd_off:fwd_off + f.numel()] = f.reshape(-1)
            if dgr_off >= 0:  # IHWO: d[ci][tap][co] = W[co][tap][ci]
                wd[s, dgr_off:dgr_off + w.numel()] = w.permute(2, 1, 0).reshape(-1)
    return wf, wd


def weight_prep_state():
    st = torch.randn(CAP, WP_S, generator=gen(21100))
    st[IDLE] = NAN
    return st


def check_weight_prep_table():
    paths = [wp_row_path(r) for r in WP_TABLE]
    assert paths == [("float4", "lds"), ("scalar", None), ("scalar", "lds"), ("float4", "gather")], paths
    assert WP_TABLE[1][2] == 3 and WP_TABLE[1][4] == 16 and WP_TABLE[2][0] % 4 != 0 and WP_TABLE[2][2] == WP_TABLE[2][4]
    assert WP_TABLE[0][1] != WP_TABLE[0][2] and WP_S % 4 == 0 and WP_W % 4 == 0
    sf, sd = [], []
    for w_off, cout, cin, k, cin_pad, fwd_off, dgr_off, _ in WP_TABLE:
        assert w_off + cout * k * k * cin <= WP_S
        if wp_row_path([w_off, cout, cin, k, cin_pad, fwd_off, dgr_off, 0])[0] == "float4":
            assert fwd_off % 4 == 0  # 8-byte stores
        sf.append((fwd_off, fwd_off + cout * k * k * cin_pad))
        if dgr_off >= 0:
            sd.append((dgr_off, dgr_off + cout * k * k * cin))
    for spans in (sf, sd):
        spans.sort()
        assert spans[0][0] > 0 and spans[-1][1] < WP_W and all(a[1] < b[0] for a, b in zip(spans[:-1], spans[1:]))
    assert WP_ZN[0] % 4 == 3 and WP_ZN[1] == 0


# ------------------------------------------------------------------------------------------------- work_gen
WG_CNT = {0: 5.0, 3: 0.0, 2: 131.0}  # slot -> images; slot 1 is not listed (NaN)
WG_SLOTS = (0, 3, 2)
WG_FIRST = (0, 160, 320)  # a capacity layout: 160 images per member region
# (per, bands, min_chunk, split, prop, red)
WG_DESCS = [(8, 1, 1, 0, 1, 0), (8, 4, 64, 1, 1, 1), (8, 4, 1, 1, 0, 1), (1, 1, 1, 0, 1, 0), (100, 1, 4, 0, 1, 1),
            (8, 1, 1, 0, 0, 0)]


def work_gen_ref(desc, elastic_rows):
    """(table [R * rows][4], red [M][4]) of one descriptor, from the host mirror of the row split."""
    per, bands, min_chunk, split, prop, _ = desc
    rows = 2 if split else 1
    totals = [int(WG_CNT[s]) * bands for s in WG_SLOTS]
    table = [[ICANARY] * 4 for _ in range(per * len(WG_SLOTS) * rows)]
    red = []
    for m, (row0, nrows, chunk) in enumerate(elastic_rows(totals, per, min_chunk, prop)):
        f, total, slot = WG_FIRST[m] * bands, totals[m], WG_SLOTS[m]
        for j in range(nrows):
            start = j * chunk
            nit = min(chunk, total - start) if start < total else 0
            for z in range(rows):
                table[(row0 + j) * rows + z] = [f + start if nit > 0 else f, nit, z, slot]
        red.append([row0 * rows, nrows * rows, 0, slot])
    return table, red


def check_work_table(desc, table, red):
    """The stated contract, independent of the mirror: per member the rows with nit > 0 tile [first * bands, first *
    bands + total) once and in order, nit == 0 rows point at the member's first iteration, the members' rows are
    disjoint and cover [0, R)."""
    per, bands, _, split, _, _ = desc
    rows = 2 if split else 1
    R = per * len(WG_SLOTS)
    assert len(table) == R * rows
    owner = {}
    for r in range(R):
        ent = table[r * rows:(r + 1) * rows]
        assert [e[2] for e in ent] == list(range(rows)) and len({(e[0], e[1], e[3]) for e in ent}) == 1, (r, ent)
        owner.setdefault(ent[0][3], []).append((r, ent[0][0], ent[0][1]))
    assert set(owner) == set(WG_SLOTS)
    seen = []
    for m, slot in enumerate(WG_SLOTS):
        f, total = WG_FIRST[m] * bands, int(WG_CNT[slot]) * bands
        rr = owner[slot]
        assert [r for r, _, _ in rr] == list(range(rr[0][0], rr[0][0] + len(rr)))  # contiguous
        seen += [r for r, _, _ in rr]
        at = f
        for _, it0, nit in rr:
            if nit > 0:
                assert it0 == at
                at += nit
            else:
                assert it0 == f
        assert at == f + total, (slot, at, f, total)
        assert red[m] == [rr[0][0] * rows, len(rr) * rows, 0, slot]
    assert sorted(seen) == list(range(R))


# -------------------------------------------------------------------------------------- BN tables (per-BN kernels)
# {run_off, C, hw, stats index, gamma_off, beta_off, 0, 0}: the statistics index is not the row number
BN_TABLE = [[10, 16, 64, 1, 40, 60, 0, 0], [50, 64, 16, 0, 90, 170, 0, 0]]
BN_S, BN_RUN_BASE, BN_G = 400, 120, 300  # state row, offset of the running statistics in it, gradient row
BN_CNT4 = {0: 3.0, 2: 2.0, 3: 0.0}


def bn_cnt4(n1=False):
    cnt = torch.full((CAP4,), NAN, dtype=torch.float64)
    for s, v in BN_CNT4.items():
        cnt[s] = 1.0 if (n1 and v > 0) else v
    return cnt


def bn_table(n1=False):
    return [[r[0], r[1], 1 if n1 else r[2]] + r[3:] for r in BN_TABLE]


@functools.lru_cache(maxsize=None)
def bn_eval_case(nrep):
    """Dyadic moving mean (k / 4, |.| <= 2) and variance (k / 4 in [0.25, 4]): n * mean and n * (var + mean^2) are
    multiples of 1 / 16 below 2^12, exact at fp32 with or without contraction."""
    k = Case()
    g = gen(21200)
    k.cnt = torch.tensor([3.0, NAN, 2.0], dtype=torch.float64)
    k.state = torch.full((CAP, BN_S), NAN, dtype=torch.float64)
    k.stats0 = (_ints(g, (len(BN_TABLE), CAP, nrep, 2, 64), 1, 9) + 0.375)  # non-zero, no dyadic the kernel writes
    k.stats = k.stats0.clone()
    for run_off, c, hw, si, _, _, _, _ in BN_TABLE:
        for s in SLOTS:
            mean, var = _ints(g, (c,), -8, 8) / 4, _ints(g, (c,), 1, 16) / 4
            o = BN_RUN_BASE + run_off
            k.state[s, o:o + c], k.state[s, o + c:o + 2 * c] = mean, var
            n = float(k.cnt[s]) * hw
            k.stats[si, s, :, :, :c] = 0
            k.stats[si, s, 0, 0, :c], k.stats[si, s, 0, 1, :c] = n * mean, n * (var + mean * mean)
    return k


def check_bn_eval(k):
    assert torch.equal(k.stats.float().double(), k.stats) and ax.is_int(k.stats[:, list(SLOTS), :, :, :16], 1 / 16)
    assert k.stats[:, list(SLOTS)].abs().max() < 2 ** 12
    assert torch.equal(k.stats[:, IDLE], k.stats0[:, IDLE])
    for _, c, _, si, _, _, _, _ in BN_TABLE:
        assert torch.equal(k.stats[si, :, :, :, c:], k.stats0[si, :, :, :, c:])
        assert bool((k.stats[si, list(SLOTS), 1:, :, :c] == 0).all()) and bool((k.stats[si, list(SLOTS), 0, 1, :c] > 0).all())


@functools.lru_cache(maxsize=None)
def bn_end_case(nrep, n1=False):
    """Operands of bn_running_update / bn_step_end: integer backward statistics spread unevenly over the replicas,
    integer gradient seed (bitwise half); forward statistics as fp32 words and a float state row (tolerant half).
    Slot 3 is listed with cnt == 0 (the kernel reads its cnt): its statistics are NaN and its rows must stay."""
    k = Case()
    g = gen(21300 + n1)
    k.n1, k.nrep = n1, nrep
    k.cnt, k.table = bn_cnt4(n1), bn_table(n1)
    nb = len(k.table)
    k.stb = torch.full((nb, CAP4, nrep, 2, 64), NAN, dtype=torch.float64)
    k.stf = torch.full((nb, CAP4, nrep, 2, 64), NAN, dtype=torch.float64)
    k.grads0 = _ints(g, (CAP4, BN_G), 1, 9)
    k.state0 = (torch.rand(CAP4, BN_S, generator=g) + 0.25).float().double()
    k.state0[IDLE4] = NAN
    k.grads = k.grads0.clone()
    k.gabs = k.grads0.abs()
    for run_off, c, hw, si, go, bo, _, _ in k.table:
        for s in SLOTS:
            tot = _ints(g, (2, c), -40, 40)
            k.stb[si, s, :, :, :c] = spread_int(g, tot, nrep)
            k.grads[s, go:go + c] += tot[1]
            k.grads[s, bo:bo + c] += tot[0]
            k.gabs[s, go:go + c] += k.stb[si, s, :, 1, :c].abs().sum(0)
            k.gabs[s, bo:bo + c] += k.stb[si, s, :, 0, :c].abs().sum(0)
            n = int(k.cnt[s]) * hw
            if n1:  # one value per channel: s = x, q = x^2 in replica 3 (the others zero): the variance is exactly 0
                x = _ints(g, (c,), -12, 12) / 8
                k.stf[si, s, :, :, :c] = 0
                k.stf[si, s, 3 % nrep, 0, :c], k.stf[si, s, 3 % nrep, 1, :c] = x, x * x
            else:
                k.stf[si, s] = fwd_stats(g, [0], [n], nrep, c, cap=1, const_ch=5)[0]
    return k


def bn_running_eval(k, dtype):
    """{(table row, slot): (new mean, its magnitude, new variance, its magnitude)} at ``dtype``."""
    out = {}
    mom, om = torch.tensor(BN_MOM, dtype=dtype), torch.tensor(BN_ONE_M, dtype=dtype)
    for row, (run_off, c, hw, si, _, _, _, _) in enumerate(k.table):
        for s in SLOTS:
            n = torch.tensor(float(k.cnt[s]) * hw, dtype=dtype)
            sq = rep_sum(k.stf[si, s, :, :, :c], dtype)
            mean = sq[0] / n
            var = torch.clamp(sq[1] / n - mean * mean, min=0)
            unb = var * n / (n - 1) if float(n) > 1 else var
            o = BN_RUN_BASE + run_off
            rm, rv = k.state0[s, o:o + c].to(dtype), k.state0[s, o + c:o + 2 * c].to(dtype)
            a, b, a2, b2 = mom * rm, om * mean, mom * rv, om * unb
            out[(row, s)] = (a + b, a.abs() + b.abs(), a2 + b2, a2.abs() + b2.abs())
    return out


def check_bn_end(k):
    sl = list(SLOTS)
    assert ax.is_int(k.stb[:, sl][..., :16]) and ax.is_int(k.grads) and k.gabs.max() < EXACT
    for _, c, hw, si, go, bo, _, _ in k.table:
        w = k.stb[si, sl, :, :, :c]
        assert bool((w.max(1).values != w.min(1).values).all()) and bool((w < 0).any())  # uneven shares
        assert bool(torch.isnan(k.stb[si, [IDLE4, EMPTY4]]).all()) and bool(torch.isnan(k.stf[si, [IDLE4, EMPTY4]]).all())
    assert torch.equal(k.grads[[IDLE4, EMPTY4]], k.grads0[[IDLE4, EMPTY4]]) and bool((k.grads0 != 0).all())
    assert k.cnt[EMPTY4] == 0 and bool(torch.isnan(k.cnt[IDLE4]))
    r64 = bn_running_eval(k, torch.float64)
    for (row, s), (m, _, v, _) in r64.items():
        assert bool(torch.isfinite(m).all()) and bool(torch.isfinite(v).all()) and bool((v > 0).all())
    if k.n1:
        assert all(float(k.cnt[s]) * r[2] == 1 for s in SLOTS for r in k.table)
    else:  # the constant channel: variance exactly 0 at both precisions
        for _, c, hw, si, _, _, _, _ in k.table:
            for s in SLOTS:
                for dt in (torch.float32, torch.float64):
                    sq = rep_sum(k.stf[si, s, :, :, :c], dt)
                    n = float(k.cnt[s]) * hw
                    assert float(sq[1][5] / n - (sq[0][5] / n) ** 2) == 0.0


# --------------------------------------------------------------------- elementwise BN kernels (BnBwdArgs / BnEwArgs)
def ew_split(hw, c, nimg, det_slab=False):
    """Mirror of dtf_bn_bwd_apply's split and of ew_split (resnet_aux.hip)."""
    if det_slab:
        return 1
    n8 = hw * c // 8
    return max(1, min(-(-2048 // nimg), -(-n8 // 256)))


def ew_chunks(hw, c, nimg, pair=False, det_slab=False):
    """Chunks (16-byte groups) each of the split * 256 threads of an image handles; pair: the trips of
    bn_bwd_reduce's two-chunks-per-trip loop as a list of chunk counts per trip."""
    n8 = hw * c // 8
    stride = ew_split(hw, c, nimg, det_slab) * 256
    out = []
    for i0 in range(stride):
        n = len(range(i0, n8, stride))
        out.append(([2] * (n // 2) + [1] * (n % 2)) if pair else n)
    return out


def ew_wraps(hw, c, nimg):
    """True if some thread's first channel c0 = (8 i) % C differs from 8 i (the modulo matters)."""
    n8 = hw * c // 8
    return any((8 * i) % c != 8 * i for i in range(n8))


def _margin_x(g, shape, scale, shift, need):
    """16-bit representable x (multiples of 1 / 8 in [-4, 4], moved by whole units where needed) with
    |x scale + shift| >= need for every element; scale / shift broadcast over x."""
    x = _ints(g, shape, -32, 32) / 8
    for _ in range(8):
        v = x * scale + shift
        bad = v.abs() < need
        if not bool(bad.any()):
            break
        x = torch.where(bad, x + torch.sign(scale) * torch.where(v >= 0, 1.0, -1.0), x)
    return x


# (C, hw, with add)
BWD_APPLY_CASES = [(16, 64, 0), (16, 64, 1), (16, 256, 1), (32, 64, 0), (32, 256, 1), (64, 64, 0), (64, 64, 1)]


@functools.lru_cache(maxsize=None)
def bwd_apply_case(c, hw, add, nrep):
    k = Case()
    g = gen(21400 + 7 * c + hw + add)
    k.c, k.hw, k.n, k.nrep = c, hw, sum(SIZES), nrep
    k.cnt = torch.tensor([3.0, NAN, 2.0], dtype=torch.float64)
    k.params, offs = param_rows(g, c, CAP, SLOTS, 1)
    k.gamma_off = offs[0][0]
    ns = [int(k.cnt[s]) * hw for s in SLOTS]
    k.stf = fwd_stats(g, SLOTS, ns, nrep, c, const_ch=3)
    k.stb = torch.full((CAP, nrep, 2, 64), NAN, dtype=torch.float64)
    for s, n in zip(SLOTS, ns):
        tot = _ints(g, (2, c), -64, 64) / 8 * n / 16
        k.stb[s, :, :, :c] = spread_pos(g, tot.abs(), nrep) * torch.sign(tot)
    k.dz, k.x = _ints(g, (k.n, hw, c), -16, 16) / 8, _ints(g, (k.n, hw, c), -32, 32) / 8
    k.add = _ints(g, (k.n, hw, c), -16, 16) / 8 if add else None
    return k


def bwd_apply_eval(k, dtype):
    """(out, magnitude) [N][hw][C] at ``dtype``."""
    out = torch.empty(k.n, k.hw, k.c, dtype=dtype)
    mag = torch.empty_like(out)
    for s, f, e in kx.ranges(SLOTS, SIZES):
        a, b, c1, c2 = bwd_coef(k.stf[s], k.stb[s], float(k.cnt[s]) * k.hw, k.params[s, k.gamma_off:k.gamma_off + k.c],
                                dtype)
        dz, x = k.dz[f:e].to(dtype), k.x[f:e].to(dtype)
        out[f:e] = a * dz + b * x + (c1 + c2)
        mag[f:e] = (a * dz).abs() + (b * x).abs() + c1.abs() + c2.abs()
        if k.add is not None:
            out[f:e] += k.add[f:e].to(dtype)
            mag[f:e] += k.add[f:e].to(dtype).abs()
    return out, mag


def check_bwd_apply(k):
    for t in (k.dz, k.x) + ((k.add,) if k.add is not None else ()):
        for dt in DTYPES:
            assert torch.equal(t.to(dt).double(), t)
    for s in SLOTS:
        for dt in (torch.float32, torch.float64):
            sq = rep_sum(k.stf[s, :, :, :k.c], dt)
            n = float(k.cnt[s]) * k.hw
            assert float(sq[1][3] / n - (sq[0][3] / n) ** 2) == 0.0  # the clamped channel
        w = k.stf[s, :, 1, :k.c]
        assert int((w.max(0).values != w.min(0).values).sum()) >= k.c - 1  # uneven but for the constant channel
    assert bool(torch.isnan(k.stf[IDLE]).all()) and bool(torch.isnan(k.stb[IDLE]).all()) and bool(torch.isnan(k.cnt[IDLE]))
    out, _ = bwd_apply_eval(k, torch.float64)
    assert bool(torch.isfinite(out).all())


# (C, hw, form): form 0 stem (no addend), 1 identity add, 2 projection BN
ADD_RELU_CASES = [(c, hw, f) for c, hw in ((16, 64), (64, 16)) for f in (0, 1, 2)]
ELASTIC_CAP = 4  # images per member region of the elastic form; members hold 3 and 2 real images


def elastic_layout():
    """(img_slot [2 * cap], real [2 * cap] bool): member k's images at [k cap, (k + 1) cap), the first cnt real."""
    slot, real = [], []
    for s, n in zip(SLOTS, SIZES):
        slot += [s] * ELASTIC_CAP
        real += [True] * n + [False] * (ELASTIC_CAP - n)
    return slot, torch.tensor(real)


@functools.lru_cache(maxsize=None)
def add_relu_case(c, hw, form, nrep):
    """Images in the elastic layout (2 x ELASTIC_CAP, the padded ones NaN); the packed form is the real images."""
    k = Case()
    g = gen(21500 + 7 * c + hw + form)
    k.c, k.hw, k.form, k.nrep = c, hw, form, nrep
    k.cnt = torch.tensor([3.0, NAN, 2.0], dtype=torch.float64)
    k.params, k.offs = param_rows(g, c, CAP, SLOTS, 2)
    ns = [int(k.cnt[s]) * hw for s in SLOTS]
    k.st1 = fwd_stats(g, SLOTS, ns, nrep, c, const_ch=3)
    k.st2 = fwd_stats(g, SLOTS, ns, nrep, c, const_ch=None)
    k.slot, k.real = elastic_layout()
    n = len(k.slot)
    k.h1 = torch.full((n, hw, c), NAN, dtype=torch.float64)
    k.h2 = torch.full((n, hw, c), NAN, dtype=torch.float64) if form else None
    for m, s in enumerate(SLOTS):
        lo, hi = m * ELASTIC_CAP, m * ELASTIC_CAP + SIZES[m]
        sc, sh, mean, _ = fwd_coef(k.st1[s], ns[m], *_gb(k, s, 0), torch.float64)
        other = torch.zeros(SIZES[m], hw, c, dtype=torch.float64)
        if form:
            k.h2[lo:hi] = _ints(g, (SIZES[m], hw, c), -32, 32) / 8
            other = k.h2[lo:hi]
            if form == 2:
                sc2, sh2, _, _ = fwd_coef(k.st2[s], ns[m], *_gb(k, s, 1), torch.float64)
                other = other * sc2 + sh2
        x = _margin_x(g, (SIZES[m], hw, c), sc, sh + other, 2.0 ** -4)
        x[..., 3] = 0.25  # the constant channel: x == mean, x scale + shift == beta = +-4 whatever inv is
        k.h1[lo:hi] = x
        if form:  # ... and its addend keeps the sum half a unit away from 0
            beta3 = k.params[s, k.offs[0][1] + 3]
            s3, t3 = (sc2[3], sh2[3]) if form == 2 else (torch.tensor(1.0, dtype=torch.float64), 0.0)
            k.h2[lo:hi, :, 3] = _margin_x(g, (SIZES[m], hw), s3, t3 + beta3, 0.5)
    return k


def _gb(k, s, pair):
    go, bo = k.offs[pair]
    return k.params[s, go:go + k.c], k.params[s, bo:bo + k.c]


def add_relu_eval(k, dtype):
    """(pre-ReLU value, magnitude) over the elastic layout at ``dtype`` (padded images NaN)."""
    v = torch.full(k.h1.shape, NAN, dtype=dtype)
    mag = torch.full(k.h1.shape, NAN, dtype=dtype)
    for m, s in enumerate(SLOTS):
        lo, hi = m * ELASTIC_CAP, m * ELASTIC_CAP + SIZES[m]
        n = float(k.cnt[s]) * k.hw
        sc, sh, _, _ = fwd_coef(k.st1[s], n, *_gb(k, s, 0), dtype)
        gam, bet = _gb(k, s, 0)
        h = k.h1[lo:hi].to(dtype)
        v[lo:hi] = h * sc + sh
        mag[lo:hi] = (h * sc).abs() + bet.to(dtype).abs() + (sh - bet.to(dtype)).abs()
        if k.form == 2:
            sc2, sh2, _, _ = fwd_coef(k.st2[s], n, *_gb(k, s, 1), dtype)
            bet2 = _gb(k, s, 1)[1].to(dtype)
            p = k.h2[lo:hi].to(dtype)
            v[lo:hi] += p * sc2 + sh2
            mag[lo:hi] += (p * sc2).abs() + bet2.abs() + (sh2 - bet2).abs()
        elif k.form == 1:
            v[lo:hi] += k.h2[lo:hi].to(dtype)
            mag[lo:hi] += k.h2[lo:hi].to(dtype).abs()
    return v, mag


def check_add_relu(k):
    v64, mag = add_relu_eval(k, torch.float64)
    v32, _ = add_relu_eval(k, torch.float32)
    r = k.real
    d = deviation(v32[r], v64[r], mag[r])
    tol = FACTOR_RSQRT * d * mag[r]
    assert bool((v64[r].abs() >= MARGIN * tol).all()), float((v64[r].abs() / tol.clamp(min=1e-300)).min())
    assert bool((v64[r] > 0).any()) and bool((v64[r] < 0).any())
    assert bool(torch.isnan(k.h1[~r]).all()) and bool(torch.isfinite(v64[r]).all())
    for t in (k.h1[r],) + ((k.h2[r],) if k.form else ()):
        for dt in DTYPES:
            assert torch.equal(t.to(dt).double(), t)
    for s in SLOTS:  # the clamped channel
        sq = rep_sum(k.st1[s, :, :, :k.c], torch.float32)
        n = float(k.cnt[s]) * k.hw
        assert float(sq[1][3] / n - (sq[0][3] / n) ** 2) == 0.0
    return d


# (C, hw, h2, sizes, elastic): hw C / 8 = 128 (threads without a chunk), 512 (split 2), and the 2048-image case with
# hw C / 8 = 768 at split 1: a two-chunk trip, then a one-chunk trip
REDUCE_CASES = [(16, 64, 0, SIZES, 0), (16, 256, 1, SIZES, 0), (32, 64, 1, SIZES, 1), (64, 64, 0, SIZES, 1),
                (64, 64, 1, SIZES, 0), (32, 192, 1, (1200, 848), 0)]


@functools.lru_cache(maxsize=2)
def reduce_case(c, hw, two, sizes, elastic, nrep):
    """bn_bwd_reduce: integer d in [-3, 3] (sum d exact), h1 / h2 multiples of 1 / 8; the accumulators carry an
    integer seed in every replica.  Elastic: the ELASTIC_CAP layout with NaN padded images."""
    k = Case()
    g = gen(21600 + 7 * c + hw + two + elastic)
    k.c, k.hw, k.two, k.sizes, k.elastic, k.nrep = c, hw, two, sizes, elastic, nrep
    k.cnt = torch.tensor([float(sizes[0]), NAN, float(sizes[1])], dtype=torch.float64)
    k.params, k.offs = param_rows(g, c, CAP, SLOTS, 2)
    ns = [n * hw for n in sizes]
    k.st1 = fwd_stats(g, SLOTS, ns, nrep, c, const_ch=3)
    k.st2 = fwd_stats(g, SLOTS, ns, nrep, c, const_ch=None)
    if elastic:
        k.slot, k.real = elastic_layout()
        k.first = [m * ELASTIC_CAP for m in range(len(SLOTS))]
    else:
        k.slot, k.real = img_slots(sizes), torch.ones(sum(sizes), dtype=torch.bool)
        k.first = [f for _, f, _ in kx.ranges(SLOTS, sizes)]
    n = len(k.slot)
    k.d = torch.randint(-3, 4, (n, hw, c), generator=g).double()
    k.h1 = torch.randint(-32, 33, (n, hw, c), generator=g).double() / 8
    k.h2 = torch.randint(-32, 33, (n, hw, c), generator=g).double() / 8 if two else None
    for t in (k.d, k.h1) + ((k.h2,) if two else ()):
        t[~k.real] = NAN
    k.seed1, k.seed2 = _ints(g, (CAP, nrep, 2, 64), 1, 4), _ints(g, (CAP, nrep, 2, 64), 1, 4)
    k.members = [(s, torch.tensor([i for i in range(n) if k.slot[i] == s and bool(k.real[i])])) for s in SLOTS]
    return k


def reduce_eval(k, dtype):
    """{"sd": [CAP][64] sum d (seed of all replicas included), "x1", "x2": (value, magnitude) of the xhat rows,
    "img_sd": [N][C] per-image sum d}; images are added in order, one at a time, at ``dtype``."""
    c = k.c
    out = {"sd": (k.seed1[:, :, 0].sum(1).to(dtype), None), "img_sd": torch.zeros(len(k.slot), c, dtype=dtype)}
    x = {1: [k.seed1[:, :, 1].sum(1).to(dtype), k.seed1[:, :, 1].sum(1).to(dtype)],
         2: [k.seed2[:, :, 1].sum(1).to(dtype), k.seed2[:, :, 1].sum(1).to(dtype)]}
    sd2 = k.seed2[:, :, 0].sum(1).to(dtype)
    for s, idx in k.members:
        n = float(k.cnt[s]) * k.hw
        d = k.d[idx].to(dtype)
        per = d.sum(1)
        out["img_sd"][idx] = per
        for which, h, st in ((1, k.h1, k.st1), (2, k.h2, k.st2)):
            if which == 2 and not k.two:
                continue
            _, _, mean, inv = fwd_coef(st[s], n, *_gb(k, s, which - 1), dtype)
            t = d * (h[idx].to(dtype) * inv + (-mean * inv))
            tm = (d * h[idx].to(dtype) * inv).abs() + (d * mean * inv).abs()
            pv, pm = t.sum(1), tm.sum(1)
            acc, accm = torch.zeros(c, dtype=dtype), torch.zeros(c, dtype=dtype)
            for i in range(pv.shape[0]):  # image order, one add per image
                acc, accm = acc + pv[i], accm + pm[i]
            x[which][0][s, :c] += acc
            x[which][1][s, :c] += accm
        tot = per.sum(0)
        out["sd"][0][s, :c] += tot
        if k.two:
            sd2[s, :c] += tot
    out["sd2"] = sd2
    out["x1"], out["x2"] = tuple(x[1]), tuple(x[2])
    return out


def check_reduce(k):
    r = k.real
    assert ax.is_int(k.d[r]) and k.d[r].abs().max() <= 3 and bool(torch.isnan(k.d[~r]).all())
    for t in (k.h1[r],) + ((k.h2[r],) if k.two else ()):
        for dt in DTYPES:
            assert torch.equal(t.to(dt).double(), t)
    for s, idx in k.members:
        assert k.d[idx].abs().sum((0, 1)).max() + k.seed1[s, :, 0].sum(0).max() < EXACT
        assert len(idx) == int(k.cnt[s])
    assert bool((k.seed1 != 0).all()) and bool((k.seed2 != 0).all()) and ax.is_int(k.seed1)


# ------------------------------------------------------------------------------------------------------ head
# (hw, ncls, v2, train, loss_scale, slab)
HEAD_CASES = [(32, 10, 1, 1, 1.0, 1), (64, 16, 1, 1, 128.0, 0), (128, 10, 1, 1, 1.0, 0), (128, 16, 0, 1, 128.0, 1),
              (32, 16, 0, 1, 1.0, 0), (64, 10, 0, 1, 1.0, 1), (64, 10, 1, 0, 1.0, 0), (64, 16, 0, 0, 1.0, 1)]
HEAD_REJECTS = [dict(C=32), dict(hw=48), dict(hw=160), dict(ncls=17), dict(ncls=0)]
HEAD_SIZES = (5, 4)
# (img0, nimg, 0, slot): several images per item (prefetch + both LDS parities), the members' items interleaved
HEAD_WORK = [[0, 3, 0, 0], [5, 2, 0, 2], [3, 2, 0, 0], [7, 1, 0, 2], [8, 1, 0, 2]]
HEAD_P, HEAD_GAMMA, HEAD_BETA, HEAD_DW, HEAD_DB = 1400, 21, 101, 190, 1230


@functools.lru_cache(maxsize=None)
def head_case(hw, ncls, v2, nrep):
    """v2: final BN from fp32 statistic words, x with a ReLU margin, float dense weights.  v1 (gamma_off < 0): integer
    x in [-3, 4], integer weights in [-2, 2] and bias: the pooled features are multiples of 1 / hw and the logits
    multiples of 1 / hw below 2^11, exact at fp32 in any order."""
    k = Case()
    g = gen(21700 + hw + 3 * ncls + v2)
    k.hw, k.ncls, k.v2, k.nrep, k.n = hw, ncls, v2, nrep, sum(HEAD_SIZES)
    k.cnt = torch.tensor([float(HEAD_SIZES[0]), NAN, float(HEAD_SIZES[1])], dtype=torch.float64)
    k.params = torch.full((CAP, HEAD_P), NAN, dtype=torch.float64)
    k.stf = torch.full((CAP, nrep, 2, 64), NAN, dtype=torch.float64)
    k.x = torch.empty(k.n, hw, 64, dtype=torch.float64)
    if v2:
        k.stf = fwd_stats(g, SLOTS, [n * hw for n in HEAD_SIZES], nrep, 64, const_ch=3)
    for s, f, e in kx.ranges(SLOTS, HEAD_SIZES):
        if v2:
            k.params[s, HEAD_GAMMA:HEAD_GAMMA + 64] = _ints(g, (64,), 4, 12) / 8 * (2 * _ints(g, (64,), 0, 1) - 1)
            k.params[s, HEAD_BETA:HEAD_BETA + 64] = _ints(g, (64,), -8, 8) / 8 + 1 / 16
            k.params[s, HEAD_BETA + 3] = 4.0 - 8.0 * (s == 0)  # the constant channel: x scale + shift == beta
            k.params[s, HEAD_DW:HEAD_DW + ncls * 64] = _ints(g, (ncls * 64,), -16, 16) / 16
            k.params[s, HEAD_DB:HEAD_DB + ncls] = _ints(g, (ncls,), -8, 8) / 8
            sc, sh, _, _ = fwd_coef(k.stf[s], (e - f) * hw, k.params[s, HEAD_GAMMA:HEAD_GAMMA + 64],
                                    k.params[s, HEAD_BETA:HEAD_BETA + 64], torch.float64)
            k.x[f:e] = _margin_x(g, (e - f, hw, 64), sc, sh, 2.0 ** -4)
            k.x[f:e, :, 3] = 0.25
        else:
            k.params[s, HEAD_DW:HEAD_DW + ncls * 64] = _ints(g, (ncls * 64,), -2, 2)
            k.params[s, HEAD_DB:HEAD_DB + ncls] = _ints(g, (ncls,), -3, 3)
            k.x[f:e] = _ints(g, (e - f, hw, 64), -3, 4)
    r = head_eval(k, 1.0, torch.float64)
    # labels: class 0 and class ncls - 1 occur, image 1 is labelled with its runner-up (wrong), the rest are mixed
    order = r["logits"][0].argsort(1, descending=True)
    k.labels = order[:, 0].clone()
    k.labels[1], k.labels[2], k.labels[6] = order[1, 1], 0, ncls - 1
    k.labels[4] = order[4, 2]
    k.loss0, k.correct0 = _ints(g, (CAP,), 1, 4) / 4, _ints(g, (CAP,), 1, 5)
    k.grads0 = (_ints(g, (CAP, HEAD_P), 1, 8) * (2 * _ints(g, (CAP, HEAD_P), 0, 1) - 1) / 8)
    k.stb0 = _ints(g, (CAP, nrep, 2, 64), 1, 4) / 4
    return k


def head_eval(k, loss_scale, dtype, det=False):
    """Every output of head_kernel at ``dtype`` as {name: (value, magnitude)}: logits [N][ncls], li [N] (per-image
    CE), item_loss [items] (loss_acc / bsz per work item), dfeat [N][64], dw [items][ncls][64], db [items][ncls],
    sdz / sdzx [items][64], mask pre-activation v [N][hw][64], argmax / gap [N]."""
    hw, ncls = k.hw, k.ncls
    t = lambda a: a.to(dtype)
    n = k.n
    logits, lmag = torch.empty(n, ncls, dtype=dtype), torch.empty(n, ncls, dtype=dtype)
    feat = torch.empty(n, 64, dtype=dtype)
    v = torch.empty(n, hw, 64, dtype=dtype)
    xm = torch.empty(n, hw, 64, dtype=dtype)  # (x - mean) inv
    vmag = torch.empty(n, hw, 64, dtype=dtype)
    wts = {}
    for s, f, e in kx.ranges(SLOTS, HEAD_SIZES):
        if k.v2:
            sc, sh, mean, inv = fwd_coef(k.stf[s], (e - f) * hw, k.params[s, HEAD_GAMMA:HEAD_GAMMA + 64],
                                         k.params[s, HEAD_BETA:HEAD_BETA + 64], dtype)
        else:
            sc, sh, mean, inv = (torch.ones(64, dtype=dtype), torch.zeros(64, dtype=dtype), torch.zeros(64, dtype=dtype),
                                 torch.ones(64, dtype=dtype))
        x = t(k.x[f:e])
        v[f:e] = x * sc + sh
        vmag[f:e] = (x * sc).abs() + (sh + mean * sc).abs() + (mean * sc).abs()
        xm[f:e] = (x - mean) * inv
        feat[f:e] = torch.relu(v[f:e]).sum(1) * (1.0 / hw)
        w, b = t(k.params[s, HEAD_DW:HEAD_DW + ncls * 64]).view(ncls, 64), t(k.params[s, HEAD_DB:HEAD_DB + ncls])
        wts[s] = w
        logits[f:e] = feat[f:e] @ w.T + b
        lmag[f:e] = feat[f:e].abs() @ w.abs().T + b.abs()
    out = {"logits": (logits, lmag), "v": v, "vmag": vmag}
    top = logits.sort(1, descending=True).values
    out["argmax"], out["gap"] = logits.argmax(1), top[:, 0] - top[:, 1]
    if not hasattr(k, "labels"):
        return out
    slots = img_slots(HEAD_SIZES)
    lse = torch.logsumexp(logits, 1)
    ll = logits.gather(1, k.labels.view(-1, 1))[:, 0]
    li = lse - ll
    bsz = t(k.cnt[slots])
    onehot = torch.nn.functional.one_hot(k.labels, ncls).to(dtype)
    p = torch.exp(logits - lse.unsqueeze(1))
    gsc = (torch.tensor(loss_scale, dtype=dtype) / bsz).unsqueeze(1)
    dl, dlm = (p - onehot) * gsc, (p + onehot) * gsc
    dfeat, dfm = torch.empty(n, 64, dtype=dtype), torch.empty(n, 64, dtype=dtype)
    for s, f, e in kx.ranges(SLOTS, HEAD_SIZES):
        dfeat[f:e], dfm[f:e] = dl[f:e] @ wts[s] * (1.0 / hw), dlm[f:e] @ wts[s].abs() * (1.0 / hw)
    out["dfeat"] = (dfeat, dfm)
    mask = (v > 0).to(dtype)
    gz = dfeat.unsqueeze(1) * mask
    gzm = dfm.unsqueeze(1) * mask
    items = {"item_loss": [], "item_lmag": [], "dw": [], "dwm": [], "db": [], "dbm": [], "sdz": [], "sdzm": [],
             "sdzx": [], "sdzxm": []}
    for img0, nimg, _, s in HEAD_WORK:
        sl = slice(img0, img0 + nimg)
        b = t(k.cnt[s])
        il, im = li[sl].sum() / b, (lse[sl].abs() + ll[sl].abs()).sum() / b
        if det:
            il = torch.round(il * 65536) / 65536
        items["item_loss"].append(il)
        items["item_lmag"].append(im)
        items["dw"].append(dl[sl].T @ feat[sl])
        items["dwm"].append(dlm[sl].T @ feat[sl].abs())
        items["db"].append(dl[sl].sum(0))
        items["dbm"].append(dlm[sl].sum(0))
        items["sdz"].append(gz[sl].sum((0, 1)))
        items["sdzm"].append(gzm[sl].sum((0, 1)))
        items["sdzx"].append((gz[sl] * xm[sl]).sum((0, 1)))
        items["sdzxm"].append((gzm[sl] * xm[sl].abs()).sum((0, 1)))
    for name, mname in (("item_loss", "item_lmag"), ("dw", "dwm"), ("db", "dbm"), ("sdz", "sdzm"), ("sdzx", "sdzxm")):
        out[name] = (torch.stack(items[name]), torch.stack(items[mname]))
    out["li"] = li
    return out


def head_totals(k, r, nrep):
    """Per-slot totals of the per-item results r (one precision): loss [CAP], dense gradient rows [CAP][HEAD_P] and
    statistic replica sums [CAP][2][64], each as (value, magnitude), seeds included."""
    dt = r["dw"][0].dtype
    loss, lm = k.loss0.to(dt).clone(), k.loss0.to(dt).abs()
    gr, gm = k.grads0.to(dt).clone(), k.grads0.to(dt).abs()
    sb = k.stb0.sum(1).to(dt)
    sbm = k.stb0.abs().sum(1).to(dt)
    for i, (_, _, _, s) in enumerate(HEAD_WORK):
        loss[s] += r["item_loss"][0][i]
        lm[s] += r["item_loss"][1][i]
        gr[s, HEAD_DW:HEAD_DW + k.ncls * 64] += r["dw"][0][i].reshape(-1)
        gm[s, HEAD_DW:HEAD_DW + k.ncls * 64] += r["dw"][1][i].reshape(-1)
        gr[s, HEAD_DB:HEAD_DB + k.ncls] += r["db"][0][i]
        gm[s, HEAD_DB:HEAD_DB + k.ncls] += r["db"][1][i]
        if k.v2:
            sb[s, 0] += r["sdz"][0][i]
            sbm[s, 0] += r["sdz"][1][i]
            sb[s, 1] += r["sdzx"][0][i]
            sbm[s, 1] += r["sdzx"][1][i]
    return {"loss": (loss, lm), "grads": (gr, gm), "st_b": (sb, sbm)}


def head_correct(k):
    r = head_eval(k, 1.0, torch.float64)
    c = k.correct0.clone()
    for i, s in enumerate(img_slots(HEAD_SIZES)):
        c[s] += float(r["argmax"][i] == k.labels[i])
    return c


def check_head(k):
    r64, r32 = head_eval(k, 1.0, torch.float64), head_eval(k, 1.0, torch.float32)
    d = deviation(r32["logits"][0], *r64["logits"])
    tol = FACTOR_EXP * d * r64["logits"][1]
    assert bool((r64["gap"] >= MARGIN * 2 * tol.max(1).values).all()), "argmax margin"
    lab = k.labels
    assert 0 in lab.tolist() and k.ncls - 1 in lab.tolist() and int(lab[1]) != int(r64["argmax"][1])
    assert bool((lab == r64["argmax"]).any())
    v64, v32 = r64["v"], r32["v"]
    if k.v2:
        vm = r64["vmag"]
        dv = deviation(v32, v64, vm)
        assert bool((v64.abs() >= MARGIN * FACTOR_EXP * dv * vm).all()), "ReLU margin"
        assert bool((v64 > 0).any()) and bool((v64 < 0).any())
    else:  # x scale + shift == x exactly: the mask has no rounding; logits exact
        assert torch.equal(v64, k.x) and torch.equal(r32["logits"][0].double(), r64["logits"][0])
        assert ax.is_int(r64["logits"][0] * k.hw) and r64["logits"][1].max() * k.hw < EXACT
        assert bool((k.x == 0).any()) and bool((k.x < 0).any())
    for dt in DTYPES:
        assert torch.equal(k.x.to(dt).double(), k.x)
    assert bool(torch.isnan(k.params[IDLE]).all()) and bool(torch.isnan(k.cnt[IDLE]))
    # the work list: every image once, several images in an item, the members interleaved
    cover = sorted(i for img0, nimg, _, s in HEAD_WORK for i in range(img0, img0 + nimg))
    assert cover == list(range(k.n)) and max(w[1] for w in HEAD_WORK) >= 3
    assert all(img_slots(HEAD_SIZES)[i] == s for img0, nimg, _, s in HEAD_WORK for i in range(img0, img0 + nimg))
    assert [w[3] for w in HEAD_WORK][:3] == [0, 2, 0]


# (hw, v2)
HEAD_BWD_CASES = [(32, 1), (64, 1), (32, 0), (64, 0)]


@functools.lru_cache(maxsize=None)
def head_bwd_case(hw, v2, nrep):
    k = Case()
    g = gen(21800 + hw + v2)
    k.hw, k.v2, k.nrep, k.c, k.n = hw, v2, nrep, 64, sum(SIZES)
    k.cnt = torch.tensor([3.0, NAN, 2.0], dtype=torch.float64)
    k.params, k.offs = param_rows(g, 64, CAP, SLOTS, 1)
    ns = [n * hw for n in SIZES]
    k.stf = fwd_stats(g, SLOTS, ns, nrep, 64, const_ch=3)
    k.stb = torch.full((CAP, nrep, 2, 64), NAN, dtype=torch.float64)
    k.dfeat = _ints(g, (k.n, 64), -16, 16) / 64
    k.x = torch.empty(k.n, hw, 64, dtype=torch.float64)
    for (s, f, e), n in zip(kx.ranges(SLOTS, SIZES), ns):
        tot = _ints(g, (2, 64), -64, 64) / 64
        k.stb[s] = spread_pos(g, tot.abs(), nrep) * torch.sign(tot)
        if v2:
            sc, sh, _, _ = fwd_coef(k.stf[s], n, *_gb(k, s, 0), torch.float64)
            k.x[f:e] = _margin_x(g, (e - f, hw, 64), sc, sh, 2.0 ** -4)
            k.x[f:e, :, 3] = 0.25
        else:
            k.x[f:e] = _ints(g, (e - f, hw, 64), -24, 32) / 8
    return k


def head_bwd_eval(k, dtype):
    """(out, magnitude, mask pre-activation) at ``dtype``."""
    out = torch.empty(k.n, k.hw, 64, dtype=dtype)
    mag, v, vmag = torch.empty_like(out), torch.empty_like(out), torch.zeros_like(out)
    for s, f, e in kx.ranges(SLOTS, SIZES):
        x, df = k.x[f:e].to(dtype), k.dfeat[f:e].to(dtype).unsqueeze(1)
        if k.v2:
            n = float(k.cnt[s]) * k.hw
            gam, bet = _gb(k, s, 0)
            a, b, c1, c2 = bwd_coef(k.stf[s], k.stb[s], n, gam, dtype)
            sc, sh, _, _ = fwd_coef(k.stf[s], n, gam, bet, dtype)
            v[f:e] = x * sc + sh
            vmag[f:e] = (x * sc).abs() + bet.to(dtype).abs() + (sh - bet.to(dtype)).abs()
            dz = df * (v[f:e] > 0)
            out[f:e] = a * dz + b * x + (c1 + c2)
            mag[f:e] = (a * dz).abs() + (b * x).abs() + c1.abs() + c2.abs()
        else:
            v[f:e] = x
            out[f:e] = torch.where(x > 0, df, torch.zeros_like(df))  # the kernel selects: +0 where masked
            mag[f:e] = out[f:e].abs()
    return out, mag, v, vmag


def check_head_bwd(k):
    o64, mag, v64, vm = head_bwd_eval(k, torch.float64)
    o32, _, v32, _ = head_bwd_eval(k, torch.float32)
    if k.v2:
        dv = deviation(v32, v64, vm)
        assert bool((v64.abs() >= MARGIN * FACTOR_RSQRT * dv * vm).all()), "ReLU margin"
    else:
        assert torch.equal(v64, k.x) and bool((k.x == 0).any())
    assert bool((v64 > 0).any()) and bool((v64 <= 0).any()) and bool(torch.isfinite(o64).all())
    for dt in DTYPES:
        assert torch.equal(k.x.to(dt).double(), k.x)


# ---------------------------------------------------------------------------------- step_advance / step_end / shadow
def step_case(n_listed):
    """Capacity n + 1 population, slot list reversed ([2, 0] for n = 2); member 0 inactive."""
    k = Case()
    g = gen(21900 + n_listed)
    cap = n_listed + 1
    k.cap, k.S, k.col, k.h_step = cap, 24, 17, 6
    k.slots = [s for s in range(cap - 1, -1, -1) if s != 1][:n_listed]
    k.state = _ints(g, (cap, k.S), 1, 50)
    k.hyper = _ints(g, (cap, 8), 1, 9)
    k.hyper[0, 7] = 0.0
    k.loss = _ints(g, (cap,), 1, 1000) / 8
    return k


def step_expected(k, calls=1):
    st, hy = k.state.clone(), k.hyper.clone()
    for s in k.slots:
        inc = calls if k.hyper[s, 7] != 0 else 0
        st[s, k.col] += inc
        hy[s, k.h_step] += inc
    return st, hy, k.loss[k.slots]


SHADOW_P = 512 * 1024 + 1024  # above one pass of 512 blocks x 1024 elements: the grid-stride loop's second trip


def shadow_values(n, dt, seed):
    """fp32 values with 16 significant bits and a final half-ulp bit in every second one: round-to-nearest-even ties
    of the 16-bit type among ordinary roundings."""
    g = gen(seed)
    keep = 8 if dt == torch.bfloat16 else 11
    m = torch.randint(2 ** (keep - 1), 2 ** keep, (n,), generator=g).double()  # `keep` significant bits
    tie = (torch.arange(n) % 2).double() * 0.5
    e = torch.randint(-4, 4, (n,), generator=g).double()
    sgn = 2.0 * torch.randint(0, 2, (n,), generator=g).double() - 1
    return (sgn * (m + tie) * torch.exp2(e - keep)).float()


# --------------------------------------------------------------------------------------------- fused optimizer
F32 = lambda v: float(torch.tensor(v, dtype=torch.float32))  # the kernel's float constants, exactly


def opt_layout(P):
    Pp = -(-P // 64) * 64 + 64  # padding [ceil4(P), Pp) of at least 64 words
    return Pp, 3 * Pp + 40


def opt_update(code, w, a, b, g, h, dtype):
    """One optimizer step at ``dtype`` (TF1 semantics, engine/optim.py's table written out; constants are the kernel's
    fp32 constants).  h: (lr, mom, dec, t).  Returns (w, a, b, magnitude of w's terms, of a's, of b's)."""
    c = lambda v: torch.tensor(F32(v), dtype=dtype)
    lr, mom, dec, t = (torch.tensor(v, dtype=dtype) for v in h)
    z = torch.zeros_like(w)
    if code == 0:
        return w - lr * g, a, b, w.abs() + (lr * g).abs(), z, z
    if code == 1:
        a2 = mom * a + g
        return w - lr * a2, a2, b, w.abs() + (lr * a2).abs(), (mom * a).abs() + g.abs(), z
    if code == 2:
        lr_t = lr * torch.sqrt(1 - c(0.999) ** t) / (1 - c(0.9) ** t)
        a2, b2 = c(0.9) * a + c(0.1) * g, c(0.999) * b + c(0.001) * g * g
        u = lr_t * a2 / (torch.sqrt(b2) + c(1e-8))
        return w - u, a2, b2, w.abs() + u.abs(), (c(0.9) * a).abs() + (c(0.1) * g).abs(), \
            (c(0.999) * b).abs() + (c(0.001) * g * g).abs()
    if code == 3:
        a2 = a + g * g
        u = lr * g / torch.sqrt(a2)
        return w - u, a2, b, w.abs() + u.abs(), a.abs() + g * g, z
    if code == 4:
        a2 = c(0.95) * a + c(0.05) * g * g
        u = torch.sqrt(b + c(1e-8)) / torch.sqrt(a2 + c(1e-8)) * g
        b2 = c(0.95) * b + c(0.05) * u * u
        return w - lr * u, a2, b2, w.abs() + (lr * u).abs(), (c(0.95) * a).abs() + (c(0.05) * g * g).abs(), \
            (c(0.95) * b).abs() + (c(0.05) * u * u).abs()
    a2 = dec * a + (1 - dec) * g * g
    u = lr * g / torch.sqrt(a2 + c(1e-10))
    b2 = mom * b + u
    return w - b2, a2, b2, w.abs() + b2.abs(), (dec * a).abs() + ((1 - dec) * g * g).abs(), (mom * b).abs() + u.abs()


OWNS = {0: (False, False), 1: (True, False), 2: (True, True), 3: (True, False), 4: (True, True), 5: (True, True)}
# slot -> (code, lr, momentum, grad_decay, wd, reg code, t); slot 4 inactive.  The active slots are scattered and no
# two members share a hyper-parameter; the Adam member is at t = 1
OPT_MEMBERS = {5: (0, 0.0625, 0.0, 0.0, 0.001, 1, 4), 0: (1, 0.03, 0.7, 0.0, 0.002, 2, 9), 6: (2, 0.002, 0.0, 0.0, 0.003, 3, 1),
               2: (3, 0.05, 0.0, 0.0, 0.004, 0, 3), 1: (4, 1.0, 0.0, 0.0, 0.0005, 2, 7), 3: (5, 0.004, 0.6, 0.85, 0.006, 1, 12)}
OPT_G, OPT_INACTIVE = 7, 4


def opt_case(P, n_reg, seed=0, dyadic=False):
    """[G][S] state, [G][Pp] gradients, [G][8] hyper rows (fp32 values as float64).  dyadic (codes 0 / 1 on members 5
    and 0 only, the others inactive): w, g multiples of 1 / 16 with |.| <= 4 (zeros among them), lr, momentum, wd and
    the gradient scale powers of two, so every product and sum is a multiple of 2^-14 below 2^5: exact at fp32."""
    k = Case()
    g = gen(22000 + P % 9973 + 7 * n_reg % 1009 + seed)
    Pp, S = opt_layout(P)
    k.P, k.Pp, k.S, k.n_reg, k.dyadic = P, Pp, S, n_reg, dyadic
    k.hyper = torch.zeros(OPT_G, 8, dtype=torch.float64)
    for s, (code, lr, mom, dec, wd, reg, t) in OPT_MEMBERS.items():
        act = 1.0
        if dyadic:
            lr, mom, wd = {0: 0.125, 1: 0.25}.get(code, lr), 0.5, 0.25
            act = 1.0 if code in (0, 1) else 0.0
            reg = {0: 3, 1: 1}.get(code, reg)
        k.hyper[s] = torch.tensor([code, lr, mom, dec, wd, reg, t, act], dtype=torch.float32).double()
    k.hyper[OPT_INACTIVE] = torch.tensor([2, 0.01, 0.5, 0.5, 0.01, 3, 2, 0.0], dtype=torch.float32).double()
    if dyadic:
        k.state = _ints(g, (OPT_G, S), -64, 64) / 16
        k.grads = _ints(g, (OPT_G, Pp), -64, 64) / 16
        k.state[:, 0:P:5] = 0.0  # sign(0) = 0
    else:
        k.state = torch.randn(OPT_G, S, generator=g).float().double()
        k.state[:, Pp:3 * Pp] = k.state[:, Pp:3 * Pp].abs() * 0.5 + 0.05  # second-moment slots positive
        k.grads = torch.randn(OPT_G, Pp, generator=g).float().double()
        k.state[:, 0:P:7] = 0.0
        k.state = k.state.float().double()  # every word an fp32 value
    # [P, ceil4(P)): the kernel's last float4 of a row reaches these words.  The engine zeroes the whole row and the
    # gradient buffer and initialises the slots over [0, P) only, so weights, BOTH slots (Adagrad's 0.1 too) and
    # gradients are zero here; every lane at or past P must keep its words (Adagrad: 0 * rsqrt(0) would be NaN)
    p4 = -(-P // 4) * 4
    k.p4 = p4
    for o in (0, Pp, 2 * Pp):
        k.state[:, o + P:o + p4] = 0.0
    k.grads[:, P:p4] = 0.0
    return k


def opt_eval(k, gscale, dtype):
    """(state, magnitude) [G][S] after one launch at ``dtype``; columns outside [0, P) of each region, regions the
    member's optimizer does not own and inactive rows are returned unchanged (magnitude 0: bitwise)."""
    P, Pp, p4 = k.P, k.Pp, k.P
    st, mag = k.state.to(dtype).clone(), torch.zeros(OPT_G, k.S, dtype=dtype)
    for s in range(OPT_G):
        code, lr, mom, dec, wd, reg, t, act = k.hyper[s].tolist()
        if act == 0:
            continue
        code, reg = int(code), int(reg)
        w, a, b = (k.state[s, o:o + p4].to(dtype) for o in (0, Pp, 2 * Pp))
        g = k.grads[s, :p4].to(dtype) * torch.tensor(gscale, dtype=dtype)
        gm = g.abs()
        wdt = torch.tensor(wd, dtype=dtype)
        inreg = torch.arange(p4) < k.n_reg
        if reg in (2, 3):
            g, gm = torch.where(inreg, g + wdt * w, g), torch.where(inreg, gm + (wdt * w).abs(), gm)
        if reg in (1, 3):
            g, gm = torch.where(inreg, g + wdt * torch.sign(w), g), torch.where(inreg, gm + (wdt * torch.sign(w)).abs(), gm)
        w2, a2, b2, wm, am, bm = opt_update(code, w, a, b, g, (lr, mom, dec, t), dtype)
        own_a, own_b = OWNS[code]
        st[s, :p4], mag[s, :p4] = w2, wm
        if own_a:
            st[s, Pp:Pp + p4], mag[s, Pp:Pp + p4] = a2, am
        if own_b:
            st[s, 2 * Pp:2 * Pp + p4], mag[s, 2 * Pp:2 * Pp + p4] = b2, bm
    return st, mag


def check_opt(k):
    act = [s for s in range(OPT_G) if k.hyper[s, 7] != 0]
    assert OPT_INACTIVE not in act and k.hyper[OPT_INACTIVE, 7] == 0
    if k.dyadic:
        assert sorted(int(k.hyper[s, 0]) for s in act) == [0, 1]
        st, _ = opt_eval(k, 0.5, torch.float64)
        st32, _ = opt_eval(k, 0.5, torch.float32)
        assert torch.equal(st32.double(), st) and ax.is_int(st[act] * 2.0 ** 14) and st[act].abs().max() < 2 ** 5
        assert bool((k.state[act, :k.P] == 0).any()) and (k.n_reg == 0 or bool((k.state[act, :k.n_reg] == 0).any()))
    else:
        assert sorted(int(k.hyper[s, 0]) for s in act) == [0, 1, 2, 3, 4, 5]
        assert len({tuple(k.hyper[s, 1:7].tolist()) for s in act}) == 6
        assert [k.hyper[s, 6] for s in act if k.hyper[s, 0] == 2] == [1.0]
        assert act != sorted(act, key=lambda s: k.hyper[s, 0])  # scattered: slot order is not code order
        st, _ = opt_eval(k, 1.0, torch.float64)
        assert bool(torch.isfinite(st).all())
    if 0 < k.n_reg < k.P:  # the first word past the regularised prefix would change if it were regularised
        assert bool((k.state[act, k.n_reg] != 0).all()) and bool((k.hyper[act, 4] != 0).all())
        assert k.dyadic or bool((k.hyper[[s for s in act if k.hyper[s, 0] != 3], 5] != 0).all())
    for o in (0, k.Pp, 2 * k.Pp):  # the engine's padding: zero weight, zero slots, zero gradient
        assert bool((k.state[:, o + k.P:o + k.p4] == 0).all())
    assert bool((k.grads[:, k.P:k.p4] == 0).all())
