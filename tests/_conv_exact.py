"""Constructions for the exact (tolerance 0) tests of the CIFAR forward convolution kernels of ops/csrc/conv.hip
(``dtf_conv_fwd_s1``, ``dtf_conv_fwd``): operands, float64 references, exactness conditions, buffer layouts and
hand-built work lists, all without a device.  Used by tests/test_gpu_conv_fwd.py and, for the conditions themselves,
by tests/test_conv_exact_constructions.py; the layout / work-list half is meant for the backward family too.

Why the comparison can be bitwise.  Both kernels compute the output statistics from the ROUNDED stored value, and the
input BN reads its statistics from a buffer the caller supplies, so the test chooses them.  Every conv input lies on
a grid of unit u (1 for the identity input, 0.5 behind the BN+ReLU input) and every weight is an integer, so each
product and each partial sum, in any order, is a multiple of u; with (``check_case``, asserted on the reference
alone)

* sum of |terms| < 2^24 u per output,
* |y + res| <= 256 u (every multiple of u up to there is a bf16 and an fp16 value),
* per member and channel sum |y| < 2^24 u and sum y^2 < 2^24 u^2 (the seed of the accumulator row included),

every partial sum is exact in fp32 under the MFMA, the LDS and the global atomics in any order, so the atomic and
the fixed-order builds give the same words as the float64 reference.

BN+ReLU input (MODE 1), the snap construction.  ``bn_fwd_coef`` evaluates inv = rsqrtf(max(q / n - mean^2, 0) + 1e-5),
scale = gamma * inv, shift = beta - mean * scale in fp32, none of it bit-specified.  Per (member, channel) the test
picks a target inv in {0.5, 1, 2}, a target mean in {0, +-1, +-2, 0.5}, gamma in {+-0.5, +-1, +-2} and a half-integer
beta, writes q = (1 / inv^2 - 1e-5 + mean^2) n and s = mean n as fp32 words split unevenly over the NREP replicas (one
share negative), and builds x = mean + m / min(|scale|, 1) with a small integer m: x * scale + shift is then ideally
beta + m * max(|scale|, 1) = k + 0.5.  The reference evaluates the transform in float64 FROM THE SAME fp32 replica
words and asserts per staged element v

* |v - snap(v)| <= 2^-12 max(|v|, 1) and |snap(v)| >= 0.5 (nothing on the ReLU edge: the kernel's ReLU runs after the
  rounding), and
* |v - snap(v)| + E < (spacing of bf16 at snap(v)) / 4, where E bounds the kernel's own fp32 error: the replica sums
  carry at most (NREP + 3) 2^-24 A relative error (A = sum |shares| / |sum|), the variance amplifies it by
  K = (q / n) / (var + eps) <= 17, rsqrtf and the two products add a few 2^-24; because the kernel derives shift from
  its own scale, an error d of scale moves v by (x - mean) d only, so E = |v - beta| e_inv + (|x scale| + |shift| +
  |v|) 2^-22 with e_inv = K (NREP + 3) 2^-24 A + 2^-21.  The float64 deviation itself is about 1e-6 relative, the
  bf16 half-spacing is 2^-9 at |v| = 0.5 and grows with |v|,

then uses relu(snap(v)) as the conv input.  One channel per member has gamma = 0, beta = 1.5 and q / n < mean^2 - 1e-5:
with the ``fmaxf(..., 0)`` clamp the staged value is exactly 1.5, without it NaN.

Population.  Capacity 3; hand-listed cases have members in slots 0 and 2 with 3 and 2 images, the arithmetic
(``u_items``) cases members in slots 0 and 1 with 3 images each.  The idle slot's weights, params, statistics and image
count are NaN: any output that read them differs.  Images of all members are packed in one tensor in slot order.
"""
import functools

import torch
import torch.nn.functional as F

import _convg_exact as cx

CAP, EXACT = cx.CAP, cx.EXACT
CANARY = 0.375  # guard / pre-fill word: off the 0.5 grid of the MODE 1 outputs (cx.Y_CANARY = 0.5 is on it)
PRE = 64  # guard elements before and after every device buffer (a multiple of 16 bytes for every element size)
W_OFF, W_TAIL = 24, 40  # weight row: words before the [Co][K][K][Ci] block and after it (NaN)
P_MSTRIDE, IN_GAMMA, IN_BETA = 400, 37, 211  # params row (wider than needed), gamma / beta offsets
BN_EPS = 1e-5
LISTED = ((0, 2), (3, 2))  # (slots, images per member) of the hand-listed cases
UNIFORM = ((0, 1), (3, 3))  # of the arithmetic work-item cases: equal batches, slots packed 0 .. n-1
_M32 = 0xFFFFFFFF


def _hash(shape, seed):
    """A 32-bit mix of the element coordinates: position-dependent, no symmetric or constant planes."""
    h = torch.full(tuple(shape), (seed * 0x632BE5AB + 0x1234567) & _M32, dtype=torch.int64)
    for d, n in enumerate(shape):
        v = [1] * len(shape)
        v[d] = n
        h = h + torch.arange(n, dtype=torch.int64).reshape(v) * (0x9E3779B1 + 2 * 0x51ED27 * d)
        h = (h & _M32) * 0x85EBCA77 & _M32
        h = h ^ (h >> 15)
    h = (h * 0xC2B2AE3D) & _M32
    return h ^ (h >> 16)


def hints(shape, lo, hi, seed):
    """float64 integers in [lo, hi] from the coordinate hash."""
    return (lo + _hash(shape, seed) % (hi - lo + 1)).double()


def hpick(shape, values, seed):
    return torch.tensor(values, dtype=torch.float64)[_hash(shape, seed) % len(values)]


def ranges(slots, sizes):
    """[(slot, first image, end image)] of the packed image tensor."""
    out, f = [], 0
    for s, n in zip(slots, sizes):
        out.append((s, f, f + n))
        f += n
    return out


# --------------------------------------------------------------------------------------------------- work lists
def iter_cuts(lo, hi, bands):
    """Cuts of one member's iterations [lo, hi) (iteration = image * bands + band): a single iteration, then an item
    that starts inside an image, crosses an image boundary and ends inside the next image (whole-image bands: an item
    of several images), then the rest."""
    if bands == 1:
        return sorted({lo, lo + 1, hi})
    return sorted({lo, lo + 1, min(hi, lo + bands + (bands + 1) // 2), hi})


def listed_items(slots, sizes, bands):
    """(it0, nit, 0, slot) rows; the members' items alternate, so neighbouring workgroups serve different members."""
    per = []
    for s, f, e in ranges(slots, sizes):
        cuts = iter_cuts(f * bands, e * bands, bands)
        per.append([[a, b - a, 0, s] for a, b in zip(cuts[:-1], cuts[1:])])
    out = []
    for j in range(max(len(p) for p in per)):
        out += [p[j] for p in reversed(per) if j < len(p)]
    return out


def items_coverage(items, bands):
    nits = {}
    for it0, nit, _, s in items:
        nits.setdefault(s, []).append(nit)
    return {"single_iteration": any(nit == 1 for _, nit, _, _ in items),
            "crosses_image_inside": any(it0 // bands != (it0 + nit - 1) // bands for it0, nit, _, _ in items),
            "uneven_split": any(len(set(v)) > 1 for v in nits.values()),
            "first_item_not_slot0": items[0][3] != 0}


ITEMS_NEED = ("single_iteration", "crosses_image_inside", "uneven_split", "first_item_not_slot0")


def assert_tiling(items, slots, sizes, bands):
    """Every iteration of every member is covered exactly once, by an item of its own slot."""
    want = {s: list(range(f * bands, e * bands)) for s, f, e in ranges(slots, sizes)}
    got = {s: [] for s in slots}
    for it0, nit, z, s in items:
        assert nit >= 1 and z == 0 and s in got, (it0, nit, z, s)
        got[s] += list(range(it0, it0 + nit))
    assert {s: sorted(v) for s, v in got.items()} == want


def uniform_geo(per, chunk):
    """(u_items, u_chunk, u_per) as hip_resnet._set_uniform takes them from _work_iters: (ceil(total / chunk), chunk,
    total) of one member."""
    return -(-per // chunk), chunk, per


def work_item_at(b, u_items, u_chunk, u_per):
    """Host mirror of conv.hip work_item_at for u_items > 0."""
    m = b // u_items
    k = b - m * u_items
    it0 = k * u_chunk
    return [m * u_per + it0, min(u_chunk, u_per - it0), 0, m]


def uniform_chunk(per):
    """A chunk that does not divide `per` (the last item of every member is short)."""
    assert per > 2, per
    return next(c for c in range(min(per - 1, 5), 1, -1) if per % c)


def poison_work(n, idle):
    """A work table the arithmetic form must not read: every row a valid one-iteration item of the idle slot (NaN
    weights and statistics), so a kernel that did read it stays in bounds and writes NaN over image 0."""
    return [[0, 1, 0, idle]] * n


# ------------------------------------------------------------------------------------------------------- cases
class FwdCase:
    """x [N][Hi][Wi][Ci] raw input, xin the conv input (x, or relu(snap(BN(x)))), w [CAP][Co][K][K][Ci], res / y
    [N][Ho][Wo][Co], st [CAP][2][64] the statistics the launch adds; MODE 1: gamma / beta [CAP][Ci], st_in
    [CAP][nrep][2][64] fp32, v the float64 staged values before the snap.  All values float64 unless noted."""


def _weights(c, seed, nz):
    ktot = c.k * c.k * c.cin
    shape = (CAP, c.cout, c.k, c.k, c.cin)
    vals = [-2.0, -1.0, 1.0, 2.0] if c.mode == 0 else [-1.0, 1.0]
    w = hpick(shape, vals, seed)
    keep = _hash(shape, seed + 1) % ktot < nz  # about nz non-zero taps per output channel
    return w * keep


def _bn_input(c, seed):
    """MODE 1 operands of case c (see the module docstring)."""
    n_img = sum(c.sizes)
    ci = c.cin
    inv = hpick((CAP, ci), [0.5, 1.0, 2.0], seed + 10)
    mean = hpick((CAP, ci), [0.0, 1.0, -1.0, 2.0, -2.0, 0.5], seed + 11)
    gamma = hpick((CAP, ci), [0.5, -0.5, 1.0, -1.0, 2.0, -2.0], seed + 12)
    beta = hpick((CAP, ci), [-2.5, -1.5, -0.5, 0.5, 1.5, 2.5], seed + 13)
    qn = 1.0 / inv ** 2 - BN_EPS + mean ** 2  # q / n
    c.clamp_ch = {}
    for s in range(CAP):
        cc = (5 + 3 * s) % ci
        c.clamp_ch[s] = cc
        gamma[s, cc], beta[s, cc], mean[s, cc] = 0.0, 1.5, 2.0
        qn[s, cc] = 4.0 - 1e-3  # variance -1e-3: below -eps, so the sum under the rsqrt is negative without the clamp
    scale = gamma * inv
    step = 1.0 / scale.abs().clamp(max=1.0).clamp(min=0.25)  # x spacing that makes (x - mean) scale an integer
    mmax = (8.0 / scale.abs().clamp(min=1.0)).floor().clamp(min=2.0)
    m = _hash((n_img, c.hi, c.wi, ci), seed + 14)
    x = torch.empty(n_img, c.hi, c.wi, ci, dtype=torch.float64)
    for s, f, e in ranges(c.slots, c.sizes):
        span = 2 * mmax[s] + 1
        x[f:e] = mean[s] + ((m[f:e] % span.long()).double() - mmax[s]) * step[s]
    # replica words: uneven shares of (s, q), one of them negative, rounded to fp32 one by one
    nrep = c.nrep
    share = 1.0 + (_hash((CAP, nrep, 2, 64), seed + 15) % 7).double()
    share[:, 1] = -0.25 * share[:, 1]
    share = share / share.sum(1, keepdim=True)
    cnt = torch.full((CAP,), float("nan"), dtype=torch.float64)
    tot = torch.zeros(CAP, 2, 64, dtype=torch.float64)
    for s, f, e in ranges(c.slots, c.sizes):
        cnt[s] = e - f
        n = (e - f) * c.hi * c.wi
        tot[s, 0, :ci] = (mean[s] * n).float().double()
        tot[s, 1, :ci] = (qn[s] * n).float().double()
    st_in = (share * tot[:, None]).float()
    idle = [s for s in range(CAP) if s not in c.slots]
    st_in[idle] = float("nan")
    gamma[idle] = float("nan")
    beta[idle] = float("nan")
    c.x, c.gamma, c.beta, c.st_in, c.cnt, c.bn_mean, c.bn_inv = x, gamma, beta, st_in, cnt, mean, inv
    # the transform in float64 from the fp32 words the kernel reads
    c.v = torch.empty_like(x)
    c.err = torch.empty_like(x)  # E of the module docstring
    for s, f, e in ranges(c.slots, c.sizes):
        n = (e - f) * c.hi * c.wi
        w = st_in[s].double()
        sm, q = w[:, 0, :ci].sum(0), w[:, 1, :ci].sum(0)
        amp = (w[:, :, :ci].abs().sum(0) / w[:, :, :ci].sum(0).abs().clamp(min=1e-30))
        amp[0] = torch.where(sm == 0, torch.ones_like(sm), amp[0])
        mu = sm / n
        var = (q / n - mu * mu).clamp(min=0.0)
        iv = 1.0 / torch.sqrt(var + float(torch.tensor(BN_EPS, dtype=torch.float32)))
        sc = gamma[s].float().double() * iv
        sh = beta[s].float().double() - mu * sc
        c.v[f:e] = x[f:e] * sc + sh
        kap = (q / n) / (var + BN_EPS)
        e_inv = kap * (nrep + 3) * 2.0 ** -24 * amp.max(0).values + 2.0 ** -21
        e_inv = torch.where(gamma[s] == 0, torch.zeros_like(e_inv), e_inv)  # scale = 0 * inv exactly
        c.err[f:e] = (c.v[f:e] - beta[s]).abs() * e_inv + ((x[f:e] * sc).abs() + sh.abs() + c.v[f:e].abs()) * 2.0 ** -22
    c.snap = torch.floor(c.v) + 0.5
    c.xin = torch.relu(c.snap)


@functools.lru_cache(maxsize=None)
def fwd_case(cin, cout, s, k, mode, resid, hi, wi, rows, uniform=False, nrep=8):
    c = FwdCase()
    c.cin, c.cout, c.s, c.k, c.mode, c.resid, c.hi, c.wi, c.rows, c.nrep = cin, cout, s, k, mode, resid, hi, wi, rows, nrep
    c.slots, c.sizes = UNIFORM if uniform else LISTED
    c.uniform = uniform
    c.ho, c.wo, c.pad = hi // s, wi // s, (k - 1) // 2
    c.bands = c.ho // rows
    c.unit = 1.0 if mode == 0 else 0.5
    seed = ((cin * 131 + cout) * 7 + s * 3 + k) * 1009 + mode * 97 + resid * 31 + hi * 5 + wi + rows * 13 + uniform * 7919
    n_img = sum(c.sizes)
    c.w = _weights(c, seed, 24 if mode == 0 else 12)
    if mode == 0:
        c.x = hints((n_img, hi, wi, cin), -3, 3, seed + 2)
        c.xin = c.x
        c.cnt = torch.full((CAP,), float("nan"), dtype=torch.float64)
        for sl, f, e in ranges(c.slots, c.sizes):
            c.cnt[sl] = e - f
        c.gamma = c.beta = torch.full((CAP, cin), float("nan"), dtype=torch.float64)
        c.st_in = torch.full((CAP, nrep, 2, 64), float("nan"))
    else:
        _bn_input(c, seed)
    c.res = hints((n_img, c.ho, c.wo, cout), -8, 8, seed + 3) if resid else None
    c.y = torch.empty(n_img, c.ho, c.wo, cout, dtype=torch.float64)
    c.absy = torch.empty_like(c.y)  # sum of |terms| behind each output
    c.st = torch.zeros(CAP, 2, 64, dtype=torch.float64)
    c.st_abs = torch.zeros(CAP, 64, dtype=torch.float64)
    for sl, f, e in ranges(c.slots, c.sizes):
        wn = c.w[sl].permute(0, 3, 1, 2).contiguous()
        xn = c.xin[f:e].permute(0, 3, 1, 2).contiguous()
        y = F.conv2d(xn, wn, stride=s, padding=c.pad).permute(0, 2, 3, 1)
        ab = F.conv2d(xn.abs(), wn.abs(), stride=s, padding=c.pad).permute(0, 2, 3, 1)
        if resid:
            y, ab = y + c.res[f:e], ab + c.res[f:e].abs()
        c.y[f:e], c.absy[f:e] = y, ab
        c.st[sl, 0, :cout], c.st[sl, 1, :cout] = y.sum((0, 1, 2)), (y * y).sum((0, 1, 2))
        c.st_abs[sl, :cout] = y.abs().sum((0, 1, 2))
    idle = [sl for sl in range(CAP) if sl not in c.slots]
    c.idle = idle[0]
    c.w[idle] = float("nan")
    c.st_seed = 1.0 + hints((CAP, nrep, 2, 64), 0, 4, seed + 4)  # the accumulator rows before the launch: 1 .. 5
    if uniform:
        c.u = uniform_geo(c.sizes[0] * c.bands, uniform_chunk(c.sizes[0] * c.bands))
        c.items = [work_item_at(b, *c.u) for b in range(c.u[0] * len(c.slots))]
    else:
        c.u = (0, 0, 0)
        c.items = listed_items(c.slots, c.sizes, c.bands)
    return c


def check_case(c):
    """Every exactness and snap condition of a case, on the operands and the reference alone."""
    u = c.unit
    for t in (c.x, c.w[list(c.slots)], c.y) + ((c.res,) if c.resid else ()):
        for dt in (torch.bfloat16, torch.float16):
            assert torch.equal(t.to(dt).double(), t), "operand not representable"
    assert bool((c.w[list(c.slots)] == c.w[list(c.slots)].round()).all())
    assert bool((c.xin / u == (c.xin / u).round()).all()) and bool((c.y / u == (c.y / u).round()).all())
    assert c.absy.max() < EXACT * u, float(c.absy.max())
    assert c.y.abs().max() <= 256 * u, float(c.y.abs().max())
    seed_abs = c.st_seed.abs().sum(1).max()
    assert c.st_abs.max() + seed_abs < EXACT * u, float(c.st_abs.max())
    assert c.st[:, 1].max() + seed_abs < EXACT * u * u, float(c.st[:, 1].max())
    assert bool((c.st_seed != 0).all()) and bool((c.st_seed == c.st_seed.round()).all())
    # no constant or mirror-symmetric input planes, every input channel (the padded stem channels too) used
    assert bool((c.x.flip(1) != c.x).any()) and bool((c.x.flip(2) != c.x).any())
    assert bool((c.x.reshape(-1, c.cin).std(0) > 0).all())
    for sl in c.slots:
        assert bool(((c.w[sl] != 0).sum((0, 1, 2)) > 0).all()), "an input channel without a weight"
        assert bool(((c.w[sl] != 0).sum((1, 2, 3)) > 0).all()), "an output channel without a weight"
    assert not torch.equal(c.w[c.slots[0]], c.w[c.slots[1]])
    assert bool(torch.isnan(c.w[c.idle]).all()) and bool(torch.isnan(c.cnt[c.idle]))
    if c.mode == 1:
        v, sn = c.v, c.snap
        assert bool(((v - sn).abs() <= 2.0 ** -12 * v.abs().clamp(min=1.0)).all()), float((v - sn).abs().max())
        assert sn.abs().min() >= 0.5 and sn.abs().max() <= 63.5
        quarter = 2.0 ** (torch.floor(torch.log2(sn.abs())) - 7 - 2)  # bf16 spacing at snap / 4 (fp16 is finer)
        assert bool(((v - sn).abs() + c.err < quarter).all()), float(((v - sn).abs() + c.err).max())
        for sl, f, e in ranges(c.slots, c.sizes):
            cc = c.clamp_ch[sl]
            assert c.gamma[sl, cc] == 0 and bool((v[f:e, :, :, cc] == 1.5).all())
            w = c.st_in[sl].double()
            n = (e - f) * c.hi * c.wi
            assert float(w[:, 1, cc].sum() / n - (w[:, 0, cc].sum() / n) ** 2) < -BN_EPS  # NaN without the clamp
            assert bool((c.gamma[sl] < 0).any()) and bool((c.bn_mean[sl] != 0).any())
            share = w[:, :, :c.cin]  # uneven replica shares, one negative (a zero sum has zero shares)
            nz = share.sum(0) != 0
            assert bool(((share < 0).any(0) | ~nz).all()) and bool(((share.max(0).values != share.min(0).values) | ~nz).all())
        assert bool(torch.isnan(c.st_in[c.idle]).all()) and bool(torch.isnan(c.gamma[c.idle]).all())
    assert_tiling(c.items, c.slots, c.sizes, c.bands)
    if c.uniform:
        ui, uc, up = c.u
        assert up % uc != 0 and ui == -(-up // uc) and c.slots == tuple(range(len(c.slots))) and len(set(c.sizes)) == 1
    else:
        cov = items_coverage(c.items, c.bands)
        assert all(cov[k] for k in ITEMS_NEED), cov


# --------------------------------------------------------------------------------------------- buffer layouts
def guarded(t, dt):
    """Host buffer [PRE canaries | t | PRE canaries] of dtype dt (the live region starts PRE elements in)."""
    flat = torch.full((t.numel() + 2 * PRE,), CANARY, dtype=dt)
    flat[PRE:PRE + t.numel()] = t.reshape(-1).to(dt)
    return flat


def live(buf, shape):
    n = 1
    for d in shape:
        n *= d
    return buf[PRE:PRE + n].reshape(shape)


def guards_intact(buf, n):
    b = buf.double()
    return bool((b[:PRE] == CANARY).all()) and bool((b[PRE + n:] == CANARY).all())


def weight_rows(c):
    """[CAP][w_mstride]: NaN, then the member's [Co][K][K][Ci] block at W_OFF (the idle slot: NaN throughout)."""
    n = c.cout * c.k * c.k * c.cin
    rows = torch.full((CAP, W_OFF + n + W_TAIL), float("nan"), dtype=torch.float64)
    rows[:, W_OFF:W_OFF + n] = c.w.reshape(CAP, -1)
    return rows


def param_rows(c):
    rows = torch.full((CAP, P_MSTRIDE), float("nan"), dtype=torch.float64)
    if c.mode == 1:
        rows[:, IN_GAMMA:IN_GAMMA + c.cin] = c.gamma
        rows[:, IN_BETA:IN_BETA + c.cin] = c.beta
    return rows


def lds_s1(c, wpitch, cpad_fwd):
    """Dynamic LDS of a dtf_conv_fwd_s1 launch (hip_resnet._conv_fwd)."""
    return 1280 + 2 * (((c.rows + 2) * wpitch * cpad_fwd + 8 + 63) // 64 * 64) * 2


def lds_generic(c, cpad):
    """Dynamic LDS of a dtf_conv_fwd launch (hip_resnet._conv_fwd, with the tile width from Wi)."""
    rows_in = (c.rows - 1) * c.s + c.k
    return 1280 + 2 * ((rows_in * (c.wi + 2 * c.pad) * cpad + 8 + 63) // 64 * 64) * 2


def generic_fits(c):
    """The launch limits _conv_fwd keeps: whole bands, whole 16-pixel tiles, at most 4 staging chunks per thread and
    MAXT = 4 output tiles per wave."""
    rows_in = (c.rows - 1) * c.s + c.k
    wpt = 4 // (c.cout // 16)
    return (c.ho % c.rows == 0 and (c.rows * c.wo) % 16 == 0
            and rows_in * (c.wi + 2 * c.pad) * (c.cin // 8) <= 4 * 256 and c.rows * c.wo // 16 <= 4 * wpt)


# ------------------------------------------------------------------------------------------------- case tables
# dtf_conv_fwd_s1: (C, mode, resid, rows); the geometry is the kernel's own (H = W = 512 / C)
S1_CASES = [(16, 0, 0, 8), (32, 0, 0, 8), (64, 0, 0, 8)] + [(cc, 1, r, 8) for cc in (16, 32, 64) for r in (0, 1)] + [
    (64, 1, 0, 4), (64, 1, 1, 4)]
S1_REJECTS = [(32, 1, 0, 4), (64, 0, 0, 4), (48, 1, 0, 8)]  # rows = 4 at C = 32, rows = 4 with mode 0, C = 48


def s1_case(cc, mode, resid, rows, uniform, nrep=8):
    return fwd_case(cc, cc, 1, 3, mode, resid, 512 // cc, 512 // cc, rows, uniform, nrep)


# dtf_conv_fwd: every FWD_CASE row (cin, cout, s, k, mode, resid, stats) at the production geometry (Hi, Wi, rows)
GEN_CASES = [
    (16, 16, 1, 3, 0, 0, 1, 32, 32, 8), (16, 16, 1, 3, 1, 0, 1, 32, 32, 8), (16, 16, 1, 3, 1, 1, 1, 32, 32, 8),
    (32, 32, 1, 3, 1, 0, 1, 16, 16, 8), (32, 32, 1, 3, 1, 1, 1, 16, 16, 8),
    (64, 64, 1, 3, 1, 0, 1, 8, 8, 8), (64, 64, 1, 3, 1, 1, 1, 8, 8, 8),
    (16, 32, 2, 3, 1, 0, 1, 32, 32, 4), (32, 64, 2, 3, 1, 0, 1, 16, 16, 4),
    (16, 16, 1, 1, 1, 0, 0, 32, 32, 8), (16, 32, 2, 1, 1, 0, 0, 32, 32, 8), (32, 64, 2, 1, 1, 0, 0, 16, 16, 8),
    (16, 32, 2, 3, 0, 0, 1, 32, 32, 4), (32, 64, 2, 3, 0, 0, 1, 16, 16, 4),
    (16, 16, 1, 1, 0, 0, 1, 32, 32, 8), (16, 32, 2, 1, 0, 0, 1, 32, 32, 8), (32, 64, 2, 1, 0, 0, 1, 16, 16, 8),
    (32, 32, 1, 3, 0, 0, 1, 16, 16, 8), (64, 64, 1, 3, 0, 0, 1, 8, 8, 8),
]
# second, smaller geometries (Hi 16, band height other than 8) and non-square images (the planner only sends squares)
GEN_EXTRA = [
    (16, 32, 2, 3, 1, 0, 1, 16, 16, 2), (16, 32, 2, 3, 1, 0, 1, 32, 16, 4),
    (16, 16, 1, 3, 1, 1, 1, 16, 16, 4), (16, 16, 1, 3, 1, 1, 1, 16, 32, 2),
]
GEN_REJECT = (16, 64, 2, 3, 1, 0, 1)  # no such instantiation


def gen_case(row, nrep=8):
    cin, cout, s, k, mode, resid, stats, hi, wi, rows = row
    c = fwd_case(cin, cout, s, k, mode, resid, hi, wi, rows, False, nrep)
    return c, stats


def all_cases(nrep):
    out = [s1_case(*r, uniform=u, nrep=nrep) for r in S1_CASES for u in (False, True)]
    return out + [gen_case(r, nrep)[0] for r in GEN_CASES + GEN_EXTRA]
