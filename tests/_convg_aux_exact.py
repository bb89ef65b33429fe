"""Constructions and float64 CPU references for the kernel-level tests of the ImageNet auxiliary kernels
(ops/csrc/convg_aux.hip and the fp32 pool of ops/csrc/f32net.hip), built without a device.  Used by
tests/test_gpu_convg_aux.py and, for the exactness conditions themselves, tests/test_convg_aux_constructions.py.

The pattern is that of tests/_convg_exact.py: operands are small integers held in the 16-bit activation type,
coefficients small integers (powers of two where a kernel multiplies by 1 / sigma), so every product and partial
sum is an integer (or a multiple of 1/2 resp. 1/16 where noted) far below 2^24 -- exact in fp32 in any order, under
atomics and in the deterministic build's fixed point -- and every stored value is representable in bf16 and fp16.
A correct kernel reproduces the float64 reference bit for bit.  Two members sit in slots 0 and 2 of a capacity-3
table, their images packed ragged (2 + 3) in one tensor; the unused slot's rows hold non-zero data.

The launchers that use rsqrtf / __expf / __logf (BN finalize, softmax cross-entropy) are evaluated by one formula
in float64 (the reference) and in float32 (the yardstick of the tolerance): ``deviation`` scales every error by the
sum of the magnitudes of the terms behind the element, so cancellation does not inflate it.
"""
import functools

import torch
import torch.nn.functional as F

from _convg_exact import CAP, EXACT, INT_EXACT, SLOTS, _ints, member_ranges  # noqa: F401 (re-exported)

ACMAX = 2056  # row length of the coefficient / sum tables: wider than the widest layer, so rows have dead tails
CANARY = 0.5  # output pre-fill: no integer
AM_CANARY = 0xEE  # argmax-byte pre-fill: no tap number
SIZES = (2, 3)
BN_EPS = float(torch.tensor(1e-5, dtype=torch.float32))  # the kernels' float constants, exactly
BN_MOM = float(torch.tensor(0.997, dtype=torch.float32))
BN_ONE_M = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(0.997, dtype=torch.float32))


class Case:
    pass


def img_slots(sizes):
    return [s for s, f, e in member_ranges(sizes) for _ in range(f, e)]


def is_int(t, unit=1.0):
    return bool(((t / unit) == (t / unit).round()).all())


def per_image(table, sizes, row, c):
    """[N][1][c]: row ``row`` of every image's member in a [CAP][4][ACMAX] table."""
    return table[img_slots(sizes), row, :c].unsqueeze(1)


def int_table(g, rows):
    """[CAP][4][ACMAX] of integers, row r uniform in rows[r] = (lo, hi), over the whole width and every slot."""
    return torch.stack([_ints(g, (CAP, ACMAX), lo, hi) for lo, hi in rows], 1)


def pow2_row(g):
    return torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (CAP, ACMAX), generator=g)]


# ------------------------------------------------------------------------------------------------- max-pool
POOL_GEO = [(8, 8), (6, 10), (7, 5)]  # (H, W); Ho = ceil(H / 2): even sizes -> bwd2 kernel, (7, 5) -> per-pixel
POOL_C = (8, 24)
POOL_GEO_F32 = [(8, 8), (7, 5)]
POOL_C_F32 = (4, 12)
POOL_N = 3


def pool_out(h):
    return (h + 1) // 2


def pool_taps(x):
    """[9][N][Ho][Wo][C]: tap t = 3 dy + dx of window o is x[2 oy + dy][2 ox + dx], -inf outside the image."""
    n, h, w, c = x.shape
    ho, wo = pool_out(h), pool_out(w)
    xp = F.pad(x, (0, 0, 0, 2 * wo + 1 - w, 0, 2 * ho + 1 - h), value=float("-inf"))
    return torch.stack([xp[:, dy:dy + 2 * ho:2, dx:dx + 2 * wo:2] for dy in range(3) for dx in range(3)])


def pool_fwd_ref(x):
    """(y, argmax): the clipped 3x3 / 2 window; the first tap in row-major order that attains the maximum."""
    t = pool_taps(x)
    y = t.max(0).values
    first = torch.arange(9, 0, -1).view(9, 1, 1, 1, 1)
    return y, 9 - ((t == y) * first).max(0).values


def pool_bwd_ref(g, am, h, w):
    """(dx, sum of |terms|): every output's gradient goes to the pixel its argmax names."""
    n, ho, wo, c = g.shape
    dp = torch.zeros(n, 2 * ho + 1, 2 * wo + 1, c, dtype=torch.float64)
    ab = torch.zeros_like(dp)
    for t in range(9):
        dy, dx = divmod(t, 3)
        dp[:, dy:dy + 2 * ho:2, dx:dx + 2 * wo:2] += g * (am == t)
        ab[:, dy:dy + 2 * ho:2, dx:dx + 2 * wo:2] += g.abs() * (am == t)
    assert bool((ab[:, h:] == 0).all()) and bool((ab[:, :, w:] == 0).all())  # no argmax names a padding tap
    return dp[:, :h, :w].contiguous(), ab[:, :h, :w].contiguous()


@functools.lru_cache(maxsize=None)
def pool_case(h, w, c):
    k = Case()
    g = torch.Generator().manual_seed(7000 + 100 * h + 10 * w + c)
    k.h, k.w, k.c, k.ho, k.wo = h, w, c, pool_out(h), pool_out(w)
    k.x = _ints(g, (POOL_N, h, w, c), -3, 3)
    k.x[1] = _ints(g, (h, w, c), -3, -1)  # an all-negative image: padding must act as -inf, not 0
    k.y, k.am = pool_fwd_ref(k.x)
    k.g = _ints(g, (POOL_N, k.ho, k.wo, c), -2, 2)
    k.dx, k.dx_abs = pool_bwd_ref(k.g, k.am, h, w)
    return k


def check_pool(k):
    assert is_int(k.x) and k.x.abs().max() <= 3 and k.x[1].max() <= -1 and is_int(k.g) and k.g.abs().max() <= 2
    assert is_int(k.y) and k.y.abs().max() <= 3 and k.am.min() >= 0 and k.am.max() <= 8
    assert is_int(k.dx) and k.dx_abs.max() <= 4 * 2  # at most 4 windows hold one pixel
    t = pool_taps(k.x)
    assert torch.equal(t.gather(0, k.am.unsqueeze(0))[0], k.y)  # x[argmax] == y
    earlier = torch.arange(9).view(9, 1, 1, 1, 1) < k.am.unsqueeze(0)
    assert not bool(((t == k.y) & earlier).any())  # no earlier tap attains the maximum
    assert bool(((t == k.y).sum(0) > 1).any()), "ties must occur"
    if k.h % 2 == 0:  # the last window has no third row: taps 6, 7, 8 absent
        assert k.am[:, -1].max() <= 5
    if k.w % 2 == 0:
        assert bool((k.am[:, :, -1] % 3 != 2).all())
    assert bool((k.y[1] <= -1).all())


# --------------------------------------------------------------------------------- elementwise BN apply passes
def apply_path(c, hw, nimg):
    """Mirror of the launchers dtf_cg_bn_relu_apply / _bwd_apply / _bn_add_relu: which kernel, its grid, and
    whether slots u >= 1 of the EW_U = 4 unroll run ('multi') and some thread stops inside an unroll ('mid')."""
    n8 = hw * c // 8
    split = max(1, min(-(-4096 // nimg), -(-n8 // 256)))
    cpp = c >> 3
    p = {"n8": n8}
    if c % 8 == 0 and 1 <= cpp <= 256 and cpp & (cpp - 1) == 0:
        ppi = 256 // cpp
        mp = -(-hw // ppi)
        sp = min(split, mp)
        p.update(kernel="cf", ppi=ppi, mp=mp, grid_y=sp, units=hw, step=sp * ppi, ragged=hw % ppi != 0)
    else:
        p.update(kernel="walk", grid_y=split, units=n8, step=split * 256, ragged=n8 % 256 != 0)
    counts = {-(-(p["units"] - u0) // p["step"]) for u0 in range(min(p["units"], p["step"]))}
    p["multi"] = max(counts) > 1
    p["mid"] = any(n % 4 for n in counts if n > 1)
    return p


# (name, C, hw, sizes, expected kernel, multi)
APPLY_SMALL = [("cf-c8", 8, 9, SIZES, "cf", False), ("cf-c64", 64, 49, SIZES, "cf", False),
               ("cf-c2048", 2048, 49, SIZES, "cf", False), ("walk-c24", 24, 49, SIZES, "walk", False),
               ("walk-c72", 72, 49, SIZES, "walk", False)]
# the smallest multi-pass shapes: the channel-fixed kernels need ceil(4096 / images) < ceil(hw / ppi), about 8.4 M
# elements whatever the width; one width per kernel
APPLY_MULTI = {"relu": ("cf-multi-c512", 512, 196, (63, 65), "cf", True),
               "bwd": ("cf-multi-c64", 64, 529, (127, 129), "cf", True),
               "add": ("cf-multi-c2048", 2048, 66, (31, 33), "cf", True)}
APPLY_WALK_MULTI = ("walk-multi-c24", 24, 74 * 74, (31, 33), "walk", True)


def apply_geos(kind):
    return APPLY_SMALL + [APPLY_MULTI[kind], APPLY_WALK_MULTI]


# variants: relu (0,), bwd (0: no add, 1: add), add (0: identity shortcut, 1: projection BN); the 8 M-element
# shapes run the fuller variant only
def apply_variants(kind, multi):
    return (0,) if kind == "relu" else ((1,) if multi else (0, 1))


@functools.lru_cache(maxsize=4)
def apply_case(kind, c, hw, sizes, variant):
    k = Case()
    g = torch.Generator().manual_seed(9000 + 13 * c + hw + 7 * variant + {"relu": 0, "bwd": 1, "add": 2}[kind])
    n = sum(sizes)
    k.kind, k.c, k.hw, k.sizes, k.variant, k.n = kind, c, hw, sizes, variant, n
    if kind == "relu":
        k.coef = int_table(g, [(1, 2), (-3, 3), (-3, 3), (-3, 3)])
        k.h = _ints(g, (n, hw, c), -4, 4)
        k.out = torch.relu(k.h * per_image(k.coef, sizes, 0, c) + per_image(k.coef, sizes, 1, c))
        k.bound = 4 * 2 + 3
    elif kind == "bwd":
        k.coef = int_table(g, [(-2, 2), (-2, 2), (-2, 2), (-3, 3)])
        k.dz, k.h = _ints(g, (n, hw, c), -3, 3), _ints(g, (n, hw, c), -3, 3)
        k.add = _ints(g, (n, hw, c), -3, 3) if variant else None
        k.out = k.dz * per_image(k.coef, sizes, 0, c)
        k.out += k.h * per_image(k.coef, sizes, 1, c)
        k.out += per_image(k.coef, sizes, 2, c)
        if variant:
            k.out += k.add
        k.bound = 2 * 3 + 2 * 3 + 2 + 3
    else:
        k.coef = int_table(g, [(1, 2), (-3, 3), (-3, 3), (-3, 3)])
        k.coef_s = int_table(g, [(1, 2), (-3, 3), (-3, 3), (-3, 3)]) if variant else None
        k.h, k.s = _ints(g, (n, hw, c), -4, 4), _ints(g, (n, hw, c), -4, 4)
        k.out = k.h * per_image(k.coef, sizes, 0, c) + per_image(k.coef, sizes, 1, c)
        if variant:
            k.out += k.s * per_image(k.coef_s, sizes, 0, c) + per_image(k.coef_s, sizes, 1, c)
        else:
            k.out += k.s
        k.out = torch.relu(k.out)
        k.bound = 2 * (4 * 2 + 3)
    return k


def check_apply(k):
    assert is_int(k.out) and k.out.abs().max() <= k.bound <= min(INT_EXACT.values())
    assert is_int(k.coef) and is_int(k.h)
    if k.kind == "relu" or k.kind == "add":
        assert bool(((k.coef[:, 0] == 1) | (k.coef[:, 0] == 2)).all()) and k.coef[:, 1].abs().max() <= 3
        assert k.h.abs().max() <= 4 and bool((k.out == 0).any()) and bool((k.out > 0).any())
    else:
        assert k.coef[:, :3].abs().max() <= 2 and k.dz.abs().max() <= 3 and k.h.abs().max() <= 3
    assert bool((k.coef[1] != 0).any())  # the unused slot's rows are not zero


# ------------------------------------------------------------------------ channel statistics, BN-backward sums
STAT_C = (8, 64, 2048)
STAT_HW = (1, 49)
STAT_REJECT = (24, 4096)


def stats_split(c):
    """Mirror of dtf_cg_chan_stats / dtf_cg_bn_bwd_sums: workgroups per image, or None where they return -2."""
    if c > 2048 or c % 8 or 2048 % c:
        return None
    return max(1, min(8, 2048 // c))


def _acc_rows(g):
    return _ints(g, (CAP, 2, ACMAX), -3, 3)


def _scatter_sums(dst, absd, vals, sizes, c, row):
    """dst[slot][row][:c] += sum over the member's images and pixels of vals [N][hw][c]; |.| likewise."""
    for s, f, e in member_ranges(sizes):
        dst[s, row, :c] += vals[f:e].sum((0, 1))
        absd[s, row, :c] += vals[f:e].abs().sum((0, 1))


@functools.lru_cache(maxsize=None)
def stats_case(c, hw):
    k = Case()
    g = torch.Generator().manual_seed(11000 + c + hw)
    k.c, k.hw, k.sizes = c, hw, SIZES
    k.x = _ints(g, (sum(SIZES), hw, c), -3, 3)
    k.prefill = _acc_rows(g)
    k.ref, k.absref = k.prefill.clone(), k.prefill.abs()
    _scatter_sums(k.ref, k.absref, k.x, SIZES, c, 0)
    _scatter_sums(k.ref, k.absref, k.x * k.x, SIZES, c, 1)
    return k


def check_stats(k):
    assert is_int(k.x) and k.x.abs().max() <= 3 and is_int(k.ref) and k.absref.max() < EXACT
    assert torch.equal(k.ref[1], k.prefill[1]) and torch.equal(k.ref[:, :, k.c:], k.prefill[:, :, k.c:])
    assert stats_split(k.c) is not None and (stats_split(k.c) * 256 * 8) % k.c == 0  # the kernel's own condition


@functools.lru_cache(maxsize=None)
def bnsum_case(c, hw, two):
    """sum dz and sum dz (h - mean) inv per member and channel (and the second BN's, which shares sum dz); mean an
    integer and inv a power of two, so every term is a multiple of 1/2."""
    k = Case()
    g = torch.Generator().manual_seed(12000 + c + hw + two)
    k.c, k.hw, k.sizes, k.two = c, hw, SIZES, two
    n = sum(SIZES)
    k.dz, k.h = _ints(g, (n, hw, c), -3, 3), _ints(g, (n, hw, c), -3, 3)
    k.fc = int_table(g, [(-3, 3), (-3, 3), (-2, 2), (0, 0)])
    k.fc[:, 3] = pow2_row(g)
    k.prefill = _acc_rows(g)
    k.ref, k.absref = k.prefill.clone(), k.prefill.abs()
    _scatter_sums(k.ref, k.absref, k.dz, SIZES, c, 0)
    _scatter_sums(k.ref, k.absref, k.dz * (k.h - per_image(k.fc, SIZES, 2, c)) * per_image(k.fc, SIZES, 3, c),
                  SIZES, c, 1)
    k.prefill2 = _acc_rows(g)
    k.ref2, k.absref2 = k.prefill2.clone(), k.prefill2.abs()
    k.h2 = k.fc2 = None
    if two:
        k.h2 = _ints(g, (n, hw, c), -3, 3)
        k.fc2 = int_table(g, [(-3, 3), (-3, 3), (-2, 2), (0, 0)])
        k.fc2[:, 3] = pow2_row(g)
        _scatter_sums(k.ref2, k.absref2, k.dz, SIZES, c, 0)
        _scatter_sums(k.ref2, k.absref2,
                      k.dz * (k.h2 - per_image(k.fc2, SIZES, 2, c)) * per_image(k.fc2, SIZES, 3, c), SIZES, c, 1)
    return k


def check_bnsum(k):
    for t in (k.dz, k.h) + ((k.h2,) if k.two else ()):
        assert is_int(t) and t.abs().max() <= 3
    for fc in (k.fc,) + ((k.fc2,) if k.two else ()):
        assert is_int(fc[:, 2]) and fc[:, 2].abs().max() <= 2
        assert bool(((fc[:, 3] == 0.5) | (fc[:, 3] == 1) | (fc[:, 3] == 2)).all())
    for r, a in ((k.ref, k.absref), (k.ref2, k.absref2)):
        assert is_int(r, 0.5) and 2 * a.max() < EXACT  # in units of 1/2
    assert torch.equal(k.ref[1], k.prefill[1]) and torch.equal(k.ref2[1], k.prefill2[1])
    if not k.two:
        assert torch.equal(k.ref2, k.prefill2)


# ----------------------------------------------------------------------------------------------------- GAP
GAP_C = (8, 64, 2048)
GAP_HW = (1, 4, 16)


@functools.lru_cache(maxsize=None)
def gap_case(c, hw, v2):
    """which 0: feat = mean_p relu(x scale + shift) (v2) or mean_p x (v1); which 1 (v2): the final BN's backward sums
    of dz = dfeat / hw where x scale + shift > 0; which 2: A dz + B x + C (v2) or dfeat / hw where x > 0 (v1).
    dfeat holds multiples of hw, so dfeat / hw is an integer at any hw (1 / hw itself is exact for hw 1, 4, 16)."""
    k = Case()
    g = torch.Generator().manual_seed(13000 + c + 3 * hw + v2)
    k.c, k.hw, k.v2, k.sizes = c, hw, v2, SIZES
    n = sum(SIZES)
    k.x = _ints(g, (n, hw, c), -4, 4)
    k.coef = int_table(g, [(1, 2), (-3, 3), (-2, 2), (0, 0)])
    k.coef[:, 3] = pow2_row(g)
    k.bcoef = int_table(g, [(-2, 2), (-2, 2), (-2, 2), (-3, 3)])
    k.dfeat = _ints(g, (n, c), -2, 2) * hw
    gg = (k.dfeat / hw).unsqueeze(1)  # [N][1][c]
    if v2:
        a = torch.relu(k.x * per_image(k.coef, SIZES, 0, c) + per_image(k.coef, SIZES, 1, c))
        mask = (a > 0).double()
        k.act_sum = a.sum(1)
        k.n_masked = int((mask == 0).sum())
        dz = gg * mask
        k.out = dz * per_image(k.bcoef, SIZES, 0, c) + k.x * per_image(k.bcoef, SIZES, 1, c) + \
            per_image(k.bcoef, SIZES, 2, c)
        k.prefill = _acc_rows(g)
        k.ref, k.absref = k.prefill.clone(), k.prefill.abs()
        _scatter_sums(k.ref, k.absref, dz, SIZES, c, 0)
        _scatter_sums(k.ref, k.absref,
                      dz * (k.x - per_image(k.coef, SIZES, 2, c)) * per_image(k.coef, SIZES, 3, c), SIZES, c, 1)
    else:
        k.act_sum = k.x.sum(1)
        k.out = gg * (k.x > 0)
    k.feat = k.act_sum / hw
    return k


def check_gap(k, exact=True):
    assert is_int(k.x) and k.x.abs().max() <= 4 and is_int(k.dfeat / k.hw) and (k.dfeat / k.hw).abs().max() <= 2
    assert is_int(k.act_sum) and k.act_sum.abs().max() <= min(INT_EXACT.values())
    assert is_int(k.out) and k.out.abs().max() <= 2 * 2 + 2 * 4 + 2
    if exact:
        assert k.hw & (k.hw - 1) == 0 and k.hw <= 16  # sum / hw keeps the sum's (<= 8) significant bits
        for dt in INT_EXACT:
            assert torch.equal(k.feat.to(dt).double(), k.feat)
    if k.v2:
        assert k.n_masked * 8 > k.x.numel(), "many pixels with x scale + shift <= 0"
        assert is_int(k.ref, 0.5) and 2 * k.absref.max() < EXACT and torch.equal(k.ref[1], k.prefill[1])


# ---------------------------------------------------------------------------- layout + rounding (prep kernels)
def s2d_blocks(img):
    """[N][H][W][c] -> [N][H/2][W/2][16]: channel (2 dy + dx) c_in + c = img[2 by + dy][2 bx + dx][c], rest zero."""
    n, h, w, c = img.shape
    out = torch.zeros(n, h // 2, w // 2, 16, dtype=img.dtype)
    out[..., :4 * c] = img.reshape(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n, h // 2, w // 2, 4 * c)
    return out


# cg_weight_prep table rows {w_off, cout, cin, k, cin_pad, fwd_off, dgr_off, 0}: the vector row (1 x 1, cin_pad ==
# cin, element count a multiple of 4, 16-byte aligned source in every slot) without a data-gradient copy; a padded 3 x 3
# row (cin 3 -> 8) and an unpadded scalar row (15 elements) at odd offsets, both with the flipped / transposed copy
WP_S, WP_W = 400, 800  # state / shadow row strides (multiples of 4)
WP_TABLE = [[8, 16, 8, 1, 8, 8, -1, 0], [139, 8, 3, 3, 8, 144, 5, 0], [357, 3, 5, 1, 5, 729, 229, 0]]


def weight_prep_expected(state, dt):
    """(wf, wd) [CAP][WP_W] as doubles after the launch over SLOTS, from canary-filled buffers."""
    wf = torch.full((CAP, WP_W), CANARY, dtype=torch.float64)
    wd = torch.full((CAP, WP_W), CANARY, dtype=torch.float64)
    for s in SLOTS:
        for w_off, cout, cin, k, cin_pad, fwd_off, dgr_off, _ in WP_TABLE:
            kk = k * k
            w = state[s, w_off:w_off + cout * kk * cin].to(dt).double().view(cout, kk, cin)
            f = torch.zeros(cout, kk, cin_pad, dtype=torch.float64)
            f[:, :, :cin] = w
            wf[s, fwd_off:fwd_off + f.numel()] = f.reshape(-1)
            if dgr_off >= 0:  # d[ci][tap][co] = W[co][kk - 1 - tap][ci]
                wd[s, dgr_off:dgr_off + w.numel()] = w.flip(1).permute(2, 1, 0).reshape(-1)
    return wf, wd


def check_weight_prep_table():
    spans_f, spans_d = [], []
    for row, (w_off, cout, cin, k, cin_pad, fwd_off, dgr_off, _) in enumerate(WP_TABLE):
        nf = cout * k * k * cin_pad
        vec = cin_pad == cin and nf % 4 == 0
        assert vec == (row == 0)
        if vec:
            assert all((s * WP_S + w_off) % 4 == 0 and (s * WP_W + fwd_off) % 4 == 0 for s in SLOTS)
        assert w_off + cout * k * k * cin <= WP_S
        spans_f.append((fwd_off, fwd_off + nf))
        if dgr_off >= 0:
            spans_d.append((dgr_off, dgr_off + cout * k * k * cin))
    for spans in (spans_f, spans_d):
        spans.sort()
        assert spans[0][0] > 0 and spans[-1][1] < WP_W and all(a[1] < b[0] for a, b in zip(spans[:-1], spans[1:]))


# --------------------------------------------------------------------------------- non-exact: scaled deviation
def deviation(got, ref, mag):
    """max |got - ref| / mag over the elements (mag: the summed magnitude of the terms behind each element, from
    the float64 evaluation); where mag == 0 the element must be reproduced exactly."""
    got, ref, mag = got.double(), ref.double(), mag.double()
    zero = mag == 0
    assert torch.equal(got[zero], ref[zero])
    if bool(zero.all()):
        return 0.0
    return float(((got - ref).abs()[~zero] / mag[~zero]).max())


# ------------------------------------------------------------------------------------------------ BN finalize
BNF_C = 72  # not a multiple of 64: the workgroup's tail threads return
BNF_GAMMA, BNF_BETA, BNF_RUN = 16, 16 + BNF_C + 8, 16 + 2 * (BNF_C + 8)
BNF_S = BNF_RUN + 2 * BNF_C + 24
BNF_CNT = {0: 2.0, 1: 5.0, 2: 3.0}


@functools.lru_cache(maxsize=None)
def bnfin_case(hw):
    """hw 4: sums of integer data in [-2, 2] with two entries forced to -2 and +2 (variance >= 8 / n >= 0.66, |mean|
    <= 2) and channel 0 constant 2 (variance exactly 0: inv = rsqrt(eps)); hw 1 with one image per member: every
    channel is constant and n == 1 (the unbiased variance keeps the biased one)."""
    k = Case()
    g = torch.Generator().manual_seed(14000 + hw)
    k.hw, k.c = hw, BNF_C
    k.cnt = torch.tensor([BNF_CNT[s] if hw > 1 else 1.0 for s in range(CAP)], dtype=torch.float64)
    k.sums = torch.zeros(CAP, 2, ACMAX, dtype=torch.float64)
    k.minvar = float("inf")
    for s in range(CAP):
        n = int(k.cnt[s]) * hw
        d = _ints(g, (n, ACMAX), -2, 2)
        if n > 1:
            d[0], d[1] = -2.0, 2.0
            d[:, 0] = 2.0
            k.minvar = min(k.minvar, float(d[:, 1:].var(0, unbiased=False).min()))
        k.sums[s, 0], k.sums[s, 1] = d.sum(0), (d * d).sum(0)
    k.state = (torch.rand(CAP, BNF_S, generator=g) + 0.25).float().double()  # gamma, running variance > 0
    k.state[:, BNF_BETA:BNF_BETA + BNF_C] -= 0.75
    k.state[:, BNF_RUN:BNF_RUN + BNF_C] -= 0.75
    k.coef0 = (torch.rand(CAP, 4, ACMAX, generator=g) + 0.5).float().double()  # coefficient table before the launch
    # backward: sums in units of 2^-10 (exact in fp32 and in the 2^-36 fixed point), the forward table's mean / inv
    k.bsums = _ints(g, (CAP, 2, ACMAX), -2 ** 14, 2 ** 14) / 1024
    k.fcoef = (torch.rand(CAP, 4, ACMAX, generator=g) * 1.5 + 0.5).float().double()
    k.fcoef[:, 2] -= 1.25
    k.grads0 = (torch.rand(CAP, BNF_S, generator=g) * 8 - 4).float().double()
    return k


def bnfin_eval(k, mode, dtype):
    """The launcher's formulas in plain operation order at ``dtype``.  Returns {name: (value, magnitude)} with
    [len(SLOTS)][C] entries; mode 0 forward, 1 backward, 2 eval."""
    c, sl = k.c, list(SLOTS)
    t = lambda v: v.to(dtype)
    eps, mom, om = (torch.tensor(v, dtype=dtype) for v in (BN_EPS, BN_MOM, BN_ONE_M))
    gamma, beta = t(k.state[sl, BNF_GAMMA:BNF_GAMMA + c]), t(k.state[sl, BNF_BETA:BNF_BETA + c])
    rm, rv = t(k.state[sl, BNF_RUN:BNF_RUN + c]), t(k.state[sl, BNF_RUN + c:BNF_RUN + 2 * c])
    n = t(k.cnt[sl] * k.hw).unsqueeze(1)
    out = {}
    if mode == 1:
        sdz, sdzx = t(k.bsums[sl, 0, :c]), t(k.bsums[sl, 1, :c])
        mean, inv = t(k.fcoef[sl, 2, :c]), t(k.fcoef[sl, 3, :c])
        scale = gamma * inv
        m1, m2 = sdz / n, sdzx / n
        t1, t2 = -scale * m1, scale * inv * mean * m2
        b = -scale * inv * m2
        g0, g1 = t(k.grads0[sl, BNF_GAMMA:BNF_GAMMA + c]), t(k.grads0[sl, BNF_BETA:BNF_BETA + c])
        out.update(c0=(scale, scale.abs()), c1=(b, b.abs()), c2=(t1 + t2, t1.abs() + t2.abs()),
                   dgamma=(g0 + sdzx, g0.abs() + sdzx.abs()), dbeta=(g1 + sdz, g1.abs() + sdz.abs()))
        return out
    if mode == 0:
        mean = t(k.sums[sl, 0, :c]) / n
        var = torch.clamp(t(k.sums[sl, 1, :c]) / n - mean * mean, min=0)
    else:
        mean, var = rm, rv
    inv = 1 / torch.sqrt(var + eps)
    scale = gamma * inv
    ms = mean * scale
    out.update(c0=(scale, scale.abs()), c1=(beta - ms, beta.abs() + ms.abs()), c2=(mean, mean.abs()),
               c3=(inv, inv.abs()))
    if mode == 0:
        unb = torch.where(n > 1, var * n / (n - 1), var)
        a, b = mom * rm, om * mean
        out["run_mean"] = (a + b, a.abs() + b.abs())
        a, b = mom * rv, om * unb
        out["run_var"] = (a + b, a.abs() + b.abs())
    return out


def check_bnfin(k):
    assert is_int(k.sums) and k.sums[:, 1].max() < EXACT
    if k.hw > 1:
        assert k.minvar >= 0.25
        for s in range(CAP):
            n = BNF_CNT[s] * k.hw
            assert (k.sums[s, 0] / n).abs().max() <= 2
            assert bool((k.sums[s, 1, 0] / n == (k.sums[s, 0, 0] / n) ** 2))  # the constant channel
    else:
        assert bool((k.cnt * k.hw == 1).all()) and torch.equal(k.sums[:, 1], k.sums[:, 0] ** 2)
    assert torch.equal(k.bsums.float().double(), k.bsums) and is_int(k.bsums * 2.0 ** 36)
    assert bool((k.state[:, BNF_RUN + k.c:BNF_RUN + 2 * k.c] > 0).all())


# --------------------------------------------------------------------------------------- softmax cross-entropy
SM_SHAPES = [(10, 64), (1001, 1024)]
SM_SIZES = (2, 4)  # 6 images: the second workgroup holds 2 live waves
SM_B_OFF, SM_TAIL = 24, 40


@functools.lru_cache(maxsize=None)
def softmax_case(ncls, ld):
    """Logits and bias in units of 1/16 (their fp32 sum is exact, so maxima tie exactly).  Image 0: the maximum is
    shared by the label and a LOWER index (wrong: the lower index wins); image 2: by the label and a HIGHER index
    (correct); image 3: logits of +-80, label at a -80; at 1001 classes image 4's tie partner sits 64 below the
    label (the same lane of the wave), and random ties among 1001 values of 129 levels are everywhere."""
    k = Case()
    g = torch.Generator().manual_seed(15000 + ncls)
    n = sum(SM_SIZES)
    k.ncls, k.ld, k.n, k.sizes = ncls, ld, n, SM_SIZES
    k.s_stride = SM_B_OFF + ncls + SM_TAIL
    k.state = _ints(g, (CAP, k.s_stride), -32, 32) / 16
    k.logits = _ints(g, (n, ld), -64, 64) / 16  # the padding columns hold data too (never read)
    k.labels = torch.randint(0, ncls, (n,), generator=g)
    slots = img_slots(SM_SIZES)
    bias = k.state[slots, SM_B_OFF:SM_B_OFF + ncls]
    k.logits[3, :ncls] = (2 * _ints(g, (ncls,), 0, 1) - 1) * 80 - bias[3]
    k.logits[3, 1], k.logits[3, 4] = 80 - bias[3, 1], -80 - bias[3, 4]
    k.labels[3] = 4

    def tie(img, lab, other):
        k.labels[img] = lab
        k.logits[img, lab], k.logits[img, other] = 7 - bias[img, lab], 7 - bias[img, other]  # random z <= 6

    tie(0, 5, 2)
    tie(2, 3, 7)
    if ncls > 128:
        tie(4, 70 + 64, 70)
        tie(5, 9, 9 + 64)
    k.z = k.logits[:, :ncls] + bias
    k.cnt = torch.tensor([float(SM_SIZES[0]), 7.0, float(SM_SIZES[1])], dtype=torch.float64)
    mx = k.z.max(1, keepdim=True).values
    idx = torch.arange(ncls).expand(n, ncls)
    k.argmax = torch.where(k.z == mx, idx, torch.full_like(idx, ncls)).min(1).values  # lowest index wins
    k.correct0 = _ints(g, (CAP,), 0, 5)
    k.correct = k.correct0.clone()
    for i, s in enumerate(slots):
        k.correct[s] += float(k.argmax[i] == k.labels[i])
    k.loss0 = _ints(g, (CAP,), 1, 4) / 4
    # never zero: in the deterministic build every add is quantised to 2^-36, which must stay small against the row
    k.grads0 = _ints(g, (CAP, k.s_stride), 1, 8) * (2 * _ints(g, (CAP, k.s_stride), 0, 1) - 1) / 8
    return k


def softmax_eval(k, loss_scale, dtype):
    """{name: (value, magnitude)}: loss [CAP], dbias [CAP][s_stride] (the whole gradient rows), dl [N][ld]."""
    slots = img_slots(k.sizes)
    z = k.z.to(dtype)
    logp = torch.log_softmax(z, 1)
    onehot = F.one_hot(k.labels, k.ncls).to(dtype)
    bsz = k.cnt[slots].to(dtype).unsqueeze(1)
    li = -(logp * onehot).sum(1, keepdim=True) / bsz
    p = torch.exp(logp)
    gsc = torch.tensor(loss_scale, dtype=dtype) / bsz
    # magnitude: a probability below the fp32 normal range (exp(-160) on the +-80 row) counts as that range's end
    d, dm = (p - onehot) * gsc, (p.clamp(min=2.0 ** -126) + onehot) * gsc
    loss, lmag = k.loss0.to(dtype).clone(), k.loss0.to(dtype).abs()
    gr, gmag = k.grads0.to(dtype).clone(), k.grads0.to(dtype).abs()
    for i, s in enumerate(slots):
        loss[s] += li[i, 0]
        lmag[s] += li[i, 0].abs()
        gr[s, SM_B_OFF:SM_B_OFF + k.ncls] += d[i]
        gmag[s, SM_B_OFF:SM_B_OFF + k.ncls] += dm[i]
    dl, dlm = torch.zeros(k.n, k.ld, dtype=dtype), torch.zeros(k.n, k.ld, dtype=dtype)
    dl[:, :k.ncls], dlm[:, :k.ncls] = d, dm
    return {"loss": (loss, lmag), "dbias": (gr, gmag), "dl": (dl, dlm)}


def ulp16(v, dtype):
    """One unit in the last place of ``dtype`` at |v| (float64 tensor in, float64 out), subnormals included."""
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -140))).clamp(min=emin)
    return torch.exp2(e - mant)


def check_softmax(k):
    assert is_int(k.logits * 16) and is_int(k.state * 16) and is_int(k.z * 16)
    assert torch.equal(k.z.float().double(), k.z) and k.z.abs().max() <= 80
    mx = k.z.max(1).values
    lab = k.labels
    assert k.z[0, 5] == mx[0] == k.z[0, 2] and lab[0] == 5 and k.argmax[0] == 2
    assert k.z[2, 3] == mx[2] == k.z[2, 7] and lab[2] == 3 and k.argmax[2] == 3
    assert set(k.z[3].abs().tolist()) == {80.0} and k.z[3, int(lab[3])] == -80 and mx[3] == 80
    if k.ncls > 128:
        assert k.z[4, 134] == mx[4] == k.z[4, 70] and lab[4] == 134 and k.argmax[4] == 70
        assert k.z[5, 9] == mx[5] == k.z[5, 73] and lab[5] == 9 and k.argmax[5] == 9
    assert is_int(k.correct) and k.correct[1] == k.correct0[1]


# -------------------------------------------------------------------------- GAP at hw = 49 (1 / hw not exact)
def gap_reduce_eval(k, dtype):
    """cg_gap_bwd_reduce's sums at ``dtype``: {name: (value, magnitude)} over the whole [CAP][2][ACMAX] table."""
    c, t = k.c, (lambda v: v.to(dtype))
    gg = (t(k.dfeat) * (torch.tensor(1.0, dtype=dtype) / k.hw)).unsqueeze(1)
    x = t(k.x)
    mask = (x * t(per_image(k.coef, k.sizes, 0, c)) + t(per_image(k.coef, k.sizes, 1, c)) > 0).to(dtype)
    dz = gg * mask
    q = dz * (x - t(per_image(k.coef, k.sizes, 2, c))) * t(per_image(k.coef, k.sizes, 3, c))
    ref, mag = t(k.prefill).clone(), t(k.prefill).abs()
    _scatter_sums(ref, mag, dz, k.sizes, c, 0)
    _scatter_sums(ref, mag, q, k.sizes, c, 1)
    return {"sums": (ref, mag)}
