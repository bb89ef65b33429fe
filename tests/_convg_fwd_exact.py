"""Integer constructions for the exact (tolerance 0) tests of the generic ImageNet conv / data-gradient kernel
(ops/csrc/convg.hip ``convg_fwd_kernel`` behind ``dtf_convg_fwd``) and of the plain forward / data gradient of
``convg_t3_kernel``: the case table, inputs, float64 CPU references and hand-built work lists, built without a device.
Used by tests/test_gpu_convg_fwd.py, tests/test_gpu_convg_t3.py and, for the conditions themselves,
tests/test_convg_fwd_exact_constructions.py.  The argument for a bitwise comparison is the one of _convg_exact.py:
every operand, coefficient and result is a small integer, so every partial sum is exact in any order.

Operands: x, x2 (h), res, xm integers in [-2, 2]; x3 in [-1, 1]; weights in {-1, 0, 1} with 1 in 4 non-zero for
K <= 64, 1 in 8 up to K = 400, 1 in 16 above, per member [o][ky][kx][i] at ``W_OFF`` of a row of ``w_mstride`` words
whose other words are 3 (NaN in the idle row).  Coefficient tables [CAP][4][CMAX], all integers so that every
transform is exact whatever the fma contraction does:
  MODE 1        scale {1, 2}, shift {-1, 0, 1, 2} (at least half > 0)              T = relu(x scale + shift)
  MODE 2 / 3    A {1, 2}, B {-1, 0, 1}, C {-1, 0, 1, 2} (at least half != 0)        T = A x + B h + C [+ x3]
  epilogue      scale {1, 2}, shift {-1, 0, 1}, mean {-1, 0, 1}, inv {1, 2}
(a padded or masked-off element that is wrongly transformed becomes non-zero).  Columns [C, CMAX) of every table and
every row of the idle slot are NaN.

Images: 4 of them -- member slot 0 owns images 0 and 1, image 2 belongs to nobody (NaN in every tensor; its output
keeps the canary), member slot 2 owns image 3 (an odd first image).

References (float64, per member): forward ``conv2d(T(x))`` (explicit zero padding, so the 4x4 / 1 stem fallback with
Ho = Hi has its 2-before / 1-after padding); data gradient ``conv_transpose2d(T(dy))`` over the forward-layout weights
(stride 2: output_padding 1, dx 14 x 12 from dy 7 x 6) -- the math, not the kernel's gather; then [+ res] (EPI bit 0;
EPI bit 3: res compact [N][Ho/2][Wo/2][Co], added at even (y, x) only), mask ``xm scale + shift > 0`` (strict),
statistics of the stored values (sum y, sum y^2; masked: sum dz, sum dz (xm - mean) inv).  MODE 3 also yields
xout = T, with and without x3.

Conditions, asserted on the reference alone by ``check_case``: every |y|, |xout| <= 256 (the bf16 integer range);
for every statistics element sum |terms| + |pre-seed| < 2^24; for the masked sums also max |term| x 64 pixels < 2^18:
the deterministic build drops a partial whose magnitude reaches 2^18 at the gradient scale (common.h DTF_FX_LIMIT),
and a wave's partial covers a quarter of a tile of at most 256 pixels (for convg_t3: 448 pixels, 112 per wave); at
least half of the unmasked outputs that have a tap at all are non-zero (the odd parity classes of the 1x1 stride-2
data gradient have none: they must store zeros, or the residual); in every masked case at least 8 elements have
``xm scale + shift == 0`` exactly and at least a quarter fall on each side of the strict decision; every coefficient
is inside its set.
"""
import functools
import os
import re
import zlib

import torch
import torch.nn.functional as F

from _convg_exact import CAP, CMAX, EXACT, FX_GRAD, FX_STAT, INT_EXACT, Y_CANARY, _ints, assert_partition  # noqa: F401

NAN = float("nan")
RANGES = [(0, 0, 2), (2, 3, 4)]  # (slot, first image, end image); image 2 is nobody's
N_IMG, IDLE_IMG, IDLE_SLOT = 4, 2, 1
W_OFF, W_TAIL = 24, 40  # words (multiples of 8: 16-byte rows) before / after a member's weight block
FX_LIMIT = 2 ** 18  # DTF_FX_LIMIT at the gradient scale

# the dispatch table of dtf_convg_fwd: (MODE, EPI, TRANS, AKM), in the order of its CG_ALL_TC lines
ROWS = [(0, 4, 0, 0), (0, 5, 0, 0), (0, 7, 0, 0), (1, 4, 0, 0), (1, 0, 0, 0), (1, 5, 0, 0), (1, 1, 0, 0), (0, 0, 0, 0),
        (0, 6, 0, 1), (2, 6, 0, 1), (3, 6, 0, 1), (2, 7, 0, 1), (0, 7, 0, 1), (0, 15, 0, 1), (0, 0, 0, 1), (2, 0, 0, 1),
        (0, 3, 0, 1),
        (0, 6, 1, 1), (2, 6, 1, 1), (2, 7, 1, 1), (0, 7, 1, 1), (0, 0, 1, 1), (2, 0, 1, 1)]
TCS = (64, 128)
CO = {64: 72, 128: 136}  # a full channel tile plus an 8-channel last one
V_BASE, V_BK64, V_TP256, V_M32 = 0, 4, 8, 8 | 16  # tile variants: the upper bits of the launcher's `trans`


def variants(row, tc):
    """Legal tile variants of one (row, tc): base, BK 64, 256-pixel tiles, and 32x32 MFMA tiles (tc 128, plain A)."""
    return [V_BASE, V_BK64, V_TP256] + ([V_M32] if tc == 128 and not row[3] else [])


def tile_pixels(variant):
    return 256 if variant & 8 else 128


def trans_arg(row, variant):
    return row[2] | (row[3] << 1) | variant


def instantiations():
    """Every convg_fwd_kernel instantiation reachable through dtf_convg_fwd."""
    return [(row, tc, v) for row in ROWS for tc in TCS for v in variants(row, tc)]


def source_rows(path=None):
    """The CG_ALL_TC(...) lines of convg.hip."""
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "distributedtf_amd", "ops", "csrc",
                                "convg.hip")
    text = open(path).read()
    return [(int(m), int(e), int(t == "true"), int(k)) for m, e, t, k in
            re.findall(r"^\s*CG_ALL_TC\((\d+),\s*(\d+),\s*(true|false),\s*(\d+)\)", text, re.M)]


# shape name -> (kind, k, stride, forward pad, gathered (Hi, Wi), output (Ho, Wo), fixed Ci or None)
# kinds: "fwd" forward conv; "akm" stride-1 data gradient (kernel pad' = k - 1 - pad); "trans" stride-2 data gradient
SHAPES = {
    "1x1s1": ("fwd", 1, 1, 0, (13, 11), (13, 11), 32),
    "3x3s1": ("fwd", 3, 1, 1, (13, 11), (13, 11), None),
    "3x3s2": ("fwd", 3, 2, 1, (13, 11), (7, 6), None),
    "stem7": ("fwd", 7, 2, 3, (13, 11), (7, 6), 8),      # non-incremental gather, K = 392: ragged last k-step
    "s2dfb": ("fwd", 4, 1, 2, (13, 11), (13, 11), 16),   # the s2d stem fallback: Ho = Hi, 2 before / 1 after
    "1x1c256": ("fwd", 1, 1, 0, (13, 11), (13, 11), 256),
    "d1x1s1": ("akm", 1, 1, 0, (13, 11), (13, 11), None),
    "d3x3s1": ("akm", 3, 1, 1, (13, 11), (13, 11), None),
    "d1x1c256": ("akm", 1, 1, 0, (13, 11), (13, 11), 256),
    "dcompact": ("akm", 1, 1, 0, (7, 6), (7, 6), None),  # 1x1 stride-2 data gradient kept at the dy resolution
    "d1x1s1e": ("akm", 1, 1, 0, (14, 12), (14, 12), None),  # even sizes: EPI 15 reads a compact residual
    "d3x3s1e": ("akm", 3, 1, 1, (14, 12), (14, 12), None),
    "t3x3s2": ("trans", 3, 2, 1, (7, 6), (14, 12), None),
    "t1x1s2": ("trans", 1, 2, 0, (7, 6), (14, 12), None),  # parity classes 1, 2, 3 have K = 0
}


def row_shapes(row):
    mode, epi, trans, akm = row
    if trans:
        return ["t3x3s2", "t1x1s2"]
    if akm:
        if mode == 3:
            return ["d1x1s1"]  # MODE 3 is the stride-1 1x1 data gradient only (xout is indexed by the gather)
        if epi == 15:
            return ["d1x1s1e", "d3x3s1e"]
        return (["d1x1s1", "d3x3s1"] + (["dcompact"] if (mode, epi) == (0, 0) else [])
                + (["d1x1c256"] if (mode, epi) == (2, 6) else []))
    return (["1x1s1", "3x3s1", "3x3s2"] + (["stem7", "s2dfb"] if mode == 0 and epi in (0, 4) else [])
            + (["1x1c256"] if (mode, epi) == (1, 4) else []))


def shape_ci(shape, variant):
    """Gathered channels: 64 where BK 64 needs it on the one-tap-per-k-step path, else 32 (or the shape's own)."""
    fixed = SHAPES[shape][6]
    return fixed if fixed is not None else (64 if variant == V_BK64 else 32)


def launches(row, tc):
    """[(variant, shape, Ci)] of one pytest case."""
    return [(v, sh, shape_ci(sh, v)) for v in variants(row, tc) for sh in row_shapes(row)]


def density(K):
    return 4 if K <= 64 else (8 if K <= 400 else 16)


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _pick(g, shape, values):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), shape, generator=g)]


def in_coefs(g, mode, c):
    t = torch.full((CAP, 4, CMAX), NAN, dtype=torch.float64)
    if mode == 0:
        return t
    for s, _, _ in RANGES:
        t[s, 0, :c] = _ints(g, (c,), 1, 2)
        if mode == 1:
            t[s, 1, :c] = _pick(g, (c,), [-1, 0, 1, 2, 1, 2])
        else:
            t[s, 1, :c] = _ints(g, (c,), -1, 1)
            t[s, 2, :c] = _pick(g, (c,), [-1, 0, 1, 2, 1, 2])
    return t


def ep_coefs(g, c):
    t = torch.full((CAP, 4, CMAX), NAN, dtype=torch.float64)
    for s, _, _ in RANGES:
        t[s, 0, :c], t[s, 1, :c] = _ints(g, (c,), 1, 2), _ints(g, (c,), -1, 1)
        t[s, 2, :c], t[s, 3, :c] = _ints(g, (c,), -1, 1), _ints(g, (c,), 1, 2)
    return t


def _images(g, h, w, c, lo, hi):
    t = _ints(g, (N_IMG, h, w, c), lo, hi)
    t[IDLE_IMG] = NAN
    return t


class Case:
    pass


def transform(c, s, f, e, has3):
    t = c.x[f:e]
    ci = c.ci
    if c.mode == 1:
        t = torch.relu(t * c.c_in[s, 0, :ci] + c.c_in[s, 1, :ci])
    elif c.mode >= 2:
        t = c.c_in[s, 0, :ci] * t + c.c_in[s, 1, :ci] * c.x2[f:e] + c.c_in[s, 2, :ci]
        if c.mode == 3 and has3:
            t = t + c.x3[f:e]
    return t


def conv_ref(c, t, w):
    """t [n][Hi][Wi][Ci] (float64) -> [n][Ho][Wo][Co]; w: the member's weights in the forward layout."""
    tn = t.permute(0, 3, 1, 2)
    if c.kind == "fwd":  # w [Co][k][k][Ci]
        pa_h = (c.ho - 1) * c.stride + c.k - c.hi - c.padf
        pa_w = (c.wo - 1) * c.stride + c.k - c.wi - c.padf
        assert pa_h >= 0 and pa_w >= 0
        y = F.conv2d(F.pad(tn, (c.padf, pa_w, c.padf, pa_h)), w.permute(0, 3, 1, 2), stride=c.stride)
    else:  # w [Ci (dy channel)][k][k][Co (dx channel)]
        y = F.conv_transpose2d(tn, w.permute(0, 3, 1, 2), stride=c.stride, padding=c.padf,
                               output_padding=c.stride - 1)
    assert y.shape[2:] == (c.ho, c.wo), (y.shape, c.ho, c.wo)
    return y.permute(0, 2, 3, 1)


def epilogue_ref(c, s, f, e, y):
    """[+ res], mask, statistics of member s: (y, st [2][Co], |.|-sums [2][Co], largest |term| of the masked row 1)."""
    co = c.co
    if c.epi & 8:
        y = y.clone()
        y[:, ::2, ::2] += c.res[f:e]
    elif c.epi & 1:
        y = y + c.res[f:e]
    big = 0.0
    if c.epi & 2:
        keep = c.xm[f:e] * c.c_ep[s, 0, :co] + c.c_ep[s, 1, :co] > 0
        y = torch.where(keep, y, torch.zeros_like(y))
    st = ab = None
    if c.epi & 4:
        if c.epi & 2:
            q = y * (c.xm[f:e] - c.c_ep[s, 2, :co]) * c.c_ep[s, 3, :co]
            big = float(q.abs().max())
        else:
            q = y * y
        st = torch.stack([y.sum((0, 1, 2)), q.sum((0, 1, 2))])
        ab = torch.stack([y.abs().sum((0, 1, 2)), q.abs().sum((0, 1, 2))])
    return y, st, ab, big


def _finish(c, g):
    """References of both members, for MODE 3 with and without x3: c.out[has3] = (y, st, stabs, xout)."""
    c.seed_st = _ints(g, (CAP, 2, CMAX), -3, 3)  # the kernel accumulates: pre-seeded statistics rows
    c.out, c.big = {}, 0.0
    for has3 in ((True, False) if c.mode == 3 else (True,)):
        y = torch.full((N_IMG, c.ho, c.wo, c.co), Y_CANARY, dtype=torch.float64)
        st, ab = c.seed_st.clone(), c.seed_st.abs()
        xout = torch.full((N_IMG, c.hi, c.wi, c.ci), NAN, dtype=torch.float64)
        for s, f, e in RANGES:
            t = transform(c, s, f, e, has3)
            xout[f:e] = t
            ym, sm, am, big = epilogue_ref(c, s, f, e, conv_ref(c, t, c.w[s]))
            y[f:e] = ym
            c.big = max(c.big, big)
            if sm is not None:
                st[s, :, :c.co] += sm
                ab[s, :, :c.co] += am
        c.out[has3] = (y, st, ab, xout if c.mode == 3 else None)
    return c


@functools.lru_cache(maxsize=None)
def fwd_case(row, tc, shape, ci):
    c = Case()
    c.row, c.tc, c.shape = row, tc, shape
    c.mode, c.epi, c.trans, c.akm = row
    c.kind, c.k, c.stride, c.padf, (c.hi, c.wi), (c.ho, c.wo), _ = SHAPES[shape]
    assert c.kind == ("trans" if c.trans else ("akm" if c.akm else "fwd"))
    c.ci, c.co = ci, CO[tc]
    c.pad = c.padf if c.kind == "fwd" else c.k - 1 - c.padf  # the kernel's pad
    c.kstride = c.stride  # CgArgs.stride (the data gradient of a stride-2 conv gathers "transposed")
    g = torch.Generator().manual_seed(_seed(row, tc, shape, ci))
    c.x = _images(g, c.hi, c.wi, ci, -2, 2)
    c.x2 = _images(g, c.hi, c.wi, ci, -2, 2) if c.mode >= 2 else None
    c.x3 = _images(g, c.hi, c.wi, ci, -1, 1) if c.mode == 3 else None
    c.res = c.xm = None
    if c.epi & 8:
        assert c.ho % 2 == 0 and c.wo % 2 == 0
        c.res = _images(g, c.ho // 2, c.wo // 2, c.co, -2, 2)
    elif c.epi & 1:
        c.res = _images(g, c.ho, c.wo, c.co, -2, 2)
    if c.epi & 2:
        c.xm = _images(g, c.ho, c.wo, c.co, -2, 2)
    c.K = c.k * c.k * ci
    c.dens = density(c.K)
    wshape = (CAP, c.co, c.k, c.k, ci) if c.kind == "fwd" else (CAP, ci, c.k, c.k, c.co)
    w = 2 * _ints(g, wshape, 0, 1) - 1
    c.w = w * (torch.randint(0, c.dens, wshape, generator=g) == 0)
    c.c_in, c.c_ep = in_coefs(g, c.mode, ci), ep_coefs(g, c.co)
    return _finish(c, g)


def weight_rows(c):
    """[CAP][w_mstride]: each member's block at W_OFF, 3 around it, NaN in the idle row."""
    n = c.w[0].numel()
    rows = torch.full((CAP, W_OFF + n + W_TAIL), 3.0, dtype=torch.float64)
    rows[:, W_OFF:W_OFF + n] = c.w.reshape(CAP, -1)
    rows[IDLE_SLOT] = NAN
    return rows


def live_outputs(c):
    """Outputs that have at least one tap: all, except the odd parity classes of the 1x1 stride-2 data gradient."""
    live = torch.ones(N_IMG, c.ho, c.wo, c.co, dtype=torch.bool)
    if c.kind == "trans" and c.k == 1:
        live[:] = False
        live[:, ::2, ::2] = True
    live[IDLE_IMG] = False
    return live


def _in_set(t, values):
    ok = torch.zeros_like(t, dtype=torch.bool)
    for v in values:
        ok |= t == v
    return bool(ok.all())


def check_case(c, dtype=torch.bfloat16, wave_pixels=64):
    """Every condition of the module docstring, on the inputs and the reference alone."""
    ci, co = c.ci, c.co
    member = [i for _, f, e in RANGES for i in range(f, e)]
    for t, lim in ((c.x, 2), (c.x2, 2), (c.res, 2), (c.xm, 2), (c.x3, 1)):
        if t is not None:
            assert bool(t[IDLE_IMG].isnan().all()) and t[member].abs().max() <= lim
            assert bool((t[member] == t[member].round()).all())
    assert bool(c.w.abs().max() <= 1) and bool((c.w == c.w.round()).all())
    nz = float((c.w != 0).double().mean())
    assert 0.6 / c.dens < nz < 1.5 / c.dens, (nz, c.dens)
    assert c.dens == (4 if c.K <= 64 else 8 if c.K <= 400 else 16)
    for s, _, _ in RANGES:
        if c.mode == 1:
            assert _in_set(c.c_in[s, 0, :ci], (1, 2)) and _in_set(c.c_in[s, 1, :ci], (-1, 0, 1, 2))
            assert int((c.c_in[s, 1, :ci] > 0).sum()) * 2 >= ci, "at least half of the shifts > 0"
        elif c.mode >= 2:
            assert _in_set(c.c_in[s, 0, :ci], (1, 2)) and _in_set(c.c_in[s, 1, :ci], (-1, 0, 1))
            assert _in_set(c.c_in[s, 2, :ci], (-1, 0, 1, 2))
            assert int((c.c_in[s, 2, :ci] != 0).sum()) * 2 >= ci, "at least half of C != 0"
        assert _in_set(c.c_ep[s, 0, :co], (1, 2)) and _in_set(c.c_ep[s, 1, :co], (-1, 0, 1))
        assert _in_set(c.c_ep[s, 2, :co], (-1, 0, 1)) and _in_set(c.c_ep[s, 3, :co], (1, 2))
        assert bool(c.c_ep[s, :, co:].isnan().all()) and bool(c.c_in[s, :, ci:].isnan().all())
    assert bool(c.c_in[IDLE_SLOT].isnan().all()) and bool(c.c_ep[IDLE_SLOT].isnan().all())
    live = live_outputs(c)
    for has3, (y, st, ab, xout) in c.out.items():
        ym = y[member]
        assert bool((ym == ym.round()).all()) and ym.abs().max() <= INT_EXACT[torch.bfloat16], float(ym.abs().max())
        assert ym.abs().max() <= INT_EXACT[dtype]
        assert bool((y[IDLE_IMG] == Y_CANARY).all())
        if xout is not None:
            assert xout[member].abs().max() <= INT_EXACT[torch.bfloat16] and bool(xout[IDLE_IMG].isnan().all())
        assert ab.max() < EXACT, float(ab.max())
        assert bool((ab >= st.abs()).all()) and bool((st == st.round()).all())
        assert torch.equal(st[IDLE_SLOT], c.seed_st[IDLE_SLOT]) and torch.equal(st[:, :, co:], c.seed_st[:, :, co:])
        if not c.epi & 4:
            assert torch.equal(st, c.seed_st)
        sel = live.clone()
        if c.epi & 2:
            for s, f, e in RANGES:
                sel[f:e] &= c.xm[f:e] * c.c_ep[s, 0, :co] + c.c_ep[s, 1, :co] > 0
        assert float((y[sel] != 0).double().mean()) >= 0.5, float((y[sel] != 0).double().mean())
    if c.epi & 2:
        assert c.big * wave_pixels < FX_LIMIT, c.big
        zero = pos = tot = 0
        for s, f, e in RANGES:
            u = c.xm[f:e] * c.c_ep[s, 0, :co] + c.c_ep[s, 1, :co]
            zero, pos, tot = zero + int((u == 0).sum()), pos + int((u > 0).sum()), tot + u.numel()
        assert zero >= 8 and pos * 4 >= tot and (tot - pos) * 4 >= tot, (zero, pos, tot)


# ------------------------------------------------------------------------------------------------- work lists
def grid(c):
    """(rows, columns) of the pixel grid the work items index: the output's, for TRANS the gathered dy's."""
    return (c.hi, c.wi) if c.trans else (c.ho, c.wo)


def classes(c):
    """Parity classes py * 2 + px of a TRANS launch, in the product's order."""
    if not c.trans:
        return (0,)
    return (3, 1, 2, 0) if c.k == 3 else (0, 1, 2, 3)


def _pieces(a, b, tp):
    return list(range(a, b, tp)) + [b] if a < b else [b]


def pixel_cuts(lo, hi, hw, tp, ragged):
    """Cut points of one member's pixels [lo, hi).  ragged: a one-pixel item, then tp-sized pieces up to 21 pixels
    before the member's first image boundary, an item of 37 pixels across that boundary (it starts inside an image
    row; 37 is no multiple of 16), then tp-sized pieces with a short tail.  Otherwise tp-sized pieces from lo (the
    member's 286 pixels at 13 x 11: a full 256-pixel tile and a ragged one)."""
    if not ragged:
        return _pieces(lo, hi, tp)
    b = lo + hw
    if b >= hi:  # a single image: nothing to cross
        return [lo] + _pieces(lo + 1, hi, tp)
    return sorted(set([lo] + _pieces(lo + 1, b - 21, tp) + _pieces(b + 16, hi, tp)))


def tile_words(c, only=None):
    return [o0 | (cls << 16) for cls in (classes(c) if only is None else only) for o0 in range(0, c.co, c.tc)]


def work_items(c, tp, reverse_tiles=False, only=None):
    """(slot, p0, p1, o0 | class << 16): co-tile 0 runs the ragged cuts, the last co-tile the plain ones.
    only: the parity classes to launch (TRANS; default all)."""
    gh, gw = grid(c)
    hw = gh * gw
    words = tile_words(c, only)
    if reverse_tiles:
        words = words[::-1]
    items = []
    for s, f, e in RANGES:
        for w in words:
            cuts = pixel_cuts(f * hw, e * hw, hw, tp, ragged=(w & 0xffff) == 0)
            items += [[s, a, b, w] for a, b in zip(cuts[:-1], cuts[1:])]
    return items


def coverage(items, c, tp):
    gh, gw = grid(c)
    hw = gh * gw
    return {"one_pixel": any(b - a == 1 for _, a, b, _ in items),
            "starts_inside_row": any(a % gw != 0 for _, a, b, _ in items),
            "crosses_image_ragged": any(a % gw != 0 and a // hw != (b - 1) // hw and (b - a) % 16 != 0
                                        for _, a, b, _ in items),
            "full_tile": any(b - a == tp for _, a, b, _ in items),
            "short_tail": any(b - a < tp and (b - a) % 16 != 0 and b % hw == 0 for _, a, b, _ in items),
            "member_at_odd_image": any(f % 2 == 1 for _, f, _ in RANGES),
            "two_co_tiles": len({w & 0xffff for _, _, _, w in items}) == 2,
            "all_classes": {w >> 16 for _, _, _, w in items} == set(classes(c))}


def need(c, tp):
    """What work_items promises; the GPU test asserts it on the list it launches.  A full tile needs a member with more
    than tp pixels (the 13 x 11 and 14 x 12 grids; the 7 x 6 grids have 84)."""
    gh, gw = grid(c)
    out = ["one_pixel", "starts_inside_row", "crosses_image_ragged", "short_tail", "member_at_odd_image",
           "two_co_tiles", "all_classes"]
    return out + (["full_tile"] if 2 * gh * gw > tp else [])


def check_items(items, c, tp, only=None):
    gh, gw = grid(c)
    hw = gh * gw
    assert all(0 < b - a <= tp for _, a, b, _ in items), "an item has at most TP pixels (the kernel's contract)"
    assert_partition(items, [(s, f * hw, e * hw) for s, f, e in RANGES], tile_words(c, only))
    cov = coverage(items, c, tp)
    missing = [k for k in need(c, tp) if not cov[k] and not (only is not None and k == "all_classes")]
    assert not missing, missing


def class_expected(c, only):
    """(y, statistics) of a TRANS launch of the parity classes ``only`` alone (class = py * 2 + px, the contract of the
    work word): the other classes' outputs keep the canary and add nothing to the statistics."""
    yref = c.out[True][0]
    y = torch.full_like(yref, Y_CANARY)
    st = c.seed_st.clone()
    for cls in only:
        py, px = cls >> 1, cls & 1
        for s, f, e in RANGES:
            v = yref[f:e, py::2, px::2]
            y[f:e, py::2, px::2] = v
            if c.epi & 4:
                if c.epi & 2:
                    q = v * (c.xm[f:e, py::2, px::2] - c.c_ep[s, 2, :c.co]) * c.c_ep[s, 3, :c.co]
                else:
                    q = v * v
                st[s, 0, :c.co] += v.sum((0, 1, 2))
                st[s, 1, :c.co] += q.sum((0, 1, 2))
    return y, st


# -------------------------------------------------------------- convg_t3: plain forward and data gradient, exact
T3_GEO = [(56, 64), (28, 128), (14, 256)]
T3_RANGES = [(0, 0, 1), (2, 1, 3)]  # members of 1 + 2 images


@functools.lru_cache(maxsize=None)
def t3_case(hw, ch, dgrad):
    """Stride-1 3x3 ch -> ch: forward (statistics sum y, sum y^2) or data gradient (mask by BN(xm), sums dz,
    dz xhat) over weights [slot][o][ky][kx][i]; K = 9 ch > 400: 1 weight in 16 non-zero."""
    c = Case()
    g = torch.Generator().manual_seed(_seed("t3", hw, ch, dgrad))
    c.hw, c.ch, c.dgrad, c.co = hw, ch, dgrad, ch
    c.x = _ints(g, (3, hw, hw, ch), -2, 2)
    c.xm = _ints(g, (3, hw, hw, ch), -2, 2)
    w = 2 * _ints(g, (CAP, ch, 3, 3, ch), 0, 1) - 1
    c.w = w * (torch.randint(0, 16, w.shape, generator=g) == 0)
    c.w[IDLE_SLOT] = NAN
    c.c_ep = ep_coefs(g, ch)
    c.seed_st = _ints(g, (CAP, 2, CMAX), -3, 3)
    c.y = torch.empty(3, hw, hw, ch, dtype=torch.float64)
    c.st, c.ab, c.big = c.seed_st.clone(), c.seed_st.abs(), 0.0
    for s, f, e in T3_RANGES:
        xn, wn = c.x[f:e].permute(0, 3, 1, 2), c.w[s].permute(0, 3, 1, 2)
        if dgrad:
            y = F.conv_transpose2d(xn, wn, padding=1).permute(0, 2, 3, 1)
            y = torch.where(c.xm[f:e] * c.c_ep[s, 0, :ch] + c.c_ep[s, 1, :ch] > 0, y, torch.zeros_like(y))
            q = y * (c.xm[f:e] - c.c_ep[s, 2, :ch]) * c.c_ep[s, 3, :ch]
            c.big = max(c.big, float(q.abs().max()))
        else:
            y = F.conv2d(xn, wn, padding=1).permute(0, 2, 3, 1)
            q = y * y
        c.y[f:e] = y
        c.st[s, :, :ch] += torch.stack([y.sum((0, 1, 2)), q.sum((0, 1, 2))])
        c.ab[s, :, :ch] += torch.stack([y.abs().sum((0, 1, 2)), q.abs().sum((0, 1, 2))])
    return c


def check_t3(c, dtype=torch.bfloat16):
    assert c.x.abs().max() <= 2 and c.xm.abs().max() <= 2 and bool((c.y == c.y.round()).all())
    nz = float((c.w[[0, 2]] != 0).double().mean())
    assert 0.6 / 16 < nz < 1.5 / 16, nz
    assert c.y.abs().max() <= INT_EXACT[torch.bfloat16] and c.y.abs().max() <= INT_EXACT[dtype]
    assert c.ab.max() < EXACT and bool((c.ab >= c.st.abs()).all())
    assert torch.equal(c.st[IDLE_SLOT], c.seed_st[IDLE_SLOT]) and torch.equal(c.st[:, :, c.ch:], c.seed_st[:, :, c.ch:])
    ch = c.ch
    sel = torch.ones_like(c.y, dtype=torch.bool)
    if c.dgrad:
        assert c.big * 112 < FX_LIMIT, c.big  # a wave's partial: a quarter of the 448- / 224-pixel tile
        zero = 0
        for s, f, e in T3_RANGES:
            u = c.xm[f:e] * c.c_ep[s, 0, :ch] + c.c_ep[s, 1, :ch]
            sel[f:e] = u > 0
            zero += int((u == 0).sum())
        assert zero >= 8 and 0.25 <= float(sel.double().mean()) <= 0.75
    assert float((c.y[sel] != 0).double().mean()) >= 0.5


# ------------------------------------------------------------------------------- device side (GPU tests only)
def bits(t):
    """The 16-bit words of an activation tensor (NaN compares equal to itself)."""
    return t.contiguous().view(torch.int16)


GUARD = 64  # canary words before and after every output


def guarded(shape, fill, dt, dev):
    """A device buffer of ``fill`` with GUARD words around a payload of ``shape``: (buffer, view of the payload)."""
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=dt, device=dev)
    return buf, buf[GUARD:GUARD + n].view(shape)
