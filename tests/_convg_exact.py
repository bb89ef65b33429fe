"""Integer constructions for the exact (tolerance 0) tests of the width-specialised ImageNet kernels of convg.hip:
inputs, float64 CPU references and hand-built work lists, built without a device.  Used by tests/test_gpu_convg_wgrad.py,
tests/test_gpu_stem_s2d.py, tests/test_gpu_convg_t3.py and, for the exactness conditions themselves,
tests/test_convg_exact_constructions.py.

Why the comparison can be bitwise.  Every operand is a small integer held in the 16-bit activation type, so every
product and every partial sum, in any order, is an integer; as long as the sum of the ABSOLUTE values of all terms
of one result stays below 2^24, each partial sum is exact in the fp32 MFMA accumulators, under fp32 atomics in any
order, and in the deterministic build's int64 fixed point.  A correct kernel then reproduces the float64 reference
bit for bit, and any indexing / masking / halo / remap error changes an integer.  Conditions (asserted on the
reference alone, ``check_*`` below):

* weight gradients: x and dy integers in [-2, 2]; with the folded operand (MX = 1) per-channel scale in {1, 2} and
  shift in {-1, 0, 1, 2} (at least half of the shifts > 0: a padded pixel wrongly transformed becomes relu(shift) > 0),
  so relu(x * scale + shift) is an integer <= 6; the gradient rows are pre-filled with integers in [-3, 3] (the
  kernels accumulate); sum |dy| |x'| + |prefill| < 2^24 for every element;
* stem forward: image values in [-1, 1], weights in {-1, 0, 1} with about 1 in 8 non-zero; |y| <= 256 (the exact
  integer range of bf16; fp16 reaches 2048), and sum(y^2) < 2^24 per (member, channel) for the statistics (the
  signed sums then are exact too: |y| <= y^2 for integers);
* folded 3x3 forward (convg_t3 XF): x in [-2, 2] with the same coefficients, weights in {-1, 0, 1} with about 1 in
  16 non-zero; the same two output conditions.

Every case has two members in slots 0 and 2 of a capacity-3 buffer (slot * stride is not image order); the images of
both are packed in one tensor and every neighbour image, unused slot row and coefficient row holds non-zero data.
"""
import functools

import torch
import torch.nn.functional as F

CAP, SLOTS, CMAX = 3, (0, 2), 512
EXACT = 2 ** 24  # integers below this are exact in fp32, in any order of accumulation
FX_GRAD, FX_STAT = 36, 24  # common.h DTF_FX_GRAD / DTF_FX_STAT: fixed-point shifts of the deterministic build
G_OFF, G_TAIL = 24, 40  # gradient row: g_off words before the [Co][Kr] block, a tail after it (both canaries)
INT_EXACT = {torch.bfloat16: 256, torch.float16: 2048}  # every integer of magnitude <= this is representable
Y_CANARY = 0.5  # output pre-fill: not an integer, so no computed output equals it


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _coefs(g, c):
    """[CAP][4][CMAX] BN coefficient table: row 0 scale in {1, 2}, row 1 shift in {-1, 0, 1, 2} (2 of 3 > 0)."""
    t = torch.zeros(CAP, 4, CMAX, dtype=torch.float64)
    t[:, 0, :c] = _ints(g, (CAP, c), 1, 2)
    t[:, 1, :c] = torch.tensor([-1.0, 0.0, 1.0, 2.0, 1.0, 2.0], dtype=torch.float64)[
        torch.randint(0, 6, (CAP, c), generator=g)]
    return t


def fold(x, coef, slot):
    """relu(x * scale + shift) of NHWC ``x`` with member ``slot``'s coefficients."""
    c = x.shape[-1]
    return torch.relu(x * coef[slot, 0, :c] + coef[slot, 1, :c])


def member_ranges(sizes):
    """[(slot, first image, end image)] of the packed image tensor."""
    out, f = [], 0
    for s, n in zip(SLOTS, sizes):
        out.append((s, f, f + n))
        f += n
    return out


# ------------------------------------------------------------------------------------------- weight gradients
class WgradCase:
    """x [N][Hi][Wi][Ci], dy [N][Ho][Wo][Co] (float64 integers), coef [CAP][4][CMAX], prefill / ref / absref
    [CAP][g_mstride]: the gradient buffer before the launch, after it, and the sum of |terms| behind each element."""


def _wgrad_finish(c, dws):
    """dws: per member (slot, dW [Co][Kr], |.|-reduction [Co][Kr]) -> prefill / ref / absref rows."""
    n = c.co * c.kr
    c.g_mstride = G_OFF + n + G_TAIL
    g = torch.Generator().manual_seed(977 + n)
    c.prefill = _ints(g, (CAP, c.g_mstride), -3, 3)
    c.ref, c.absref = c.prefill.clone(), c.prefill.abs()
    for s, dw, ab in dws:
        c.ref[s, G_OFF:G_OFF + n] += dw.reshape(-1)
        c.absref[s, G_OFF:G_OFF + n] += ab.reshape(-1)
    return c


@functools.lru_cache(maxsize=None)
def wgrad_case(hw, ci, co, k, stride, sizes, mode_x):
    """k x k / stride conv (pad (k - 1) / 2) over hw x hw x ci images; reference rows [o][ky][kx][i]."""
    c = WgradCase()
    g = torch.Generator().manual_seed(100003 * hw + 1009 * ci + 101 * co + 11 * k + 3 * stride + mode_x)
    c.hw, c.ci, c.co, c.k, c.stride, c.pad, c.sizes, c.mode_x = hw, ci, co, k, stride, (k - 1) // 2, sizes, mode_x
    c.ho = (hw + stride - 1) // stride
    c.kr = k * k * ci
    n = sum(sizes)
    c.x, c.dy, c.coef = _ints(g, (n, hw, hw, ci), -2, 2), _ints(g, (n, c.ho, c.ho, co), -2, 2), _coefs(g, ci)
    dws = []
    for s, f, e in member_ranges(sizes):
        xs = fold(c.x[f:e], c.coef, s) if mode_x else c.x[f:e]
        xn, dn = xs.permute(0, 3, 1, 2).contiguous(), c.dy[f:e].permute(0, 3, 1, 2).contiguous()
        wg = [torch.nn.grad.conv2d_weight(a, (co, ci, k, k), b, stride=stride, padding=c.pad).permute(0, 2, 3, 1)
              for a, b in ((xn, dn), (xn.abs(), dn.abs()))]
        dws.append((s, wg[0], wg[1]))
    return _wgrad_finish(c, dws)


def check_wgrad(c):
    """The exactness conditions of a weight-gradient case, on the inputs and the reference alone."""
    assert c.x.abs().max() <= 2 and c.dy.abs().max() <= 2 and bool((c.x == c.x.round()).all())
    assert bool((c.dy == c.dy.round()).all()) and bool((c.ref == c.ref.round()).all())
    if getattr(c, "mode_x", 0):
        sc, sh = c.coef[:, 0, :c.ci], c.coef[:, 1, :c.ci]
        assert bool(((sc == 1) | (sc == 2)).all()) and sh.min() >= -1 and sh.max() <= 2 and bool((sh == sh.round()).all())
        assert all(int((sh[s] > 0).sum()) * 2 >= c.ci for s in range(CAP)), "at least half of the shifts > 0"
        for s, f, e in member_ranges(c.sizes):
            xs = fold(c.x[f:e], c.coef, s)
            assert xs.max() <= 6 and xs.min() >= 0
    assert c.absref.max() < EXACT, float(c.absref.max())
    assert bool((c.absref >= c.ref.abs()).all())


# ---- row-band work lists (convg_wgrad_t3 / convg_stem_s2d): (slot, first band, end band, o0 | ci chunk << 16)
def band_cuts(lo, hi, bpi, kind, member):
    """Band boundaries of one member's [lo, hi).  'ragged': a single band, then an item that starts mid-image, crosses
    an image boundary and ends mid-image, then the rest (whole-image bands, bpi = 1: one item over all images);
    'even': member 0 as one item, the others in equal chunks that ignore the image boundaries."""
    if kind == "ragged":
        if bpi == 1:
            return [lo, hi]
        return sorted({lo, lo + 1, min(hi, lo + bpi + 3), hi})
    if member == 0:
        return [lo, hi]
    step = max(1, -(-(hi - lo) // 4))
    return list(range(lo, hi, step)) + [hi]


def band_items(sizes, bpi, tiles, kind):
    items = []
    for m, (s, f, e) in enumerate(member_ranges(sizes)):
        cuts = band_cuts(f * bpi, e * bpi, bpi, kind, m)
        for b0, b1 in zip(cuts[:-1], cuts[1:]):
            items += [[s, b0, b1, w] for w in tiles]
    return items


def band_coverage(items, sizes, bpi):
    mem = {s: (f * bpi, e * bpi) for s, f, e in member_ranges(sizes)}
    return {"starts_off_first_band": any(b0 % bpi != 0 for _, b0, b1, _ in items),
            "crosses_image": any(b0 // bpi != (b1 - 1) // bpi for _, b0, b1, _ in items),
            "single_band": any(b1 - b0 == 1 for _, b0, b1, _ in items),
            "ends_mid_image": any(b1 % bpi != 0 for _, b0, b1, _ in items),
            "whole_member": any((b0, b1) == mem[s] for s, b0, b1, _ in items)}


def band_need(bpi, kind):
    """What band_cuts promises; the tests assert it on the list they launch."""
    if kind == "even":
        return ("whole_member",)
    if bpi == 1:
        return ("crosses_image", "single_band", "whole_member")
    return ("starts_off_first_band", "crosses_image", "single_band", "ends_mid_image")


def assert_partition(items, ranges, tiles):
    """Every unit (band / pixel) of every member is covered exactly once per tile, inside the member's own range."""
    for w in tiles:
        for s, lo, hi in ranges:
            segs = sorted((a, b) for t, a, b, ww in items if t == s and ww == w)
            assert segs and segs[0][0] == lo and segs[-1][1] == hi, (s, w, segs)
            assert all(a < b for a, b in segs) and all(p[1] == n[0] for p, n in zip(segs[:-1], segs[1:])), (s, w, segs)
    assert {(t, ww) for t, _, _, ww in items} == {(s, w) for s, _, _ in ranges for w in tiles}


def t3_tiles(ci, co, bkc=32):
    return [o0 | (cc << 16) for o0 in range(0, co, 64) for cc in range(ci // bkc)]


# ---- split-K work lists (convg_wgrad / convg_wgrad_wide): (slot, p0, p1, o0 | n0 / 8 << 16)
def pixel_items(sizes, hwo, tiles):
    """Per member: a one-pixel item, an item that starts inside an image row and has a ragged last k-step, the rest."""
    items = []
    for s, f, e in member_ranges(sizes):
        lo, hi = f * hwo, e * hwo
        cuts = [lo, lo + 1, lo + 1 + (hi - lo) * 3 // 5, hi]
        for p0, p1 in zip(cuts[:-1], cuts[1:]):
            items += [[s, p0, p1, w] for w in tiles]
    return items


def pixel_coverage(items, sizes, hwo, wo_):
    return {"p0_inside_row": any(p0 % wo_ != 0 for _, p0, p1, _ in items),
            "short_tail": any(p1 - p0 > 32 and (p1 - p0) % 32 != 0 for _, p0, p1, _ in items),
            "one_pixel": any(p1 - p0 == 1 for _, p0, p1, _ in items),
            "crosses_image": any(p0 // hwo != (p1 - 1) // hwo for _, p0, p1, _ in items),
            "member_at_odd_image": any(f % 2 == 1 for _, f, _ in member_ranges(sizes)),
            "range_not_multiple_of_32": any(((e - f) * hwo) % 32 != 0 for _, f, e in member_ranges(sizes))}


PIXEL_NEED = ("p0_inside_row", "short_tail", "one_pixel", "crosses_image", "member_at_odd_image",
              "range_not_multiple_of_32")


def gemm_tiles(co, K, wo, wt):
    return [o0 | ((n0 // 8) << 16) for o0 in range(0, co, wo) for n0 in range(0, K, wt)]


# ------------------------------------------------------------------------------ space-to-depth stem (7x7 / 2)
def s2d_input(img):
    """Host mirror of cg_prep_input_s2d: [N][H][W][3] -> [N][H/2][W/2][16], channel (2 dy + dx) * 3 + c =
    img[2 by + dy][2 bx + dx][c], channels 12 .. 15 zero."""
    n, h, w, c = img.shape
    out = torch.zeros(n, h // 2, w // 2, 16, dtype=img.dtype)
    out[..., :4 * c] = img.reshape(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n, h // 2, w // 2, 4 * c)
    return out


def s2d_weight(w):
    """Host mirror of cg_weight_prep's s2d rows: W'[co][a][b][(2 dy + dx) * 3 + c] = W[co][2a + dy - 1][2b + dx - 1][c]."""
    out = torch.zeros(w.shape[0], 4, 4, 16, dtype=w.dtype)
    for a in range(4):
        for b in range(4):
            for q in range(4):
                ky, kx = 2 * a + (q >> 1) - 1, 2 * b + (q & 1) - 1
                if 0 <= ky < 7 and 0 <= kx < 7:
                    out[:, a, b, 3 * q:3 * q + 3] = w[:, ky, kx, :]
    return out


def s2d_weight_inverse(w4):
    """[Co][4][4][16] -> [Co][7][7][3]: the column remap of the weight-gradient writers (cin_real = -3)."""
    out = torch.zeros(w4.shape[0], 7, 7, 3, dtype=w4.dtype)
    for a in range(4):
        for b in range(4):
            for q in range(4):
                ky, kx = 2 * a + (q >> 1) - 1, 2 * b + (q & 1) - 1
                if 0 <= ky < 7 and 0 <= kx < 7:
                    out[:, ky, kx, :] = w4[:, a, b, 3 * q:3 * q + 3]
    return out


STEM_HW, STEM_CO, STEM_SIZES, STEM_BPI = 224, 64, (1, 2), 56
STEM_W_OFF = 8  # offset of the [64][7][7][3] fp32 kernel in the members' state rows
STEM_S = STEM_W_OFF + STEM_CO * 147 + 16
# band items of the stem: member 0 (image 0) with a single band at the bottom of its image (the "1 after" padding
# rows); member 1 (images 1, 2) with a mid-image start and an image crossing.  The forward list stops at band 150:
# rows 76 .. 111 of image 2 stay out of the launch and keep the output canary.
STEM_CUTS_WGRAD = {0: [0, 1, 56], 2: [56, 100, 130, 168]}
STEM_CUTS_FWD = {0: [0, 3, 55, 56], 2: [56, 100, 130, 150]}


def stem_items(cuts):
    return [[s, b0, b1, 0] for s in sorted(cuts) for b0, b1 in zip(cuts[s][:-1], cuts[s][1:])]


class StemCase:
    pass


@functools.lru_cache(maxsize=None)
def stem_case():
    c = StemCase()
    g = torch.Generator().manual_seed(224)
    n = sum(STEM_SIZES)
    c.img = _ints(g, (n, STEM_HW, STEM_HW, 3), -1, 1)
    w = 2 * _ints(g, (CAP, STEM_CO, 7, 7, 3), 0, 1) - 1
    c.w = w * (torch.randint(0, 8, w.shape, generator=g) == 0)  # about 1 in 8 non-zero
    c.dy = _ints(g, (n, STEM_HW // 2, STEM_HW // 2, STEM_CO), -2, 2)
    c.state = _ints(g, (CAP, STEM_S), -1, 1)  # the members' fp32 state rows around the kernel
    c.state[:, STEM_W_OFF:STEM_W_OFF + STEM_CO * 147] = c.w.reshape(CAP, -1)
    xn = c.img.permute(0, 3, 1, 2).contiguous()
    # forward: the ORIGINAL operation, 7x7 stride 2 pad 3 over the 3-channel image
    c.y = torch.stack([F.conv2d(xn[i:i + 1], c.w[s].permute(0, 3, 1, 2), stride=2, padding=3)[0].permute(1, 2, 0)
                       for s, f, e in member_ranges(STEM_SIZES) for i in range(f, e)])
    return c


def stem_fwd_expected(c, items):
    """(y_expected [N][112][112][64] with the canary where no item writes, statistics [CAP][2][CMAX])."""
    hb = STEM_HW // 2
    yexp = torch.full_like(c.y, Y_CANARY)
    st = torch.zeros(CAP, 2, CMAX, dtype=torch.float64)
    for s, b0, b1, _ in items:
        for b in range(b0, b1):
            img, r = b // STEM_BPI, (b % STEM_BPI) * 2
            blk = c.y[img, r:r + 2]
            yexp[img, r:r + 2] = blk
            st[s, 0, :STEM_CO] += blk.sum((0, 1))
            st[s, 1, :STEM_CO] += (blk * blk).sum((0, 1))
    assert hb == STEM_BPI * 2
    return yexp, st


def check_stem_fwd(c, dtype=torch.bfloat16):
    assert c.img.abs().max() <= 1 and c.w.abs().max() <= 1 and bool((c.y == c.y.round()).all())
    nz = float((c.w != 0).double().mean())
    assert 0.09 < nz < 0.16, nz
    assert c.y.abs().max() <= INT_EXACT[dtype], float(c.y.abs().max())
    for s, f, e in member_ranges(STEM_SIZES):
        assert (c.y[f:e] ** 2).sum((0, 1, 2)).max() < EXACT


@functools.lru_cache(maxsize=None)
def stem_wgrad_case():
    """The stem's weight gradient, rows [o][7][7][3] (Kr = 147): the 7x7 / 2 convolution's, not the 4x4 one's."""
    s = stem_case()
    c = WgradCase()
    c.hw, c.ho, c.ci, c.co, c.kr, c.sizes, c.mode_x = STEM_HW, STEM_HW // 2, 3, STEM_CO, 147, STEM_SIZES, 0
    c.x, c.dy, c.coef = s.img, s.dy, torch.zeros(CAP, 4, CMAX, dtype=torch.float64)  # (no folded form of the stem)
    xn = c.x.permute(0, 3, 1, 2).contiguous()
    dws = []
    for sl, f, e in member_ranges(c.sizes):
        dn = c.dy[f:e].permute(0, 3, 1, 2).contiguous()
        wg = [torch.nn.grad.conv2d_weight(a, (STEM_CO, 3, 7, 7), b, stride=2, padding=3).permute(0, 2, 3, 1)
              for a, b in ((xn[f:e], dn), (xn[f:e].abs(), dn.abs()))]
        dws.append((sl, wg[0], wg[1]))
    return _wgrad_finish(c, dws)


# --------------------------------------------------------------------------------- folded 3x3 forward (t3 XF)
class FwdCase:
    pass


@functools.lru_cache(maxsize=None)
def t3_fold_case(hw, ch):
    """Stride-1 3x3 conv of relu(x * scale + shift) (padding stays zero), ch -> ch channels, members of 1 and 2
    images; y [N][hw][hw][ch] and the statistics rows [CAP][2][CMAX] (sum, sum of squares per member and channel)."""
    c = FwdCase()
    g = torch.Generator().manual_seed(31 * hw + ch)
    c.hw, c.ch, c.sizes = hw, ch, (1, 2)
    n = sum(c.sizes)
    c.x, c.coef = _ints(g, (n, hw, hw, ch), -2, 2), _coefs(g, ch)
    w = 2 * _ints(g, (CAP, ch, 3, 3, ch), 0, 1) - 1  # [slot][o][ky][kx][i]
    c.w = w * (torch.randint(0, 16, w.shape, generator=g) == 0)  # about 1 in 16 non-zero
    c.y = torch.empty(n, hw, hw, ch, dtype=torch.float64)
    c.st = torch.zeros(CAP, 2, CMAX, dtype=torch.float64)
    for s, f, e in member_ranges(c.sizes):
        xs = fold(c.x[f:e], c.coef, s).permute(0, 3, 1, 2)
        y = F.conv2d(xs, c.w[s].permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
        c.y[f:e] = y
        c.st[s, 0, :ch], c.st[s, 1, :ch] = y.sum((0, 1, 2)), (y * y).sum((0, 1, 2))
    return c


def check_t3_fold(c, dtype=torch.bfloat16):
    assert c.x.abs().max() <= 2 and c.w.abs().max() <= 1 and bool((c.y == c.y.round()).all())
    sh = c.coef[:, 1, :c.ch]
    assert all(int((sh[s] > 0).sum()) * 2 >= c.ch for s in range(CAP))
    assert c.y.abs().max() <= INT_EXACT[dtype], float(c.y.abs().max())
    assert c.st[:, 1].max() < EXACT, float(c.st[:, 1].max())


# ------------------------------------------------------------------------------------------------- case tables
# (W, rows per band): convg_wgrad_t3_kernel<56, 4>, <28, 7>, <14, 14>; images per member: 2 + 3 where an item can
# start mid-image (more than one band per image), else 1 + 2
T3_GEO = [(56, 4), (28, 7), (14, 14)]


def t3_sizes(w, r):
    return (2, 3) if w // r > 1 else (1, 2)


# dtf_convg_wgrad_wide sub-cases at 14 x 14: (name, k, stride, Ci, wt)
WIDE_SUB = [("3x3s1", 3, 1, 64, 288), ("3x3s2", 3, 2, 64, 288), ("1x1s1-P1", 1, 1, 256, 256),
            ("1x1s2-table", 1, 2, 256, 256)]
WIDE_SIZES = (1, 2)
# dtf_convg_wgrad (generic split-K, modes (0, 0)) at 14 x 14, shapes the wide tiles do not take:
# (name, k, stride, Ci, Co, flags)
GENERIC_SUB = [("128-row", 3, 2, 32, 128, 0), ("64-row", 3, 2, 32, 64, 8), ("p1x1", 1, 1, 128, 128, 0),
               ("64-row-1x1", 1, 1, 128, 64, 8)]
T3_FOLD_GEO = [(56, 64), (28, 128), (14, 256)]


def all_wgrad_cases():
    """Every weight-gradient construction the GPU tests launch (the CPU test checks each one's conditions)."""
    out = []
    for w, r in T3_GEO:
        for mx in (0, 1):
            out.append(wgrad_case(w, 64, 64, 3, 1, t3_sizes(w, r), mx))
    out.append(wgrad_case(56, 64, 72, 3, 1, t3_sizes(56, 4), 1))
    for co in (128, 64):
        for _, k, stride, ci, _ in WIDE_SUB:
            for mx in (0, 1):
                out.append(wgrad_case(14, ci, co, k, stride, WIDE_SIZES, mx))
    for _, k, stride, ci, co, _ in GENERIC_SUB:
        out.append(wgrad_case(14, ci, co, k, stride, WIDE_SIZES, 0))
    out.append(stem_wgrad_case())
    return out


# ------------------------------------------------------------------------------- device side (GPU tests only)
def gpu_env():
    """(ops, hip_imagenet with its launchers registered, device, fixed-point accumulators?) of this process's library."""
    from distributedtf_amd import ops
    from distributedtf_amd.engine import hip_imagenet as hi
    hi._register()
    return ops, hi, torch.device("cuda"), bool(ops.lib().dtf_fixed_acc())


def acc_upload(t, shift, det, dev):
    """float64 integers -> the accumulator words of the loaded library (fp32, or int64 fixed point 2^-shift)."""
    return ((t * 2.0 ** shift).to(torch.int64) if det else t.float()).to(dev)


def acc_download(t, shift, det):
    """Accumulator words -> fp32 values (integers decode exactly)."""
    t = t.cpu()
    return (t.double() * 2.0 ** -shift).float() if det else t


def s2d_device_input(img, ops, dev):
    """The images through the project's cg_prep_input_s2d; compared with the host mirror on the way."""
    n = img.shape[0]
    src = img.float().to(dev)
    xs = torch.full((n, STEM_HW // 2, STEM_HW // 2, 16), 3.0, dtype=ops.act_dtype(), device=dev)
    rc = ops.lib().dtf_cg_prep_input_s2d(src.data_ptr(), xs.data_ptr(), n, STEM_HW, STEM_HW, 3, ops.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert torch.equal(xs.cpu().double(), s2d_input(img))
    return xs
