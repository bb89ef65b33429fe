"""Constructions for the exact tests of the projection shortcut computed inside conv_a's forward launch
(ops/csrc/conv.hip, the PROJ instantiations of ``conv_fwd_s1_kernel`` / ``conv_fwd_kernel``; ``ConvArgs.y2`` /
``w2_off``).  The conv_a case itself -- operands, float64 reference, work lists -- is tests/_conv_exact.py's, unchanged;
this module adds the second weight block and the second output.

The projection is a 1x1 conv of conv_a's stride over the SAME staged input (``c.xin``: relu(snap(BN(x))), on the 0.5
grid) with integer weights, so the argument of _conv_exact carries over word for word: every product and partial sum
is a multiple of u = 0.5, and with

* sum of |terms| < 2^24 u per output and
* |y2| <= 256 u

(``check_proj``, asserted on the reference alone) the MFMA's fp32 sums are exact in any order and the stored bf16 /
fp16 word is the float64 reference.  About six of the Ci weights of an output channel are non-zero (+-1): with inputs
up to ~10 a dense row of 32 could leave the 256 u range."""
import functools

import torch
import torch.nn.functional as F

import _conv_exact as kx

CAP, EXACT = kx.CAP, kx.EXACT
W_GAP = 16  # NaN words between conv_a's weight block and the projection's (keeps the block 16-byte aligned)
NZ = 6      # non-zero weights per projection output channel (about)

# dtf_conv_fwd_s1 with y2: C = 16 (H = W = 32 is the kernel's own), the listed and the arithmetic work items
S1_PROJ = [(16, False), (16, True)]
# dtf_conv_fwd with y2: (cin, cout, Hi, rows) -- the smallest geometry hip_resnet._conv_fwd's band rule admits
# (Ho = 4: rows = 4 is the largest r <= min(8, Ho) with Ho % r == 0 and r * Ho % 16 == 0; one band per image, one
# 16-pixel tile per band)
GEN_PROJ = [(16, 32, 8, 4), (32, 64, 8, 4)]
# y2 set where no PROJ instantiation exists: (launcher, arguments after the ConvArgs pointer up to nblocks)
S1_REJECT = (32, 1, 0, 8)              # dtf_conv_fwd_s1: c, mode, resid, rows
GEN_REJECT = (16, 16, 1, 3, 1, 0, 1)   # dtf_conv_fwd: cin, cout, s, k, mode, resid, stats (the stride-1 generic row)


def band_rule_rows(hi, s, k, cin):
    """The band height hip_resnet._conv_fwd picks for a square Hi x Hi input."""
    ho, p = hi // s, (k - 1) // 2
    for r in range(min(8, ho), 0, -1):
        rows_in = (r - 1) * s + k
        if ho % r == 0 and (r * ho) % 16 == 0 and rows_in * (hi + 2 * p) * (cin // 8) <= 4 * 256:
            return r
    return None


class ProjCase:
    """c: the conv_a FwdCase; w2 [CAP][Co][Ci] (idle slot NaN), y2 / absy2 [N][Ho][Wo][Co] float64."""


@functools.lru_cache(maxsize=None)
def proj_case(cin, cout, s, hi, rows, uniform=False, nrep=8):
    c = kx.fwd_case(cin, cout, s, 3, 1, 0, hi, hi, rows, uniform, nrep)
    p = ProjCase()
    p.c = c
    seed = 77003 + cin * 131 + cout * 7 + s * 3 + hi + 7919 * uniform
    shape = (CAP, cout, cin)
    p.w2 = kx.hpick(shape, [-1.0, 1.0], seed) * (kx._hash(shape, seed + 1) % cin < NZ)
    p.y2 = torch.empty_like(c.y)
    p.absy2 = torch.empty_like(c.y)
    for sl, f, e in kx.ranges(c.slots, c.sizes):
        wn = p.w2[sl].reshape(cout, cin, 1, 1)
        xn = c.xin[f:e].permute(0, 3, 1, 2).contiguous()
        p.y2[f:e] = F.conv2d(xn, wn, stride=s).permute(0, 2, 3, 1)
        p.absy2[f:e] = F.conv2d(xn.abs(), wn.abs(), stride=s).permute(0, 2, 3, 1)
    p.w2[c.idle] = float("nan")
    n = cout * 9 * cin
    p.w2_off = kx.W_OFF + n + W_GAP
    return p


def check_proj(p):
    """The exactness conditions of the projection output, on the operands and the reference alone."""
    c, u = p.c, p.c.unit
    assert u == 0.5 and c.mode == 1 and c.k == 3 and not c.resid
    live = p.w2[list(c.slots)]
    assert bool((live == live.round()).all())
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(live.to(dt).double(), live) and torch.equal(p.y2.to(dt).double(), p.y2)
    assert bool((p.y2 / u == (p.y2 / u).round()).all())
    assert p.absy2.max() < EXACT * u, float(p.absy2.max())
    assert p.y2.abs().max() <= 256 * u, float(p.y2.abs().max())
    for sl in c.slots:
        assert bool(((p.w2[sl] != 0).sum(0) > 0).all()), "an input channel without a projection weight"
        assert bool(((p.w2[sl] != 0).sum(1) > 0).all()), "an output channel without a projection weight"
    assert not torch.equal(p.w2[c.slots[0]], p.w2[c.slots[1]])
    assert bool(torch.isnan(p.w2[c.idle]).all())
    # the two outputs differ (a kernel that stored conv_a's tile twice fails), and the projection is not constant
    assert not torch.equal(p.y2, c.y) and float(p.y2.std()) > 0
    # one workgroup serves two or more iterations: the centre tap is read from the second tile buffer too
    assert any(nit >= 2 for _, nit, _, _ in c.items)
    assert p.w2_off % 8 == 0


def weight_rows(p):
    """[CAP][w_mstride]: NaN | conv_a's [Co][3][3][Ci] at W_OFF | NaN | the projection's [Co][Ci] at w2_off | NaN."""
    c = p.c
    n, n2 = c.cout * 9 * c.cin, c.cout * c.cin
    rows = torch.full((CAP, p.w2_off + n2 + kx.W_TAIL), float("nan"), dtype=torch.float64)
    rows[:, kx.W_OFF:kx.W_OFF + n] = c.w.reshape(CAP, -1)
    rows[:, p.w2_off:p.w2_off + n2] = p.w2.reshape(CAP, -1)
    return rows


def all_cases(nrep):
    out = [proj_case(cc, cc, 1, 512 // cc, 8, u, nrep) for cc, u in S1_PROJ]
    return out + [proj_case(ci, co, 2, hi, rows, False, nrep) for ci, co, hi, rows in GEN_PROJ]
