"""The constructions of tests/_convg_aux_exact.py, without a device: every case tests/test_gpu_convg_aux.py launches
satisfies the conditions that make its comparison bitwise (integrality, the exact-integer range of bfloat16 AND
float16, sum |terms| < 2^24), the pool reference agrees with F.max_pool2d and its argmax is the first maximal tap,
and the mirrored launcher arithmetic puts each apply case on the kernel and pass structure it claims -- so a GPU
mismatch cannot be blamed on the reference."""
import pytest
import torch
import torch.nn.functional as F

import _convg_aux_exact as ax

DTYPES = [torch.bfloat16, torch.float16]


def _round_trips(t, dt):
    return torch.equal(t.to(dt).double(), t)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_reference(dtype):
    geos = [(h, w, c) for h, w in ax.POOL_GEO for c in ax.POOL_C] + \
           [(h, w, c) for h, w in ax.POOL_GEO_F32 for c in ax.POOL_C_F32]
    for h, w, c in geos:
        k = ax.pool_case(h, w, c)
        ax.check_pool(k)
        assert (k.ho, k.wo) == (-(-h // 2), -(-w // 2))
        for t in (k.x, k.y, k.g, k.dx):
            assert _round_trips(t, dtype) and t.abs().max() <= ax.INT_EXACT[dtype]
        if h % 2 == 0 and w % 2 == 0:  # -inf padding at the end == the clipped window
            xp = F.pad(k.x.permute(0, 3, 1, 2), (0, 1, 0, 1), value=float("-inf"))
            assert torch.equal(F.max_pool2d(xp, 3, 2).permute(0, 2, 3, 1), k.y)
        # the backward is the adjoint of the forward's selection: <dx, x> == <g, y>
        assert float((k.dx * k.x).sum()) == float((k.g * k.y).sum())
    assert {(h % 2, w % 2) for h, w in ax.POOL_GEO} == {(0, 0), (1, 1)} and (6, 10) in ax.POOL_GEO  # H != W


@pytest.mark.parametrize("kind", ["relu", "bwd", "add"])
def test_apply_cases_are_exact_and_on_their_path(kind):
    geos = ax.apply_geos(kind)
    seen = set()
    for name, c, hw, sizes, kernel, multi in geos:
        p = ax.apply_path(c, hw, sum(sizes))
        assert (p["kernel"], p["multi"]) == (kernel, multi), (name, p)
        if multi:
            assert p["mid"], (name, p)  # some thread stops inside the 4-slot unroll
        seen.add((kernel, multi))
        if multi:
            continue  # the 8 M-element constructions: same generator and ranges, checked on the GPU side
        for v in ax.apply_variants(kind, multi):
            k = ax.apply_case(kind, c, hw, sizes, v)
            ax.check_apply(k)
            for dt in DTYPES:
                assert _round_trips(k.out, dt) and k.bound <= ax.INT_EXACT[dt]
    assert seen == {("cf", False), ("cf", True), ("walk", False), ("walk", True)}
    by = {g[0]: ax.apply_path(g[1], g[2], sum(g[3])) for g in geos}
    assert by["cf-c8"]["ppi"] == 256 and by["cf-c8"]["ragged"] and by["cf-c64"]["ragged"]
    assert by["cf-c2048"]["ppi"] == 1 and by["cf-c2048"]["grid_y"] == 49
    assert by["walk-multi-c24"]["n8"] > by["walk-multi-c24"]["grid_y"] * 256
    # the issue's example shape, and the benchmark's (1024 images: split 4)
    p = ax.apply_path(512, 196, 128)
    assert (p["grid_y"], p["ppi"], p["multi"]) == (32, 4, True)
    assert ax.apply_path(256, 56 * 56, 1024)["grid_y"] == 4


def test_statistics_constructions_are_exact():
    for c in ax.STAT_C:
        for hw in ax.STAT_HW:
            ax.check_stats(ax.stats_case(c, hw))
            for two in (0, 1):
                ax.check_bnsum(ax.bnsum_case(c, hw, two))
    assert ax.stats_case(8, 1).x.shape[1] * 8 // 8 < 256  # n8 smaller than a workgroup
    assert [ax.stats_split(c) for c in ax.STAT_C] == [8, 8, 1]
    assert all(ax.stats_split(c) is None for c in ax.STAT_REJECT)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gap_constructions_are_exact(dtype):
    for c in ax.GAP_C:
        for hw in ax.GAP_HW:
            for v2 in (0, 1):
                k = ax.gap_case(c, hw, v2)
                ax.check_gap(k)
                for t in (k.x, k.feat, k.out):
                    assert _round_trips(t, dtype)
    ax.check_gap(ax.gap_case(64, 49, 1), exact=False)


def test_prep_tables_and_non_exact_constructions():
    ax.check_weight_prep_table()
    for hw in (4, 1):
        k = ax.bnfin_case(hw)
        ax.check_bnfin(k)
        for mode in (0, 1, 2):
            r64, r32 = ax.bnfin_eval(k, mode, torch.float64), ax.bnfin_eval(k, mode, torch.float32)
            d = max(ax.deviation(r32[n][0], r64[n][0], r64[n][1]) for n in r64)
            assert 0 < d < 1e-5, (hw, mode, d)  # a few fp32 roundings, no cancellation blow-up
        f = ax.bnfin_eval(k, 0, torch.float64)
        top = 1 / torch.sqrt(torch.tensor(ax.BN_EPS, dtype=torch.float64))  # rsqrt(eps): the variance clamped to 0
        if hw == 1:
            assert bool((f["c3"][0] == top).all())
        else:
            assert bool((f["c3"][0][:, 0] == top).all()) and f["c3"][0][:, 1:].max() <= 2.0
    for ncls, ld in ax.SM_SHAPES:
        k = ax.softmax_case(ncls, ld)
        ax.check_softmax(k)
        r64 = ax.softmax_eval(k, 128.0, torch.float64)
        r32 = ax.softmax_eval(k, 128.0, torch.float32)
        d = max(ax.deviation(r32[n][0], r64[n][0], r64[n][1]) for n in r64)
        assert 0 < d < 1e-4, d
        assert bool(torch.isfinite(r64["loss"][0]).all()) and bool((r64["dl"][0][:, ncls:] == 0).all())
    assert float(ax.ulp16(torch.tensor([1.5], dtype=torch.float64), torch.bfloat16)) == 2.0 ** -7
    assert float(ax.ulp16(torch.tensor([1.5], dtype=torch.float64), torch.float16)) == 2.0 ** -10
