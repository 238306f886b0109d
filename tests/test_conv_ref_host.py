"""The fp64 convolution reference of tests/conv_ref.py is itself checked on the CPU against ATen (F.conv2d, torch.nn.grad.conv2d_input /
conv2d_weight in fp64), `assert_exact_domain` must reject a case of each kind that leaves the exact domain, and the LEDGER: the case
table of tests/igemm_cases.py must name every first-generation kernel instantiation csrc/conv_igemm.hip can launch, minus an
exclusion list whose every entry carries one of two admissible reasons."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
import igemm_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#        N  H   W   C   K  R  s  p  groups
GEOMS = [
    (2, 9, 9, 5, 7, 3, 1, 1, 1),
    (2, 9, 10, 4, 6, 3, 2, 1, 1),       # stride 2, odd x even
    (1, 10, 9, 3, 5, 3, 2, 0, 1),       # pad 0, even x odd
    (2, 11, 11, 4, 3, 5, 2, 2, 1),
    (1, 12, 7, 2, 4, 5, 2, 4, 1),       # pad R-1
    (2, 14, 9, 3, 2, 7, 2, 3, 1),
    (2, 10, 11, 4, 5, 3, 3, 1, 1),      # stride 3
    (1, 7, 7, 3, 3, 1, 3, 0, 1),        # 1x1 stride 3: most pixels untouched
    (2, 8, 7, 6, 4, 1, 2, 0, 1),        # 1x1 stride 2
    (2, 8, 9, 3, 4, 4, 2, 1, 1),        # even filter
    (3, 2, 3, 2, 3, 3, 2, 2, 1),        # classes of one row
    (2, 1, 6, 3, 4, 5, 2, 4, 1),        # H = 1
    (2, 9, 9, 8, 8, 3, 1, 1, 4),        # grouped
    (1, 9, 8, 12, 12, 3, 2, 1, 3),      # grouped, stride 2
    (1, 13, 13, 2, 3, 9, 2, 4, 1),      # 9x9
]


@pytest.mark.parametrize("geom", GEOMS)
def test_reference_matches_aten_in_fp64(geom):
    N, H, W, C, K_, Rf, s, p, G = geom
    g = torch.Generator().manual_seed(H * 31 + W + C)
    x = torch.randn((N, C, H, W), generator=g, dtype=torch.float64)
    w = torch.randn((K_, C // G, Rf, Rf), generator=g, dtype=torch.float64)
    y = F.conv2d(x, w, None, s, p, 1, G)
    assert (R.out_extent(H, Rf, s, p), R.out_extent(W, Rf, s, p)) == tuple(y.shape[2:])
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    scale, shift = torch.randn((K_,), generator=g, dtype=torch.float64), torch.randn((K_,), generator=g, dtype=torch.float64)
    res, add = torch.randn(y.shape, generator=g, dtype=torch.float64), torch.randn(x.shape, generator=g, dtype=torch.float64)
    mask = torch.rand(x.shape, generator=g) > 0.4
    tol = 1e-12 * Rf * Rf * C
    assert float((R.conv_fwd(x, w, s, p, G) - y).abs().max()) < tol
    fused = torch.relu(y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1) + res)
    assert float((R.conv_fwd(x, w, s, p, G, scale, shift, res, relu=True) - fused).abs().max()) < tol
    dx = torch.nn.grad.conv2d_input(x.shape, w, dy, s, p, 1, G)
    assert float((R.conv_dgrad(dy, w, (H, W), s, p, G) - dx).abs().max()) < tol
    assert float((R.conv_dgrad(dy, w, (H, W), s, p, G, add, mask) - (dx + add) * mask).abs().max()) < tol
    dw = torch.nn.grad.conv2d_weight(x, w.shape, dy, s, p, 1, G)
    assert float((R.conv_wgrad(x, dy, Rf, Rf, s, p, G) - dw).abs().max()) < tol * N * H * W
    st = R.channel_stats(y)
    assert torch.allclose(st[0], y.sum((0, 2, 3))) and torch.allclose(st[1], (y * y).sum((0, 2, 3)))
    assert torch.allclose(R.column_sums(dx), dx.sum((0, 2, 3)))


def test_operand_generators_stay_in_their_ranges():
    g = torch.Generator().manual_seed(3)
    x, dy, dyw = R.activations((2, 5, 7, 7), g), R.gradients((2, 5, 7, 7), g), R.gradients((2, 5, 7, 7), g, for_wgrad=True)
    assert float(x.abs().max()) == 4 and float(dy.abs().max()) == 4 and float(dyw.abs().max()) == 3 and bool((x == x.round()).all())
    w = R.fwd_filters(6, 5, 3, 3, 12, g)
    assert tuple(w.shape) == (6, 5, 3, 3) and bool(((w != 0).sum((1, 2, 3)) == 12).all()) and float(w.abs().max()) <= 2
    wd = R.dgrad_filters(6, 5, 3, 3, 12, g)
    assert tuple(wd.shape) == (6, 5, 3, 3) and bool(((wd != 0).sum((0, 2, 3)) == 12).all())       # per INPUT channel
    wg = R.dgrad_filters_grouped(8, 4, 3, 3, 12, g)                                               # 2 groups of 4
    assert tuple(wg.shape) == (8, 4, 3, 3)
    per_input = torch.stack([(wg[(c // 4) * 4:(c // 4) * 4 + 4, c % 4] != 0).sum() for c in range(8)])
    assert bool((per_input == 12).all())
    assert int((R.fwd_filters(4, 1, 1, 1, 12, g) != 0).sum()) == 4                                 # fewer positions than non-zeros asked for


def test_exact_domain_accepts_an_integer_case_and_rejects_one_of_each_kind():
    g = torch.Generator().manual_seed(5)
    x, w = R.activations((2, 8, 9, 9), g), R.fwd_filters(6, 8, 3, 3, 12, g)
    y = R.conv_fwd(x, w, 1, 1)
    R.assert_exact_domain(stored=[y], abs_sums=[R.conv_fwd(x.abs(), w.abs(), 1, 1)], stats_of=y, colsum_of=y)
    R.assert_exact_domain(stored=[y * 0.5], half_integers=True)
    ok = torch.zeros((1, 1, 2, 2), dtype=torch.float64)
    with pytest.raises(AssertionError, match="not an integer"):
        R.assert_exact_domain(stored=[y * 0.5])
    with pytest.raises(AssertionError, match="not an integer"):
        R.assert_exact_domain(stored=[y * 0.25], half_integers=True)
    with pytest.raises(AssertionError, match="> 256"):
        R.assert_exact_domain(stored=[ok + 257])
    with pytest.raises(AssertionError, match="reaches 2\\^24"):
        R.assert_exact_domain(abs_sums=[ok + 2.0 ** 24])
    with pytest.raises(AssertionError, match="max y\\^2"):
        R.assert_exact_domain(stats_of=ok + 363)                   # 128 * 363^2 = 16 866 432 >= 2^24 (362 is the last value inside)
    R.assert_exact_domain(stats_of=ok + 362)
    with pytest.raises(AssertionError, match="max \\|dx\\|"):
        R.assert_exact_domain(colsum_of=ok + 2.0 ** 17)
    with pytest.raises(AssertionError, match="column sum reaches"):
        R.assert_exact_domain(colsum_of=torch.full((64, 1, 512, 512), 1.0, dtype=torch.float64))       # 2^24 ones in one channel
    with pytest.raises(AssertionError, match="reaches 2\\^24"):                                          # weight gradient: sum |x||dy|
        big = torch.full((1, 1, 2048, 2048), 2.0, dtype=torch.float64)
        R.assert_exact_domain(abs_sums=[R.conv_wgrad(big, big, 1, 1, 1, 0)])


# ------------------------------------------------------------------------------------------------ the ledger
def test_case_table_reaches_every_instantiation_outside_the_exclusion_list():
    ledger = set(T.LEDGER)
    assert len(ledger) == len(T.LEDGER) == 44 + 24 + 14
    assert set(T.EXCLUSIONS) <= ledger
    ids = [c["id"] for c in T.CASES]
    assert len(ids) == len(set(ids))
    reached = {c["variant"] for c in T.CASES}
    assert reached == ledger - set(T.EXCLUSIONS), (sorted(ledger - set(T.EXCLUSIONS) - reached), sorted(reached - (ledger - set(T.EXCLUSIONS))))
    for name, (reason, argument) in T.EXCLUSIONS.items():
        assert reason in (T.GIB2, T.NO_ENTRY) and len(argument) > 20, name
        # no LDS-DMA MODE 0 or 1 instantiation of either dtype on any tile may be excluded
        assert not re.match(r"igemm_dma_kernel<\w+,\d+,\d+,[01],", name), name
    # the A/B children: register-staged path with CELLSEG_WGRAD_SPEC = 1, LDS-DMA path with CELLSEG_WGRAD_SPEC = 2
    ab = {T.ab_variant(c["variant"], path, spec, c["ab_reg"]) for c in T.CASES for path, spec in ((0, 1), (1, 1), (0, 2))}
    assert set(T.EXCLUSIONS) - ab == T.AB_COLUMN_MISSING
    assert ab <= ledger
    # tile coverage: a forward and a data gradient per dtype on each tile
    for t in (T.BF, T.F32):
        for bm, bn in ((64, 64), (64, 128), (128, 64), (128, 128)):
            for op in ("fwd", "dgrad"):
                assert any(c["op"].split("+")[0] == op and c["variant"].startswith(f"igemm_dma_kernel<{t},{bm},{bn},") for c in T.CASES), (t, bm, bn, op)


def test_every_launch_site_of_the_first_generation_is_in_the_ledger():
    """A new launch_dma< / launch_reg< / launch_wgrad< call site (or a new note_variant format) must be added to igemm_cases.LEDGER, and
    with it to the case table or the exclusion list, before it can merge."""
    src = open(os.path.join(ROOT, "cellsegmentation_amd", "csrc", "conv_igemm.hip")).read()
    tiles = sorted(set(re.findall(r"launch_igemm<T, (\d+), (\d+)>\(", src)))
    assert tiles == [("128", "128"), ("128", "64"), ("64", "128"), ("64", "64")]
    named = set()
    sites = re.findall(r"launch_dma<T, BM, BN, (\d), (BF|true|false), (true|false)>\(", src)
    assert len(sites) == len(re.findall(r"launch_dma<[^>]*>\(", src)) - 0 and len(sites) >= 9
    for mode, pf, uni in sites:
        for t in (T.BF, T.F32):
            pf_ = (t == T.BF) if pf == "BF" else pf == "true"
            for bm, bn in tiles:
                named.add(T.D(t, bm, bn, mode, pf_, uni == "true"))
    sites = re.findall(r"launch_reg<T, BM, BN, (\d)>\(", src)
    assert len(sites) == len(re.findall(r"launch_reg<[^>]*>\(", src)) and sites
    for mode in sites:
        named |= {T.REG(t, bm, bn, mode) for t in (T.BF, T.F32) for bm, bn in tiles}
    sites = re.findall(r"launch_wgrad<(float|bf16_t), (\d+), 128, (true|false)>\(", src)
    assert len(sites) == len(re.findall(r"launch_wgrad<[^>]*>\(", src)) and sites
    for t, bm, tr in sites:
        t_ = T.F32 if t == "float" else T.BF
        named.add(T.WG(t_, bm, tr == "true"))
        if t_ == T.BF and tr == "true":                # the LDS-DMA kernels launch_wgrad itself selects for bf16 transposing reads
            named |= {T.WDMA(bm, 0), T.WDMA(bm, 1), T.WSPEC(bm, 0), T.WSPEC(bm, 1)}
    # (the template definitions `void launch_dma(`, `void launch_reg(`, `int launch_wgrad(` carry no argument list: not matched above)
    formats = set(re.findall(r'note_variant\("([^"]+)"', src))
    assert formats == {"igemm_dma_kernel<%s,%d,%d,%d,%s,%s>", "igemm_kernel<%s,%d,%d,%d>", "wgrad_spec_kernel<%d,%d,%s,%d>",
                       "wgrad_dma_kernel<%d,%d,%s,%d>", "wgrad_kernel<%s,%d,%d,%s>"}
    assert named == set(T.LEDGER), (sorted(named - set(T.LEDGER)), sorted(set(T.LEDGER) - named))
