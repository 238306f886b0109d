"""Host: the restated depthwise planners of tests/dw_cases.py against literal values worked out by hand from the formulas of
csrc/dwse.hip, and the exactness of the reference side of tests/test_depthwise_routes_gpu.py (torch's fp32 CPU convolution against an
int64 restatement on the rows' integer operands)."""
import pytest
import torch

import dw_cases as DW


def _case(id):
    return DW.CASES[DW.IDS.index(id)]


def test_ledger_ids_are_unique_and_small():
    assert len(set(DW.IDS)) == len(DW.IDS)
    for c in DW.CASES:
        C, k, s, H, W = c["geom"]
        assert C in (8, 16, 48, 72, 144, 264, 288) and H <= 21 and W <= 21 and k in (3, 5, 7) and s in (1, 2)


def test_strip_shape_by_hand():
    # 144 pairs: 9 chunks of 16 use every lane (score 1 - 0.0045) and beat 4 x 36 (252 of 256 lanes: 0.984 - 0.002)
    assert DW.dw_strip_shape(288) == (9, 16)
    # 132 pairs: 9 x 15 (255 lanes, fill 132 / 135: 0.974 - 0.0045) beats 8 x 17 (255 lanes, fill 132 / 136: 0.967 - 0.004)
    assert DW.dw_strip_shape(264) == (9, 15)
    # 36 pairs: 1 x 36, 2 x 18 and 3 x 12 all use 252 lanes: the fewest chunks win
    assert DW.dw_strip_shape(72) == (1, 36)
    assert DW.dw_strip_shape(16) == (1, 8) and DW.dw_strip_shape(8) == (1, 4)


def test_strip_plan_by_hand():
    # Q = 11 at stride 2: 12 columns with TS 4, 15 with TS 5; 2 * 11 * 3 = 66 items, 4096 / 9 = 455 blocks -> 1 item each, raised to
    # 2 items per item lane = 2 * (256 / 16) = 32 -> 3 workgroups
    assert DW.dw_strip_plan(2, 11, 11, 288, 2, 2048) == (4, 32, 9, 16, 3)
    # Q = 15 at stride 1: 15 columns with TS 5, 16 with TS 8; 90 items, 256 / 36 = 7 item lanes -> 14 per workgroup -> 7 workgroups
    assert DW.dw_strip_plan(2, 15, 15, 72, 1, 2048) == (5, 14, 1, 36, 7)
    # ties go to the longer strip: Q = 40 is 40 columns either way
    assert DW.dw_strip_plan(1, 1, 40, 16, 1, 2048)[0] == 8 and DW.dw_strip_plan(1, 1, 20, 16, 2, 2048)[0] == 4
    # the row cap: 4 * 200 * 25 = 20000 items on 4096 blocks would be 5 each -> 4000 workgroups; capped at 128 rows -> 157 each
    assert DW.dw_strip_plan(4, 200, 200, 16, 1, 128) == (8, 157, 1, 8, 128)


def test_tile_planners_by_hand():
    assert DW.dw_tile_shape(288) == (2, 18) and DW.dw_tile_shape(144) == (1, 18) and DW.dw_tile_shape(8) == (1, 1) and DW.dw_tile_shape(264) == (2, 17)
    # 64 items on 2048 blocks -> 1, raised to 4 per pixel lane = 4 * (256 / 18) = 56
    assert DW.dw_tile_items(64, 1, 18) == 56
    # 64 * 150 * 75 items on 2048 / 2 blocks
    assert DW.dw_tile_items(720000, 2, 18) == 704


def test_wgrad_split_and_stats_grid_by_hand():
    # 7x7, 16 channels: 1 chunk x 6 tap groups -> 170 slabs wanted; 18 output rows, at least ceil(64 / 9) = 8 rows each -> 3 slabs
    assert DW.dw_wgrad_split(2, 9, 9, 16, 7) == (8, 3)
    # 9600 output rows, 288 channel groups = 5 chunks of 64 -> 1024 / 5 = 204 slabs wanted -> ceil(9600 / 204) = 48 rows each -> 200 slabs
    assert DW.dw_wgrad_split(64, 150, 150, 2304, 3) == (48, 200)
    # 9 channel groups: granule 9 / gcd(9, 256) = 9; 756 threads want 3 workgroups -> 9
    assert DW.dw_stats_grid(2, 7, 6, 72) == 9
    assert DW.dw_stats_grid(2, 9, 10, 8) == 1
    # 32 groups: granule 1; capped at 1024
    assert DW.dw_stats_grid(64, 150, 150, 256) == 1024


@pytest.mark.parametrize("id,op,want,rows", [
    ("bf16_3x3s2_c288", "fwd_stats", "dw_conv_strip_kernel<3,2,4,true,false> grid=(3,9,1) per=32 lanes=16", 3),
    ("bf16_3x3s2_c144", "fwd", "dw_conv_strip_kernel<3,2,4,false,false> grid=(3,2,1) per=14 lanes=36", 0),
    ("f32_3x3s1_c16", "fwd", "dw_tile_kernel<f32,3,1,false,false> grid=(1,1,1) per=512 lanes=2", 0),
    ("bf16_3x3s1_q15", "dgrad", "dw_conv_strip_kernel<3,1,5,false,true> grid=(7,1,1) per=14 lanes=36", 0),
    ("bf16_7x7s1", "wgrad", "dw_wgrad_kernel<bf16> grid=(3,1,6) per=72 lanes=0", 3),
    ("bf16_7x7s2", "fwd_stats", "dw_fwd_stats_kernel<bf16> grid=(9,1,1) per=0 lanes=0", 9),
    ("f32_3x3s2_c288", "dgrad", "dw_dgrad_s2_kernel<f32,3> grid=(4,2,1) per=56 lanes=18", 0),
    ("f32_5x5s1_c264", "fwd", "dw_fwd_kernel<f32> grid=(15,1,1) per=0 lanes=0", 0),
])
def test_expected_strings_by_hand(id, op, want, rows):
    assert DW.expect(_case(id), op) == (want, rows)


@pytest.mark.parametrize("case", DW.CASES, ids=DW.IDS)
def test_reference_side_is_exact(case):
    """torch's fp32 CPU results on the integer operands equal an int64 restatement (unfold + integer sums) bit for bit"""
    C, k, s, H, W = case["geom"]
    x, w, dy, y, dx, dw = DW.reference(case)
    pad = (k - 1) // 2
    xi, wi, dyi = x.long(), w.long(), dy.long()
    P, Q = dy.shape[2:]
    xp = torch.nn.functional.pad(xi, (pad, pad, pad, pad))
    yi = torch.zeros_like(dyi)
    dxp = torch.zeros_like(xp)
    dwi = torch.zeros_like(wi)
    for kh in range(k):
        for kw in range(k):
            win = xp[:, :, kh:kh + (P - 1) * s + 1:s, kw:kw + (Q - 1) * s + 1:s]
            yi += win * wi[:, 0, kh, kw].view(1, C, 1, 1)
            dwi[:, 0, kh, kw] = (win * dyi).sum(dim=(0, 2, 3))
            dxp[:, :, kh:kh + (P - 1) * s + 1:s, kw:kw + (Q - 1) * s + 1:s] += dyi * wi[:, 0, kh, kw].view(1, C, 1, 1)
    assert torch.equal(y.long(), yi) and torch.equal(y, yi.float())
    assert torch.equal(dx, dxp[:, :, pad:pad + H, pad:pad + W].float())
    assert torch.equal(dw, dwi.float())
