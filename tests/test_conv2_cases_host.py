"""Host: the restated planners of tests/conv2_cases.py against the built library's host-side queries (cs_conv2d_packed_supported,
cs_conv2d_packed_partial_rows, cs_conv2d_wgrad2_supported, cs_conv2d_wgrad_batched_splits) and against literal values worked out by
hand from the formulas of csrc/conv_v2.hip and csrc/wgrad_v2.hip; the hand-written variant names of the ledger against `expect()`;
the completeness of the ledger (every instantiation production routing can reach at 256 compute units has a row); and the exact domain
of every row's reference for both draws (tests/test_conv2_ledger_gpu.py compares with torch.equal: a row outside the domain would fail
-- or pass -- for the wrong reason)."""
import ctypes
import itertools

import pytest
import torch

import conv2_cases as C2

from cellsegmentation_amd import _lib
from cellsegmentation_amd import kernels as K

# the geometries the restatement is compared on, and over which the reachable instantiations are enumerated
GRID_N = (1, 2, 3, 4, 5, 6, 8, 12, 16, 24, 32, 40, 64)
GRID_HW = ((1, 1), (2, 2), (3, 3), (5, 3), (5, 5), (7, 5), (9, 10), (10, 13), (9, 17), (19, 19), (25, 31), (38, 38), (45, 57), (57, 97), (97, 57),
           (75, 75), (75, 131), (97, 131), (150, 150))
GRID_CH = ((64, 64), (64, 128), (128, 64), (128, 128), (64, 512), (512, 64), (128, 512), (512, 128), (256, 256), (192, 128), (1024, 256), (2048, 512),
           (72, 128), (128, 320))
GRID_RSP = ((3, 1, 0), (3, 1, 1), (3, 1, 2), (3, 1, 3), (3, 2, 1), (1, 1, 0), (1, 2, 0), (1, 3, 0), (1, 1, 1))


def _grid():
    for N, (H, W), (C, Kc), (R, s, p) in itertools.product(GRID_N, GRID_HW, GRID_CH, GRID_RSP):
        if C2.out_size(H, R, s, p) >= 1 and C2.out_size(W, R, s, p) >= 1:
            yield (N, H, W, C, Kc, R, s, p)


def _cus():
    """what cs_device_cus_ answers in this process: the device's count, 256 without one"""
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def _case(id):
    return C2.CASES[C2.IDS.index(id)]


def test_ledger_ids_are_unique():
    assert len(set(C2.IDS)) == len(C2.IDS) and len(set(C2.WGRAD_IDS)) == len(C2.WGRAD_IDS)


def test_restated_planners_agree_with_the_library():
    lib, cus, n = _lib.load(), _cus(), 0
    for geom in _grid():
        N, H, W, C, Kc, R, s, p = geom
        g = K.make_geom(N, H, W, C, Kc, R, R, s, p)
        for dg in (0, 1):
            pl = C2.plan_any(geom, dg, cus)
            got = (lib.cs_conv2d_packed_supported(ctypes.byref(g), dg), lib.cs_conv2d_packed_partial_rows(ctypes.byref(g), dg))
            assert got == ((1, pl["rows"]) if pl else (0, 0)), (geom, dg, pl)
            n += 1
    assert n > 20000


def test_restated_refusals_at_the_31_bit_limits():
    """the extents the planners refuse because a byte offset or a pixel index would not fit (host queries only: nothing is allocated)"""
    lib, cus = _lib.load(), _cus()
    want = {
        (16, 1024, 1024, 64, 128, 3, 1, 1): (0, 0),        # forward source 16 * 2^20 px * 128 bytes = 2^31 bytes; the gradient's is twice that
        (16, 1024, 1023, 64, 128, 3, 1, 1): (1, 0),        # one column less
        (8, 1024, 1023, 128, 128, 3, 1, 1): (1, 1),
        (2, 2048, 2048, 64, 65536, 3, 1, 1): (0, 0),       # destination 2^23 px * 2^17 bytes = 2^40 bytes (the gradient: source bytes)
        (2, 2048, 2047, 64, 65536, 3, 1, 1): (1, 0),
        (1, 8, 8, 16384, 8192, 3, 1, 1): (0, 0),           # packed weights 8192 * 9 * 16384 * 2 bytes >= 2^31, either direction
        (1, 8, 8, 8192, 8192, 3, 1, 1): (1, 1),
        (16, 1024, 1024, 64, 128, 1, 1, 0): (0, 0),        # the same source limit in plan_gemm
        (16, 1024, 1023, 64, 128, 1, 1, 0): (1, 0),
        (1, 8, 8, 32768, 32768, 1, 1, 0): (0, 0),          # 1x1 packed weights 2^31 bytes
        (1, 8, 8, 16384, 32768, 1, 1, 0): (1, 1),
    }
    for geom, served in want.items():
        N, H, W, C, Kc, R, s, p = geom
        g = K.make_geom(N, H, W, C, Kc, R, R, s, p)
        for dg in (0, 1):
            pl = C2.plan_any(geom, dg, cus)
            assert bool(pl) == bool(served[dg]), (geom, dg)
            assert lib.cs_conv2d_packed_supported(ctypes.byref(g), dg) == served[dg], (geom, dg)
            assert lib.cs_conv2d_packed_partial_rows(ctypes.byref(g), dg) == (pl["rows"] if pl else 0), (geom, dg)
    code = K._code(torch.bfloat16)
    want = {
        (104, 1024, 158, 64, 64, 1): 0, (103, 1024, 158, 64, 64, 1): 1,        # x: N * 1024 * 158 px * 128 bytes against 2^31
        (52, 1024, 158, 64, 128, 1): 0, (51, 1024, 158, 64, 128, 1): 1,        # dy: 256 bytes per pixel
        (1, 8, 8, 8192, 8192, 1): 0, (1, 8, 8, 4096, 8192, 1): 1,              # one slab: K * 9 * C * 4 bytes
    }
    for wg, served in want.items():
        N, H, W, C, Kc, items = wg
        g = K.make_geom(N, H, W, C, Kc, 3, 3, 1, 1)
        assert bool(C2.plan_wgrad2(*wg)) == bool(served), wg
        assert lib.cs_conv2d_wgrad2_supported(ctypes.byref(g), code) == served, wg


def test_restated_wgrad_plan_agrees_with_the_library():
    lib, code, n, classes = _lib.load(), K._code(torch.bfloat16), 0, set()
    widths = (1, 2, 3, 9, 10, 11, 12, 19, 22, 23, 24, 38, 39, 40, 75, 78, 79, 80, 131, 150, 158, 159, 160)
    for N, H, W, (C, Kc), items in itertools.product((1, 2, 3, 5, 64), (1, 2, 7, 38, 97), widths, ((64, 64), (128, 64), (192, 256), (512, 512), (64, 72)),
                                                     (1, 2, 3, 5, 8)):
        g = K.make_geom(N, H, W, C, Kc, 3, 3, 1, 1)
        pl = C2.plan_wgrad2(N, H, W, C, Kc, items)
        assert lib.cs_conv2d_wgrad2_supported(ctypes.byref(g), code) == int(bool(pl)), (N, H, W, C, Kc)
        if Kc % 8 == 0:
            want = pl["nsplit"] if pl else C2.wgrad1_splits(N * H * W, Kc, 9 * C, items)
            assert lib.cs_conv2d_wgrad_batched_splits(ctypes.byref(g), code, items) == want, (N, H, W, C, Kc, items)
        if pl:
            classes.add(C2.W2(pl["bl"], pl["xr"]))
            assert pl["per_xcd"] * 8 >= pl["total_work"] > (pl["per_xcd"] - 1) * 8
        n += 1
    assert n > 2000
    # completeness: every stage class has a row, and the rows name nothing else
    assert classes == {c["variant"] for c in C2.WGRAD_CASES if c["variant"].startswith("wgrad2_kernel")} and len(classes) == 5
    # nothing but these geometries is ever taken: other strides, pads, filter sizes and fp32 go to the first generation
    for g in (K.make_geom(2, 19, 19, 64, 64, 3, 3, 2, 1), K.make_geom(2, 19, 19, 64, 64, 3, 3, 1, 0), K.make_geom(2, 19, 19, 64, 64, 1, 1, 1, 0)):
        assert lib.cs_conv2d_wgrad2_supported(ctypes.byref(g), code) == 0
    g = K.make_geom(2, 19, 19, 64, 64, 3, 3, 1, 1)
    assert lib.cs_conv2d_wgrad2_supported(ctypes.byref(g), K._code(torch.float32)) == 0
    assert lib.cs_conv2d_wgrad_batched_splits(ctypes.byref(g), code, 9) == C2.wgrad1_splits(2 * 19 * 19, 64, 576, 9)      # more than 8 items


@pytest.mark.parametrize("case", C2.CASES, ids=C2.IDS)
def test_hand_written_names_follow_from_the_rules(case):
    for op in ("fwd", "dgrad"):
        assert C2.expect(case, op)[0] == case[op], (case["id"], op)


@pytest.mark.parametrize("case", C2.WGRAD_CASES, ids=C2.WGRAD_IDS)
def test_hand_written_wgrad_names_follow_from_the_rules(case):
    assert C2.expect_wgrad(case)[0] == case["variant"]


def test_ledger_names_every_reachable_instantiation():
    """at 256 compute units: the instantiations the restated planners produce over the grid == the ones the ledger names"""
    reachable = set()
    for geom in _grid():
        for dg in (0, 1):
            pl = C2.plan_any(geom, dg, 256)
            if pl:
                reachable.add(C2.variant_of(pl, dg))
    named = {c[op] for c in C2.CASES for op in ("fwd", "dgrad") if c[op]}
    assert reachable - named == set(), "reachable without a ledger row"
    assert named - reachable == set(), "named by the ledger, not produced by the grid"
    # 20 halo (TM 3 / 4 x NBW 3 / 4 / 5 / 8, the 2-D tiles, the 64-channel form) + 12 wide 3x3 + 4 wide 1x1 + 6 ring, forward and gradient
    assert len(named) == 42
    # what production routing cannot reach: halo TM 2 is not instantiated (pick_tm answers 3 or 4); ring<2,1,4> is, for the A/B knob only
    assert not any(v.startswith("conv2_halo_kernel<9,3,2,") or v.startswith("conv2_ring_kernel<2,1,4,") for v in reachable)


def test_tile_height_rules_by_hand():
    # 33174 px on one channel tile: 260 workgroups of 128 px (in 257..512), 346 of 96 (<= 512): TM 3
    assert C2.pick_tm(33174, 1) == 3
    # 49125 px: 384 and 512 workgroups: still 3; 96 px more: 513 workgroups of 96: 4
    assert C2.pick_tm(49125, 1) == 3 and C2.pick_tm(49249, 1) == 4
    # 8448 px x 4 channel tiles: 264 / 352;  32768 px x 1: exactly 256 workgroups is not "more than 256"
    assert C2.pick_tm(8448, 4) == 3 and C2.pick_tm(32768, 1) == 4 and C2.pick_tm(260, 1) == 4
    # wide: cost = rounds x height over 8, 6, 4; 13376 px x 4: 212 (8), 280 (2 x 6), 420 (2 x 4): the taller on the tie
    assert C2.pick_wide_tm(13376, 4, 2) == 8
    # 8448 px x 4: 132 (8), 176 (6), 264 (2 x 4)
    assert C2.pick_wide_tm(8448, 4, 2) == 6
    # few tiles: one round of everything, the shortest wins;  one chunk: never
    assert C2.pick_wide_tm(260, 1, 2) == 4 and C2.pick_wide_tm(260, 1, 1) == 0
    # 100000 px: 391 (2 x 8), 521 (3 x 6), 782 (4 x 4): TM 8 is cheapest but not resident at once
    assert C2.pick_wide_tm(100000, 1, 2) == 0
    # half a chip: 33174 px: 130 (2 x 8), 173 (2 x 6), 260 (3 x 4): TM 6 with 173 > 128 tiles
    assert C2.pick_wide_tm(33174, 1, 2, 256) == 6 and C2.pick_wide_tm(33174, 1, 2, 128) == 0
    # 1x1: 6 or 4 only, from 8 chunks
    assert C2.pick_wide1_tm(33174, 1, 8) == 6 and C2.pick_wide1_tm(260, 1, 8) == 4 and C2.pick_wide1_tm(260, 1, 7) == 0


def test_window_blocks_by_hand():
    # 128 px of a 13x10 destination in a 14x11 padded source: 127 + 13 row ends x 1 + 1 image end x 11 = 151, + 2 rows + 2 + 1 = 176 rows
    assert C2.window_blocks(128, 13, 10, 14, 11) == 11
    # 96 px of 57x97 in 58x98: 95 + 1 + 98 + 199 = 393 rows
    assert C2.window_blocks(96, 57, 97, 58, 98) == 25
    # a destination that fills its padded source: no row or image gaps: 255 + 2 * 131 + 3 = 520 rows
    assert C2.window_blocks(256, 97, 131, 97, 131) == 33
    # 128 px of a 3x3 destination in 5x5: 127 + 43 x 2 + 15 x 10 + 13 = 376 rows
    assert C2.window_blocks(128, 3, 3, 5, 5) == 24
    # exactly a multiple of 16 rows: 127 + 0 + 0 + (2 * 6 + 3) = 142 -> 9; Wp 7: 144 -> 9; Wp 8: 146 -> 10
    assert [C2.window_blocks(128, 4, w, 4, w) for w in (6, 7, 8)] == [9, 9, 10]


@pytest.mark.parametrize("id,op,want,rows", [
    ("halo4_nb3_f", "fwd", "conv2_halo_kernel<9,3,4,1,4,3,false,false>", 3),              # 260 px / 128
    ("halo64_p2", "fwd", "conv2_halo_kernel<9,3,4,2,2,8,false,false>", 6),                # 532 px / 256 = 3 tiles x 2 wave rows
    ("halo64_p2", "dgrad", "conv2_halo_kernel<9,3,4,2,2,8,true,false>", 4),
    ("t2d_f", "fwd", "conv2_halo_kernel<9,3,4,1,4,3,false,true>", 3),                     # one 8 x 16 tile per image
    ("wide8_nb9_f", "dgrad", "conv2_halo_kernel<9,3,4,1,4,3,true,true>", 450),            # 5 x ceil(75 / 8) x ceil(131 / 16)
    ("wide8_nb9_f", "fwd", "conv2_wide_kernel<8,9,false,9>", 201),                        # 51205 px / 256
    ("halo3_nb8_d", "dgrad", "conv2_halo_kernel<9,3,3,1,4,8,true,false>", 346),           # 33174 px / 96
    ("ring222", "dgrad", "conv2_ring_kernel<2,2,2,true,false>", 6),                       # 260 px / 128 = 3 tiles x 2
    ("s2_ring222_f", "dgrad", "conv2_ring_kernel<4,1,4,true,false>", 7),                  # compact: 2 x 19 x 21 = 798 px / 128
    ("s2_ring414_f", "fwd", "conv2_ring_kernel<4,1,4,false,false>", 3),                   # 3 x 11 x 9 = 297 px
    ("wide1_tm6_d", "dgrad", "conv2_wide_kernel<6,6,true,2>", 173),                       # 33174 px / 192
    ("ring414_c5", "dgrad", None, 0),
])
def test_expected_strings_by_hand(id, op, want, rows):
    assert C2.expect(_case(id), op) == (want, rows)


def test_wgrad_plans_by_hand():
    def plan(*geom):
        pl = C2.plan_wgrad2(*geom)
        return pl and (pl["bl"], pl["xr"], pl["n_stages"], pl["stages_per_split"], pl["nsplit"], pl["total_work"], pl["per_xcd"])
    # 5 x 159 = 795 positions: 13 stages of 64; 384 splits wanted, at most 13 / 4 = 3: ceil(13 / 3) = 5 stages each: 5 + 5 + 3
    assert plan(1, 4, 158, 64, 64, 1) == (64, 384, 13, 5, 3, 3, 1)
    # ResNet-50 layer1, three layers: 2 x 76 x 76 = 11552 positions: 181 stages; 128 wanted, 45 allowed: 5 stages each: 37 splits
    assert plan(2, 75, 75, 64, 64, 3) == (64, 224, 181, 5, 37, 111, 14)
    # layer4: 64 x 11 x 11 = 7744 positions: 61 stages of 128; 64 tiles: 6 splits of 11 (the last one 6)
    assert plan(64, 10, 10, 512, 512, 1) == (128, 152, 61, 11, 6, 384, 48)
    assert plan(3, 2, 2, 64, 64, 1) == (128, 152, 1, 1, 1, 1, 1)
    assert plan(2, 5, 159, 64, 64, 1) is None and plan(3, 1, 10, 64, 64, 2) is None and plan(3, 10, 1, 64, 64, 2) is None
    assert plan(2, 13, 13, 128, 192, 9) is None and plan(2, 13, 13, 96, 192, 1) is None
    assert C2.expect_wgrad(C2.WGRAD_CASES[C2.WGRAD_IDS.index("w158")]) == ("wgrad2_kernel<64,384>", 3, 5)
    assert C2.expect_wgrad(C2.WGRAD_CASES[C2.WGRAD_IDS.index("w38")]) == ("wgrad2_kernel<64,144>", 2, 6)
    # the first generation on 2 x 5 x 159 = 1590 px, 64 x 576: 5 tiles -> 103 splits wanted, 25 allowed: 64 px each
    assert C2.wgrad1_splits(1590, 64, 576, 1) == 25


def test_split_of_pixels_by_hand():
    # 1 x 4 x 158, Wp = 159, splits of 5 stages x 64 = 320 positions: rows 0, 1 start at D = 0, 159; D = 320 is row 2, column 2
    s = C2.split_of_pixels(1, 4, 158, 64, 5)[0, 0]
    assert s[1, 157] == 0 and s[2, 1] == 0 and s[2, 2] == 1 and s[3, 157] == (3 * 159 + 157) // 320 == 1
    assert int(C2.split_of_pixels(1, 4, 158, 64, 5).max()) + 1 <= 3


@pytest.mark.parametrize("kind", C2.KINDS)
@pytest.mark.parametrize("case", C2.CASES, ids=C2.IDS)
def test_rows_stay_inside_the_exact_domain(case, kind):
    """`reference` asserts the domain itself (stored integers <= 256, column sums < 2^24); here it must do so without raising, its
    operands must be the small integers the draw promises, and the dense draw must leave no channel pair with a minority of taps"""
    N, H, W, C, Kc, R, s, p = case["geom"]
    d = C2.reference(case, kind)
    for name, bound in (("x", 4), ("dy", 4), ("w", 2), ("wt", 2), ("shift", 8), ("res", 16), ("add", 16)):
        t = d[name]
        assert bool((t == t.round()).all()) and float(t.abs().max()) <= bound, name
    assert float(d["x"].abs().max()) > 0 and float(d["dy"].abs().max()) > 0
    if kind == "dense":
        for w in (d["w"], d["wt"]):
            assert float(w.abs().max()) == 1
            assert int((w != 0).sum(dim=(2, 3)).min()) >= (R * R + 1) // 2
        m = 232 // (4 * R * R)
        assert int((d["x"] != 0).sum(dim=1).max()) == min(m, C) == int((d["x"] != 0).sum(dim=1).min())
        assert int((d["dy"] != 0).sum(dim=1).max()) == min(m, Kc)
    for name in ("y", "y_full") if case["fwd"] else ():
        assert float(d[name].abs().max()) <= 256
    for name in ("dx", "dx2") + (("dx2c",) if "cadd" in d and case["dgrad"] else ()) if case["dgrad"] else ():
        assert float(d[name].abs().max()) <= 256
    if case["fwd"]:
        assert float(d["y"].abs().max()) > 0
    if case["dgrad"]:
        assert float(d["dx"].abs().max()) > 0 and float(d["colsum"].abs().max()) < 2 ** 24


@pytest.mark.parametrize("case", C2.WGRAD_CASES, ids=C2.WGRAD_IDS)
def test_wgrad_rows_stay_inside_the_exact_domain(case):
    N, H, W, C, Kc, items = case["geom"]
    xs, dys = C2.draw_wgrad(case)
    assert len(xs) == len(dys) == items
    refs = [C2.wgrad_reference(x, dy) for x, dy in zip(xs, dys)]
    for i, r in enumerate(refs):
        assert bool((r == r.round()).all()) and float(r.abs().max()) < 2 ** 24
        for j in range(i):
            assert not torch.equal(r, refs[j]), "every item has its own operands"
    # torch's own answer on all-ones operands is the closed form the GPU test uses
    ones = C2.wgrad_reference(torch.ones((N, C, H, W)), torch.ones((N, Kc, H, W)))
    r = torch.tensor([H - 1, H, H - 1]).view(3, 1) * torch.tensor([W - 1, W, W - 1]).view(1, 3) * N
    assert torch.equal(ones, r.float().expand(Kc, C, 3, 3))
