"""The ledger of second-generation bf16 convolution kernels (pure data + a restatement of the launch planners: imported by
tests/test_conv2_ledger_gpu.py and checked on the host by tests/test_conv2_cases_host.py).

Every row names, for the forward and the data gradient, the kernel instantiation the production library must reach, as
`cs_last_conv_variant()` reports it after the launch (launch_plan and its launch_*_t in csrc/conv_v2.hip,
launch_t in csrc/wgrad_v2.hip).  The names are written BY HAND from the dispatcher's rules, restated here so a reader can check a row.
M = destination pixels, NOUT = destination channels, ncc = source channels / 64 (forward: N*P*Q, K, C/64; data gradient: N*H*W, C, K/64):

  3x3, stride 1, pad 0..2 (plan_halo), NOUT a multiple of 128
    wide kernel   conv2_wide_kernel<TM,NBW,DG,9> where ncc >= 2 and every (32*TM px) x 128 ch tile is resident at once: TM from {8, 6, 4}
                  by the least ceil(tiles / CUs) * TM (the taller on ties), taken only if its tiles <= CUs; nb = window blocks per wave:
                  NBW = lo for nb <= lo, lo + 2 for nb <= lo + 2 (lo = 3 / 5 / 7 for TM 4 / 6 / 8); a wider window falls through to
    halo kernel   conv2_halo_kernel<9,3,TM,1,4,NBW,DG,false>: TM = 3 where 256 < ceil(M/128)*NOUT/128 <= 512 and ceil(M/96)*NOUT/128
                  <= 512, else 4 (pick_tm; a TM-3 window that does not fit retries TM 4); served for nb <= 8 with one chunk, nb <= 5 with
                  more; NBW = max(nb, 3), and 6..8 -> 8 (one LDS stage, one chunk only)
    2-D tiles     conv2_halo_kernel<9,3,4,1,4,3,DG,true> for what neither serves (wide images)
  3x3, NOUT = 64 and one chunk: conv2_halo_kernel<9,3,4,2,2,8,DG,false> (256 px x 64 ch) for nb(256 px) <= 8; nothing else with NOUT = 64
  window blocks   rows of 16 source positions that the BM destination pixels of a tile reach, in padded-linear coordinates (Wp = SW + PW
                  columns, Hp = SH + PW rows per image, PW = pad, or 2 - pad for the data gradient):
                  span = BM-1 + ceil((BM-1)/DW) * (Wp-DW) + ceil((BM-1)/(DH*DW)) * (Hp-DH) * Wp;  blocks = ceil((span + 2*Wp + 3) / 16);
                  per wave: nb = ceil(blocks / 4)
  1x1, pad 0 (plan_gemm); a stride-2 data gradient is compact (destination = the P x Q grid), a stride-2 forward gathers
    NOUT % 128 == 0   conv2_ring_kernel<TM,1,4,DG,false>, TM by pick_tm (3 or 4); at stride 1 with ncc a multiple of 4 and >= 8, where all
                  tiles are resident at once (TM from {6, 4} like the wide rule): conv2_wide_kernel<TM,TM,DG,2>
    NOUT == 64    conv2_ring_kernel<2,2,2,DG,false>
  partial rows    ceil(M / (32*TM)) for the 1 x 4 wave layouts, 2 * ceil(M / 256) resp. 2 * ceil(M / 128) for the 2 x 2 ones (halo / ring),
                  N * ceil(DH/8) * ceil(DW/16) for the 2-D tiles
  weight gradient (wgrad_v2.hip plan; 3x3, stride 1, pad 1, bf16, 1..8 items): wgrad2_kernel<BL,XR> by Wp = W + 1: <= 11 <128,152>,
                  <= 23 <128,176>, <= 39 <64,144>, <= 79 <64,224>, <= 159 <64,384>; wider, or H = 1 or W = 1: first generation
                  (wgrad_dma_kernel<BM,3,false,32>, BM = 128 for K > 64 else 64; an output of one row or column: wgrad_kernel<bf16,BM,128,true>).
                  n_stages = ceil(N*Hp*Wp / BL); splits wanted = ceil(384 / (K/64 * C/64 * items)), at most n_stages / 4 (at least 1);
                  stages_per_split = ceil(n_stages / wanted), nsplit = ceil(n_stages / stages_per_split)

The partial-row counts and the weight-gradient split plans are NOT written by hand: `expect()` / `expect_wgrad()` derive them from the
planners restated below; tests/test_conv2_cases_host.py pins the restatement to the built library's host queries and to literals."""
from conv_ref import sparse_pm1

CUS = 256                  # compute units of an unpartitioned MI355X: the count the hand-written names assume


def _b(v):
    return "true" if v else "false"


def HALO(tm, nbw, dg, t2d=False):
    return f"conv2_halo_kernel<9,3,{tm},1,4,{nbw},{_b(dg)},{_b(t2d)}>"


def HALO64(dg):
    return f"conv2_halo_kernel<9,3,4,2,2,8,{_b(dg)},false>"


def WIDE(tm, nbw, dg, ntap=9):
    return f"conv2_wide_kernel<{tm},{nbw},{_b(dg)},{ntap}>"


def RING(tm, wm, wn, dg):
    return f"conv2_ring_kernel<{tm},{wm},{wn},{_b(dg)},false>"


def W2(bl, xr):
    return f"wgrad2_kernel<{bl},{xr}>"


# ---- the planners of csrc/conv_v2.hip, restated
def _cdiv(a, b):
    return (a + b - 1) // b


def out_size(H, R, stride, pad):
    return (H + 2 * pad - R) // stride + 1


def _resident_tm(M, n_ntiles, cus, heights):
    """the tile height with the least rounds-of-residency x height (first of `heights` on ties), 0 unless its tiles all run at once"""
    best, best_cost, best_tiles = 0, 1 << 60, 0
    for tm in heights:
        tiles = _cdiv(M, 32 * tm) * n_ntiles
        cost = _cdiv(tiles, cus) * tm
        if cost < best_cost:
            best, best_cost, best_tiles = tm, cost, tiles
    return best if best_tiles <= cus else 0


def pick_wide_tm(M, n_ntiles, ncc, cus=CUS):
    return 0 if ncc < 2 else _resident_tm(M, n_ntiles, cus, (8, 6, 4))


def pick_wide1_tm(M, n_ntiles, ncc, cus=CUS):
    return 0 if ncc < 8 else _resident_tm(M, n_ntiles, cus, (6, 4))


def pick_tm(M, n_ntiles):
    """(the 256 / 512 of this rule are literals in the library, not the CU count)"""
    wg4, wg3 = _cdiv(M, 128) * n_ntiles, _cdiv(M, 96) * n_ntiles
    return 3 if 256 < wg4 <= 512 and wg3 <= 512 else 4


def window_blocks(BM, DH, DW, Hp, Wp):
    """16-position blocks of the padded-linear source window under BM consecutive destination pixels of a 3x3 convolution"""
    span = (BM - 1) + _cdiv(BM - 1, DW) * (Wp - DW) + _cdiv(BM - 1, DH * DW) * ((Hp - DH) * Wp)
    return (span + 2 * Wp + 2 + 1 + 15) // 16


def _sides(geom, dgrad, compact=False):
    """(SC, NOUT, SH, SW, DH, DW): source channels / extent and destination channels / extent of the launch"""
    N, H, W, C, K, R, stride, pad = geom
    P, Q = out_size(H, R, stride, pad), out_size(W, R, stride, pad)
    if dgrad:
        return K, C, P, Q, (P if compact else H), (Q if compact else W)
    return C, K, H, W, P, Q


def plan_halo(geom, dgrad, cus=CUS):
    """dict(cfg, tm, nbw, t2d, ncc, rows) of a 3x3 launch, None = not served.  cfg 1: 1 x 4 waves, 2: 2 x 2 waves (64 channels), 3: wide"""
    N, H, W, C, K, R, stride, pad = geom
    if R != 3 or stride != 1 or pad < 0 or pad > 2:
        return None
    SC, NOUT, SH, SW, DH, DW = _sides(geom, dgrad)
    if SC % 64 or NOUT % 64 or DH < 2 or DW < 2 or SH < 1 or SW < 1:
        return None
    PW = R - 1 - pad if dgrad else pad
    M = N * DH * DW
    if M >= (1 << 31) - 512 or N * SH * SW * SC * 2 >= 1 << 31 or M * NOUT * 2 >= 1 << 40:
        return None
    Wp, Hp = SW + PW, SH + PW
    if Wp < 2 or Hp < 2 or Wp < DW or Hp < DH or N * Hp * Wp + 4096 >= 1 << 31:
        return None
    ncc = SC // 64
    nb_of = lambda BM: (window_blocks(BM, DH, DW, Hp, Wp) + 3) // 4  # noqa: E731
    cfg, nbw, tm, t2d = 0, 0, 4, 0
    if NOUT % 128 == 0:
        wtm = pick_wide_tm(M, NOUT // 128, ncc, cus)
        if wtm:
            nb, lo = nb_of(32 * wtm), {4: 3, 6: 5, 8: 7}[wtm]
            if nb <= lo + 2:
                cfg, tm, nbw = 3, wtm, (lo if nb <= lo else lo + 2)
    if not cfg and NOUT % 128 == 0:
        tm = pick_tm(M, NOUT // 128)
        while tm <= 4:
            nb = nb_of(32 * tm)
            if nb <= (8 if ncc == 1 else 5):
                cfg, nbw = 1, max(nb, 3)
                break
            tm += 1
    elif not cfg and NOUT == 64 and ncc == 1:
        if nb_of(256) <= 8:
            cfg, nbw = 2, 8
    if not cfg and NOUT % 128 == 0:           # (a 10 x 18 window is 180 <= 192 rows: always true for 3x3)
        cfg, nbw, tm, t2d = 1, 3, 4, 1
    if not cfg:
        return None
    if cfg == 1 and ncc == 1 and nbw > 5:
        nbw = 8
    n_tiles = N * _cdiv(DW, 16) * _cdiv(DH, 8)
    if t2d and n_tiles >= 1 << 28:
        return None
    if _cdiv(NOUT, 32) * 32 * 9 * SC * 2 >= 1 << 31:
        return None
    BM = 32 * tm if cfg != 2 else 256
    rows = n_tiles if t2d else _cdiv(M, BM) * (1 if cfg != 2 else 2)
    return dict(cfg=cfg, tm=tm if cfg != 2 else 4, nbw=nbw, t2d=t2d, ncc=ncc, rows=rows)


def plan_gemm(geom, dgrad, cus=CUS):
    """the same for a 1x1 launch.  cfg 6: ring 1 x 4 waves, 7: ring 2 x 2 waves (64 channels), 8: wide kernel on two-plane stages"""
    N, H, W, C, K, R, stride, pad = geom
    if R != 1 or pad != 0 or stride < 1:
        return None
    compact = bool(dgrad) and stride != 1
    if compact and stride != 2:
        return None
    SC, NOUT, SH, SW, DH, DW = _sides(geom, dgrad, compact)
    if SC % 64 or NOUT % 64 or DH < 1 or DW < 1:
        return None
    if not dgrad and stride > 1 and (DH < 2 or DW < 2):
        return None
    ncc = SC // 64
    M = N * DH * DW
    if M >= (1 << 31) - 512 or N * SH * SW * SC * 2 >= 1 << 31:
        return None
    cfg = 6 if NOUT % 128 == 0 else 7 if NOUT == 64 else 0
    if not cfg or _cdiv(NOUT, 32) * 32 * SC * 2 >= 1 << 31:
        return None
    n_ntiles = _cdiv(NOUT, 128 if cfg == 6 else 64)
    tm = pick_tm(M, n_ntiles) if cfg == 6 else 2
    rows = _cdiv(M, 32 * tm) if cfg == 6 else _cdiv(M, 128) * 2
    nbw = 0
    if cfg == 6 and (dgrad or stride == 1) and not compact and ncc % 4 == 0:
        wtm = pick_wide1_tm(M, n_ntiles, ncc, cus)
        if wtm:
            cfg, tm, nbw, rows = 8, wtm, wtm, _cdiv(M, 32 * wtm)
    return dict(cfg=cfg, tm=tm, nbw=nbw, t2d=0, ncc=ncc, rows=rows)


def plan_any(geom, dgrad, cus=CUS):
    return plan_halo(geom, dgrad, cus) or plan_gemm(geom, dgrad, cus)


def variant_of(pl, dgrad):
    """the name launch_plan reports for a plan"""
    dg = bool(dgrad)
    if pl["cfg"] == 3:
        return WIDE(pl["tm"], pl["nbw"], dg)
    if pl["cfg"] == 2:
        return HALO64(dg)
    if pl["cfg"] == 1:
        return HALO(4, 3, dg, True) if pl["t2d"] else HALO(pl["tm"], pl["nbw"] if pl["nbw"] in (3, 4, 5) else 8, dg)
    if pl["cfg"] == 8:
        return WIDE(pl["tm"], pl["tm"], dg, 2)
    if pl["cfg"] == 6:
        return RING(pl["tm"], 1, 4, dg)
    return RING(2, 2, 2, dg)


def expect(case, op, cus=CUS):
    """(variant string, partial rows) of `op` in {fwd, dgrad} for a ledger row; (None, 0) where the packed kernels do not serve it"""
    pl = plan_any(case["geom"], op == "dgrad", cus)
    return (variant_of(pl, op == "dgrad"), pl["rows"]) if pl else (None, 0)


# ---- the planner of csrc/wgrad_v2.hip, and the first generation's split count (csrc/conv_igemm.hip wgrad_splits) for what it declines
W2_CLASSES = ((11, 128, 152), (23, 128, 176), (39, 64, 144), (79, 64, 224), (159, 64, 384))       # (largest Wp, BL, XR)


def plan_wgrad2(N, H, W, C, K, items):
    """dict(bl, xr, n_stages, stages_per_split, nsplit, total_work, per_xcd) of a 3x3 / stride 1 / pad 1 bf16 weight gradient, None = declined"""
    if C % 64 or K % 64 or items < 1 or items > 8:
        return None
    Wp, Hp = W + 1, H + 1
    if Wp == 2 or Hp == 2:
        return None
    cls = [c for c in W2_CLASSES if Wp <= c[0]]
    if not cls:
        return None
    _, bl, xr = cls[0]
    D = N * Hp * Wp
    if D + 4096 >= 0x7fffffff or N * H * W * max(C, K) * 2 >= 1 << 31 or K * 9 * C * 4 >= 1 << 31:
        return None
    n_stages = _cdiv(D, bl)
    tiles = (K // 64) * (C // 64) * items
    want = max(min(_cdiv(384, tiles), max(n_stages // 4, 1)), 1)
    sps = _cdiv(n_stages, want)
    nsplit = _cdiv(n_stages, sps)
    return dict(bl=bl, xr=xr, n_stages=n_stages, stages_per_split=sps, nsplit=nsplit, total_work=tiles * nsplit, per_xcd=_cdiv(tiles * nsplit, 8))


def wgrad1_splits(M, K, QE, items):
    """split count of the first-generation batched weight gradient (M pixels, QE = taps * C)"""
    tiles = _cdiv(K, 128 if K > 64 else 64) * _cdiv(QE, 128) * max(items, 1)
    want = max(min(_cdiv(512, tiles), _cdiv(M, 64)), 1)
    per = _cdiv(_cdiv(M, want), 32) * 32
    return _cdiv(M, per)


def expect_wgrad(case):
    """(variant string, nsplit, stages_per_split) of a weight-gradient row; stages_per_split = 0 where the first generation serves it"""
    N, H, W, C, K, items = case["geom"]
    pl = plan_wgrad2(N, H, W, C, K, items)
    if pl:
        return W2(pl["bl"], pl["xr"]), pl["nsplit"], pl["stages_per_split"]
    from igemm_cases import WDMA, WG, WSPEC
    bm = 128 if K > 64 else 64
    name = WG("bf16", bm, True) if H == 1 or W == 1 else (WSPEC if bm == 128 and K >= 256 else WDMA)(bm, False)
    return name, wgrad1_splits(N * H * W, K, 9 * C, items), 0


def C_(id, geom, fwd, dgrad, note=""):
    return dict(id=id, geom=geom, fwd=fwd, dgrad=dgrad, note=note)


F_, T_ = False, True
# geom = (N, H, W, Cin, Cout, R, stride, pad); fwd / dgrad: the instantiation at 256 CUs, None = the packed kernels decline (3x3 into 64
# channels from more than one chunk).  "nb" in the notes: window blocks per wave of the tile height tried.
CASES = [
    # ---- 3x3 halo kernel, 128-pixel tiles (TM 4): one partial tile, then several tiles with a tail
    C_("halo4_nb3_f1", (1, 3, 3, 64, 128, 3, 1, 2), HALO(4, 3, F_), None, "5x5 output = its padded source, 25 px: 127 + 0 + 0 + 13 = 140 rows -> 9 blocks: nb 3"),
    C_("halo4_nb3_f", (2, 13, 10, 64, 128, 3, 1, 1), HALO(4, 3, F_), None, "260 px: 3 tiles, tail of 4; Wp 11, Hp 14: 127 + 13 + 11 + 25 = 176 rows -> 11 blocks: nb 3"),
    C_("halo4_nb3_d", (2, 13, 10, 128, 64, 3, 1, 0), None, HALO(4, 3, T_), "valid convolution: the gradient's source 11x8, padded by 2, is its destination 13x10: 127 + 0 + 0 + 23 = 150 rows: nb 3"),
    C_("halo4_nb4_f", (3, 13, 10, 64, 128, 3, 1, 0), HALO(4, 4, F_), None, "11x8 output in an unpadded 13x10 source: 127 + 32 + 40 + 23 = 222 rows -> 14 blocks: nb 4"),
    C_("halo4_nb4_d", (2, 13, 10, 128, 64, 3, 1, 2), None, HALO(4, 4, T_), "pad 2: source 15x12 unpadded, destination 13x10: 127 + 26 + 24 + 27 = 204 rows -> 13 blocks: nb 4"),
    C_("halo4_nb5_f1", (1, 7, 5, 64, 128, 3, 1, 0), HALO(4, 5, F_), None, "5x3 output, 15 px, in a 7x5 source: 127 + 86 + 90 + 13 = 316 rows: nb 5"),
    C_("halo4_nb5_d1", (1, 5, 3, 128, 64, 3, 1, 2), None, HALO(4, 5, T_), "its mirror image: source 7x5, destination 5x3"),
    C_("halo4_nb5_f", (2, 26, 31, 64, 128, 3, 1, 0), HALO(4, 5, F_), None, "24x29 output in 26x31: 127 + 10 + 62 + 65 = 264 rows -> 17 blocks: nb 5; 11 tiles"),
    C_("halo4_nb5_d", (2, 26, 31, 128, 64, 3, 1, 2), None, HALO(4, 5, T_), "source 28x33 unpadded, destination 26x31: 127 + 10 + 66 + 69 = 272 rows: nb 5; 13 tiles"),
    C_("halo4_nb8_f1", (1, 5, 5, 64, 128, 3, 1, 0), HALO(4, 8, F_), None, "3x3 output in 5x5: 127 + 86 + 150 + 13 = 376 rows -> 24 blocks: nb 6 -> the one-stage NBW 8"),
    C_("halo4_nb8_d1", (1, 3, 3, 128, 64, 3, 1, 2), None, HALO(4, 8, T_), "its mirror image"),
    C_("halo4_nb8_f", (1, 40, 75, 64, 128, 3, 1, 1), HALO(4, 8, F_), None, "Wp 76: 127 + 2 + 76 + 155 = 360 rows -> 23 blocks: nb 6 -> 8; 24 tiles, tail of 56"),
    C_("halo4_nb8_d", (1, 40, 75, 128, 64, 3, 1, 1), None, HALO(4, 8, T_), "pad 1 is its own mirror: the same window"),
    # ---- 3x3 into 64 channels from one chunk: 256-pixel tiles on 2 x 2 waves
    C_("halo64_p2", (2, 12, 17, 64, 64, 3, 1, 2), HALO64(F_), HALO64(T_), "forward 14x19 = 532 px: 3 tiles, 296 rows -> 19 blocks: nb 5; gradient 408 px: 2 tiles, 255 + 30 + 76 + 41 = 402 rows -> 26 blocks: nb 7"),
    C_("halo64_p0", (2, 19, 15, 64, 64, 3, 1, 0), HALO64(F_), HALO64(T_), "forward 17x13 = 442 px: 2 tiles, 255 + 40 + 60 + 33 = 388 rows: nb 7; gradient 570 px: 3 tiles, 288 rows: nb 5"),
    # ---- 3x3 on 2-D tiles: what the linear window does not serve
    C_("t2d_f1", (1, 5, 5, 128, 128, 3, 1, 0), HALO(4, 3, F_, True), WIDE(4, 3, T_), "two chunks and nb 6 (halo4_nb8_f1's window): neither wide (<= 5) nor halo (<= 5)"),
    C_("t2d_d1", (1, 3, 3, 128, 128, 3, 1, 2), WIDE(4, 3, F_), HALO(4, 3, T_, True), "the mirror image; its forward is halo4_nb3_f1's window on two chunks: wide, TM 4"),
    C_("t2d_f", (3, 5, 7, 128, 128, 3, 1, 0), HALO(4, 3, F_, True), WIDE(4, 3, T_), "3x5 output in 5x7: 127 + 52 + 126 + 17 = 322 rows -> 21 blocks: nb 6; one 8x16 tile per image: 3 tiles"),
    # ---- 3x3 wide kernel, TM 4 (a single round of 128-pixel tiles costs 4, less than 6 or 8)
    C_("wide4_nb3", (2, 13, 10, 128, 128, 3, 1, 1), WIDE(4, 3, F_), WIDE(4, 3, T_), "halo4_nb3_f's window on two chunks, both directions; 3 tiles"),
    C_("wide4_nb5_f", (3, 13, 10, 128, 128, 3, 1, 0), WIDE(4, 5, F_), WIDE(4, 3, T_), "halo4_nb4_f's window: nb 4 -> the next instantiated count, 5"),
    C_("wide4_nb5_d", (2, 13, 10, 128, 128, 3, 1, 2), WIDE(4, 3, F_), WIDE(4, 5, T_), "halo4_nb4_d's window: nb 4 -> 5"),
    # ---- 1x1 ring and wide kernels, stride 1
    C_("ring222", (2, 13, 10, 64, 64, 1, 1, 0), RING(2, 2, 2, F_), RING(2, 2, 2, T_), "64 destination channels either way; 260 px: 3 tiles of 128"),
    C_("ring414_f", (2, 13, 10, 64, 128, 1, 1, 0), RING(4, 1, 4, F_), RING(2, 2, 2, T_), "3 tiles: pick_tm 4"),
    C_("ring414_d", (2, 13, 10, 128, 64, 1, 1, 0), RING(2, 2, 2, F_), RING(4, 1, 4, T_), "two chunks: ncc % 4 != 0 keeps the ring kernel"),
    C_("ring414_c5", (1, 5, 5, 320, 128, 1, 1, 0), RING(4, 1, 4, F_), None, "five chunks (the slot ring wraps), one partial tile; 320 is no multiple of 128 nor 64: no gradient"),
    C_("wide1_tm4_f", (2, 13, 10, 512, 128, 1, 1, 0), WIDE(4, 4, F_, 2), RING(4, 1, 4, T_), "8 chunks, 3 tiles resident: TM 4 (cost 4 < 6); gradient: 2 chunks -> ring"),
    C_("wide1_tm4_d", (2, 13, 10, 128, 512, 1, 1, 0), RING(4, 1, 4, F_), WIDE(4, 4, T_, 2), "the gradient contracts the 512"),
    # ---- 1x1 at stride 2: gathered forward, compact data gradient (destination = the P x Q grid)
    C_("s2_ring222_f", (2, 37, 41, 256, 64, 1, 2, 0), RING(2, 2, 2, F_), RING(4, 1, 4, T_), "19x21 output; the compact gradient has 256 channels: 1 x 4 waves, 7 tiles"),
    C_("s2_ring414_f", (3, 21, 17, 64, 256, 1, 2, 0), RING(4, 1, 4, F_), RING(2, 2, 2, T_), "11x9 output, 297 px; the compact gradient into 64 channels"),
    # ---- tile heights 3, 6 and 8: by the rules these need tens of thousands of pixel-channels (0.3 - 7.5 GMAC)
    C_("halo3_nb3_f", (64, 9, 10, 64, 512, 3, 1, 2), HALO(3, 3, F_), None, "11x12 output, 8448 px x 4 channel tiles: 264 workgroups of 128 px, 352 of 96: TM 3; the output fills its padded source: 95 + 0 + 0 + 27 rows -> 8 blocks: nb 2 -> 3"),
    C_("halo3_nb3_d", (64, 10, 13, 512, 64, 3, 1, 0), None, HALO(3, 3, T_), "8320 px x 4: 260 / 348 workgroups; the destination 10x13 is its padded source: 95 + 0 + 0 + 29 rows: nb 2 -> 3"),
    C_("halo3_nb4_f", (3, 45, 57, 64, 512, 3, 1, 2), HALO(3, 4, F_), None, "47x59 output, 8319 px x 4: 260 / 348; Wp 59: 95 + 0 + 0 + 121 = 216 rows -> 14 blocks: nb 4"),
    C_("halo3_nb4_d", (6, 97, 57, 128, 64, 3, 1, 0), None, HALO(3, 4, T_), "33174 px x 1 channel tile: 260 / 346; Wp 57 = DW: 95 + 0 + 0 + 117 = 212 rows -> 14 blocks: nb 4"),
    C_("halo3_nb5_f", (6, 97, 57, 64, 128, 3, 1, 1), HALO(3, 5, F_), None, "Wp 58: 95 + 2 + 58 + 119 = 274 rows -> 18 blocks: nb 5"),
    C_("halo3_nb5_d", (6, 57, 97, 128, 64, 3, 1, 0), None, HALO(3, 5, T_), "Wp 97 = DW: 95 + 0 + 0 + 197 = 292 rows -> 19 blocks: nb 5"),
    C_("halo3_nb8_f", (6, 57, 97, 64, 128, 3, 1, 1), HALO(3, 8, F_), None, "Wp 98: 95 + 1 + 98 + 199 = 393 rows -> 25 blocks: nb 7 -> 8"),
    C_("halo3_nb8_d", (6, 57, 97, 128, 64, 3, 1, 1), None, HALO(3, 8, T_), "pad 1 is its own mirror: the same window"),
    C_("ring314_f", (6, 57, 97, 64, 128, 1, 1, 0), RING(3, 1, 4, F_), RING(2, 2, 2, T_), "33174 px: 260 workgroups of 128 px, 346 of 96: TM 3; gradient: 260 tiles on 2 x 2 waves"),
    C_("ring314_d", (6, 57, 97, 128, 64, 1, 1, 0), RING(2, 2, 2, F_), RING(3, 1, 4, T_), "the same the other way round; two chunks"),
    C_("wide1_tm6_f", (6, 57, 97, 512, 128, 1, 1, 0), WIDE(6, 6, F_, 2), RING(4, 1, 4, T_), "8 chunks; 173 tiles of 192 px run at once (cost 6), 260 of 128 px take two rounds (8); gradient: 2 chunks, 1040 workgroups: ring, TM 4"),
    C_("wide1_tm6_d", (6, 57, 97, 128, 512, 1, 1, 0), RING(4, 1, 4, F_), WIDE(6, 6, T_, 2), "the same the other way round"),
    C_("wide6_nb5_f", (64, 9, 10, 128, 512, 3, 1, 2), WIDE(6, 5, F_), WIDE(4, 5, T_), "8448 px x 4: 132 tiles of 256 px (cost 8), 176 of 192 (6), 264 of 128 (two rounds: 8): TM 6; 191 + 0 + 0 + 27 rows -> 14 blocks: nb 4 -> 5; "
       "gradient 5760 px x 1: 45 tiles of 128 (cost 4); 9x10 in an 11x12 source: 127 + 26 + 48 + 27 rows -> 15 blocks: nb 4 -> 5"),
    C_("wide6_nb5_d", (6, 97, 57, 128, 128, 3, 1, 0), HALO(4, 3, F_, True), WIDE(6, 5, T_), "gradient 33174 px: 130 / 173 / 260 tiles: TM 6; 191 + 0 + 0 + 117 rows -> 20 blocks: nb 5; "
       "forward 95x55, 245 tiles of 128 (cost 4): 127 + 6 + 114 + 117 rows -> 23 blocks: nb 6 fits neither wide nor halo (two chunks): 2-D tiles"),
    C_("wide6_nb7", (6, 97, 57, 128, 128, 3, 1, 1), WIDE(6, 7, F_), WIDE(6, 7, T_), "Wp 58: 191 + 4 + 58 + 119 = 372 rows -> 24 blocks: nb 6 -> 7, both directions"),
    C_("wide8_nb7_f", (64, 9, 17, 128, 512, 3, 1, 2), WIDE(8, 7, F_), WIDE(4, 5, T_), "11x19 output, 13376 px x 4: 212 tiles of 256 px (cost 8), 280 of 192 (two rounds: 12), 420 of 128 (8): the taller on the tie; "
       "255 + 0 + 0 + 41 rows -> 19 blocks: nb 5 -> 7; gradient 9792 px x 1: TM 4, 127 + 16 + 38 + 41 rows: nb 4 -> 5"),
    C_("wide8_nb7_d", (16, 25, 31, 512, 128, 3, 1, 0), WIDE(4, 5, F_), WIDE(8, 7, T_), "gradient 12400 px x 4: 196 / 260 / 388 tiles: 8 / 12 / 8: TM 8; 255 + 0 + 0 + 65 rows -> 20 blocks: nb 5 -> 7; "
       "forward 23x29 x 1, 84 tiles of 128: 127 + 10 + 62 + 65 rows -> 17 blocks: nb 5; eight chunks"),
    C_("wide8_nb9_f", (5, 75, 131, 128, 128, 3, 1, 2), WIDE(8, 9, F_), HALO(4, 3, T_, True), "77x133 output, 51205 px: 201 / 267 / 401 tiles: 8 / 12 / 8: TM 8; 255 + 0 + 0 + 269 rows -> 33 blocks: nb 9; "
       "gradient 49125 px: 256 tiles of 192 run at once but nb 12 > 7, and the halo windows (nb 10 at TM 3, 11 at TM 4) exceed 5: 2-D tiles, 450 of them"),
    C_("wide8_nb9_d", (1, 97, 131, 512, 128, 3, 1, 0), HALO(4, 3, F_, True), WIDE(8, 9, T_), "gradient 12707 px x 4: 200 / 268 / 400 tiles: TM 8; 255 + 0 + 0 + 265 rows -> 33 blocks: nb 9; forward 95x129: nb 11: 2-D tiles"),
]
IDS = [c["id"] for c in CASES]


def W_(id, geom, variant, note=""):
    return dict(id=id, geom=geom, variant=variant, note=note)


# weight-gradient rows: geom = (N, H, W, C, K, items), every item with its own operands.  Both sides of every stage-class boundary
# (XR = BL + 2 * Wp + 2 rows is exact at the last width of a class), with enough positions for several splits and a short last one.
WGRAD_CASES = [
    W_("w2", (40, 7, 2, 64, 64, 1), W2(128, 152), "Wp = 3, the smallest magic divisor; 960 positions: 8 stages in splits of 4"),
    W_("w10", (4, 23, 10, 64, 64, 1), W2(128, 152), "Wp = 11, the last of its class: 152 = 128 + 22 + 2; 1056 positions: 9 stages in splits of 5 + 4"),
    W_("w11", (4, 23, 11, 64, 64, 1), W2(128, 176), "Wp = 12; 1152 positions: 9 stages exactly"),
    W_("w22", (3, 15, 22, 64, 64, 1), W2(128, 176), "Wp = 23: 176 = 128 + 46 + 2; 1104 positions: 9 stages"),
    W_("w23", (3, 9, 23, 64, 64, 1), W2(64, 144), "Wp = 24; 720 positions: 12 stages of 64 in splits of 4"),
    W_("w38", (2, 8, 38, 64, 64, 1), W2(64, 144), "Wp = 39: 144 = 64 + 78 + 2; 702 positions: 11 stages in splits of 6 + 5"),
    W_("w39", (2, 8, 39, 64, 64, 1), W2(64, 224), "Wp = 40; 720 positions: 12 stages"),
    W_("w78", (1, 8, 78, 64, 64, 1), W2(64, 224), "Wp = 79: 224 = 64 + 158 + 2; 711 positions: 12 stages"),
    W_("w79", (1, 8, 79, 64, 64, 1), W2(64, 384), "Wp = 80; 720 positions: 12 stages"),
    W_("w158", (1, 4, 158, 64, 64, 1), W2(64, 384), "Wp = 159, the last served width: 384 = 64 + 318 + 2; 795 positions: 13 stages in splits of 5 + 5 + 3 (the last one holds only the zero row behind the image: an all-zero slab)"),
    W_("w158_n2", (2, 3, 158, 64, 64, 1), W2(64, 384), "1272 positions: 20 stages in five splits of 4; two images"),
    W_("w159", (2, 5, 159, 64, 64, 1), "wgrad_dma_kernel<64,3,false,32>", "Wp = 160 is declined: the first generation serves it"),
    W_("h1", (3, 1, 10, 64, 64, 2), "wgrad_kernel<bf16,64,128,true>", "H = 1 (Hp = 2 has no magic divisor) is declined; nor has the first generation's DMA pixel walk "
       "one for P = 1: its register-staged kernel"),
    W_("h1_k128", (3, 1, 10, 64, 128, 1), "wgrad_kernel<bf16,128,128,true>", "the same with K > 64: BM = 128"),
    W_("w1", (3, 10, 1, 64, 64, 1), "wgrad_kernel<bf16,64,128,true>", "W = 1: the same for Q = 1"),
    W_("items8", (2, 13, 13, 128, 192, 8), W2(128, 176), "eight different operand pairs; a 3 x 2 tile grid: 48 tiles, 4 stages: one split"),
    W_("work6", (2, 19, 19, 128, 64, 3), W2(128, 176), "6 work items: not a multiple of the 8 XCD runs"),
    W_("one_stage", (3, 2, 2, 64, 64, 1), W2(128, 152), "27 positions: a single stage, a single split"),
    W_("items5_splits", (3, 9, 23, 64, 128, 5), W2(64, 144), "five items x two k tiles x three splits of 4 stages: 30 work items"),
]
WGRAD_IDS = [c["id"] for c in WGRAD_CASES]


# ---- operands and references
def _pm(shape, a, g):
    """integers of magnitude 1..a with a random sign"""
    import torch
    return torch.randint(1, a + 1, shape, generator=g).float() * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


def _few_channels(N, C, H, W, m, a, g):
    """NCHW integers with exactly min(m, C) non-zero channels per pixel, of magnitude 1..a"""
    import torch
    m = min(m, C)
    idx = torch.rand((N, H, W, C), generator=g).topk(m, dim=-1).indices
    t = torch.zeros((N, H, W, C)).scatter_(-1, idx, _pm((N, H, W, m), a, g))
    return t.permute(0, 3, 1, 2).contiguous()


def _dense_pm1(rows, cols, taps, g):
    """[rows][cols][taps] in {-1, 0, 1}: every (row, col) pair keeps at least half of its taps (all of a single one) non-zero"""
    import torch
    w = _pm((rows, cols, taps), 1, g)
    zeros = torch.randint(0, taps // 2 + 1, (rows, cols, 1), generator=g)                  # how many taps of the pair are zeroed
    rank = torch.rand((rows, cols, taps), generator=g).argsort(dim=-1).argsort(dim=-1)
    return w * (rank >= zeros)


def draw(case, kind):
    """Integer operands of a row (NCHW / KCRS fp32 on the CPU) in one of two kinds:

    sparse   x, dy in {-4..4}; twelve weights of +-1 / +-2 per output row (forward: per output channel; the data gradient has its own
             filter, sparse per input channel): sums <= 96
    dense    weights in {-1, 0, 1} with at least half of the taps of EVERY channel pair non-zero, so that no mis-indexed tap or chunk
             hides behind a zero weight; x and dy with m = 232 / (4 * taps) non-zero channels per pixel of magnitude <= 4 (6 for 3x3,
             58 for 1x1): sums <= taps * m * 4 <= 232

    plus shift in {-8..8}, residual and add in {-16..16}, a mask keeping 60 %, and for the 1x1 stride-1 rows a compact add operand
    `cadd` [N][C][ceil(H/2)][ceil(W/2)] in {-16..16}.  Every stored value is then an integer of magnitude <= 256."""
    import torch
    N, H, W, C, K, R, stride, pad = case["geom"]
    P, Q = out_size(H, R, stride, pad), out_size(W, R, stride, pad)
    g = torch.Generator().manual_seed(4000 + 2 * IDS.index(case["id"]) + (kind == "dense"))
    if kind == "sparse":
        x = torch.randint(-4, 5, (N, C, H, W), generator=g).float()
        dy = torch.randint(-4, 5, (N, K, P, Q), generator=g).float()
        w = sparse_pm1((K, C, R, R), min(12, C * R * R), g)
        wt = sparse_pm1((C, K, R, R), min(12, K * R * R), g).permute(1, 0, 2, 3).contiguous()
    else:
        assert kind == "dense", kind
        m = 232 // (4 * R * R)
        x = _few_channels(N, C, H, W, m, 4, g)
        dy = _few_channels(N, K, P, Q, m, 4, g)
        w = _dense_pm1(K, C, R * R, g).view(K, C, R, R)
        wt = _dense_pm1(K, C, R * R, g).view(K, C, R, R)
    d = dict(x=x, dy=dy, w=w, wt=wt)
    d["shift"] = torch.randint(-8, 9, (K,), generator=g).float()
    d["res"] = torch.randint(-16, 17, (N, K, P, Q), generator=g).float()
    d["add"] = torch.randint(-16, 17, (N, C, H, W), generator=g).float()
    d["mask"] = torch.rand((N, C, H, W), generator=g) > 0.4
    if R == 1 and stride == 1:
        d["cadd"] = torch.randint(-16, 17, (N, C, (H + 1) // 2, (W + 1) // 2), generator=g).float()
    return d


KINDS = ("sparse", "dense")
_REF = {}
_KEEP = 1 << 20            # rows with at most this many activation elements keep their reference for the other tests of the run


def reference(case, kind):
    """draw(case, kind) plus torch's CPU fp32 results, with the exact domain asserted on them (stored values <= 256, column sums
    < 2^24): y, y_full = relu(y + shift + res), dx, dx2 = (dx + add) * mask, colsum of dx2, and for the 1x1 stride-1 rows
    dx2c = (dx + cadd at the even pixels) * mask with its colsum.  Shared between tests: do not modify."""
    key = (case["id"], kind)
    if key in _REF:
        return _REF[key]
    import torch
    import torch.nn.functional as F
    N, H, W, C, K, R, stride, pad = case["geom"]
    d = draw(case, kind)
    stored = []
    if case["fwd"]:
        d["y"] = F.conv2d(d["x"], d["w"], stride=stride, padding=pad)
        d["y_full"] = torch.relu(d["y"] + d["shift"].view(1, -1, 1, 1) + d["res"])
        stored += [d["y"], d["y"] + d["shift"].view(1, -1, 1, 1) + d["res"]]
    if case["dgrad"]:
        d["dx"] = torch.nn.grad.conv2d_input((N, C, H, W), d["wt"], d["dy"], stride=stride, padding=pad)
        d["dx2"] = (d["dx"] + d["add"]) * d["mask"]
        stored += [d["dx"], d["dx"] + d["add"]]
        sums = [d["dx2"]]
        if "cadd" in d:
            dense = torch.zeros((N, C, H, W))
            dense[:, :, ::2, ::2] = d["cadd"]
            d["dx2c"] = (d["dx"] + dense) * d["mask"]
            stored.append(d["dx"] + dense)
            sums.append(d["dx2c"])
            d["colsum_c"] = d["dx2c"].sum(dim=(0, 2, 3))
        d["colsum"] = d["dx2"].sum(dim=(0, 2, 3))
        for t in sums:
            assert float(t.abs().sum(dim=(0, 2, 3)).max()) < 2 ** 24, (key, "a column sum leaves the exact domain")
    for t in stored:
        assert float(t.abs().max()) <= 256 and bool((t == t.round()).all()), (key, "a stored value leaves the exact domain")
    if N * max(C * H * W, K * d["dy"].shape[2] * d["dy"].shape[3]) <= _KEEP:
        _REF[key] = d
    return d


def draw_wgrad(case):
    """`items` different operand pairs (x [N][C][H][W] in {-4..4}, dy [N][K][H][W] in {-3..3}) of a weight-gradient row"""
    import torch
    N, H, W, C, K, items = case["geom"]
    g = torch.Generator().manual_seed(7000 + WGRAD_IDS.index(case["id"]))
    xs = [torch.randint(-4, 5, (N, C, H, W), generator=g).float() for _ in range(items)]
    dys = [torch.randint(-3, 4, (N, K, H, W), generator=g).float() for _ in range(items)]
    return xs, dys


def wgrad_reference(x, dy):
    """torch's CPU fp32 weight gradient [K][C][3][3] of a 3x3 / stride 1 / pad 1 convolution; sums of |x||dy| stay below 2^24"""
    import torch
    N, C, H, W = x.shape
    assert N * H * W * float(x.abs().max()) * float(dy.abs().max()) < 2 ** 24, "a weight-gradient sum could leave the exact domain"
    return torch.nn.grad.conv2d_weight(x, (dy.shape[1], C, 3, 3), dy, stride=1, padding=1)


def split_of_pixels(N, H, W, bl, stages_per_split):
    """[N][1][H][W] int64: the split whose stages hold the padded-linear position D = (n * Hp + y) * Wp + x of every dy pixel"""
    import torch
    n, y, x = torch.meshgrid(torch.arange(N), torch.arange(H), torch.arange(W), indexing="ij")
    return (((n * (H + 1) + y) * (W + 1) + x) // (bl * stages_per_split)).view(N, 1, H, W)
