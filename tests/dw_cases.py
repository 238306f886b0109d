"""The ledger of depthwise kernel instantiations (pure data + a restatement of the launch planners: imported by
tests/test_depthwise_routes_gpu.py and checked on the host by tests/test_dw_cases_host.py).

Every row names, per operation, the kernel instantiation the production library must reach, as `cs_last_conv_variant()` reports it
after the launch (dw_note_variant in csrc/dwse.hip): `<kernel template name> grid=(x,y,z) per=<items per workgroup> lanes=<cpt or cgt>`.
The kernel names are written BY HAND from the dispatcher's rules ("Depthwise routing"), restated here so a reader can
check a row; all rows use "same" padding, pad = (k - 1) / 2:

  strips         bf16, k in {3, 5}, stride in {1, 2}: forward, forward + statistics, weight gradient, and the stride-1 data gradient
                 (the mirrored-filter convolution: FLIP = true, source dy, destination dx, so its strips run along W, not Q).
                 TS from {8, 5} at stride 1 and {4, 5} at stride 2: the one that wastes fewer columns of the destination row
                 (Q = 16 -> 8, Q = 15 -> 5; stride 2: Q = 8 or 11 -> 4, Q = 10 -> 5); ties go to 8 / 4.
  no exception   dw_strip_fwd_ok keeps the bf16 3x3 stride-2 forward with C <= 144 on dw_tile_kernel only where dw_tiled_geometry
                 admits the geometry, and for a stride-2 forward that takes C >= 288: in production the two never meet, and these
                 forwards run on strips like every other (the A/B flavour's CELLSEG_DW_UNTILED=2 is what makes the exception bite)
  stride-2 dgrad k in {3, 5}: dw_dgrad_s2_kernel (2 x 2 input blocks), both dtypes
  f32 forward    3x3 at stride 1, or at stride 2 with C >= 288: dw_tile_kernel; everything else (every 5x5, whatever C) element-per-thread
  f32 dgrad      stride 1 with C <= 48: dw_tile_kernel with FLIP; stride 1 with more channels: element-per-thread
  f32 wgrad      dw_wgrad_kernel
  7x7 (any k outside {3, 5}): the element-per-thread kernels for every operation and dtype

grid, per, lanes and the partial-row counts are NOT written by hand: `expect()` derives them from the planners of csrc/dwse.hip, restated
below in Python from the formulas (dw_strip_shape, dw_strip_plan, dw_tile_shape, dw_tile_items, dw_wgrad_split, dw_stats_grid);
tests/test_dw_cases_host.py pins that restatement to literal values worked out by hand."""
import math

BF, F32 = "bf16", "f32"
N = 2                      # batch of every row


def _b(v):
    return "true" if v else "false"


def STRIP(r, s, ts, flip=False):
    return f"dw_conv_strip_kernel<{r},{s},{ts},false,{_b(flip)}>"


def WSTRIP(r, s, ts):
    return f"dw_wgrad_strip_kernel<{r},{s},{ts}>"


def TILE(t, r, s, flip=False):
    return f"dw_tile_kernel<{t},{r},{s},false,{_b(flip)}>"


def S2(t, r):
    return f"dw_dgrad_s2_kernel<{t},{r}>"


def EL(kind, t):
    return f"dw_{kind}_kernel<{t}>"


def stats_variant(fwd):
    """the forward + statistics instantiation that goes with a plain forward: STATS = true / the statistics kernel"""
    return fwd.replace(",false,false>", ",true,false>").replace("dw_fwd_kernel<", "dw_fwd_stats_kernel<")


# ---- the planners of csrc/dwse.hip, restated
def _cdiv(a, b):
    return (a + b - 1) // b


def dw_strip_shape(C):
    """(chunks, cpt): the channel-pair tile that keeps most of the 256 lanes busy, at least 16 pairs; score = lane use * fill - ch / 2000"""
    CP = C // 2
    best, chunks, cpt = None, 1, min(CP, 256)
    for ch in range(_cdiv(CP, 256), _cdiv(CP, 16) + 1):
        t = _cdiv(CP, ch)
        if t > 256:
            continue
        score = ((256 // t) * t / 256.0) * (CP / (float(ch) * t)) - 0.0005 * ch          # (doubles, in the order of the C++)
        if best is None or score > best:
            best, chunks, cpt = score, ch, t
    return chunks, cpt


def dw_strip_plan(n, P, Q, C, stride, rows_cap):
    """(ts, per, chunks, cpt, nblk) of a strip launch over the destination n x P x Q; ~4096 workgroups, at most rows_cap along x"""
    a, b = (8 if stride == 1 else 4), 5
    ts = b if _cdiv(Q, b) * b < _cdiv(Q, a) * a else a
    chunks, cpt = dw_strip_shape(C)
    items = n * P * _cdiv(Q, ts)
    blocks = min(max(4096 // chunks, 1), rows_cap)
    per = max(_cdiv(items, blocks), 2 * (256 // cpt))
    return ts, per, chunks, cpt, _cdiv(items, per)


def dw_tile_shape(C):
    CG = C // 8
    chunks = _cdiv(CG, 32)
    return chunks, _cdiv(CG, chunks)


def dw_tile_items(items, chunks, cgt):
    blocks = max(2048 // chunks, 1)
    return max(_cdiv(items, blocks), 4 * (256 // cgt))


def dw_wgrad_split(n, P, Q, C, R):
    """(rows per block, slabs) of the element-per-thread weight gradient"""
    rows = n * P
    chunks = _cdiv(C // 8, 64) * _cdiv(R * R, 9)
    slabs = min(max(1024 // chunks, 1), max((32 << 20) // (R * R * C * 4), 256))
    rpb = max(_cdiv(rows, slabs), _cdiv(64, Q))
    return rpb, _cdiv(rows, rpb)


def dw_stats_grid(n, P, Q, C):
    CG = C // 8
    m = CG // math.gcd(CG, 256)
    return max(_cdiv(min(_cdiv(n * P * Q * CG, 256), 1024), m) * m, m)


def grid_ew(total):
    return min(max(_cdiv(total, 256), 1), 16384)


def out_size(H, k, s):
    return (H + 2 * ((k - 1) // 2) - k) // s + 1


def expect(case, op):
    """(variant string, partial rows) of `op` in {fwd, fwd_stats, dgrad, wgrad} for a ledger row"""
    C, k, s, H, W = case["geom"]
    P, Q = out_size(H, k, s), out_size(W, k, s)
    name = stats_variant(case["fwd"]) if op == "fwd_stats" else case[op]
    kernel = name.split("<")[0]
    z = 1
    if kernel in ("dw_conv_strip_kernel", "dw_wgrad_strip_kernel"):
        dP, dQ = (H, W) if op == "dgrad" else (P, Q)
        cap = max((32 << 20) // (k * k * C * 4), 128) if op == "wgrad" else 2048
        ts, per, y, lanes, x = dw_strip_plan(N, dP, dQ, C, s, cap)
        assert name.split(",")[2].rstrip(">") == str(ts), (case["id"], op, ts)
    elif kernel in ("dw_tile_kernel", "dw_dgrad_s2_kernel"):
        y, lanes = dw_tile_shape(C)
        if kernel == "dw_dgrad_s2_kernel":
            items = N * _cdiv(H, 2) * _cdiv(W, 2)
        else:
            dP, dQ = (H, W) if op == "dgrad" else (P, Q)
            items = N * dP * _cdiv(dQ, 2)
        per = dw_tile_items(items, y, lanes)
        x = _cdiv(items, per)
    elif kernel == "dw_wgrad_kernel":
        rpb, x = dw_wgrad_split(N, P, Q, C, k)
        per, lanes, y, z = rpb * Q, 0, _cdiv(C // 8, 64), _cdiv(k * k, 9)
    else:
        per = lanes = 0
        y = 1
        x = dw_stats_grid(N, P, Q, C) if op == "fwd_stats" else grid_ew(N * (H * W if op == "dgrad" else P * Q) * (C // 8))
    rows = x if op in ("fwd_stats", "wgrad") else 0
    return f"{name} grid=({x},{y},{z}) per={per} lanes={lanes}", rows


def C_(id, geom, dtype, fwd, dgrad, wgrad, note=""):
    return dict(id=id, geom=geom, dtype=dtype, fwd=fwd, dgrad=dgrad, wgrad=wgrad, note=note)


# geom = (C, k, stride, H, W)
CASES = [
    # ---- bf16
    C_("bf16_3x3s1_q16", (16, 3, 1, 16, 16), BF, STRIP(3, 1, 8), STRIP(3, 1, 8, True), WSTRIP(3, 1, 8), "Q = W = 16: TS 8"),
    C_("bf16_3x3s1_q15", (72, 3, 1, 15, 15), BF, STRIP(3, 1, 5), STRIP(3, 1, 5, True), WSTRIP(3, 1, 5), "Q = W = 15: TS 5; 36 channel pairs"),
    C_("bf16_5x5s1_q16", (48, 5, 1, 9, 16), BF, STRIP(5, 1, 8), STRIP(5, 1, 8, True), WSTRIP(5, 1, 8), "H != W"),
    C_("bf16_5x5s1_q15", (264, 5, 1, 7, 15), BF, STRIP(5, 1, 5), STRIP(5, 1, 5, True), WSTRIP(5, 1, 5), "132 pairs: several channel chunks"),
    C_("bf16_3x3s2_c288", (288, 3, 2, 21, 21), BF, STRIP(3, 2, 4), S2(BF, 3), WSTRIP(3, 2, 4), "Q = 11: TS 4 (12 < 15); several pixel blocks"),
    C_("bf16_3x3s2_c264_q10", (264, 3, 2, 9, 19), BF, STRIP(3, 2, 5), S2(BF, 3), WSTRIP(3, 2, 5), "Q = 10: TS 5; first C above the 144 exception"),
    C_("bf16_3x3s2_c144", (144, 3, 2, 16, 16), BF, STRIP(3, 2, 4), S2(BF, 3), WSTRIP(3, 2, 4), "C <= 144: still strips in production"),
    C_("bf16_3x3s2_c8", (8, 3, 2, 7, 5), BF, STRIP(3, 2, 4), S2(BF, 3), WSTRIP(3, 2, 4), "4 channel pairs, odd sizes, Q = 3"),
    C_("bf16_5x5s2_q10", (48, 5, 2, 19, 19), BF, STRIP(5, 2, 5), S2(BF, 5), WSTRIP(5, 2, 5), "no C exception for 5x5"),
    C_("bf16_5x5s2_q8", (8, 5, 2, 15, 16), BF, STRIP(5, 2, 4), S2(BF, 5), WSTRIP(5, 2, 4), "4 channel pairs: cpt below a wave"),
    C_("bf16_7x7s1", (16, 7, 1, 9, 9), BF, EL("fwd", BF), EL("dgrad", BF), EL("wgrad", BF), "49 taps: six tap groups in the weight gradient"),
    C_("bf16_7x7s2", (72, 7, 2, 13, 11), BF, EL("fwd", BF), EL("dgrad", BF), EL("wgrad", BF), "9 channel groups: statistics granule 9"),
    # ---- f32
    C_("f32_3x3s1_c16", (16, 3, 1, 16, 15), F32, TILE(F32, 3, 1), TILE(F32, 3, 1, True), EL("wgrad", F32), "C <= 48: mirrored tile; odd Q"),
    C_("f32_3x3s1_c48", (48, 3, 1, 11, 21), F32, TILE(F32, 3, 1), TILE(F32, 3, 1, True), EL("wgrad", F32), "C = 48: last mirrored tile"),
    C_("f32_3x3s1_c72", (72, 3, 1, 15, 14), F32, TILE(F32, 3, 1), EL("dgrad", F32), EL("wgrad", F32), "C > 48: element data gradient"),
    C_("f32_3x3s2_c288", (288, 3, 2, 21, 20), F32, TILE(F32, 3, 2), S2(F32, 3), EL("wgrad", F32), "C >= 288: stride-2 forward on tile; 36 channel groups: 2 chunks"),
    C_("f32_3x3s2_c264", (264, 3, 2, 10, 11), F32, EL("fwd", F32), S2(F32, 3), EL("wgrad", F32), "C < 288: element forward; 33 channel groups"),
    C_("f32_5x5s1_c48", (48, 5, 1, 9, 9), F32, EL("fwd", F32), TILE(F32, 5, 1, True), EL("wgrad", F32), "5x5 mirrored tile"),
    C_("f32_5x5s1_c264", (264, 5, 1, 8, 7), F32, EL("fwd", F32), EL("dgrad", F32), EL("wgrad", F32), "C < 288"),
    C_("f32_5x5s1_c288", (288, 5, 1, 6, 7), F32, EL("fwd", F32), EL("dgrad", F32), EL("wgrad", F32), "5x5 forwards are element whatever C"),
    C_("f32_5x5s2_c16", (16, 5, 2, 19, 18), F32, EL("fwd", F32), S2(F32, 5), EL("wgrad", F32), "5x5 2 x 2 blocks"),
    C_("f32_7x7s1", (8, 7, 1, 9, 10), F32, EL("fwd", F32), EL("dgrad", F32), EL("wgrad", F32), ""),
]
IDS = [c["id"] for c in CASES]


def draw(case):
    """Integer operands of a row, NCHW fp32 on the CPU: x and dy in {-3..3} ({-2..2} for 7x7), filter taps in {-2..2}; every product sum
    then stays below 256 in magnitude (exact in bf16) and every weight-gradient / statistics sum below 2^24 (exact in fp32)."""
    import torch
    C, k, s, H, W = case["geom"]
    gen = torch.Generator().manual_seed(1000 + IDS.index(case["id"]))
    a = 2 if k == 7 else 3
    x = torch.randint(-a, a + 1, (N, C, H, W), generator=gen).float()
    w = torch.randint(-2, 3, (C, 1, k, k), generator=gen).float()
    dy = torch.randint(-a, a + 1, (N, C, out_size(H, k, s), out_size(W, k, s)), generator=gen).float()
    return x, w, dy


_REF = {}


def reference(case):
    """(x, w, dy, y, dx, dw) of a row: torch's CPU fp32 convolution and its gradients; computed once per row and shared (do not modify)"""
    if case["id"] not in _REF:
        import torch
        import torch.nn.functional as F
        C, k, s, H, W = case["geom"]
        x, w, dy = draw(case)
        pad = (k - 1) // 2
        y = F.conv2d(x, w, None, s, pad, 1, C)
        dx = torch.nn.grad.conv2d_input(x.shape, w, dy, s, pad, 1, C)
        dw = torch.nn.grad.conv2d_weight(x, w.shape, dy, s, pad, 1, C)
        assert float(y.abs().max()) < 256 and float(dx.abs().max()) < 256, case["id"]
        assert float(dw.abs().max()) < 2 ** 24 and float((y.double() ** 2).sum(dim=(0, 2, 3)).max()) < 2 ** 24, case["id"]
        _REF[case["id"]] = (x, w, dy, y, dx, dw)
    return _REF[case["id"]]
