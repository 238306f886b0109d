"""The case table of tests/test_igemm_exact_gpu.py and the ledger of first-generation kernel instantiations (pure data: imported by
the GPU test and by the host tests of tests/test_conv_ref_host.py).

Every case names the kernel instantiation it must reach, as `cs_last_conv_variant()` reports it after the launch (note_variant in
csrc/conv_igemm.hip).  The strings are written BY HAND from the dispatcher's rules, restated here so a reader can check a row:

  chunk          ce = 8 elements (bf16) / 4 (f32); stored channels Cp, Kp = channels rounded up to 8; SCc = source channels / ce
  forward        M = N*P*Q, NOUT = Kp, source channels Cp;   data gradient: M = N*H*W, NOUT = Cp, source channels Kp
  tile           NOUT > 64 and 5 * ceil64(NOUT) > 4 * ceil128(NOUT)  (65..128, 193..256, ...):  BN = 128, and BM = 128 from
                 ceil(M/128) * ceil(NOUT/128) >= 1536 workgroups, else 64;   otherwise BN = 64, BM = 128 from ceil(M/128) >= 1536
                 grouped: BN = 64, BM = 128 from ceil(M/128) >= 384
  MODE           0: 1x1, stride 1, pad 0, ungrouped;  2: more than 64 taps (9x9), forward or data gradient of any stride;  else 1
  K-steps        nk = ceil(taps * SCc / 8)
  PF             bf16, nk > 1, a residual / add / mask operand, identity row -> pixel mapping (not a strided data gradient)
  UNI            MODE 0: always;  MODE 1: SCc % 8 == 0 and taps <= 32;  MODE 2: never
  stride-2 dgrad one merged launch over the parity classes: MODE 1, PF false, UNI = SCc % 8 == 0, tile from the LARGEST class
  stride-3 dgrad one launch per class (py, px); the variant is that of the LAST class (2, 2): MODE 1, PF false, its own taps
  statistics     rows = ceil(M / BM): fp64 atomics from the epilogue up to 512 rows, partial rows + fold above
  column sums    rows as above (summed over the classes of a merged launch); the fold has two phases from 128 rows
  weight grad    BM = 128 for K > 64 (ungrouped) else 64, BN = 128.  f32 and use_tr_read = 0: wgrad_kernel<T,BM,128,false>.
                 bf16 transposing reads: grouped -> wgrad_kernel<bf16,64,128,true>; else PLAIN = 1x1 / stride 1 / pad 0, and
                 wgrad_spec_kernel<BM,4,PLAIN,32> when deep (BM = 128, Kp >= 256, taps * Cp >= 256) or stem-like (not PLAIN,
                 Cp <= 8), else wgrad_dma_kernel<BM,3,PLAIN,32>; not PLAIN with an output of one row or one column (P = 1 or Q = 1):
                 wgrad_kernel<bf16,BM,128,true> (the DMA kernels' pixel walk has no 32-bit magic divisor for 1)

In the A/B flavour's children (test_wave_specialised_weight_gradient_on_every_shape) the expected string follows from the production
one by `ab_variant`: the register-staged path turns igemm_dma_kernel<T,BM,BN,MODE,..> into igemm_kernel<T,BM,BN,MODE> (a stride-2
data gradient is then un-merged and reports its last class (1, 1); a row whose tile differs there carries an `ab_reg` override),
CELLSEG_WGRAD_SPEC = 1 turns every wgrad_dma_kernel into wgrad_spec_kernel and = 2 the reverse."""
import re

BF, F32 = "bf16", "f32"


def D(t, bm, bn, mode, pf, uni):
    return f"igemm_dma_kernel<{t},{bm},{bn},{mode},{'true' if pf else 'false'},{'true' if uni else 'false'}>"


def REG(t, bm, bn, mode):
    return f"igemm_kernel<{t},{bm},{bn},{mode}>"


def WG(t, bm, tr):
    return f"wgrad_kernel<{t},{bm},128,{'true' if tr else 'false'}>"


def WDMA(bm, plain):
    return f"wgrad_dma_kernel<{bm},3,{'true' if plain else 'false'},32>"


def WSPEC(bm, plain):
    return f"wgrad_spec_kernel<{bm},4,{'true' if plain else 'false'},32>"


def ab_variant(variant, igemm_path=0, wgrad_spec=0, ab_reg=None):
    """the string the same case reports in the A/B flavour with cs_set_igemm_path(igemm_path) and CELLSEG_WGRAD_SPEC=wgrad_spec"""
    m = re.fullmatch(r"igemm_dma_kernel<(\w+),(\d+),(\d+),(\d),\w+,\w+>", variant)
    if m and igemm_path == 1:
        return ab_reg or f"igemm_kernel<{m.group(1)},{m.group(2)},{m.group(3)},{m.group(4)}>"
    if wgrad_spec == 1:
        return variant.replace("wgrad_dma_kernel<64,3,", "wgrad_spec_kernel<64,4,").replace("wgrad_dma_kernel<128,3,", "wgrad_spec_kernel<128,4,")
    if wgrad_spec == 2:
        return variant.replace("wgrad_spec_kernel<64,4,", "wgrad_dma_kernel<64,3,").replace("wgrad_spec_kernel<128,4,", "wgrad_dma_kernel<128,3,")
    return variant


# Operations (the `op` column); flags after '+':
#   fwd            plain forward                       fwd+fused  scale in {1, 2}, shift, residual, ReLU
#   fwd+bits       shift, residual, ReLU + sign bits   fwd+stats  plain forward + per-channel sum / sum of squares
#   dgrad          plain;  +add  +mask (16-bit mask tensor)  +bits (mask bit plane)  +colsum (immediate)  +defer (partial rows, folded
#                  by cs_fold_partial_rows through kernels.PartialColsum.vector)
#   wgrad+tr / wgrad   cs_conv2d_wgrad with / without transposing reads;   wgradN+tr  cs_conv2d_wgrad_batched with N items
#   stem_fwd, stem_fwd+stats, stem_wgrad+tr, stem_wgrad   the pixel-paired 7x7 stem (geometry column: the 7x7 / stride 2 / pad 3 layer)
# `note`: what the row is there for; `rows`: partial rows / statistics rows the launch must produce (checked against M and the tile).
def C(id, geom, dtype, op, variant, note="", rows=None, ab_reg=None):
    return dict(id=id, geom=geom, dtype=dtype, op=op, variant=variant, note=note, rows=rows, ab_reg=ab_reg)


BIG = (31, 80, 80)          # 198400 = 1550 * 128 pixels: an exact multiple of the 128-row tile, >= 1536 tiles
BIGT = (31, 80, 81)         # 200880 = 1569 * 128 + 48: a tail tile
BIG1 = (1, 49, 4049)        # 198401 = 1550 * 128 + 1
WIDE1 = (1, 5, 19661)       # 98305 = 768 * 128 + 1: 769 M tiles x 2 N tiles of 128 = 1538 workgroups

#        id                    N   H   W  Cin Cout R  s  p  g
CASES = [
    # ------------------------------------------------------------------ bf16, tile 128 x 128
    C("b128x128-m0",          (16, 80, 80, 8, 256, 1, 1, 0, 1), BF, "fwd", D(BF, 128, 128, 0, 0, 1), "800 x 2 workgroups, one K-step, single LDS stage"),
    C("b128x128-m0-pf",       WIDE1 + (128, 256, 1, 1, 0, 1), BF, "fwd+fused", D(BF, 128, 128, 0, 1, 1), "M = k*128 + 1, two K-steps"),
    C("b128x128-m1",          BIGT + (72, 8, 3, 1, 1, 1), BF, "dgrad", D(BF, 128, 128, 1, 0, 0), "NOUT 72 (65..127), SCc = 1"),
    C("b128x128-m1-uni",      BIG + (64, 72, 3, 1, 1, 1), BF, "fwd", D(BF, 128, 128, 1, 0, 1)),
    C("b128x128-m1-pf",       BIGT + (8, 72, 3, 1, 1, 1), BF, "fwd+fused", D(BF, 128, 128, 1, 1, 0)),
    C("b128x128-m1-pf-uni",   BIG + (64, 72, 3, 1, 1, 1), BF, "fwd+fused", D(BF, 128, 128, 1, 1, 1)),
    C("b128x128-m2",          BIGT + (72, 8, 9, 2, 4, 1), BF, "dgrad+add+mask", D(BF, 128, 128, 2, 0, 0), "9x9 stride-2 data gradient: 81 taps, not split into classes"),
    # ------------------------------------------------------------------ bf16, tile 128 x 64
    C("b128x64-m0",           BIG1 + (8, 8, 1, 1, 0, 1), BF, "fwd+stats", D(BF, 128, 64, 0, 0, 1), "M = k*128 + 1; Cout 8; statistics on the slab path", rows=1551),
    C("b128x64-m0-pf",        BIG + (8, 128, 1, 1, 0, 1), BF, "dgrad+add", D(BF, 128, 64, 0, 1, 1)),
    C("b128x64-m1",           (32, 80, 80, 16, 64, 3, 1, 1, 1), BF, "fwd", D(BF, 128, 64, 1, 0, 0), "1600 tiles"),
    C("b128x64-m1-uni",       BIGT + (8, 64, 3, 1, 1, 1), BF, "dgrad+colsum", D(BF, 128, 64, 1, 0, 1), "two-phase fold of 1570 rows", rows=1570),
    C("b128x64-m1-pf",        BIGT + (32, 16, 3, 1, 1, 1), BF, "dgrad+add+bits+defer", D(BF, 128, 64, 1, 1, 0), rows=1570),
    C("b128x64-m1-pf-uni",    BIG + (64, 8, 3, 1, 1, 1), BF, "fwd+fused", D(BF, 128, 64, 1, 1, 1)),
    C("b128x64-m2",           BIG + (8, 8, 9, 1, 4, 1), BF, "fwd", D(BF, 128, 64, 2, 0, 0), "9x9 forward"),
    # ------------------------------------------------------------------ bf16, tile 64 x 128
    C("b64x128-m0",           (2, 19, 19, 24, 72, 1, 1, 0, 1), BF, "fwd", D(BF, 64, 128, 0, 0, 1), "SCc = 3: dead lanes of the only K-step"),
    C("b64x128-m0-pf",        (2, 19, 19, 72, 128, 1, 1, 0, 1), BF, "dgrad+add+mask+colsum", D(BF, 64, 128, 0, 1, 1), rows=12),
    C("b64x128-m0-224",       (1, 8, 16, 64, 224, 1, 1, 0, 1), BF, "fwd+bits", D(BF, 64, 128, 0, 0, 1), "Cout 224 (193..256): wide tiles; M = 128 exactly; one K-step"),
    C("b64x128-m1",           (2, 13, 13, 24, 100, 3, 1, 1, 1), BF, "fwd", D(BF, 64, 128, 1, 0, 0), "Kp = 104"),
    C("b64x128-m1-7x7",       (2, 13, 13, 64, 72, 7, 1, 3, 1), BF, "fwd", D(BF, 64, 128, 1, 0, 0), "49 taps > 32: lane-by-lane walk although SCc = 8; 64-bit tap mask"),
    C("b64x128-m1-uni",       (2, 19, 19, 128, 64, 3, 1, 1, 1), BF, "dgrad", D(BF, 64, 128, 1, 0, 1)),
    C("b64x128-m1-pf",        (2, 19, 19, 96, 24, 3, 1, 1, 1), BF, "dgrad+add+bits+defer", D(BF, 64, 128, 1, 1, 0), "one-phase fold", rows=12),
    C("b64x128-m1-pf-uni",    (2, 19, 19, 64, 128, 3, 1, 1, 1), BF, "fwd+bits", D(BF, 64, 128, 1, 1, 1)),
    C("b64x128-m2",           (2, 13, 13, 72, 8, 9, 2, 4, 1), BF, "dgrad", D(BF, 64, 128, 2, 0, 0)),
    # ------------------------------------------------------------------ bf16, tile 64 x 64
    C("b64x64-m0-M1",         (1, 1, 1, 8, 8, 1, 1, 0, 1), BF, "fwd", D(BF, 64, 64, 0, 0, 1), "a single pixel"),
    C("b64x64-m0-pf",         (1, 8, 8, 136, 40, 1, 1, 0, 1), BF, "fwd+fused", D(BF, 64, 64, 0, 1, 1), "M = 64 exactly; SCc = 17: three K-steps, tail"),
    C("b64x64-m0-136",        (2, 19, 19, 64, 136, 1, 1, 0, 1), BF, "fwd", D(BF, 64, 64, 0, 0, 1), "Cout 136 (129..191): three 64-wide N tiles"),
    C("b64x64-m1",            (2, 13, 13, 24, 40, 3, 1, 1, 1), BF, "fwd", D(BF, 64, 64, 1, 0, 0)),
    C("b64x64-m1-uni",        (1, 5, 13, 64, 64, 3, 1, 1, 1), BF, "fwd", D(BF, 64, 64, 1, 0, 1), "M = 65 = 64 + 1"),
    C("b64x64-m1-pf",         (2, 11, 11, 40, 24, 5, 2, 2, 1), BF, "fwd+fused", D(BF, 64, 64, 1, 1, 0), "5x5 stride 2"),
    C("b64x64-m1-pf-uni",     (2, 19, 19, 64, 64, 3, 1, 1, 1), BF, "dgrad+add+mask+colsum", D(BF, 64, 64, 1, 1, 1), rows=12),
    C("b64x64-m1-s3",         (2, 19, 19, 64, 20, 3, 3, 1, 1), BF, "fwd+fused", D(BF, 64, 64, 1, 1, 1), "stride-3 forward; Cout 20 -> 24 stored, the padding exactly zero"),
    C("b64x64-m2",            (2, 13, 13, 8, 16, 9, 1, 4, 1), BF, "fwd", D(BF, 64, 64, 2, 0, 0)),
    C("b64x64-cin3",          (2, 13, 13, 3, 64, 3, 1, 1, 1), BF, "dgrad+add+mask", D(BF, 64, 64, 1, 1, 1), "Cin 3 -> 8 stored channels: the data gradient's padding is exactly zero"),
    C("b64x64-cin20",         (2, 13, 13, 20, 12, 3, 1, 1, 1), BF, "dgrad", D(BF, 64, 64, 1, 0, 0), "Cin 20 -> 24, Cout 12 -> 16 stored"),
    C("b64x64-cin3-fwd",      (2, 37, 37, 3, 64, 7, 2, 3, 1), BF, "fwd+fused", D(BF, 64, 64, 1, 1, 0), "the generic 7x7 stem"),
    # ------------------------------------------------------------------ f32, tile 128 x 128
    C("f128x128-m0",          (16, 80, 80, 8, 256, 1, 1, 0, 1), F32, "fwd", D(F32, 128, 128, 0, 0, 1)),
    C("f128x128-m1",          BIGT + (72, 8, 3, 1, 1, 1), F32, "dgrad+add+mask+colsum", D(F32, 128, 128, 1, 0, 0), rows=1570),
    C("f128x128-m1-uni",      BIG + (32, 72, 3, 1, 1, 1), F32, "fwd+fused", D(F32, 128, 128, 1, 0, 1)),
    C("f128x128-m2",          BIGT + (72, 8, 9, 2, 4, 1), F32, "dgrad", D(F32, 128, 128, 2, 0, 0)),
    # ------------------------------------------------------------------ f32, tile 128 x 64
    C("f128x64-m0",           BIG1 + (8, 8, 1, 1, 0, 1), F32, "dgrad", D(F32, 128, 64, 0, 0, 1)),
    C("f128x64-m1",           (32, 80, 80, 16, 64, 3, 1, 1, 1), F32, "fwd", D(F32, 128, 64, 1, 0, 0)),
    C("f128x64-m1-uni",       BIGT + (8, 32, 3, 1, 1, 1), F32, "dgrad+add+mask", D(F32, 128, 64, 1, 0, 1)),
    C("f128x64-m2",           BIG + (8, 8, 9, 1, 4, 1), F32, "fwd+stats", D(F32, 128, 64, 2, 0, 0), rows=1550),
    # ------------------------------------------------------------------ f32, tile 64 x 128
    C("f64x128-m0",           (2, 19, 19, 24, 72, 1, 1, 0, 1), F32, "fwd+fused", D(F32, 64, 128, 0, 0, 1)),
    C("f64x128-m1",           (2, 13, 13, 100, 24, 3, 1, 1, 1), F32, "dgrad", D(F32, 64, 128, 1, 0, 0)),
    C("f64x128-m1-uni",       (2, 19, 19, 32, 128, 3, 1, 1, 1), F32, "fwd+bits", D(F32, 64, 128, 1, 0, 1)),
    C("f64x128-m2",           (2, 13, 13, 72, 8, 9, 2, 4, 1), F32, "dgrad+add", D(F32, 64, 128, 2, 0, 0)),
    # ------------------------------------------------------------------ f32, tile 64 x 64
    C("f64x64-m0-M1",         (1, 1, 1, 8, 16, 1, 1, 0, 1), F32, "dgrad+add", D(F32, 64, 64, 0, 0, 1), "a single pixel"),
    C("f64x64-m1",            (2, 13, 13, 3, 20, 3, 1, 1, 1), F32, "fwd+fused", D(F32, 64, 64, 1, 0, 0), "Cin 3, Cout 20"),
    C("f64x64-m1-uni",        (2, 13, 13, 40, 32, 3, 1, 1, 1), F32, "dgrad+add+mask+defer", D(F32, 64, 64, 1, 0, 1), rows=6),
    C("f64x64-m2",            (2, 13, 13, 8, 16, 9, 1, 4, 1), F32, "fwd", D(F32, 64, 64, 2, 0, 0)),
    # ------------------------------------------------------------------ statistics: atomic / slab, the 512 | 513 boundary
    C("stats-atomic-12",      (2, 19, 19, 64, 128, 1, 1, 0, 1), BF, "fwd+stats", D(BF, 64, 128, 0, 0, 1), rows=12),
    C("stats-atomic-512",     (8, 64, 64, 8, 16, 1, 1, 0, 1), BF, "fwd+stats", D(BF, 64, 64, 0, 0, 1), "rows = 512: the last atomic launch", rows=512),
    C("stats-slab-513",       (1, 1, 32769, 8, 16, 1, 1, 0, 1), BF, "fwd+stats", D(BF, 64, 64, 0, 0, 1), "rows = 513: the first slab launch", rows=513),
    C("stats-slab-3x3",       (9, 64, 64, 16, 40, 3, 1, 1, 1), BF, "fwd+stats", D(BF, 64, 64, 1, 0, 0), rows=576),
    C("stats-atomic-f32",     (3, 21, 17, 32, 64, 3, 1, 1, 1), F32, "fwd+stats", D(F32, 64, 64, 1, 0, 1), rows=17),
    # ------------------------------------------------------------------ deferred column sums, one- and two-phase fold
    C("defer-12-rows",        (2, 19, 19, 64, 64, 1, 1, 0, 1), BF, "dgrad+defer", D(BF, 64, 64, 0, 0, 1), rows=12),
    C("defer-127-rows",       (1, 64, 127, 8, 8, 3, 1, 1, 1), BF, "dgrad+add+defer", D(BF, 64, 64, 1, 1, 0), "the last one-phase fold", rows=127),
    C("defer-128-rows",       (2, 64, 64, 8, 8, 3, 1, 1, 1), BF, "dgrad+add+defer", D(BF, 64, 64, 1, 1, 0), "the first two-phase fold", rows=128),
    C("defer-512-rows",       (8, 64, 64, 16, 24, 1, 1, 0, 1), BF, "dgrad+defer", D(BF, 64, 64, 0, 0, 1), rows=512),
    # ------------------------------------------------------------------ grouped (slab-dense)
    C("grouped-fwd",          (2, 19, 19, 128, 128, 3, 1, 1, 32), BF, "fwd+fused", D(BF, 64, 64, 1, 1, 1)),
    C("grouped-fwd-s2",       (2, 19, 19, 128, 128, 3, 2, 1, 32), BF, "fwd", D(BF, 64, 64, 1, 0, 1)),
    C("grouped-fwd-f32",      (1, 10, 10, 256, 256, 3, 1, 1, 32), F32, "fwd", D(F32, 64, 64, 1, 0, 1)),
    C("grouped-fwd-128",      (8, 80, 80, 64, 64, 3, 1, 1, 16), BF, "fwd", D(BF, 128, 64, 1, 0, 1), "400 tiles of 128 rows >= 384"),
    C("grouped-dgrad",        (2, 19, 19, 128, 128, 3, 1, 1, 32), BF, "dgrad+add+mask+colsum", D(BF, 64, 64, 1, 1, 1), rows=12),
    C("grouped-dgrad-f32",    (1, 9, 9, 256, 256, 3, 1, 1, 8), F32, "dgrad", D(F32, 64, 64, 1, 0, 1)),
    C("grouped-dgrad-s2",     (2, 19, 19, 128, 128, 3, 2, 1, 32), BF, "dgrad+add", D(BF, 64, 64, 1, 0, 1), "grouped stride 2: one launch per class, never merged"),
    # ------------------------------------------------------------------ stride-2 data gradient: ONE launch over the parity classes
    C("s2-1x1-tapless",       (2, 7, 8, 8, 16, 1, 2, 0, 1), BF, "dgrad", D(BF, 64, 64, 1, 0, 0), "three classes without taps must store zeros"),
    C("s2-1x1-tapless-fused", (2, 8, 7, 32, 64, 1, 2, 0, 1), BF, "dgrad+add+bits+colsum", D(BF, 64, 64, 1, 0, 1), "tap-less classes still add / mask / sum", rows=4),
    C("s2-1x1-tapless-f32",   (2, 9, 9, 8, 32, 1, 2, 0, 1), F32, "dgrad+add+mask", D(F32, 64, 64, 1, 0, 1)),
    C("s2-3x3-p1-odd-even",   (2, 9, 10, 40, 24, 3, 2, 1, 1), BF, "dgrad", D(BF, 64, 64, 1, 0, 0)),
    C("s2-3x3-p0-even-odd",   (2, 10, 9, 96, 64, 3, 2, 0, 1), BF, "dgrad+add+bits+defer", D(BF, 64, 128, 1, 0, 1), "pad 0", rows=4),
    C("s2-3x3-p2-dh1",        (3, 2, 3, 8, 8, 3, 2, 2, 1), BF, "dgrad+add+mask+colsum", D(BF, 64, 64, 1, 0, 0), "H = 2, W = 3: classes of one row / one column", rows=4),
    C("s2-3x3-W1",            (3, 5, 1, 8, 8, 3, 2, 1, 1), BF, "dgrad+defer", D(BF, 64, 64, 1, 0, 0), "W = 1: the px = 1 classes do not exist", rows=2),
    C("s2-5x5-p2",            (2, 11, 11, 40, 24, 5, 2, 2, 1), BF, "dgrad+add+mask+colsum", D(BF, 64, 64, 1, 0, 0), rows=4),
    C("s2-5x5-p4-H1",         (3, 1, 6, 8, 64, 5, 2, 4, 1), BF, "dgrad+defer", D(BF, 64, 64, 1, 0, 1), "H = 1: the py = 1 classes do not exist; pad R-1", rows=2),
    C("s2-5x5-p0",            (2, 12, 7, 16, 8, 5, 2, 0, 1), BF, "dgrad+add", D(BF, 64, 64, 1, 0, 0)),
    C("s2-7x7-p3",            (2, 14, 9, 16, 8, 7, 2, 3, 1), BF, "dgrad", D(BF, 64, 64, 1, 0, 0)),
    C("s2-7x7-p0",            (2, 9, 12, 8, 64, 7, 2, 0, 1), BF, "dgrad+add+mask", D(BF, 64, 64, 1, 0, 1)),
    C("s2-7x7-p6",            (2, 5, 4, 8, 8, 7, 2, 6, 1), BF, "dgrad+colsum", D(BF, 64, 64, 1, 0, 0), rows=4),
    C("s2-4x4-p1",            (2, 8, 9, 8, 16, 4, 2, 1, 1), BF, "dgrad+add", D(BF, 64, 64, 1, 0, 0), "even filter: every class has 2 x 2 taps"),
    C("s2-2x2-p0",            (2, 6, 5, 8, 8, 2, 2, 0, 1), BF, "dgrad", D(BF, 64, 64, 1, 0, 0), "even filter, one tap per class"),
    C("s2-3x3-f32",           (2, 9, 8, 8, 8, 3, 2, 1, 1), F32, "dgrad+add+mask+colsum", D(F32, 64, 64, 1, 0, 0), rows=4),
    C("s2-3x3-f32-uni",       (2, 10, 11, 72, 32, 3, 2, 1, 1), F32, "dgrad+defer", D(F32, 64, 128, 1, 0, 1), rows=4),
    C("s2-3x3-128x64",        (31, 160, 161, 8, 8, 3, 2, 1, 1), BF, "dgrad+add+mask+colsum", D(BF, 128, 64, 1, 0, 0),
      "classes of 1570 + 1550 + 1570 + 1550 tiles of 128 rows", rows=6240),
    C("s2-3x3-128x128",       (31, 160, 160, 72, 64, 3, 2, 1, 1), BF, "dgrad+defer", D(BF, 128, 128, 1, 0, 1), rows=6200),
    C("s2-3x3-128x64-f32",    (31, 160, 160, 8, 32, 3, 2, 1, 1), F32, "dgrad", D(F32, 128, 64, 1, 0, 1)),
    # ------------------------------------------------------------------ stride-3 data gradient: one launch per class
    C("s3-3x3",               (2, 10, 11, 24, 16, 3, 3, 1, 1), BF, "dgrad+add+mask+colsum", D(BF, 64, 64, 1, 0, 0), "class (2, 2): one tap"),
    C("s3-5x5-uni",           (2, 11, 10, 8, 64, 5, 3, 2, 1), BF, "dgrad+add", D(BF, 64, 64, 1, 0, 1), "class (2, 2): 2 x 2 taps, SCc = 8"),
    C("s3-1x1-tapless-f32",   (2, 7, 7, 8, 8, 1, 3, 0, 1), F32, "dgrad+add+mask", D(F32, 64, 64, 1, 0, 0), "eight classes without taps"),
    # ------------------------------------------------------------------ weight gradient
    C("wg-3x3-dma64",         (2, 13, 13, 24, 40, 3, 1, 1, 1), BF, "wgrad+tr", WDMA(64, 0), "338 pixels, not a multiple of the slice"),
    C("wg-3x3-one-row-reg128", (3, 1, 13, 24, 72, 3, 1, 1, 1), BF, "wgrad+tr", WG(BF, 128, 1), "P = 1: no 32-bit magic divisor for the DMA pixel walk: register-staged"),
    C("wg-3x3-one-col-reg64", (3, 13, 1, 24, 40, 3, 1, 1, 1), BF, "wgrad+tr", WG(BF, 64, 1), "Q = 1: the same, BM = 64"),
    C("wg-3x3-reg64",         (2, 13, 13, 24, 40, 3, 1, 1, 1), BF, "wgrad", WG(BF, 64, 0)),
    C("wg-1x1-dma128",        (2, 19, 19, 64, 128, 1, 1, 0, 1), BF, "wgrad+tr", WDMA(128, 1), "K > 64"),
    C("wg-1x1-reg128",        (2, 19, 19, 64, 128, 1, 1, 0, 1), BF, "wgrad", WG(BF, 128, 0)),
    C("wg-1x1-dma64-even",    (2, 32, 32, 8, 16, 1, 1, 0, 1), BF, "wgrad+tr", WDMA(64, 1), "2048 pixels = 32 slices of 64: no tail"),
    C("wg-1x1-one-split",     (2, 5, 5, 8, 8, 1, 1, 0, 1), BF, "wgrad+tr", WDMA(64, 1), "50 pixels: one slice, two K-steps, tail"),
    C("wg-3x3-s2-dma128",     (2, 19, 19, 64, 128, 3, 2, 1, 1), BF, "wgrad+tr", WDMA(128, 0)),
    C("wg-5x5-s2-dma64",      (2, 11, 11, 40, 24, 5, 2, 2, 1), BF, "wgrad+tr", WDMA(64, 0)),
    C("wg-deep-plain",        (1, 10, 10, 256, 256, 1, 1, 0, 1), BF, "wgrad+tr", WSPEC(128, 1), "deep: K, Cin >= 256"),
    C("wg-deep-3x3",          (1, 9, 9, 32, 264, 3, 2, 1, 1), BF, "wgrad+tr", WSPEC(128, 0), "deep: K 264 (three 128-row tiles, the last 8 rows full), 9 * 32 = 288 columns"),
    C("wg-cin3-spec64",       (2, 13, 13, 3, 16, 3, 1, 1, 1), BF, "wgrad+tr", WSPEC(64, 0), "stem-like: 8 stored input channels"),
    C("wg-cin3-spec128",      (2, 13, 13, 3, 72, 3, 1, 1, 1), BF, "wgrad+tr", WSPEC(128, 0)),
    C("wg-3x3-f32-64",        (2, 13, 13, 24, 40, 3, 1, 1, 1), F32, "wgrad", WG(F32, 64, 0)),
    C("wg-1x1-f32-128",       (2, 19, 19, 64, 128, 1, 1, 0, 1), F32, "wgrad", WG(F32, 128, 0)),
    C("wg-3x3-s2-f32-128",    (2, 10, 9, 12, 72, 3, 2, 0, 1), F32, "wgrad", WG(F32, 128, 0)),
    C("wg-grouped-tr",        (2, 19, 19, 128, 128, 3, 1, 1, 32), BF, "wgrad+tr", WG(BF, 64, 1)),
    C("wg-grouped",           (2, 9, 9, 128, 128, 3, 2, 1, 32), BF, "wgrad", WG(BF, 64, 0)),
    C("wg-grouped-f32",       (1, 10, 10, 256, 256, 3, 1, 1, 8), F32, "wgrad", WG(F32, 64, 0)),
    C("wgb1-5x5-s2",          (2, 11, 11, 40, 24, 5, 2, 2, 1), BF, "wgrad1+tr", WDMA(64, 0), "stride 2: the second-generation kernel declines"),
    C("wgb3-3x3-c24",         (2, 13, 13, 24, 40, 3, 1, 1, 1), BF, "wgrad3+tr", WDMA(64, 0), "channels not multiples of 64: declined"),
    C("wgb8-1x1",             (2, 19, 19, 64, 128, 1, 1, 0, 1), BF, "wgrad8+tr", WDMA(128, 1), "1x1: declined"),
    C("wgb3-3x3-reg",         (2, 13, 13, 24, 40, 3, 1, 1, 1), BF, "wgrad3", WG(BF, 64, 0)),
    C("wgb3-1x1-f32",         (2, 9, 9, 16, 72, 1, 1, 0, 1), F32, "wgrad3", WG(F32, 128, 0)),
    # ------------------------------------------------------------------ the pixel-paired stem
    C("stem-fwd-odd",         (3, 37, 41, 3, 64, 7, 2, 3, 1), BF, "stem_fwd", D(BF, 64, 64, 1, 0, 0), "odd W: the last pixel pairs with a zero"),
    C("stem-fwd-even-stats",  (2, 32, 32, 3, 64, 7, 2, 3, 1), BF, "stem_fwd+stats", D(BF, 64, 64, 1, 0, 0), rows=8),
    C("stem-fwd-f32",         (2, 21, 18, 3, 64, 7, 2, 3, 1), F32, "stem_fwd", D(F32, 64, 64, 1, 0, 0)),
    C("stem-wgrad-odd",       (3, 37, 41, 3, 64, 7, 2, 3, 1), BF, "stem_wgrad+tr", WSPEC(64, 0)),
    C("stem-wgrad-even",      (2, 32, 32, 3, 64, 7, 2, 3, 1), BF, "stem_wgrad+tr", WSPEC(64, 0)),
    C("stem-wgrad-reg",       (2, 21, 18, 3, 64, 7, 2, 3, 1), BF, "stem_wgrad", WG(BF, 64, 0)),
    C("stem-wgrad-f32",       (2, 21, 18, 3, 64, 7, 2, 3, 1), F32, "stem_wgrad", WG(F32, 64, 0)),
]

# Shapes the data-gradient ABI refuses (check_geom / conv2d_dgrad_impl), hence absent from the table: none by channel count -- stored
# channels are always multiples of 8, which is a multiple of both chunks; `mask_bits` / sign bits need stored channels % 32 == 0, so the
# +bits rows use such widths.


# ------------------------------------------------------------------------------------------------ the ledger
_TILES = ((64, 64), (64, 128), (128, 64), (128, 128))
# launch_igemm<T, BM, BN>: the LDS-DMA instantiations (MODE, PF, UNI) per dtype ...
_DMA_BF16 = ((0, 0, 1), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1), (2, 0, 0))
_DMA_F32 = ((0, 0, 1), (1, 0, 0), (1, 0, 1), (2, 0, 0))
LEDGER = (
    [D(BF, bm, bn, m, pf, u) for bm, bn in _TILES for m, pf, u in _DMA_BF16] +
    [D(F32, bm, bn, m, pf, u) for bm, bn in _TILES for m, pf, u in _DMA_F32] +
    # ... their register-staged twins
    [REG(t, bm, bn, m) for t in (BF, F32) for bm, bn in _TILES for m in (0, 1, 2)] +
    # launch_wgrad<T, BM, 128, TR>
    [WG(F32, 64, 0), WG(F32, 128, 0), WG(BF, 64, 0), WG(BF, 128, 0), WG(BF, 64, 1), WG(BF, 128, 1),
     WDMA(64, 0), WDMA(64, 1), WDMA(128, 0), WDMA(128, 1), WSPEC(64, 0), WSPEC(64, 1), WSPEC(128, 0), WSPEC(128, 1)]
)
# (the merged stride-2 branch of launch_igemm names <T,BM,BN,1,false,UNI>: already in the list)

GIB2 = "needs an operand of 2 GiB or more"
NO_ENTRY = "no public entry point can produce these parameters"
# What the production-flavour table does not reach, and why.  AB_COLUMN: reached by the A/B children instead (ab_variant).
EXCLUSIONS = {
    **{REG(t, bm, bn, m): (GIB2, "the register-staged twin runs when src or weights reach 2^31 bytes; cs_set_igemm_path(1) forces it")
       for t in (BF, F32) for bm, bn in _TILES for m in (0, 1, 2)},
    WSPEC(64, 1): (NO_ENTRY, "PLAIN with BM = 64 is neither deep (BM = 128) nor stem-like (not PLAIN): only CELLSEG_WGRAD_SPEC = 1 selects it"),
}
AB_COLUMN_MISSING = set()                     # excluded in both flavours: nothing
