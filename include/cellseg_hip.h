/* cellseg_hip.h -- C ABI of libcellseg_hip.so, the MI355X (gfx950) kernel library behind the
 * per-tile CNN hot path of Newiz430/CellSegmentation.
 *
 * The reference has no FFI: its hot path is Python calling torch.nn modules (model/resnet.py,
 * model/resnext.py, model/efficientnet.py, train/train.py, train/losses.py, metrics/metrics.py,
 * inference.py).  Each entry point below replaces the ATen op(s) that a cited reference line
 * dispatches; the Python host mirror in cellsegmentation_amd/ binds them with ctypes
 * (see INTEGRATION.md for the stub a reference maintainer would add).
 *
 * Conventions
 *  - plain pointers + sizes only; every pointer is a DEVICE pointer unless named host_*;
 *  - activations are NHWC, dtype CS_F32 (parity mode, exact-f32 MFMA) or CS_BF16 (throughput
 *    mode, fp32 accumulate); channel counts are multiples of the 16-byte chunk
 *    (4 for CS_F32, 8 for CS_BF16); parameters/gradients/statistics are fp32 (torch layouts);
 *  - nothing allocates, frees or synchronises: work is enqueued on `stream` (a hipStream_t
 *    passed as void*); workspaces are caller-owned;
 *  - return value: CS_OK or a negative CS_ERR_*; cs_last_error() gives the message.
 */
#ifndef CELLSEG_HIP_H_
#define CELLSEG_HIP_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { CS_F32 = 0, CS_BF16 = 1 };
enum { CS_OK = 0, CS_ERR_INVALID_ARG = -1, CS_ERR_LAUNCH = -2, CS_ERR_UNSUPPORTED = -3 };
enum { CS_ACT_NONE = 0, CS_ACT_RELU = 1, CS_ACT_SILU = 2, CS_ACT_SIGMOID = 3 };

int cs_abi_version(void);
const char* cs_last_error(void);
/* Name of the convolution-family kernel instantiation the calling thread launched last, e.g. "igemm_dma_kernel<bf16,64,128,1,false,true>",
 * "conv2_halo_kernel<9,3,4,1,4,4>", "wgrad_dma_kernel<128,3,true,32>": the names rocprofv3 reports (template arguments without spaces),
 * so that bench.py's roofline entries can be checked against profiles/ (tools/check_bench_vs_profile.py). */
const char* cs_last_conv_variant(void);

/* Geometry of one 2-D convolution (torch.nn.Conv2d as used at model/resnet.py:20,23,51,53,55,
 * 111,183,198,164).  Input N x H x W x C (C = stored/padded channels), output N x P x Q x K. */
typedef struct CsConvGeom {
    int32_t N, H, W, C;
    int32_t K;
    int32_t R, S;       /* kernel height, width */
    int32_t stride, pad;
    int32_t P, Q;       /* output height, width */
    int32_t groups;     /* 0 or 1: dense; > 1: grouped convolution in slab-dense form (ResNeXt, see cs_weight_prep_grouped) */
} CsConvGeom;

/* ---- layout / precision changes at the module boundary ------------------------------------- */
/* x[N][C][H][W] fp32 (the reference's input layout, dataset/dataset.py:78-83 output) ->
 * y[N][H][W][Cp] dtype, channels C..Cp-1 zero-filled. */
int cs_nchw_to_nhwc(const float* x, void* y, int dtype, int N, int C, int H, int W, int Cp, void* stream);
/* y[N][H][W][Cp] dtype -> x[N][C][H][W] fp32 (first C channels).  Used for segmentation logits
 * (model/resnet.py:301-303) and to hand gradients back in torch layout. */
int cs_nhwc_to_nchw(const void* y, int dtype, float* x, int N, int C, int H, int W, int Cp, void* stream);

/* ---- BatchNorm2d in eval mode folded to per-channel scale/shift (resnet.py:254-258: the
 * freeze_bn path runs every BN with running statistics) --------------------------------------
 * scale = gamma*rsqrt(var+eps), shift = beta + (conv_bias - mean)*scale, rstd = rsqrt(var+eps);
 * conv_bias nullable (the biased 3x3 convs of upsample_conv, resnet.py:198). */
int cs_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps,
               const float* conv_bias, float* scale, float* shift, float* rstd, int C, void* stream);

/* ---- BatchNorm in train mode (batch statistics; model.train(), resnet.py:21,52,112,184,199 and the
 * BatchNorm1d of the image heads, resnet.py:134,138) over NHWC rows z[M][C] ----------------------
 * stats: the per-channel pair (sum, sum of squares) as an EXACT ACCUMULATOR (round 5, ABI 6): cs_bn_accum_words(C) = 6 C + 1
 * zero-initialised 8-byte words -- every contribution is split into three limbs (multiples of 2^0, 2^-40, 2^-80, each below 2^40 of
 * its unit) that are added with one fp64 atomic each: every partial sum of a limb stays exactly representable, so each addition is
 * exact and the totals do not depend on the order the workgroups arrive in (two runs of one step give the same bits; the reference's
 * CPU path is deterministic too) and no bit >= 2^-80 of a contribution is lost; the last word is a sticky
 * "a contribution was NaN / infinite / >= 2^40" flag that makes every total read as NaN.  The words are opaque: kernels of this
 * library produce (cs_bn_stats, cs_conv2d_fwd with `stats`, cs_bn_partial_fold, cs_bn_bwd_reduce) and consume (cs_bn_finalize,
 * cs_bn_apply_stats, cs_bn_bwd_apply) them; cs_bn_accum_read gives the two totals per channel as fp64 [2][C].  The parameters
 * keep their historical `double*` type. */
size_t cs_bn_accum_words(int C);
int cs_bn_accum_read(const double* accum, int C, double* out, void* stream);
int cs_bn_stats(const void* z, int dtype, long long M, int C, double* stats, double* workspace, void* stream);
/* `workspace` of cs_bn_stats / cs_bn_bwd_reduce (nullable, cs_bn_partial_workspace(M, C) bytes -- 0 where the launch has so few
 * row blocks and channels that it adds its sums straight into the accumulator and wants none): per-workgroup partial sums are
 * written there and folded by a second small launch instead of ~1000 atomics per channel (3x faster on large tensors). */
size_t cs_bn_partial_workspace(long long M, int C);
/* mean, rstd = 1/sqrt(biased var+eps); running_* (nullable) updated in place with `momentum` and the
 * unbiased variance, as nn.BatchNorm2d does. */
int cs_bn_finalize(const double* stats, long long M, float eps, float momentum, float* running_mean,
                   float* running_var, float* mean_out, float* rstd_out, int C, void* stream);
/* y = act( gamma*(z-mean)*rstd + beta + residual ); gamma/beta/residual nullable. */
int cs_bn_apply(const void* z, int dtype, const float* mean, const float* rstd, const float* gamma,
                const float* beta, const void* residual, int act, void* y, long long M, int C, void* stream);
/* cs_bn_finalize + cs_bn_apply in ONE launch (train-mode forward of nn.BatchNorm2d, model/resnet.py:150 / efficientnet.py:93 with
 * module.training): every thread derives mean and 1/sqrt(var + eps) of its channels from the accumulator `stats` (above) with the same
 * arithmetic as cs_bn_finalize (bit-identical results), workgroup 0 writes mean_out / rstd_out (kept for backward) and updates the
 * running statistics (nullable). */
int cs_bn_apply_stats(const void* z, int dtype, const double* stats, float eps, float momentum, float* running_mean,
                      float* running_var, const float* gamma, const float* beta, const void* residual, int act, void* y,
                      float* mean_out, float* rstd_out, long long M, int C, void* stream);
/* sums: an exact accumulator like `stats` above (cs_bn_accum_words(C) zeroed words): sum g, sum g*xhat with xhat=(z-mean)*rstd and g = dy, or for
 * act==CS_ACT_SILU g = dy*silu'(gamma*xhat+beta) (the activation that follows the BN; ReLU gradients are
 * already masked by the consumers, see engine.py). gamma/beta nullable (1/0).
 * Two flags may be OR-ed into `act` of cs_bn_bwd_reduce / cs_bn_bwd_apply (the BatchNorm1d layers of the image heads,
 * resnet.py:132-152, whose backward has no convolution epilogue to do the masking):
 *   CS_BN_BWD_OWN_RELU  g = dy * [gamma*xhat + beta > 0]: the ReLU that directly follows this normalisation;
 *   CS_BN_BWD_FROZEN    (apply) the statistics are running statistics (module.eval()): dz = gamma*rstd*g, no batch terms. */
#define CS_BN_BWD_OWN_RELU 0x100
#define CS_BN_BWD_FROZEN 0x200
int cs_bn_bwd_reduce(const void* dy, const void* z, int dtype, const float* mean, const float* rstd,
                     const float* gamma, const float* beta, int act, long long M, int C, double* sums, double* workspace, void* stream);
/* dz = gamma*rstd*( g - sums0/M - xhat*sums1/M ); dgamma=sums1, dbeta=sums0 (fp32, nullable). */
int cs_bn_bwd_apply(const void* dy, const void* z, int dtype, const float* mean, const float* rstd,
                    const float* gamma, const float* beta, int act, const double* sums, long long M, int C, void* dz,
                    float* dgamma, float* dbeta, void* stream);

/* ---- weight staging of an ungrouped convolution ---------------------------------------------
 * w[K][Cin][R][S] fp32 (torch Conv2d.weight) times the per-K scale of a folded eval-mode BatchNorm2d, gamma/sqrt(var + eps), ->
 *   w_khwc [Kp][R][S][Cp]  (forward operand)   if non-NULL
 *   w_chwk [Cp][R][S][Kp]  (dgrad operand)     if non-NULL
 * Cp/Kp = stored (padded) channel counts; padded rows/columns are zero-filled.  One descriptor per layer; ONE kernel body serves
 * every entry below, so their outputs agree bit for bit. */
typedef struct CsStageDesc {
    const float *w, *gamma, *beta, *mean, *var, *conv_bias;   /* gamma / beta / conv_bias nullable; mean == var == NULL: no statistics are folded
                                                                 * (rstd = 1; a train-mode BN layer passes gamma = beta = NULL too:
                                                                 * scale = 1, shift = conv_bias or 0) */
    void *w_khwc, *w_chwk;                                     /* either nullable */
    float *scale, *shift, *rstd;                               /* [Kp], rows k >= K zero; each nullable (not wanted) in cs_stage_conv_bn_one */
    float eps;
    int32_t K, Cin, R, S, Cp, Kp;
    int32_t block0;                                            /* cs_stage_conv_bn_multi only: first workgroup of this layer */
    /* nonzero: write that operand in the MFMA-fragment order cs_conv2d_fwd_packed / cs_conv2d_dgrad_packed read instead of
     * w_khwc / w_chwk order (needs Kp % 32 == 0 and Cp % 64 == 0 for fwd, Cp % 32 == 0 and Kp % 64 == 0 for bwd); the buffer
     * sizes are the same.  cs_pack_conv_weights, the independent implementation of that order, gives the same bits from the plain
     * operand. */
    int32_t fwd_packed, bwd_packed;
} CsStageDesc;
/* Workgroups that stage one layer (both launch shapes below size their grids with it); 0 for bad extents. */
int cs_stage_conv_bn_blocks(int K, int Cin, int R, int S, int Cp, int Kp, int want_fwd, int want_bwd);
/* One layer in one launch: BN fold (scale/shift/rstd as cs_bn_fold computes them) + both operands, plain or packed.  `host_desc` is
 * read on the HOST and travels as the kernel argument: no device table, no copy, so the call may sit inside a stream capture. */
int cs_stage_conv_bn_one(const CsStageDesc* host_desc, int dtype, void* stream);
/* The plain operands only, times an optional per-K `scale`: cs_stage_conv_bn_one with gamma = scale and nothing else set. */
int cs_weight_prep(const float* w, const float* scale, int dtype, int K, int Cin, int R, int S, int Cp, int Kp,
                   void* w_khwc, void* w_chwk, void* stream);
/* EVERY layer of a network in ONE launch (a training step re-stages all ~53 layers of a ResNet-50 after each optimizer update:
 * 53 launches of ~7 us otherwise).  `desc` is a DEVICE array of n descriptors, built once by the host for a fixed set of
 * parameter / staging buffers; block0 = prefix sum of cs_stage_conv_bn_blocks() over the layers, total_blocks = the sum. */
int cs_stage_conv_bn_multi(const CsStageDesc* desc, int n, int total_blocks, int dtype, void* stream);

/* ---- convolution family (implicit GEMM on MFMA) ---------------------------------------------
 * forward: y = act( scale[k]*conv(x,w) + shift[k] + residual ), any of scale/shift/residual NULL.
 *   Fuses Conv2d+BatchNorm2d(eval)+ReLU(+residual add) of BasicBlock/Bottleneck.forward
 *   (resnet.py:28-43, 60-78) and Conv2d(bias) of upsample_conv/seg_out_conv (resnet.py:195-200,164).
 *   stats (nullable, an exact accumulator of cs_bn_accum_words(K) zeroed words -- see cs_bn_stats --, needs `workspace`): accumulates sum and sum of squares of the STORED output per channel
 *   (BatchNorm2d train-mode batch statistics). */
int cs_conv2d_fwd(const CsConvGeom* g, int dtype, const void* x, const void* w_khwc, const float* scale,
                  const float* shift, const void* residual, int act, void* y, double* stats, void* workspace,
                  void* stream);
/* bytes of `workspace` that cs_conv2d_fwd (stats) / cs_conv2d_dgrad (colsum) need for M destination
 * pixels x n_out destination channels: per-workgroup partial sums, folded without atomics. */
size_t cs_conv2d_stats_workspace(long long M, int n_out);
/* Which BM x BN output tile the fwd/dgrad dispatcher uses for M output pixels x n_out channels
 * (returns BM*1000+BN); lets bench.py / profiles name the kernel instantiation that ran. */
int cs_igemm_tile(long long M, int n_out);
#ifdef CS_AB_SWITCHES
/* A/B flavour only (`make AB=1` -> libcellseg_hip_ab.so; not part of the production ABI).  Staging path of the fwd/dgrad
 * kernel: 0 (default) = LDS-DMA (`buffer_load ... lds`) whenever both operands are < 2 GiB; 1 = register-staged everywhere
 * (the production rule for operands >= 2 GiB, forced here so that small test shapes reach it).  Returns the previous setting;
 * any other value returns CS_ERR_INVALID_ARG and leaves the setting as it was. */
int cs_set_igemm_path(int path);
#endif
/* data gradient: dx = ( conv_transpose(dy, w) + add ) * [mask > 0]; add/mask nullable, both shaped like x.
 *   `mask` is the conv's own input activation when that input came out of a ReLU (the ReLU backward of
 *   resnet.py:41/76 fused here). colsum (nullable fp32 [C]) accumulates per-channel sums of the stored dx. */
int cs_conv2d_dgrad(const CsConvGeom* g, int dtype, const void* dy, const void* w_chwk, const void* add,
                    const void* mask, void* dx, float* colsum, void* workspace, void* stream);
/* One bit per element instead of a 16-bit mask operand (the ReLU masks are 1/6 of a training step's HBM traffic otherwise):
 * cs_conv2d_fwd_bits also writes the plane `positive_bits`: M * K / 8 bytes (M = N*P*Q pixels, K % 32 == 0), CHANNEL-BLOCK-MAJOR since
 * round 5 (ABI 6): the 32-bit word (k / 32) * M + pixel holds channels 32 (k / 32) .. + 31 of that pixel, bit k % 32 = "the stored y is
 * > 0" -- a wave's 32 words of a 32-pixel tile are 128 contiguous bytes (the pixel-major layout of rounds 1-4 put them K / 8 bytes apart:
 * 32 sectors per store instruction).  cs_conv2d_dgrad_bits takes such a plane (of a tensor shaped like x: N*H*W pixels, C channels,
 * C % 32 == 0) in place of `mask`.  Every producer / consumer of bit planes in this library uses this layout (cs_conv2d_fwd_packed,
 * cs_stem_fwd_packed, cs_conv2d_dgrad_packed, cs_positive_bits). */
int cs_conv2d_fwd_bits(const CsConvGeom* g, int dtype, const void* x, const void* w_khwc, const float* scale, const float* shift,
                       const void* residual, int act, void* y, uint8_t* positive_bits, void* stream);
int cs_conv2d_dgrad_bits(const CsConvGeom* g, int dtype, const void* dy, const void* w_chwk, const void* add,
                         const uint8_t* mask_bits, void* dx, float* colsum, void* workspace, void* stream);
/* Deferred column sums: with colsum == NULL and workspace != NULL (ungrouped launches of stride 1, and of stride 2 where
 * cs_conv2d_dgrad_partial_rows(g) > 0: the parity classes then go out as one launch with rows numbered across them) cs_conv2d_dgrad leaves the
 * per-workgroup partial rows in `workspace` -- row r holds the sums of destination-pixel tile r at [r * 2*C + c] -- and skips the
 * fold.  cs_conv2d_dgrad_partial_rows gives the row count; cs_fold_partial_rows folds one such buffer (out[c] += sum over rows, in a
 * fixed order: the unused second half of the first <= 32 partial rows serves as scratch, so `partial` is written to);
 * cs_wgrad_finalize_batched takes the partial rows as they are and folds each channel's column inside its own launch. */
int cs_conv2d_dgrad_partial_rows(const CsConvGeom* g);
int cs_fold_partial_rows(const float* partial, int rows, int n_out, float* out, void* stream);
/* weight gradient, raw split-K partials: dw_khwc[nsplit][K][R][S][Cp] fp32, slab z = sum over pixel slice z of
 *   dy (x) im2col(x), written with plain stores (no zero-fill needed; nsplit = cs_conv2d_wgrad_splits(g, grouped));
 *   cs_wgrad_finalize folds the slabs in a fixed order (bitwise reproducible). */
int cs_conv2d_wgrad_splits(const CsConvGeom* g, int grouped);
int cs_conv2d_wgrad(const CsConvGeom* g, int dtype, const void* x, const void* dy, float* dw_khwc,
                    int use_tr_read, void* stream);
/* Batched weight gradient for n_items layers of IDENTICAL geometry (the repeated blocks of a ResNet stage): one launch,
 * blockIdx.z = item*nsplit + slice, nsplit = cs_conv2d_wgrad_batched_splits(g, dtype, n_items) (fewer slices per layer ->
 * proportionally less partial-slab traffic).  x_tab / dy_tab / dw_tab: HOST arrays of n_items (<= 8) device pointers (they
 * are passed to the kernel by value, no device table, no copy); dw_tab[i] is a [nsplit][K][R][S][Cp] fp32 buffer. */
int cs_conv2d_wgrad_batched_splits(const CsConvGeom* g, int dtype, int n_items);
/* 1 when cs_conv2d_wgrad_batched serves this geometry with the second-generation kernel (wgrad_v2.hip: bf16, stride-1 pad-1 3x3,
 * C and K multiples of 64, image width <= 158): callers with a single layer then prefer the batched entry (n_items = 1). */
int cs_conv2d_wgrad2_supported(const CsConvGeom* g, int dtype);
int cs_conv2d_wgrad_batched(const CsConvGeom* g, int dtype, const void* const* x_tab, const void* const* dy_tab,
                            float* const* dw_tab, int n_items, int use_tr_read, void* stream);
/* Batched cs_wgrad_finalize (eval-BN or plain conv, no bias, not grouped) in ONE launch: `tables` = HOST array of 9*n_items
 * (n <= 8) pointers: [raw | w | scale | rstd | mean | gsum | dw | dgamma | dbeta] x n_items (scale..gsum, dgamma, dbeta used only
 * with want_bn).  gsum[i] is either the [K] vector (gsum_rows[i] == 0) or the per-workgroup partial rows a data-gradient
 * launch left behind ([gsum_rows[i]][gsum_stride] fp32, cs_conv2d_partial_rows / cs_conv2d_packed_partial_rows): the kernel
 * folds them itself.  gsum_rows: HOST array of n_items ints, or NULL (all vectors). */
int cs_wgrad_finalize_batched(const float* const* tables, const int* gsum_rows, int gsum_stride, int n_items, int nsplit, int Kp, int K,
                              int Cin, int R, int S, int Cp, int want_bn, void* stream);
/* dw[K][Cin][R][S] (torch layout, ACCUMULATED into when accumulate!=0) = scale[k]*dw_khwc[k][r][s][c];
 * dbias[k] = scale[k]*gsum[k] (conv bias); and, when dgamma/dbeta non-NULL, the eval-mode BatchNorm parameter gradients
 *   dbeta[k] = gsum[k];  dgamma[k] = rstd[k]*( sum_j w[k][j]*dw_raw[k][j] - mean[k]*gsum[k] ). */
int cs_wgrad_finalize(const float* dw_khwc, int nsplit, int Kp, const float* w, const float* scale, const float* rstd,
                      const float* mean, const float* gsum, int K, int Cin, int R, int S, int Cp,
                      float* dw, float* dbias, float* dgamma, float* dbeta, float* dot_ws /* fp32 [K] scratch ZEROED by the caller, needed with dgamma */,
                      int accumulate, void* stream);
/* ---- grouped 3x3 convolution (ResNeXt, model/resnext.py:16-19,85: groups=32) in slab-dense form ------------
 * C == K, C % 64 == 0, Cg = C/groups divides 64.  Each 64-channel destination tile contracts only over its
 * own 64 source channels with weights that are block-diagonal inside the slab:
 *   cs_weight_prep_grouped: w[K][Cg][R][S] fp32 -> w_khwc[K][R][S][64], w_chwk[C][R][S][64]
 *   cs_conv2d_fwd / _dgrad / _wgrad with CsConvGeom.groups > 1 take these operands
 *     (same signatures; dw buffer of wgrad is [K][R][S][64] fp32)
 *   cs_wgrad_finalize_grouped: picks the group diagonal out of the slab gradient -> dw[K][Cg][R][S] (+BN-eval grads) */
int cs_weight_prep_grouped(const float* w, const float* scale, int dtype, int K, int Cg, int R, int S, void* w_khwc,
                           void* w_chwk, void* stream);
int cs_wgrad_finalize_grouped(const float* dw_slab, int nsplit, const float* w, const float* scale, const float* rstd,
                              const float* mean, const float* gsum, int K, int Cg, int R, int S, float* dw, float* dgamma,
                              float* dbeta, float* dot_ws, void* stream);
/* per-channel column sums: out[c] (+)= sum_m g[m][c]; fp32 out, zeroed by the caller. */
int cs_colsum(const void* g, int dtype, long long M, int C, float* out, void* stream);
/* The same sums left as per-workgroup partial rows (layout and consumers as for cs_conv2d_dgrad's deferred column sums):
 * partial[b * 2*C + c], b < cs_colsum_partial_rows(M); no atomics, no zero-fill. */
int cs_colsum_partial_rows(long long M);
/* ---- optimizer ---------------------------------------------------------------------------------
 * torch.optim.Adam's update (the optimizer the reference's drivers construct: train_tile.py:282, train_image.py:476,
 * train_seg.py:309; L2 weight decay, no amsgrad) over up to cs_adam_max_tensors() fp32 tensors in one launch.
 *   tensors_dev : DEVICE array of {p, m, v, n} for ALL tensors of the optimizer (built once)
 *   grads_host  : HOST array of n_tensors device pointers, the gradients of tensors [t0, t0 + n_tensors) (passed by value)
 *   chunks_dev  : DEVICE array of n_chunks (tensor index, first element / cs_adam_chunk_elems()) int pairs covering those tensors
 *   step        : t >= 1 of this update; hyper-parameters as doubles (the bias corrections and 1 - beta are formed in double, as torch does) */
typedef struct CsAdamTensor { float* p; float* m; float* v; long long n; } CsAdamTensor;
int cs_adam_chunk_elems(void);
int cs_adam_max_tensors(void);
int cs_adam_step(const CsAdamTensor* tensors_dev, const void* const* grads_host, int t0, int n_tensors, const int* chunks_dev,
                 int n_chunks, double lr, double beta1, double beta2, double eps, double weight_decay, double step, void* stream);
/* The same update with the step counts in DEVICE memory (torch.optim.Adam(capturable=True)'s state layout: one fp32 scalar per
 * tensor), so that a training step captured into a HIP graph (cellsegmentation_amd.graphed.GraphedStep over the loop body
 * train/train.py:29-42) advances them at every replay.  Two launches: one thread per tensor does t = ++*steps_dev[row] and leaves
 * (lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)) -- formed in double -- in coef_dev[row]; the update kernel reads them from there.
 *   steps_dev : DEVICE array, one `float*` per ROW of tensors_dev (rows [t0, t0 + n_tensors) are used)
 *   coef_dev  : DEVICE scratch of 2 floats per row of tensors_dev (caller-owned, overwritten)
 *   lr_dev    : DEVICE double holding the learning rate, or NULL to use `lr` (a captured launch keeps its by-value arguments
 *               for ever: schedulers that change lr between replays write it here) */
int cs_adam_step_dev(const CsAdamTensor* tensors_dev, const void* const* grads_host, int t0, int n_tensors, const int* chunks_dev,
                     int n_chunks, float* const* steps_dev, float* coef_dev, const double* lr_dev, double lr, double beta1, double beta2,
                     double eps, double weight_decay, void* stream);
/* torch.optim.SGD's update (what the drivers train with when a scheduler is given: train_tile.py:280-303, train_seg.py:289-312,
 * train_image.py:483-508 -- momentum 0.9, weight_decay 1e-4), single-tensor form, on the same machinery: tensors_dev / grads_host /
 * chunks_dev as for cs_adam_step, cs_adam_chunk_elems() elements per chunk, at most cs_adam_max_tensors() tensors per call.
 *   g' = g + weight_decay * p;   buf = first ? g' : momentum * buf + (1 - dampening) * g';   g' = nesterov ? g' + momentum * buf : buf;
 *   p = p - lr * g'
 *   buf      : NULL for a tensor that takes the plain update p = p - lr * g' (momentum 0)
 *   first    : not 0 when the tensors of this launch have no momentum history yet (buf is written, not read)
 *   nesterov : requires momentum > 0 and dampening == 0, as in torch
 * The scalars are rounded to fp32 once, from double: (float)lr, (float)momentum, (float)(1 - dampening), (float)weight_decay. */
typedef struct CsSgdTensor { float* p; float* buf; long long n; } CsSgdTensor;
int cs_sgd_step(const CsSgdTensor* tensors_dev, const void* const* grads_host, int t0, int n_tensors, const int* chunks_dev, int n_chunks,
                double lr, double momentum, double dampening, double weight_decay, int nesterov, int first, void* stream);
/* The same update with hyper_dev[0] = lr and hyper_dev[1] = momentum read from DEVICE memory (two doubles, rounded to fp32 in the
 * kernel) by every workgroup: a launch captured into a HIP graph takes the values a scheduler wrote there since the last replay
 * (OneCycleLR moves both at every iteration).  dampening, weight_decay, nesterov and first are launch arguments, fixed at capture. */
int cs_sgd_step_dev(const CsSgdTensor* tensors_dev, const void* const* grads_host, int t0, int n_tensors, const int* chunks_dev, int n_chunks,
                    const double* hyper_dev, double dampening, double weight_decay, int nesterov, int first, void* stream);

/* Per-sample, per-channel sums of an NHWC tensor [N][HW][C]: out[n][c] = scale * sum_p a[n][p][c] (* b[n][p][c] when b != NULL),
 * fp32 [N][C], overwritten.  The two reductions of a squeeze-excitation block (torchvision SqueezeExcitation as used by
 * model/efficientnet.py:83,107): the average pool (b = NULL, scale = 1/HW) and ds = sum dy * x of its backward.  Row-strided
 * workgroups leave partial rows in `workspace` (cs_sample_sum_workspace bytes, caller-owned) that are added in a fixed order:
 * bitwise reproducible, no atomics. */
size_t cs_sample_sum_workspace(int N, int HW, int C);
int cs_sample_sum(const void* a, const void* b, int dtype, float scale, float* out, float* workspace, int N, int HW, int C,
                  void* stream);
/* bit plane of a bf16 NHWC tensor x[n_pixels][C] in the layout of cs_conv2d_fwd_bits (channel-block-major, below): the `mask_bits`
 * operand of cs_conv2d_dgrad_packed for a post-ReLU tensor that no convolution epilogue produced, e.g. torch.cat of two ReLU outputs,
 * resnet.py:284-294; C % 32 == 0 */
int cs_positive_bits(const void* x, int dtype, long long n_pixels, int C, uint8_t* bits, void* stream);
int cs_colsum_partial(const void* g, int dtype, long long M, int C, float* partial, void* stream);

/* ---- pooling --------------------------------------------------------------------------------
 * MaxPool2d(3, stride 2, pad 1) (resnet.py:114). */
/* argmax (nullable, uint8 [N][P][Q][C]): window tap kh*3+kw of the first maximum in scan order
 * (ATen's max_pool2d_with_indices rule: strictly-greater replaces, and so does a NaN: the LAST NaN of a window). */
int cs_maxpool3x3s2_fwd(const void* x, int dtype, void* y, uint8_t* argmax, int N, int H, int W, int C, int P, int Q,
                        void* stream);
/* dx[n][iy][ix][c] = sum over the <=4 windows containing (iy,ix) whose argmax is this pixel of
 * dy * [y_mask > 0] (y_mask nullable: the pooled output when a ReLU precedes the pool and the
 * caller wants the ReLU backward of resnet.py:113 fused). Gather form: no atomics. */
int cs_maxpool3x3s2_bwd(const void* dy, const uint8_t* argmax, const void* y_mask, int dtype, void* dx, int N, int H,
                        int W, int C, int P, int Q, void* stream);
/* AdaptiveAvgPool2d(1)+AdaptiveMaxPool2d(1) summed (resnet.py:266,274): feat[N][C] fp32,
 * argmax[N][C] int32 = first spatial index of the maximum (of the LAST NaN where the map holds one: ATen's
 * rule, as for the max pool above).  with_max==0: average only (the squeeze of
 * torchvision's SqueezeExcitation, efficientnet.py:107). */
int cs_gap_avgmax_fwd(const void* x, int dtype, float* feat, int32_t* argmax, int N, int HW, int C, int with_max,
                      void* stream);
/* dx[n][p][c] = ( dfeat[n][c]/HW + (p==argmax[n][c]) * dfeat[n][c] ) * [x>0 if relu_mask]. */
int cs_gap_avgmax_bwd(const float* dfeat, const int32_t* argmax, const void* x, int dtype, void* dx, int N, int HW,
                      int C, int relu_mask, int with_max, void* stream);

/* ---- segmentation decoder data movement ------------------------------------------------------
 * F.interpolate(mode="bilinear", align_corners=True) (resnet.py:282,287,292,297,300): x[N][H][W][C] -> y[N][P][Q][C] */
int cs_bilinear_ac_fwd(const void* x, int dtype, void* y, int N, int H, int W, int C, int P, int Q, void* stream);
/* dx = interpolate^T(dy) * [mask>0] (mask nullable, shaped like dx: the ReLU output that was upsampled) */
int cs_bilinear_ac_bwd(const void* dy, const void* mask, int dtype, void* dx, int N, int H, int W, int C, int P, int Q,
                       void* stream);
/* torch.cat([a,b], dim=1) in NHWC (resnet.py:284,289,294): out[M][Ca+Cb]; and its inverse (a or b nullable). */
int cs_concat_channels(const void* a, const void* b, int dtype, void* out, long long M, int Ca, int Cb, void* stream);
int cs_split_channels(const void* whole, int dtype, void* a, void* b, long long M, int Ca, int Cb, void* stream);

/* ---- MBConv pieces (model/efficientnet.py:81-122; torchvision 0.11.2 ConvNormActivation with groups=C,
 * SqueezeExcitation, StochasticDepth("row")) -------------------------------------------------------
 * depthwise conv: geometry with K == C, R == S; w_hwc fp32 [R][S][C]; optional fused per-channel
 * scale/shift (eval BN) and activation. */
int cs_dwconv_fwd(const CsConvGeom* g, int dtype, const void* x, const float* w_hwc, const float* scale, const float* shift,
                  int act, void* y, void* stream);
/* Depthwise forward for train-mode BN: y = raw conv output, and the per-channel sum / sum of squares of the stored y as
 * *partial_rows per-workgroup rows partial[r][2][C] (fp64, cs_dwconv_fwd_stats_workspace(g) bytes); cs_bn_partial_fold adds the
 * rows into the exact accumulator `stats` (cs_bn_accum_words(C) zeroed words) -- together they replace cs_dwconv_fwd + cs_bn_stats
 * (one pass over y less).  The query takes no dtype: it returns room for the launch plan of either dtype, the same plan the call
 * itself launches from, so *partial_rows rows always fit. */
size_t cs_dwconv_fwd_stats_workspace(const CsConvGeom* g);
int cs_dwconv_fwd_stats(const CsConvGeom* g, int dtype, const void* x, const float* w_hwc, void* y, double* partial,
                        int* partial_rows, void* stream);
int cs_bn_partial_fold(const double* partial, int rows, int C, double* stats, void* stream);
int cs_dwconv_dgrad(const CsConvGeom* g, int dtype, const void* dy, const float* w_hwc, void* dx, void* stream);
/* dw_hwc[R][S][C] fp32.  workspace: cs_dwconv_wgrad_workspace(g) bytes of per-workgroup partial rows [R*S*C] fp32 (folded by a
 * second kernel: no atomics, dw_hwc is overwritten, not accumulated into); like the statistics query, room for the launch plan of
 * either dtype */
size_t cs_dwconv_wgrad_workspace(const CsConvGeom* g);
int cs_dwconv_wgrad(const CsConvGeom* g, int dtype, const void* x, const void* dy, float* dw_hwc, float* workspace, void* stream);
/* the same with the result in the parameter's own layout [C][1][R][S] (nn.Conv2d(groups = C).weight, model/efficientnet.py:97-103) */
int cs_dwconv_wgrad_oihw(const CsConvGeom* g, int dtype, const void* x, const void* dy, float* dw_oihw, float* workspace, void* stream);
/* Depthwise filters of MANY layers, parameter layout [C][1][R][S] -> the [R][S][C] the depthwise kernels read, in one launch.
 * desc_dev: n rows in DEVICE memory, `first` (offset of the layer's first element in the launch's flat index space) ascending;
 * total = sum of C * RS. */
typedef struct { const float* src; float* dst; long long C; long long RS; long long first; } CsDwStageDesc;
int cs_dw_weights_hwc_multi(const CsDwStageDesc* desc_dev, int n, long long total, void* stream);
/* y[n][p][c] = x[n][p][c]*s[n][c] */
int cs_se_scale(const void* x, int dtype, const float* s, void* y, int N, int HW, int C, void* stream);
/* dx = dy*s + davg[n][c]/HW (davg nullable); the other half, ds[n][c] = sum_p dy*x, is cs_sample_sum(dy, x) */
int cs_se_scale_bwd_dx(const void* dy, int dtype, const float* s, const float* davg, void* dx, int N, int HW, int C, void* stream);
/* y = a*row_scale[n] + b over N rows of per_row elements (row_scale, b nullable) */
int cs_rowscale_add(const void* a, int dtype, const float* row_scale, const void* b, void* y, int N, long long per_row,
                    void* stream);

/* ---- tile construction on the device (the step before the hot path; dataset/dataset.py:203-214,718-742,78-83) ----
 * images: uint8 [n_images][H][W][3] in HBM; tile t = image tile_img[t], upper-left (row, col) = tile_rc[2t], tile_rc[2t+1];
 * out[n_tiles][size][size][8] dtype = ((u8/255) - mean)/std on channels 0..2, channels 3..7 zero (the NHWC operand of the
 * stem convolution).  mean/std are HOST arrays of 3 floats.  The caller guarantees tiles lie inside the image. */
int cs_tile_gather(const uint8_t* images, int n_images, int H, int W, const int32_t* tile_img, const int32_t* tile_rc,
                   long long n_tiles, int size, const float* host_mean3, const float* host_std3, int dtype, void* out,
                   void* stream);

/* cs_tile_gather with the reference's training augmentations (csrc/augment.hip): th x tw tiles (a whole image is one tile),
 * per tile  crop -> /255 in fp32 -> colour ops on the un-flipped crop -> flip -> (v - mean) / std,  out[n_tiles][th][tw][8].
 * flips (device int8 [n_tiles], NULL = none): the reference's transformIDX, bit 0 = horizontal, bit 1 = vertical:
 *   out[y][x] = crop[bit 1 ? th-1-y : y][bit 0 ? tw-1-x : x].
 * jitter_ops / jitter_factors (device int8 / float [n_tiles][4], both or neither; 4- and 16-byte aligned): a ColorJitter record,
 * four op codes in application order (0 brightness, 1 contrast, 2 saturation, 3 hue, anything else = unused slot) with their
 * factors, the float-image arithmetic of torchvision 0.11.2 with gray = 0.2989 r + 0.587 g + 0.114 b and
 * blend(a, b, f) = clamp(f a + (1 - f) b, 0, 1): brightness blend(x, 0, f); contrast blend(x, m, f) with m the mean of gray over
 * the tile as the ops in front of it left it, m = fp32(sum_fp64 / (th tw)); saturation blend(x, gray(x), f); hue rgb -> hsv,
 * h <- h + f - floor(h + f), hsv -> rgb.  The caller keeps a code from repeating within a record and the factors finite.
 * has_contrast: 1 = some record holds a contrast op: the call zeroes the workspace and runs the mean reduction in front of the
 * apply kernel (3 stream operations instead of 1); 0 = none does (one found is skipped) and workspace may be NULL.
 * workspace: 8-byte aligned, >= cs_stage_augmented_workspace(n_tiles) bytes (0 for an n_tiles a call would refuse).
 * The sum is order-independent (exact-limb accumulation): two calls give the same bits.  Never synchronises.  Without flips and
 * jitter the output equals cs_tile_gather's bit for bit.  The caller guarantees tiles lie inside the image. */
size_t cs_stage_augmented_workspace(long long n_tiles);
int cs_stage_augmented(const uint8_t* images, int n_images, int H, int W, const int32_t* tile_img, const int32_t* tile_rc,
                       const int8_t* flips, const int8_t* jitter_ops, const float* jitter_factors, int has_contrast,
                       long long n_tiles, int th, int tw, const float* host_mean3, const float* host_std3, int dtype, void* out,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- heads: Linear (resnet.py:126,137,140,150), losses (train/train.py:34,80-83) ------------- */
/* y[M][N] = act( x[M][K] @ w[N][K]^T + b[N] )  (fp32; b nullable; preact nullable: the value before act) */
int cs_linear_fwd(const float* x, const float* w, const float* b, float* y, float* preact, int M, int N, int K, int act,
                  void* stream);
/* dx[M][K] = g @ w (nullable dx); dw[N][K] (+)= g^T @ x; db[N] (+)= colsum(g), g = dy through the output
 * activation: `y` = stored output for ReLU / sigmoid, stored PRE-activation for SiLU. */
/* `workspace`: cs_linear_bwd_workspace(M, N, K) bytes (0 up to 512 rows: NULL is fine).  With a long batch axis -- the reference hands its
 * tile loops batches of 40 960 (train_tile.py -b), so the squeeze-excitation layers of an EfficientNet encoder see M in the thousands --
 * the weight gradient is cut into row slices whose partial results land there and are added in slice order (ABI 6). */
size_t cs_linear_bwd_workspace(int M, int N, int K);
int cs_linear_bwd(const float* x, const float* w, const float* dy, const float* y, int act, float* dx, float* dw,
                  float* db, int M, int N, int K, int accumulate, float* workspace, void* stream);
/* CrossEntropyLoss(mean) * gamma on logits[M][C]; dlogits nullable.  `loss` (here and in cs_mse): cs_loss_words() = 16 floats, all
 * overwritten -- the value in loss[0], the rest is the exact accumulator the workgroups' partial sums meet in (round 5: the value of a
 * launch with more than one workgroup no longer depends on their arrival order). */
int cs_loss_words(void);
int cs_softmax_ce(const float* logits, const int64_t* labels, float gamma, float* loss, float* dlogits, int M, int C,
                  void* stream);
/* softmax(logits,1)[:,1] (inference.py:24-27) */
int cs_softmax_prob1(const float* logits, float* p1, int M, int C, void* stream);
/* np.argmax(F.softmax(logits,1), axis=1) (inference.py:72-76, 118-119): arg max over the fp32 probabilities, first index on
 * ties (logits closer than the rounding of exp/÷ tie as probabilities); idx int64 [M]. */
int cs_softmax_argmax(const float* logits, int64_t* idx, int M, int C, void* stream);
/* sum or mean of w_i*(x_i-t_i)^2, w_i = 1 (weighted==0) or the reference's weighted_mse weights
 * (metrics/metrics.py:23-33: ln(t) if t>=20 else t).  dx nullable. scale = upstream grad factor. */
int cs_mse(const float* x, const float* t, int weighted, int mean, float* loss, float* dx, int M, void* stream);

/* Dice loss (train/losses.py:44-62 over metrics/metrics.py:36-53) on p[N][HW], t[N][HW] fp32:
 * sums = (sum p*t, sum p^2, sum t^2) per sample as an exact accumulator (see cs_bn_stats) of cs_bn_accum_words(3 N) 8-byte words,
 * cleared by cs_dice_fwd (the block sums are added in any order with the same bits: the reference's CPU path repeats too);
 * loss = mean|sum over n of 1-(2a+eps)/(b+c+eps). */
int cs_dice_fwd(const float* p, const float* t, int N, long long HW, float eps, int mean, double* sums, float* loss,
                void* stream);
int cs_dice_bwd(const float* p, const float* t, const double* sums, int N, long long HW, float eps, int mean, float* dp,
                void* stream);
/* F.softmax(logits, dim=1)[:, ch] on NCHW fp32 logits[N][C][HW] (train/train.py:189) and its backward. */
int cs_softmax_channel_fwd(const float* logits, float* pc, int N, int C, long long HW, int ch, void* stream);
int cs_softmax_channel_bwd(const float* logits, const float* dpc, float* dlogits, int N, int C, long long HW, int ch,
                           void* stream);

/* ---- adaptive top-k instance selection (inference.py:31-43) ---------------------------------
 * probs[T] fp32, groups[T] int32 non-decreasing, k_per_tile[T] int32 (k of the tile's group).
 * seg_offsets[n_groups+1] int64 (device): start of each group's run; max_run = longest run (host int).
 * Writes the reference's order[index] list: out_idx[0..*out_count) int64 (device), reproducing
 * np.lexsort((probs, groups)) + the wrap-around (i+k)%T comparison bit-exactly.  Runs of any length: up to 8192 tiles are
 * sorted in LDS, longer ones (whole-slide tile grids) in place in global memory -- the reference has no limit either.
 * workspace: >= cs_segmented_topk_workspace(T) bytes. */
size_t cs_segmented_topk_workspace(long long T);
int cs_segmented_topk(const float* probs, const int32_t* groups, const int32_t* k_per_tile,
                      const int64_t* seg_offsets, int n_groups, int max_run, long long T, int64_t* out_idx,
                      int64_t* out_count, void* workspace, size_t workspace_bytes, void* stream);

/* ---- packed-operand bf16 convolutions (csrc/conv_v2.hip): the stride-1 3x3 forward / data gradient of BasicBlock / Bottleneck
 * (model/resnet.py:20,23,53 and their autograd backward) with the source rows of ALL taps staged once per 64-channel chunk (halo
 * tile in LDS), weights streamed to registers in MFMA-fragment order and a register-direct epilogue.  CS_BF16 only.
 *   cs_conv2d_packed_supported : 1 when the geometry is served (3x3, stride 1, channel counts multiples of 64, operand < 2 GiB, ...);
 *                                otherwise use cs_conv2d_fwd / cs_conv2d_dgrad with the plain staged weights.  dgrad: 0 = forward, 1 = data gradient.
 *   cs_pack_conv_weights       : plain staged weights (w_khwc for forward, w_chwk for the data gradient, as cs_weight_prep /
 *                                cs_stage_conv_bn_* write them) -> fragment order [32-row tile][64-ch chunk][tap][16-deep step][lane][8],
 *                                cs_conv2d_packed_weight_bytes() bytes; the data-gradient form mirrors the taps.  A second launch per
 *                                operand: the staging entries write this order themselves (CsStageDesc.fwd_packed / bwd_packed).
 *                                This one packs what they do not stage (the stem's 256-column operand) and is the independent
 *                                statement of the order that the tests hold them against.
 *   cs_conv2d_fwd_packed       : y = act(conv(x, w) + shift[k] + residual); positive_bits (nullable) as cs_conv2d_fwd_bits.
 *   cs_conv2d_dgrad_packed     : dx = (conv_transpose(dy, w) + add) masked by mask_bits (nullable, as cs_conv2d_dgrad_bits);
 *                                partial_rows (nullable): fp32 [cs_conv2d_packed_partial_rows(g, 1)][2][C] per-workgroup column
 *                                sums of the stored dx (first C entries of a row), folded by cs_fold_partial_rows*.
 *                                A STRIDE-2 1x1 geometry (the shortcut of a down-sampling block, model/resnet.py:183) is served in
 *                                COMPACT form: dx is [N][P][Q][C], the values of destination pixels (2y, 2x); every other pixel of
 *                                that gradient is zero and is never written (add, mask_bits, partial_rows must be NULL).  Its
 *                                consumer -- the 1x1 data gradient that accumulates the block input's gradient -- takes it as
 *                                `add` with add_stride = 2: added at even (y, x) only, nothing elsewhere (add_stride = 1: an
 *                                ordinary destination-shaped operand). */
int cs_conv2d_packed_supported(const CsConvGeom* g, int dgrad);
size_t cs_conv2d_packed_weight_bytes(const CsConvGeom* g, int dgrad);
int cs_pack_conv_weights(const CsConvGeom* g, int dgrad, const void* w_staged, void* w_packed, void* stream);
int cs_conv2d_packed_partial_rows(const CsConvGeom* g, int dgrad);
int cs_conv2d_fwd_packed(const CsConvGeom* g, const void* x, const void* w_packed, const float* shift, const void* residual, int act,
                         void* y, uint8_t* positive_bits, void* stream);
int cs_conv2d_dgrad_packed(const CsConvGeom* g, const void* dy, const void* w_packed, const void* add, int add_stride,
                           const uint8_t* mask_bits, void* dx, float* partial_rows, void* stream);
/* The last 1x1 convolution of a bottleneck block and the block's 1x1 projection shortcut (model/resnet.py:58) in ONE launch of the
 * ring kernel: y = act(conv(x, w) + shift + bf16(conv(x_in, w_sc) + shift_sc)) -- the shortcut's output, which cs_conv2d_fwd_packed
 * would read back as `residual`, is rounded to bf16 into LDS instead of being written to memory, so y holds the bits of the two ring
 * launches it replaces.  main: 1x1, stride 1,
 * pad 0; shortcut: 1x1, pad 0, stride 1 or 2; both with the same N, P, Q, K, K a multiple of 128, both C multiples of 64.  Each
 * operand as cs_conv2d_fwd_packed takes it for its own geometry (two packed weight buffers, two nullable shift vectors);
 * positive_bits as there.  cs_conv2d_fwd_shortcut_supported: 1 where the pair is served, else 0 (two launches then). */
int cs_conv2d_fwd_shortcut_supported(const CsConvGeom* main, const CsConvGeom* shortcut);
int cs_conv2d_fwd_shortcut_packed(const CsConvGeom* main, const void* x, const void* w_packed, const float* shift,
                                  const CsConvGeom* shortcut, const void* x_in, const void* w_packed_sc, const float* shift_sc, int act,
                                  void* y, uint8_t* positive_bits, void* stream);

/* ---- stem on a pixel-paired image (Conv2d(3, 64, 7, stride 2, padding 3), model/resnet.py:111) ---------------------------
 * With 3 channels padded to one 16-byte chunk per pixel the implicit GEMM walks 49 chunks of which 147/392 elements are real.
 * Two neighbouring pixels x 4 channels per chunk make it a 7x4-tap convolution over x_pair[N][H][ceil(W/2)][8] (row stride 2,
 * pair stride 1, pad (3, 2)): 28 chunks, 1.75x less MFMA work and DMA traffic, same kernels.
 *   cs_stem_pair_input  : NHWC8 image (channels 3..7 zero) -> x_pair
 *   cs_stem_pair_weights: staged w_khwc[K][7][7][8] (BN scale already folded) -> w_pair[K][7][4][8]
 *   cs_stem_fwd         : as cs_conv2d_fwd (scale/shift/act/stats/workspace), y[N][P][Q][K], P = (H - 1) / 2 + 1
 *   cs_stem_wgrad       : raw split-K slabs dw_pair[cs_stem_wgrad_splits][K][7][4][8] from x_pair and dy
 *   cs_stem_unpair_slabs: those slabs summed into ONE ordinary raw slab dw_khwc[K][7][7][8] (input of cs_wgrad_finalize*) */
int cs_stem_pair_input(const void* x_nhwc8, int dtype, int N, int H, int W, void* x_pair, void* stream);
/* the same x_pair straight from the fp32 NCHW image [N][3][H][W] (cs_nchw_to_nhwc + cs_stem_pair_input in one pass; bf16 only) */
int cs_stem_pair_from_nchw(const float* x_nchw, int dtype, int N, int H, int W, void* x_pair, void* stream);
int cs_stem_pair_weights(const void* w_khwc, int dtype, int K, void* w_pair, void* stream);
int cs_stem_fwd(int N, int H, int W, int K, int dtype, const void* x_pair, const void* w_pair, const float* scale, const float* shift,
                int act, void* y, double* stats, void* workspace, void* stream);
/* bf16 forward on the ring kernel of conv_v2.hip (gathered operand rows): w_packed = cs_pack_conv_weights of the 1x1 geometry
 * (C = 256, K) applied to w_pair padded to [K][8][4][8] with one zero filter row; epilogue as cs_conv2d_fwd_packed. */
int cs_stem_fwd_packed(int N, int H, int W, int K, const void* x_pair, const void* w_packed, const float* shift, int act, void* y,
                       uint8_t* positive_bits, void* stream);
/* The bf16 stem forward (shift, ReLU) and the MaxPool2d(3, 2, 1) behind it in one launch (stem_pool.hip): the [N][P][Q][K] stem map is
 * never written.  w_pair as cs_stem_pair_weights leaves it; y_pool[N][PP][PQ][K] with PP = (P - 1) / 2 + 1, PQ = (Q - 1) / 2 + 1;
 * argmax (nullable) as cs_maxpool3x3s2_fwd writes it.  The values are those of cs_stem_fwd_packed + cs_maxpool3x3s2_fwd, bit for bit.
 * cs_stem_pool_fwd_supported: 1 where the launch is served (K == 64, H, W >= 7, 32-bit offsets inside one image), else 0. */
int cs_stem_pool_fwd_supported(int N, int H, int W, int K);
int cs_stem_pool_fwd(int N, int H, int W, int K, const void* x_pair, const void* w_pair, const float* shift, void* y_pool,
                     uint8_t* argmax, void* stream);
int cs_stem_wgrad_splits(int N, int H, int W, int K);
int cs_stem_wgrad(int N, int H, int W, int K, int dtype, const void* x_pair, const void* dy, float* dw_pair_slabs, int use_tr_read,
                  void* stream);
int cs_stem_unpair_slabs(const float* dw_pair_slabs, int nsplit, int K, float* dw_khwc, void* stream);

/* ---- the steps either side of the top-k -----------------------------------------------------------
 * cs_segmented_order: order = np.lexsort((probs, groups)) alone (train_seg.py:239, evaluate.py:13); order[T] int64.
 * cs_threshold_select: order[[p > threshold for p in probs[order]]] (train_seg.py:243-245), i.e. `rank`'s tile list;
 *   workspace as for cs_segmented_topk.
 * cs_evaluate_tile_counts: evaluate.py:8-27 as four exact counts, counts4 (zeroed by the caller) += {pred != real,
 *   pred & !real, !pred & real, real}; pos_from[g] (int64, host-computed, device-resident) = first sorted position labelled
 *   positive for group g or any later group.
 * cs_paint_tile_masks: utils/image_processing.py:92-98 -- masks[n_images][H][W] uint8 (zeroed by the caller) gets a
 *   tile_size^2 block of ones at tile_xy[t] = (row, col) in image groups[t] for every t in selected[0..n_selected).
 * cs_prune_excess: dataset/dataset.py:190-199 on the shuffled label array: positions kept when the first n_excess entries
 *   with labels[i] == flag are deleted (kept[] int64 ascending, *kept_count). */
int cs_segmented_order(const float* probs, const int64_t* seg_offsets, int n_groups, int max_run, long long T, int64_t* order,
                       void* stream);
int cs_threshold_select(const float* probs, const int64_t* order, long long T, float threshold, int64_t* out_idx,
                        int64_t* out_count, void* workspace, size_t workspace_bytes, void* stream);
int cs_evaluate_tile_counts(const float* probs, const int64_t* order, const int32_t* groups, const int64_t* pos_from,
                            float threshold, long long T, unsigned long long* counts4, void* stream);
int cs_paint_tile_masks(const int64_t* selected, long long n_selected, const int32_t* groups, const int32_t* tile_xy,
                        int tile_size, int H, int W, uint8_t* masks, void* stream);
int cs_prune_excess(const int32_t* labels, long long n, int flag, long long n_excess, int64_t* kept, int64_t* kept_count,
                    void* stream);

/* ---- cell localisation from segmentation probability maps (test_seg.py meanshift_cluster / cell_detect; csrc/detect.hip;
 * cs_detect_edt_*: csrc/morph.hip, on the column pass and row search of the nearest-site transform further down) ----
 * Every step is integer arithmetic or one correctly rounded fp64 operation: bit-exact and independent of launch order.
 * cs_detect_quantize : out[i] = (uint8) trunc(255.0f * probs[i]) (fp32, clamped to [0, 255]); probs 16-byte aligned.
 * cs_detect_blur     : separable integer Gaussian of N maps [N][H][W], BORDER_REFLECT_101.  src is fp32 probabilities
 *                      (src_is_f32 = 1: quantised as above on the way in) or uint8; taps_x[kx], taps_y[ky] (host arrays) are
 *                      odd counts <= 31 of non-negative integers summing to 2^14.  Row pass int32, column pass int64,
 *                      dst = (s + 2^27) >> 28.  src and dst 16-byte aligned.
 * cs_stitch_patches  : out[H][W] = 0, then patch m (patches[M][ph][pw]) written at corners[m] = (row, col) (device int32
 *                      [M][2]), the highest m winning where patches overlap (clipped at the borders);
 *                      workspace >= cs_stitch_workspace(H, W) bytes.
 * cs_stitch_logits   : the same mask built batch by batch, without the resident patches and the owner map: for the B patches
 *                      logits[B][C][ph][pw] (fp32, C >= 2) at corners[b] = (row, col) (device int32 [B][2]),
 *                      mask[row + y][col + x] = trunc(255 softmax_c(logits[b])[ch]) -- the bits of cs_softmax_channel_fwd followed by
 *                      cs_detect_quantize -- in place, one launch, no workspace.  Within the call the highest b covering a pixel
 *                      writes it, exactly once (decided from the corners alone: no atomics, any launch order); pixels that no
 *                      patch of the call covers keep their value; parts of a patch outside the mask are clipped.  Calls are
 *                      ordered by the stream only: every call for one mask must go to the same stream.  Batches of a zeroed mask
 *                      in index order give cs_stitch_patches of all patches, for any split.  H, W < 2^29.
 * cs_stitch_blend_add: overlaps blended instead of overwritten.  Per patch pixel q = (uint32)(256 clamp(255 p, 0, 255)) with p the fp32
 *                      softmax channel ch of cs_softmax_channel_fwd (q >> 8 is the byte of cs_detect_quantize; a NaN gives 0) and
 *                      w = taps_r[i] * taps_c[j] (device int32 [ph], [pw], values 1..255; (i, j) = the pixel's position inside the
 *                      patch on the slide); num[H][W] (int64) += w q and den[H][W] (int32) += w, in place, for the B patches
 *                      logits[B][C][ph][pw] at corners[b] = (row, col) (device int32 [B][2]).  flips (device uint8 [B], or NULL for
 *                      none): 1 horizontal, 2 vertical, 3 both -- logits[b] are those of the flipped tile, so slide position
 *                      (i, j) reads logit pixel (code & 2 ? ph-1-i : i, code & 1 ? pw-1-j : j).  One launch, no workspace, no
 *                      atomics: the lowest b covering a pixel sums every covering patch of the call in registers and updates
 *                      the pixel once; corners and (corner, flip) pairs may repeat.  Integer sums: any split into calls and any
 *                      patch order give the same accumulators.  Calls are ordered by the stream only.  num and den 16-byte
 *                      aligned, H, W < 2^29, B <= 32768; the caller keeps the total of w per pixel below 2^31.
 * cs_stitch_blend_finish: mask[i] = den[i] ? floor(num[i] / (256 den[i])) : 0 (uint8 [H][W]); a pixel covered once holds the byte
 *                      cs_stitch_logits writes.  Reads the accumulators only: more cs_stitch_blend_add calls may follow.
 * cs_detect_grid_size: number G of windows of get_tiles((H, W), interval, window) (-1 when the window does not fit).
 * cs_detect_meanshift: per map n, the grid windows whose blurred centre is above thr255 (fp64 compare), in grid order, each run
 *                      through cv2.meanShift (TermCriteria(EPS, 0, 1e-5): max_iter steps, stopping early at a fixed point);
 *                      pts[n][k] = (row, col) of the final window centre (int32 [N][G][2]), n_pts[n] = windows kept.
 * cs_detect_cluster  : DBSCAN(eps, min_samples=1) of pts[n][0..n_pts[n]) (int32 [N][cap][2], n_pts[n] <= cap): components of
 *                      dr^2 + dc^2 <= eps^2, numbered by lowest point index; centroid = rint(mean); weight =
 *                      blurred[n][centroid] (uint8 [N][H][W]); clusters of map n ordered by weight descending, then label
 *                      descending, written to out_pts[out_off[n] ..) (int64 [N cap][2]) and out_w (int32 [N cap]);
 *                      out_off int64 [N + 1].  Up to 2048 points per map are clustered inside one workgroup; larger maps (or
 *                      force_global) take a multi-launch path that reads one flag back per eight rounds (the host
 *                      synchronises with the stream there).  workspace >= cs_detect_cluster_workspace(N, cap) bytes.
 * cs_detect_edt_sq   : the smoothing of method="distancetransform" (test_seg.py:325-329), first half.  src as for cs_detect_blur
 *                      (fp32 needs 4-byte alignment only); foreground = u8 > thr.  d2 int32 [N][H][W] = exact squared Euclidean
 *                      distance to the nearest background pixel of the same map (0 on background; -1 everywhere in a map without
 *                      background).  Needs H^2 + W^2 < 2^31 and N <= 65535.  Three launches, no host synchronisation.
 * cs_detect_edt_smooth: dst uint8 [N][H][W] = 255 sqrt(d2 / M) rounded half to even, M = the map's own maximum of d2 (all zeros
 *                      where M <= 0), decided by the integer comparison 4 255^2 d2 <> (2k + 1)^2 M: no float decides a value.
 *                      Four launches.  Both take a 16-byte aligned workspace of cs_detect_edt_workspace(N, H, W, smooth) bytes
 *                      (smooth = 1 for cs_detect_edt_smooth; 0 for sizes a call would refuse). */
int cs_detect_quantize(const float* probs, long long n, uint8_t* out, void* stream);
int cs_detect_blur(const void* src, int src_is_f32, int N, int H, int W, const int32_t* taps_x, int kx, const int32_t* taps_y, int ky,
                   uint8_t* dst, void* stream);
size_t cs_stitch_workspace(int H, int W);
int cs_stitch_patches(const uint8_t* patches, int M, int ph, int pw, const int32_t* corners, int H, int W, uint8_t* out,
                      void* workspace, size_t workspace_bytes, void* stream);
int cs_stitch_logits(const float* logits, int B, int C, int ph, int pw, int ch, const int32_t* corners, int H, int W, uint8_t* mask,
                     void* stream);
int cs_stitch_blend_add(const float* logits, int B, int C, int ph, int pw, int ch, const int32_t* corners, const uint8_t* flips,
                        const int32_t* taps_r, const int32_t* taps_c, int H, int W, int64_t* num, int32_t* den, void* stream);
int cs_stitch_blend_finish(const int64_t* num, const int32_t* den, int H, int W, uint8_t* mask, void* stream);
int cs_detect_grid_size(int H, int W, int interval, int window);
int cs_detect_meanshift(const uint8_t* blurred, int N, int H, int W, int interval, int window, double thr255, int max_iter,
                        int32_t* pts, int32_t* n_pts, void* stream);
size_t cs_detect_cluster_workspace(int N, int cap);
int cs_detect_cluster(const int32_t* pts, const int32_t* n_pts, int N, int cap, double eps, const uint8_t* blurred, int H, int W,
                      int force_global, int64_t* out_pts, int32_t* out_w, int64_t* out_off, void* workspace,
                      size_t workspace_bytes, void* stream);
size_t cs_detect_edt_workspace(int N, int H, int W, int smooth);
int cs_detect_edt_sq(const void* src, int src_is_f32, int N, int H, int W, int thr, int32_t* d2, void* workspace,
                     size_t workspace_bytes, void* stream);
int cs_detect_edt_smooth(const void* src, int src_is_f32, int N, int H, int W, int thr, uint8_t* dst, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---- nearest-site transform, exact disk morphology and label expansion (csrc/morph.hip) --------------------------------------
 * N images [N][H][W] that share nothing; 0 < N <= 65535 and H^2 + W^2 < 2^31 per call.  A SITE is a pixel selected by a predicate
 * on the input.  Every pixel is given THE NEAREST SITE, AND AMONG EQUALLY NEAR SITES THE ONE WITH THE LOWEST ROW-MAJOR INDEX; d2 is
 * the exact squared Euclidean distance to it.  Integer work only: bit-exact and independent of launch order; three launches per
 * call, fixed by the shape, no host synchronisation.  Every call takes a 16-byte aligned workspace of cs_morph_workspace(N, H, W)
 * bytes (0 for sizes a call would refuse).  The calls that return or follow a site stage 4 bytes per pixel of a row in LDS and
 * refuse W > cs_morph_max_site_width() = 40960; cs_morph_binary stages 2 bytes and takes every W.
 * cs_morph_nearest      : sites = src != 0 (uint8 [N][H][W]; == 0 with background; int32 with src_is_labels, where background
 *                         must be 0).  d2 int32 [N][H][W] and / or site int32 [N][H][W] = row W + col of the nearest site within
 *                         the image (either may be NULL, not both); both -1 everywhere in an image without a site.  The search of
 *                         a pixel runs over offsets up to sqrt(d2): sparse sites in a wide image are its worst case.
 * cs_morph_binary       : erode = 0: out = (d2 to the nearest nonzero pixel) <= r2, the dilation by the disk dx^2 + dy^2 <= r2;
 *                         erode = 1: out = mask != 0 && (d2 to the nearest zero pixel) > r2, the erosion by it.  With
 *                         outside_is_site the pixels beyond the image edge count as sites (nonzero for the dilation, zero for the
 *                         erosion).  uint8 0 / 1 [N][H][W]; out must not overlap mask.  O(sqrt(r2)) per pixel.
 * cs_morph_expand_labels: out = labels != 0 ? labels : (d2 <= r2 ? labels[site] : 0) for the sites labels != 0, int32 [N][H][W];
 *                         out must not overlap labels.  O(sqrt(r2)) per pixel. */
int cs_morph_max_site_width(void);
size_t cs_morph_workspace(int N, int H, int W);
int cs_morph_nearest(const void* src, int src_is_labels, int background, int N, int H, int W, int32_t* d2, int32_t* site,
                     void* workspace, size_t workspace_bytes, void* stream);
int cs_morph_binary(const uint8_t* mask, int N, int H, int W, int erode, int r2, int outside_is_site, uint8_t* out, void* workspace,
                    size_t workspace_bytes, void* stream);
int cs_morph_expand_labels(const int32_t* labels, int N, int H, int W, int r2, int32_t* out, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ---- small-region clean-up of binary masks (utils/image_processing.py:14-17 remove_small_regions; csrc/regions.hip) ---------
 * Masks are uint8 [N][H][W], non-zero = foreground, N images that share nothing; 0 < N <= 65535 and N H W < 2^31 per call.
 * connectivity 1 = 4-neighbourhood, 2 = 8-neighbourhood, for the foreground and the background alike.  Integer work only:
 * bit-exact and independent of launch order; a fixed number of launches for a given (N, H, W), no host synchronisation.
 * Every call takes a 16-byte aligned workspace of cs_regions_workspace bytes (0 for sizes a call would refuse).
 * cs_regions_label       : scipy.ndimage.label per image -- labels int32 [N][H][W], 0 = background, component number = 1 + the
 *                          number of components of the image whose lowest row-major pixel index is smaller.
 * cs_regions_areas       : areas int32 [N][H][W] = pixel count of the component of EQUAL-VALUED pixels the pixel lies in
 *                          (foreground components under foreground pixels, background components under background pixels).
 * cs_regions_filter      : out = 1 - value where the pixel has `value` (0 or 1) and its component's area < min_area (strict),
 *                          else the input as 0/1: value 1 = remove_small_objects(min_size), value 0 = remove_small_holes
 *                          (area_threshold; background components that touch the border included).  out may be mask.
 * cs_regions_remove_small: the filter with (1, min_object_size), then with (0, hole_area_threshold) on its result.  out may be mask.
 * cs_regions_threshold   : out[i] = probs[i] > threshold, compared in fp32 (numpy's compare of a float32 array with a Python float).
 * cs_regions_hsv_gate    : out[i] = mask[i] != 0 && max(images_hwc[i][0..3)) <= v_max -- the V-channel gate of preprocess_masks
 *                          (image_processing.py:117-120, v_max = 170) on uint8 [..][3] pixels.  out may be mask.
 * cs_regions_number      : the labelling and numbering of cs_regions_label without the label image -- counts int32 [N] = the number
 *                          of foreground components of every image; the workspace keeps the root of every pixel and the number
 *                          of every root for a cs_regions_measure call with numbered = 1.
 * cs_regions_measure     : one table row per component, row k of image n = component number k + 1, for k < capacity (1 <= capacity
 *                          <= H W); components numbered above capacity are counted in counts and measured nowhere.  area int32
 *                          [N][capacity]; bbox int32 [N][capacity][4] = (r0, c0, r1, c1), half-open (scipy's find_objects);
 *                          sums int64 [N][capacity][2] = the sums of the pixels' rows and columns (center_of_mass = sums / area);
 *                          with intensity (uint8 [N][H][W], or NULL) also isum int64 [N][capacity] and imax int32 [N][capacity],
 *                          the sum and the maximum of the intensity under the component (both required then, else ignored).
 *                          Rows k >= min(counts[n], capacity) are all zero.  numbered = 0 labels and numbers first and writes
 *                          counts; numbered = 1 reads counts and the workspace as cs_regions_number left them for the same mask,
 *                          shape and connectivity, so nothing is labelled twice.  int64 tables are 8-byte aligned. */
size_t cs_regions_workspace(int N, int H, int W);
int cs_regions_label(const uint8_t* mask, int N, int H, int W, int connectivity, int32_t* labels, void* workspace,
                     size_t workspace_bytes, void* stream);
int cs_regions_areas(const uint8_t* mask, int N, int H, int W, int connectivity, int32_t* areas, void* workspace,
                     size_t workspace_bytes, void* stream);
int cs_regions_filter(const uint8_t* mask, int N, int H, int W, int connectivity, int value, int min_area, uint8_t* out,
                      void* workspace, size_t workspace_bytes, void* stream);
int cs_regions_remove_small(const uint8_t* mask, int N, int H, int W, int min_object_size, int hole_area_threshold, int connectivity,
                            uint8_t* out, void* workspace, size_t workspace_bytes, void* stream);
int cs_regions_threshold(const float* probs, long long n, float threshold, uint8_t* out, void* stream);
int cs_regions_hsv_gate(const uint8_t* images_hwc, const uint8_t* mask, long long n_pixels, int v_max, uint8_t* out, void* stream);
int cs_regions_number(const uint8_t* mask, int N, int H, int W, int connectivity, int32_t* counts, void* workspace,
                      size_t workspace_bytes, void* stream);
int cs_regions_measure(const uint8_t* mask, const uint8_t* intensity, int N, int H, int W, int connectivity, int capacity,
                       int numbered, int32_t* counts, int32_t* area, int32_t* bbox, int64_t* sums, int64_t* isum, int32_t* imax,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- touching cells split at detected points, and the tables of a label image (csrc/regions.hip) ---------------------------
 * Masks, sizes, connectivity and the launch contract are those of the section above; in addition H^2 + W^2 < 2^31 (every squared
 * distance fits int32) and P + H W < 2^31.
 * cs_regions_split         : points int64 [P][2] = (row, col) with offsets int64 [N + 1] are out_pts / out_off of cs_detect_cluster as
 *                            they are: image n owns points[offsets[n] .. offsets[n + 1]), and points may hold more rows than
 *                            offsets[N].  limits (int32 [N], or NULL) applies Python's slice [:c] to image n's points as hat_limit of
 *                            cs_score_points does; the S'_n points it keeps are the seeds.  An image whose offsets do not describe
 *                            rows of the buffer (offsets[n] < 0, a negative count, offsets[n + 1] > P) has no seeds: S'_n = 0, as
 *                            such an image has no live point for the spatial entry points.  Seed k (0-based within its image) is live
 *                            when it lies inside the image on a foreground pixel; live uint8 [P] reports that for every row of
 *                            points (0 for the rows that are no seed of any image), and a dead seed owns nothing.  labels int32
 *                            [N][H][W]: 0 on the background; 1 + k on a foreground pixel whose component holds a live seed, k being
 *                            the live seed OF THAT COMPONENT that minimises (dr^2 + dc^2, k) -- a nearer seed in another component
 *                            does not count, ties go to the lower index; S'_n + 1 + j on the pixels of a component without a live
 *                            seed, j = its rank among such components of the image in cs_regions_label's order.  counts int32 [N] =
 *                            S'_n + the number of components without a live seed.  With P = 0 (points, offsets, live may be NULL)
 *                            labels are those of cs_regions_label.  Integer comparisons only: bit-exact and independent of launch
 *                            order.  A Euclidean partition inside each component, not a watershed.  Cost: the labelling, plus
 *                            (foreground pixels) x (live seeds of their component) distance evaluations.  workspace: 16-byte
 *                            aligned, >= cs_regions_split_workspace(N, H, W, P) bytes (0 for sizes a call would refuse).
 * cs_regions_measure_labels: the tables of cs_regions_measure for a label image labels int32 [N][H][W] (<= 0 = background): row k of
 *                            image n belongs to label k + 1, for k < capacity (>= 1, N capacity < 2^31); larger labels are measured
 *                            nowhere.  A row whose label owns no pixel is all zero, bbox (0, 0, 0, 0) included (scipy's find_objects
 *                            gives None there).  counts (int32 [N], or NULL) is WRITTEN: the largest label of every image, also
 *                            above capacity; a caller that knows the counts (cs_regions_split's) passes NULL.  No workspace. */
size_t cs_regions_split_workspace(int N, int H, int W, int P);
int cs_regions_split(const uint8_t* mask, int N, int H, int W, int connectivity, const int64_t* points, const int64_t* offsets,
                     const int32_t* limits, int P, int32_t* labels, int32_t* counts, uint8_t* live, void* workspace,
                     size_t workspace_bytes, void* stream);
int cs_regions_measure_labels(const int32_t* labels, const uint8_t* intensity, int N, int H, int W, int capacity, int32_t* counts,
                              int32_t* area, int32_t* bbox, int64_t* sums, int64_t* isum, int32_t* imax, void* stream);

/* ---- geodesic seeded split: connected cells for non-convex clumps (csrc/regions.hip) ---------------------------------------------
 * cs_regions_split with the distance measured along paths that stay inside the component.  Masks, points, offsets, limits, seeds,
 * live, the components without a live seed, counts and the launch contract are those of cs_regions_split; only the distance changes.
 * Additions to the ABI: cs_abi_version is unchanged.
 * cs_regions_split_geodesic: a step goes from a foreground pixel to a foreground pixel of its 8-neighbourhood; an axial step costs 5
 *                            and a diagonal step 7.  With connectivity 2 every such step is allowed; with connectivity 1 a diagonal
 *                            step (r, c) -> (r + dr, c + dc) only if (r + dr, c) or (r, c + dc) is foreground, so that no step leaves
 *                            the component.  dist(p, k) = the cheapest path from the pixel of live seed k to p; p gets label 1 + k
 *                            for the k that minimises (dist(p, k), k).  Every cell is therefore connected in the 8-neighbourhood and
 *                            holds its seed pixel.  Need 7 H W < 2^31 (every distance fits int32).
 *                            The keys (dist, k) of all pixels are lowered to that fixpoint by `rounds` (>= 1) rounds of one launch
 *                            each; converged uint8 [N] = no key of image n changed in the last round run, i.e. the labels ARE the
 *                            rule's.  Of an image that has not converged only this holds: every label is 0, a live seed of the
 *                            pixel's component or the number of a component without one, and converged[n] = 0.  resume != 0: the
 *                            workspace is as an earlier call with the same arguments left it; `rounds` more rounds run on it and
 *                            labels, distance and converged are written again (counts and live are not).  The first round of a call
 *                            visits every tile that holds foreground, a later one only the tiles near a change of the round before.
 *                            distance (int32 [N][H][W], or NULL): the cost to the owner; 0 on the background, -1 in a component
 *                            without a live seed and on a pixel no round has reached yet.  Integer comparisons only: the converged
 *                            result is bit-exact and independent of launch order.  The number of launches depends on (N, H, W), on
 *                            P > 0 and on rounds alone.  workspace: 16-byte aligned, >= cs_regions_geodesic_workspace(N, H, W, P)
 *                            bytes (0 for sizes a call would refuse): cs_regions_split's plus 8 bytes per pixel and 2 per tile. */
size_t cs_regions_geodesic_workspace(int N, int H, int W, int P);
int cs_regions_split_geodesic(const uint8_t* mask, int N, int H, int W, int connectivity, const int64_t* points, const int64_t* offsets,
                              const int32_t* limits, int P, int rounds, int resume, int32_t* labels, int32_t* counts, uint8_t* live,
                              int32_t* distance /* may be NULL */, uint8_t* converged, void* workspace, size_t workspace_bytes,
                              void* stream);

/* ---- the shape of every object of a label image: boundary map, second moments, perimeter tallies (csrc/regions.hip) ---------
 * labels int32 [N][H][W]; a pixel's object id is max(label, 0), images are independent; sizes and the launch contract as above (the
 * grids depend on (N, H, W, capacity) alone, no synchronisation, capturable); no workspace.  Additions to the ABI: cs_abi_version
 * is unchanged.
 * cs_regions_edges_labels: edges uint8 [N][H][W], 1 on the edge pixels, else 0.  An edge pixel has a positive id and at least one
 *                          of its four neighbours has another id, a neighbour outside the image having id 0: per object, the object
 *                          minus its erosion by the 4-neighbourhood with border value 0.  Another positive label is "not this
 *                          object".  One launch.
 * cs_regions_shape_labels: edges is READ, as cs_regions_edges_labels wrote it for the same labels; bbox int32 [N][capacity][4] is
 *                          READ, as cs_regions_measure_labels wrote it for the same labels and capacity.  Row k of image n belongs
 *                          to label k + 1, for k < capacity; larger labels are measured nowhere (they still are objects for the
 *                          edge rule), and the row of a label without a pixel is all zero.
 *                          moments int64 [N][capacity][3] = (Sxx, Syy, Sxy) = the sums of x^2, y^2 and x y over the label's pixels
 *                          with x = r - bbox[0], y = c - bbox[1]: relative to the box so that the central moments formed from them
 *                          in float64 do not cancel on a large image; the sums of x and y follow from cs_regions_measure_labels'
 *                          sums, area and bbox.
 *                          tallies int32 [N][capacity][4] = (edge pixels, straight, diagonal, mixed).  For an edge pixel of object
 *                          l let n4 / nd be the number of its 4-neighbours / diagonal neighbours that are edge pixels of l too and
 *                          code = 1 + 2 n4 + 10 nd: straight = codes 5, 7, 15, 17, 25, 27; diagonal = 21, 33; mixed = 13, 23; any
 *                          other code is counted as an edge pixel only.  perimeter = straight + sqrt(2) diagonal + (1 + sqrt(2)) / 2
 *                          mixed is the 4-neighbourhood perimeter estimate.
 *                          Integer atomics only: independent of launch and arrival order.  Need capacity >= 1, N capacity < 2^31 and
 *                          H, W <= 32768, so that Sxx <= area (H - 1)^2 < 2^61.  Two launches. */
int cs_regions_edges_labels(const int32_t* labels, int N, int H, int W, uint8_t* edges, void* stream);
int cs_regions_shape_labels(const int32_t* labels, const uint8_t* edges, int N, int H, int W, int capacity, const int32_t* bbox,
                            int64_t* moments, int32_t* tallies, void* stream);

/* ---- how strongly every object of a label image is stained: per-cell tables of integer stain levels (csrc/regions.hip) ------
 * One pass over images uint8 [N][H][W][3] (RGB, any alignment), labels int32 [N][H][W] and, where not NULL, expanded int32
 * [N][H][W] (cs_morph_expand_labels of the labels); sizes and the launch contract are those of cs_regions_measure_labels (two
 * launches whose grids depend on (N, H, W, capacity, K, bins) alone, no synchronisation, capturable); no workspace.  Additions to
 * the ABI: cs_abi_version is unchanged.  All rules are exact integers:
 *   owner     a pixel belongs to (row labels - 1, compartment 0) where labels > 0, else to (row expanded - 1, compartment 1)
 *             where expanded is given and > 0, else to nothing.  C = 1 compartment without expanded, 2 with it.
 *   level     of stain s < K (K = 2 or 3) at a pixel of image n with the bytes (R, G, B):
 *             clamp((Mq[n][s][0] od_q[R] + Mq[n][s][1] od_q[G] + Mq[n][s][2] od_q[B] + 2^23) >> 24, 0, 255), the sum in int64,
 *             the shift arithmetic; od_q int32 [256] (device), Mq int32 [N][K][3] (device).
 *   tables    n int32 [N][capacity][C]; sum, sumsq int64 and max, pos int32 [N][capacity][C][K]: over the pixels of (row,
 *             compartment) their number and per stain the sum, the sum of squares and the maximum of the level and the number
 *             of pixels with level >= pos_levels[s] (HOST int32 [K], each in [0, 256]; NULL = 256 everywhere: pos stays 0);
 *             hist int32 [N][capacity][C][K][bins], the pixels per bin = level * bins >> 8, with bins in {16, 32, 64, 128,
 *             256}; bins = 0 goes with hist = NULL.  Every table is zeroed by the call.
 *   counts    (int32 [N], or NULL) is WRITTEN: the largest label that owns a pixel of the image, also above the capacity; rows
 *             at or above the capacity are measured nowhere.
 * Integer atomics only: independent of launch and arrival order.  Need capacity >= 1 and N capacity C K max(bins, 1) < 2^31;
 * labels, expanded, od_q, Mq on 4-byte and sum, sumsq on 8-byte boundaries. */
int cs_stain_quantify_labels(const uint8_t* images_hwc, const int32_t* labels, const int32_t* expanded /* may be NULL */, int N, int H,
                             int W, const int32_t* od_q, const int32_t* Mq, int K, const int32_t* pos_levels /* host, may be NULL */,
                             int bins, int capacity, int32_t* counts /* may be NULL */, int32_t* n, int64_t* sum, int64_t* sumsq,
                             int32_t* max, int32_t* pos, int32_t* hist /* NULL iff bins == 0 */, void* stream);

/* ---- the convex hull of every object of a label image: vertex count, area, Feret diameters (csrc/regions.hip) ----------------
 * labels int32 [N][H][W]; a pixel's object id is max(label, 0), images are independent, a label need not be connected; sizes as
 * above.  One launch whose grid depends on (N, capacity) alone, no synchronisation, capturable; no workspace and no atomics.
 * Additions to the ABI: cs_abi_version is unchanged.
 * cs_regions_hull_max_side: 1024, the largest number of rows or columns of a bounding box that is still measured.
 * cs_regions_hull_labels:   bbox int32 [N][capacity][4] is READ, as cs_regions_measure_labels wrote it for the same labels and
 *                           capacity (it is cut to the image before a pixel is read).  Row k of image n belongs to label k + 1,
 *                           for k < capacity; larger labels are measured nowhere.  An object is the union of the closed unit
 *                           squares of its pixels, pixel (r, c) having the corners (r, c), (r + 1, c), (r, c + 1), (r + 1, c + 1);
 *                           the hull is the convex hull of those lattice points, so it has at least 4 vertices and positive area.
 *                           hull int32 [N][capacity][5] = (n_vertices, area2, feret_max2, width_cross, width_len2):
 *                             n_vertices  the strict vertices (no three consecutive ones collinear);
 *                             area2       twice the area of the hull (shoelace formula);
 *                             feret_max2  the largest squared distance between two vertices;
 *                             width_*     of the hull edge e = a -> b that minimises (cross^2 / len2, len2), len2 = |b - a|^2 and
 *                                         cross = the maximum over the vertices v of |(b - a) x (v - a)|, the fractions compared by
 *                                         cross-multiplication in unsigned 64-bit integers: the minimum width is
 *                                         width_cross / sqrt(width_len2).
 *                           The row of a label without a pixel (box (0, 0, 0, 0)) is all zero; the row of a label whose box has
 *                           more than cs_regions_hull_max_side rows or columns is all -1.  Within that limit cross <= 2^21 and
 *                           len2 <= 2^21: every compared product is below 2^64 and every entry fits int32.
 *                           Need capacity >= 1 and N capacity < 2^31. */
int cs_regions_hull_max_side(void);
int cs_regions_hull_labels(const int32_t* labels, int N, int H, int W, int capacity, const int32_t* bbox, int32_t* hull, void* stream);

/* ---- the outer boundary of every object of a label image as an ordered polygon (csrc/regions.hip) ----------------------------
 * labels int32 [N][H][W]; a pixel's object id is max(label, 0), images are independent; sizes as above.  One launch whose grid
 * depends on (N, capacity) alone, no synchronisation, capturable; no workspace and no atomics, every element of both outputs is
 * written.  Additions to the ABI: cs_abi_version is unchanged.
 * cs_regions_contour_max_side: 512, the largest number of rows or columns of a bounding box that is still traced.
 * cs_regions_contour_labels:   bbox int32 [N][capacity][4] is READ, as cs_regions_measure_labels wrote it for the same labels
 *                              and capacity (it is cut to the image before a pixel is read).  Row k of image n belongs to label
 *                              k + 1.  The object of label l is the pixels with id l INSIDE its box; pixel (r, c) is the closed
 *                              unit square with the lattice corners (r, c) and (r + 1, c + 1).  A crack is a unit side of a pixel
 *                              of the object whose neighbour across it is not in the object.  The ring starts at the lattice
 *                              vertex (pr, pc) of the object's first pixel in row-major order, heading east along that pixel's top
 *                              side with the object on the right hand, and moves one crack at a time.  At the vertex reached, with
 *                              R the pixel ahead on the right and L the one ahead on the left: R out -> turn right (connectivity
 *                              2 and L in -> turn left instead); R and L in -> turn left; R in, L out -> straight.  It ends on
 *                              arriving at (pr, pc) with the new heading east, or after 2 rows cols + rows + cols steps (the
 *                              cracks of the box), which a consistent walk never needs.  A vertex is emitted where the heading
 *                              changes, (pr, pc) first: edges alternate horizontal and vertical, n_vertices is even and >= 4.
 *                              Only this ring -- the outer boundary of the 4- (connectivity 1) or 8-connected (2) component
 *                              of the first pixel -- is traced: no holes, no further pieces of the label.
 *                              contour int32 [N][capacity][4] = (n_vertices, n_cracks, area2, cracks_all):
 *                                n_vertices  the ring's vertices, the true count also above max_vertices;
 *                                n_cracks    the ring's length;
 *                                area2       twice the area the ring encloses (shoelace sum, positive);
 *                                cracks_all  all cracks of the label: == n_cracks iff the label is one piece without a hole.
 *                              vertices int32 [N][capacity][max_vertices][2] = (row, col), absolute lattice coordinates: the
 *                              first min(n_vertices, max_vertices) vertices of the ring, then (-1, -1).  vertices == NULL with
 *                              max_vertices == 0 only counts.
 *                              The row of a label without a pixel in its box is all zero; the row of a label whose box has more
 *                              than cs_regions_contour_max_side rows or columns is all -1; both have no vertex.
 *                              Need capacity >= 1, N capacity < 2^31, connectivity 1 or 2, max_vertices >= 0 and
 *                              2 N capacity max_vertices < 2^31. */
int cs_regions_contour_max_side(void);
int cs_regions_contour_labels(const int32_t* labels, int N, int H, int W, int capacity, const int32_t* bbox, int connectivity,
                              int max_vertices, int32_t* contour, int32_t* vertices, void* stream);

/* ---- how a stain is arranged inside every object of a label image: grey-level co-occurrence tables (csrc/regions.hip) --------
 * labels int32 [N][H][W] and bbox int32 [N][capacity][4] as for cs_regions_hull_labels (the box is READ and cut to the image; every
 * read stays inside the image whatever it holds).  One launch whose grid depends on (N, capacity) alone, no synchronisation,
 * capturable; no workspace, no global atomics, every element of every table is written.  An addition to the ABI: cs_abi_version
 * is unchanged.  All rules are exact integers:
 *   level     of a pixel, in 0 .. 255.  Exactly one of plane and images_hwc is not NULL: plane uint8 [N][H][W] gives the byte;
 *             images_hwc uint8 [N][H][W][3] (RGB, any alignment) comes with od_q int32 [256] and Mq int32 [N][3] (ONE stain row
 *             per image, both on the device; NULL with a plane) and gives clamp((Mq[n][0] od_q[R] + Mq[n][1] od_q[G] +
 *             Mq[n][2] od_q[B] + 2^23) >> 24, 0, 255), the sum in int64, the shift arithmetic (cs_stain_quantify_labels' level).
 *   grey      g = level * levels >> 8 with levels = L in {8, 16, 32}.
 *   offsets   direction k = 0 .. 3 is (dr, dc) = (0, d), (d, d), (d, 0), (d, -d) with d = distance in 1 .. 8.
 *   pairs     a pixel p with 0 < labels[p] = l <= capacity pairs with q = p + (dr, dc) where q lies inside the image and
 *             labels[q] == l: C_k[g(p)][g(q)] += 1.  A label need not be connected.  S_k = C_k + C_k^T.
 *   tables    per (image, row = l - 1, direction): pairs int32 [N][capacity][4] the number of pairs; diff int32
 *             [N][capacity][4][L], diff[x] = the sum of S_ij over |i - j| = x; sum int32 [N][capacity][4][2L - 1], sum[x] = the
 *             same over i + j = x; marg int32 [N][capacity][4][L], marg[i] = the sum of S_ij over j; sq int64 [N][capacity][4]
 *             = the sum of S_ij^2; cross int64 [N][capacity][4] = the sum of i j S_ij; matrix (may be NULL) int32
 *             [N][capacity][4][L][L] = S.  A label without a pixel, or a direction without a pair, is all zero.
 * Need capacity >= 1, H W <= 2^30 (then every count is below 2^31, sq < 2^62, cross < 2^41), N capacity 4 (2L - 1) < 2^31 and with
 * the matrix N capacity 4 L^2 < 2^31; the int32 operands on 4-byte and sq, cross on 8-byte boundaries. */
int cs_regions_texture_labels(const int32_t* labels, const uint8_t* plane, const uint8_t* images_hwc, const int32_t* od_q,
                              const int32_t* Mq, int N, int H, int W, int capacity, const int32_t* bbox, int levels, int distance,
                              int32_t* pairs, int32_t* diff, int32_t* sum, int32_t* marg, int64_t* sq, int64_t* cross,
                              int32_t* matrix /* may be NULL */, void* stream);

/* ---- a label image scored against another at the object level (csrc/regions.hip) --------------------------------------------
 * pred, truth int32 [N][H][W], values <= 0 = background; sizes and the launch contract as above (a fixed number of launches for
 * given (N, H, W, cap_pred, cap_truth), no synchronisation, capturable).  For image n let Ap[p] / At[g] be the pixel counts of
 * pred label p / truth label g, I(p, g) the pixels that carry both and U = Ap[p] + At[g] - I.  p and g are MATCHED iff
 * 2 I(p, g) > U, strictly, compared in 64-bit integers (IoU > 1/2; IoU exactly 1/2 is no match).  With the strict inequality a
 * label has at most one partner on the other side, so there is no assignment problem and no float decides anything.  A pixel
 * whose label exceeds its side's capacity is background on that side.  Outputs: area_pred int32 [N][cap_pred] (row p - 1 = Ap[p]);
 * area_truth int32 [N][cap_truth]; match int32 [N][cap_pred] = the matched truth label, 0 = none; inter int32 [N][cap_pred] =
 * I(p, match), 0 where unmatched; match_truth int32 [N][cap_truth] = the matched pred label, 0 = none.  counts_pred / counts_truth
 * (int32 [N], or NULL) are WRITTEN: the largest label of every image on that side, also above the capacity.  A label that owns no
 * pixel has area 0 and no match.  All integer and independent of launch order: two runs give the same bits.
 * Need cap_pred, cap_truth >= 1, N cap_pred B < 2^31 with B = max(1, bit_length(cap_truth)), N cap_truth < 2^31.  workspace:
 * 16-byte aligned, >= cs_regions_match_workspace(N, cap_pred, cap_truth) bytes (0 for sizes a call would refuse): 4 N cap_pred
 * (B + 1) bytes and padding, never a cap_pred x cap_truth table. */
size_t cs_regions_match_workspace(int N, int cap_pred, int cap_truth);
int cs_regions_match_labels(const int32_t* pred, const int32_t* truth, int N, int H, int W, int cap_pred, int cap_truth,
                            int32_t* counts_pred, int32_t* counts_truth, int32_t* area_pred, int32_t* area_truth, int32_t* match,
                            int32_t* inter, int32_t* match_truth, void* workspace, size_t workspace_bytes, void* stream);

/* ---- every overlapping pair of two label images, and each label's best partner (csrc/regions.hip) ----------------------------
 * pred, truth, the treatment of labels (<= 0 and above the side's capacity = background; counts_pred / counts_truth, int32 [N] or
 * NULL, WRITTEN with the largest labels), area_pred, area_truth and the launch contract are those of cs_regions_match_labels.
 * I(p, g) = the pixels of image n that carry pred label p and truth label g, both within capacity.  The pairs with I > 0 are held
 * in a per-image open-addressing hash table of slots = the smallest power of two >= 2 max_pairs entries at the START of the
 * workspace: keys uint64 [N][slots], key = (p << 32) | g, 0 = empty, then counts int32 [N][slots] = I(p, g); the caller may read
 * both after the call (the rest of the workspace is scratch).  Which slot a pair occupies may differ from run to run; the set of
 * (key, count) and every output below do not.  Probing is bounded by slots: a run of pixels whose pair finds no slot is left out
 * and adds 1 to dropped[n] (int32 [N]) -- the pair list and the partners of image n are then incomplete; the areas are not.
 * n_pairs int32 [N] = the occupied slots.  Per truth label g (row g - 1 of [N][cap_truth] int32 tables):
 *   iou_partner / iou_inter: the pred label p with I(p, g) > 0 that maximises I / (Ap[p] + At[g] - I), fractions compared by
 *     cross-multiplication in 64-bit integers, ties to the lower p; 0 = none; and I(p, g).
 *   inter_partner_truth / inter_truth: the pred label of largest I(p, g), ties to the lower p; 0 = none; and that I.
 * Per pred label p ([N][cap_pred]): inter_partner_pred / inter_pred: the truth label of largest I(p, g), ties to the lower g.
 * All integer and independent of launch and arrival order.  Need cap_pred, cap_truth >= 1, 1 <= max_pairs <= 2^29, N cap_pred,
 * N cap_truth, N slots < 2^31.  workspace: 16-byte aligned, >= cs_regions_overlap_workspace(N, cap_pred, cap_truth, max_pairs)
 * bytes (0 for sizes a call would refuse): 12 N slots + 8 N (2 cap_truth + cap_pred) bytes and padding, never a cap_pred x
 * cap_truth table.  Four launches. */
size_t cs_regions_overlap_workspace(int N, int cap_pred, int cap_truth, int max_pairs);
int cs_regions_overlap_labels(const int32_t* pred, const int32_t* truth, int N, int H, int W, int cap_pred, int cap_truth,
                              int max_pairs, int32_t* counts_pred, int32_t* counts_truth, int32_t* area_pred, int32_t* area_truth,
                              int32_t* n_pairs, int32_t* dropped, int32_t* iou_partner, int32_t* iou_inter,
                              int32_t* inter_partner_truth, int32_t* inter_truth, int32_t* inter_partner_pred, int32_t* inter_pred,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ---- which labels of one label image touch which: adjacency tables (csrc/regions.hip) ------------------------------------------
 * labels int32 [N][H][W], images independent; sizes and the launch contract are those of cs_regions_measure_labels.  All rules are
 * exact integers:
 *   id        a pixel's id is its label where 1 <= label <= capacity, else 0: a label above the capacity is background here.  counts
 *             (int32 [N] or NULL) is WRITTEN with the largest label of every image, also above the capacity.
 *   sides     every unordered pair of 4-adjacent pixels of the image is one interior side; a pixel side on the image edge is an
 *             exterior side of that pixel.
 *   per pair of labels a < b, both positive: sides(a, b) = the interior sides whose two ids are {a, b}; corners(a, b), counted with
 *             connectivity 2 only (else 0), = the unordered diagonal pixel pairs {(r, c), (r + 1, c + 1)} and {(r, c + 1), (r + 1, c)}
 *             whose ids are {a, b}, whether or not the two labels also share a side.  A pair is listed iff sides > 0 (connectivity 1)
 *             or sides + corners > 0 (connectivity 2).
 *   per label a (row a - 1 of the int32 [N][capacity] tables): n_neighbors = the listed pairs that contain a; contact = the sum of
 *             sides over them; background = the interior sides with ids {a, 0}; outside = the exterior sides of a's pixels; partner /
 *             partner_sides = the listed neighbour of largest sides, ties to the lower label, and that count (a neighbour met at
 *             corners only has 0 sides); partner 0 = no neighbour.  A label without pixels has an all-zero row.
 *   identity  contact + background + outside = 4 area - 2 (interior sides with both ids a): the crack length of the label.
 * The listed pairs are held as cs_regions_overlap_labels holds its pairs, in a per-image open-addressing table of slots = the smallest
 * power of two >= 2 max_pairs entries at the START of the workspace: keys uint64 [N][slots], key = (a << 32) | b, 0 = empty, then
 * sides int32 [N][slots], then corners int32 [N][slots]; the caller may read the three after the call.  n_pairs int32 [N] = the
 * occupied slots; a run of sides or corners whose pair finds no slot is left out and adds 1 to dropped[n] (int32 [N]) -- the pair
 * list, n_neighbors, contact and partner of image n are then incomplete (never too large); background and outside are not.  Which
 * slot a pair occupies may differ from run to run; everything else is integer sums and maxima under a total order, independent of
 * launch and arrival order.  The counts are int32: an image of fewer than 2^29 pixels cannot overflow them.  Need capacity >= 1,
 * 1 <= max_pairs <= 2^29, connectivity 1 or 2, N capacity < 2^31 and N slots < 2^31.  workspace: 16-byte aligned, >=
 * cs_regions_adjacency_workspace(N, capacity, max_pairs) bytes (0 for sizes a call would refuse): 16 N slots + 8 N capacity bytes
 * and padding.  Four launches. */
size_t cs_regions_adjacency_workspace(int N, int capacity, int max_pairs);
int cs_regions_adjacency_labels(const int32_t* labels, int N, int H, int W, int capacity, int max_pairs, int connectivity,
                                int32_t* counts, int32_t* n_pairs, int32_t* dropped, int32_t* n_neighbors, int32_t* contact,
                                int32_t* background, int32_t* outside, int32_t* partner, int32_t* partner_sides, void* workspace,
                                size_t workspace_bytes, void* stream);

/* ---- the seed label image of a ragged point set (csrc/regions.hip, csrc/cs_points.h) -----------------------------------------
 * points int64 [P][2] (row, col), offsets int64 [N + 1], limits int32 [N] or NULL as cs_regions_split takes them.  labels int32
 * [N][H][W] is WRITTEN: 0 everywhere, and k + 1 at the pixel of point k of its image where that point is within its image's limit and
 * inside the image; of several such points on one pixel the lowest k.  Three launches (one without points), nothing synchronises. */
int cs_regions_seed_labels(const int64_t* points, const int64_t* offsets, const int32_t* limits, long long P, int N, int H, int W,
                           int32_t* labels, void* stream);

/* ---- the squared Hausdorff distance of every object of two label images to its partner (csrc/regions.hip) -------------------
 * pred, truth, the treatment of labels (<= 0 and above the side's capacity = background) and the launch contract are those of
 * cs_regions_overlap_labels; an object is a label that owns a pixel.  For pixel sets A, B of image n: d2(A -> B) = the maximum over
 * ALL pixels a of A (not its boundary) of the minimum over the pixels b of B of dr^2 + dc^2; H2(A, B) = max(d2(A -> B), d2(B -> A)).
 * inter_partner_truth int32 [N][cap_truth] / inter_partner_pred int32 [N][cap_pred] are READ: the tables of that name written by
 * cs_regions_overlap_labels for the same pair and capacities.  Per truth label g (row g - 1 of [N][cap_truth] int32 tables):
 *   partner_truth: inter_partner_truth where that is an object of pred; otherwise the pred object of smallest H2(g, p), ties to the
 *     lower p; 0 where g is no object or pred has none.   d2_truth: H2 with that partner, -1 where partner_truth is 0.
 * Per pred label p ([N][cap_pred]): partner_pred / d2_pred, the same over the truth labels.  A partner value outside
 * [1, capacity] or naming a label without a pixel counts as none.  All integer and independent of launch and arrival order.
 * One workgroup per (object, partner or candidate) computes both directions: for A -> B the horizontal runs of B are staged in
 * LDS, cs_regions_hausdorff_stage_runs() at a time (an object with more is taken in chunks), and every pixel of A's bounding box
 * that is A's takes its minimum over them: about |box of A| runs(B) + |box of B| runs(A) distance evaluations per pair.  An
 * object without a given partner is held against every object of the other side that the bounding boxes do not rule out (the
 * edges of two boxes bound H2 from below, the box around both from above): one box test per object of the other side and one pair
 * per object that passes -- which of them a finished pair spares depends on the order of arrival, the result does not.
 * Need cap_pred, cap_truth >= 1, N (cap_pred + cap_truth) < 2^31 and (H - 1)^2 + (W - 1)^2 < 2^31 (d2 is int32).  workspace:
 * 16-byte aligned, >= cs_regions_hausdorff_workspace(N, cap_pred, cap_truth) bytes (0 for sizes a call would refuse): 32 bytes per
 * label of either side and padding, never a cap_pred x cap_truth table.  Six launches whose grids depend on the sizes alone. */
int cs_regions_hausdorff_stage_runs(void);
size_t cs_regions_hausdorff_workspace(int N, int cap_pred, int cap_truth);
int cs_regions_hausdorff_labels(const int32_t* pred, const int32_t* truth, int N, int H, int W, int cap_pred, int cap_truth,
                                const int32_t* inter_partner_truth, const int32_t* inter_partner_pred, int32_t* partner_truth,
                                int32_t* d2_truth, int32_t* partner_pred, int32_t* d2_pred, void* workspace, size_t workspace_bytes,
                                void* stream);

/* ---- detected points against annotated points (test_seg.py:120-141 get_prf1, metrics/metrics.py:56-66; csrc/score.hip) ------
 * N images that share nothing, 0 < N <= 65535.  hat int64 [T][2] with hat_off int64 [N + 1] are out_pts / out_off of
 * cs_detect_cluster as they are; gt int32 [G][2] with gt_off int64 [N + 1] are the annotations, in the same coordinate convention.
 * Per image, in the order of the detections: a detection takes the annotation of smallest dr^2 + dc^2 among those no earlier
 * detection has taken (the lowest index among equals) and keeps it when that is <= radius2 (0 <= radius2 < 2^31); otherwise it is
 * a false positive, also when a nearer annotation is already taken.  Integer comparisons only: bit-exact and independent of
 * scheduling.  A detection whose coordinate does not fit int32 matches nothing.
 * hat_limit (int32 [N], or NULL) applies Python's slice [:c] to image n's detections: c >= 0 keeps min(c, n_hat), c < 0 keeps
 * max(n_hat + c, 0); the rest are not scored (they are no false positives) and get match = -2.
 * counts int32 [N][3] = (tp, fp, fn): matches, detections scored - tp, annotations left untaken.  match (int32 [hat_off[N]], or
 * NULL): the annotation index within the detection's own image, -1 for a false positive.  An image whose offsets do not describe
 * 0 <= n < 2^31 points, or whose flags would not fit the workspace, reports counts (-1, -1, -1).
 * flags bit 0 forces the 256-thread block path on images of at most 64 annotations, which one wave scores otherwise (tests).
 * One launch, no host synchronisation.  workspace: 16-byte aligned, >= cs_score_workspace(N, total_gt) bytes with
 * total_gt >= gt_off[N] (0 for an N a call would refuse); its contents on entry do not matter. */
size_t cs_score_workspace(int N, long long total_gt);
int cs_score_points(const int64_t* hat, const int64_t* hat_off, const int32_t* hat_limit, const int32_t* gt, const int64_t* gt_off, int N,
                    int radius2, int flags, int32_t* counts, int32_t* match, void* workspace, size_t workspace_bytes, void* stream);

/* ---- neighbourhood queries over integer points on a bucket grid (csrc/spatial.hip) ------------------------------------------
 * N images that share nothing, 0 < N <= 65535, all H x W with H^2 + W^2 < 2^31.  pts int64 [P][2] = (row, col) with off int64
 * [N + 1] are out_pts / out_off of cs_detect_cluster as they are (the buffer may hold more rows than off[N]); limit (int32 [N], or
 * NULL) applies Python's slice [:c] as hat_limit of cs_score_points does.  A point is LIVE when its limit keeps it and it lies
 * inside [0, H) x [0, W); only live points ask or answer.  The targets are the points themselves (other_off NULL; then other and
 * other_limit are NULL and P_other is 0: a row is never its own neighbour, another row at the same coordinates is one at
 * distance 0) or a second set other / other_off / other_limit / P_other of the same layout (flags bit 0: its rows are (col, row));
 * an index is the target's index within its image.  An image whose offsets do not describe rows of its buffer has no live point.
 * bucket: the side in pixels of the square buckets, >= 1 (a side above max(H, W) means one bucket); N ceil(H / bucket)
 * ceil(W / bucket) may not exceed cs_spatial_max_buckets().  No result depends on it.
 * cs_spatial_nearest      : index, d2 int32 [P][k], 1 <= k <= 8: column j of a live row holds the (j + 1)-th smallest key (d2, index)
 *                           among the live targets of its image, (-1, -1) beyond their number; every other row holds (-2, -1).
 * cs_spatial_count_within : radii2 (host) int32 [n_radii], 1 <= n_radii <= 8, each >= 0.  counts int32 [P][n_radii]: the live
 *                           targets with d2 <= radii2[j], the row itself excluded when the targets are the points; -1 in the rows
 *                           that are not live.  pair_counts int64 [N][n_radii]: the sums of counts over the live rows of each image.
 * cs_spatial_bin_counts   : out int32 [N][ceil(H / bin)][ceil(W / bin)]: the live points per square bin, the grid's own count pass
 *                           (the same cap on the number of bins).  No workspace.
 * A fixed sequence of launches on one stream for given (P, P_other, N, H, W, bucket, k), no host synchronisation: capturable.
 * workspace: 16-byte aligned, >= cs_spatial_workspace(N, H, W, bucket, P, P_other) bytes, P_other = -1 without a second set
 * (0 for sizes a call would refuse); its contents on entry do not matter.  cs_spatial_threads / cs_spatial_chunk: the workgroup
 * width of the query kernels and the number of candidate records they stage in LDS at a time (the tests size their cases by them). */
int cs_spatial_threads(void);
int cs_spatial_chunk(void);
long long cs_spatial_max_buckets(void);
size_t cs_spatial_workspace(int N, int H, int W, int bucket, long long P, long long P_other);
int cs_spatial_nearest(const int64_t* pts, const int64_t* off, const int32_t* limit, long long P, const int64_t* other,
                       const int64_t* other_off, const int32_t* other_limit, long long P_other, int N, int H, int W, int bucket, int k,
                       int flags, int32_t* index, int32_t* d2, void* workspace, size_t workspace_bytes, void* stream);
int cs_spatial_count_within(const int64_t* pts, const int64_t* off, const int32_t* limit, long long P, const int64_t* other,
                            const int64_t* other_off, const int32_t* other_limit, long long P_other, int N, int H, int W, int bucket,
                            const int32_t* radii2, int n_radii, int flags, int32_t* counts, int64_t* pair_counts, void* workspace,
                            size_t workspace_bytes, void* stream);
int cs_spatial_bin_counts(const int64_t* pts, const int64_t* off, const int32_t* limit, long long P, int N, int H, int W, int bin,
                          int32_t* out, void* stream);

/* ---- density-based clustering (DBSCAN) of the live points of every image, on the same grid (csrc/spatial.hip) -----------------
 * pts / off / limit / P / N / H / W / bucket and LIVE as above; the result equals sklearn.cluster.DBSCAN(eps, min_samples) with
 * radius2 = floor(eps^2) >= 0 and min_samples >= 1, image by image:
 *   core point : a live point i with 1 + #(live points j != i of its image with d2(i, j) <= radius2) >= min_samples -- it counts
 *                itself, and another row at the same coordinates is a neighbour at distance 0;
 *   cluster    : core points joined by a chain of core points whose steps all have d2 <= radius2; the clusters of an image are
 *                numbered 0 .. C - 1 in increasing order of the smallest index that a core point of the cluster has;
 *   border     : a live point that is not core but has a core point within radius2 takes the lowest cluster number among those
 *                core points' clusters (it never joins two clusters); every other live point is noise.
 * labels int32 [P]: the cluster number, -1 noise, -2 in the rows that are not live.  core uint8 [P]: 1 on core points, else 0.
 * n_clusters int32 [N].  The tables have P rows and use the points' own offsets: cluster c of image n is row off[n] + c (an image
 * never has more clusters than points, so there is no capacity and no overflow).  size int32 [P]: core plus border points; n_core
 * int32 [P]; sums int64 [P][2] = (sum of rows, sum of columns); bbox int32 [P][4] = r0, c0, r1, c1 (half-open, as
 * cs_regions_measure).  Every other table row is all zero.  Nothing depends on bucket, the launch order or thread timing.
 * A fixed sequence of launches on one stream for given (P, N, H, W, bucket), no host synchronisation: capturable.  pts, off and
 * sums 8-byte, the int32 outputs 4-byte aligned; pts and every output but n_clusters may be NULL when P == 0.  workspace: 16-byte
 * aligned, >= cs_spatial_cluster_workspace(N, H, W, bucket, P) bytes (0 for sizes a call would refuse); its contents on entry do
 * not matter. */
size_t cs_spatial_cluster_workspace(int N, int H, int W, int bucket, long long P);
int cs_spatial_cluster(const int64_t* pts, const int64_t* off, const int32_t* limit, long long P, int N, int H, int W, int bucket,
                       int radius2, int min_samples, int32_t* labels, uint8_t* core, int32_t* n_clusters, int32_t* size, int32_t* n_core,
                       int64_t* sums, int32_t* bbox, void* workspace, size_t workspace_bytes, void* stream);

/* ---- tissue detection for whole-slide streaming (csrc/tissue.hip) -----------------------------------------------------------
 * images_hwc uint8 [N][H][W][3] (RGB), 0 < N <= 65535, 0 < H W < 2^31; pixel offsets are 64-bit, N H W 3 may pass 2^31.  No
 * alignment is asked of the images or the masks.  The pixel feature f(r, g, b) in [0, 255] is selected by `channel`:
 *   CS_TISSUE_CHROMA    max(r, g, b) - min(r, g, b)                      white glass, grey shadow and black pen all score low
 *   CS_TISSUE_DARKNESS  255 - ((77 r + 150 g + 29 b + 128) >> 8)
 * All arithmetic is integer and every result is a sum or a comparison of integers: nothing depends on the launch geometry.
 * cs_tissue_histogram : hist int64 [N][256] += the number of pixels of image n with f = v.  It ADDS: the caller zeroes hist.
 * cs_tissue_mask      : mask uint8 [N][H][W] = f > thr[n] as 0 / 1; thr int32 [N] is a DEVICE array (a threshold computed on the
 *                       device needs no round trip); the feature channel is never written anywhere.
 * cs_tissue_coverage  : cover int32 [T] = the non-zero pixels of mask uint8 [N][H][W] in the window [r, r + ph) x [c, c + pw) of image
 *                       tile_img[t], (r, c) = tile_rc[t] (int32 [T] and [T][2] on the device, the convention of cs_tile_gather);
 *                       the window is clamped to the image and an image index outside [0, N) counts 0.  ph, pw > 0, 0 <= T < 2^31.
 * cs_tissue_select    : selected int32 [T] = the indices t with cover[t] >= min_pixels in rising order, -1 from their number on;
 *                       n_selected int32 [1] = their number.  One workgroup; T is a number of patches.
 * One launch each on `stream`, no workspace, no host synchronisation: capturable. */
#define CS_TISSUE_CHROMA 0
#define CS_TISSUE_DARKNESS 1
int cs_tissue_histogram(const uint8_t* images_hwc, int N, int H, int W, int channel, int64_t* hist, void* stream);
int cs_tissue_mask(const uint8_t* images_hwc, int N, int H, int W, int channel, const int32_t* thr, uint8_t* mask, void* stream);
int cs_tissue_coverage(const uint8_t* mask, int N, int H, int W, const int32_t* tile_img, const int32_t* tile_rc, long long T, int ph,
                       int pw, int32_t* cover, void* stream);
int cs_tissue_select(const int32_t* cover, long long T, int min_pixels, int32_t* selected, int32_t* n_selected, void* stream);

/* ---- stain separation and Macenko stain normalisation (csrc/stain.hip) --------------------------------------------------------
 * images_hwc uint8 [N][H][W][3] (RGB) as for the tissue entry points: 0 < N <= 65535, 0 < H W < 2^31, 64-bit pixel offsets, no
 * alignment asked of the images, the mask or the uint8 outputs.  All arrays are DEVICE arrays.
 * od_q int32 [256] is the quantised optical density of a byte, made once on the host: od_q[v] = max(0, rint(4096 ln(Io / (v + 1))))
 * with 0 < Io <= 256, so 0 <= od_q[v] <= 22713; the float optical density is od = od_q / 4096, exact in fp32.  No kernel calls log.
 * A pixel is KEPT when none of its three od_q is below beta_q and, with `mask` uint8 [N][H][W] not NULL, its mask byte is non-zero.
 * cs_stain_moments    : moments int64 [N][10] += over the kept pixels of image n: their number, the sums of od_q r, g, b and of
 *                       the products rr, rg, rb, gg, gb, bb.  Integer only (22713^2 2^31 < 2^63): the bits do not depend on the
 *                       launch geometry.  It ADDS: the caller zeroes moments.
 * cs_stain_angle_hist : hist int64 [N][bins] += the kept pixels by clamp(floor((phi + pi/2) bins / pi), 0, bins - 1) with
 *                       p = od V (V fp32 [N][3][2]), phi = atan2f(p1, p0).  0 < bins <= 8192.  It ADDS.
 * cs_stain_conc_hist  : hist int64 [N][2][bins] += the kept pixels by clamp(floor(c_k bins / conc_max), 0, bins - 1) for each of the
 *                       two concentrations c = P od (P fp32 [N][2][3]).  0 < bins <= 4096, conc_max > 0.  It ADDS.
 * cs_stain_apply      : out uint8 [N][H][W][3] = clamp(rint(Io exp(-(A od))), 0, 255) for EVERY pixel, A fp32 [N][3][3], 0 < Io <= 256;
 *                       evaluated in fp32 as exp2(log2 Io - (A od) log2 e), within 10^-3 levels of the exact value.  out must
 *                       not overlap the images.
 * cs_stain_separate   : the concentrations c = P od of EVERY pixel, P fp32 [N][K][3], K = 2 or 3: out fp32 [N][H][W][K] (as_u8 = 0) or
 *                       uint8 [N][H][W][K] = clamp(rint(255 c_k / conc_max), 0, 255) (as_u8 = 1).
 * Every product of a matrix row with od is fmaf(b, a2, fmaf(g, a1, r a0)) in fp32; a NaN result lands in bin 0 or as level 0.
 * One launch each on `stream`, no workspace, no host synchronisation: capturable. */
int cs_stain_moments(const uint8_t* images_hwc, int N, int H, int W, const int32_t* od_q, int beta_q, const uint8_t* mask, int64_t* moments,
                     void* stream);
int cs_stain_angle_hist(const uint8_t* images_hwc, int N, int H, int W, const int32_t* od_q, int beta_q, const uint8_t* mask, const float* V,
                        int bins, int64_t* hist, void* stream);
int cs_stain_conc_hist(const uint8_t* images_hwc, int N, int H, int W, const int32_t* od_q, int beta_q, const uint8_t* mask, const float* P,
                       int bins, float conc_max, int64_t* hist, void* stream);
int cs_stain_apply(const uint8_t* images_hwc, int N, int H, int W, const int32_t* od_q, const float* A, float Io, uint8_t* out, void* stream);
int cs_stain_separate(const uint8_t* images_hwc, int N, int H, int W, const int32_t* od_q, const float* P, int K, int as_u8, float conc_max,
                      void* out, void* stream);

/* ---- annotated images: overlays, heat maps, outlines and cell dots (csrc/render.hip) -------------------------------------------
 * images uint8 [N][H][W][3], 0 < N <= 65535, N H W < 2^31 (the sizes of the regions entry points); all arrays are DEVICE arrays and
 * no alignment is asked of the images, the uint8 maps or the outputs.  Integer arithmetic throughout: the bits do not depend on
 * the launch geometry.  One launch each on `stream` (none without work), no workspace, no host synchronisation: capturable.
 * cs_render_compose : out uint8 [N][H][W][3] = per pixel and channel value c, in this order:
 *                       fill  CS_RENDER_FILL_NONE      nothing, fill_map == NULL
 *                             CS_RENDER_FILL_MASK      fill_map uint8 [N][H][W]: c = (c + 255 (m != 0)) >> 1
 *                             CS_RENDER_FILL_HEAT_U8   fill_map uint8 [N][H][W] = h
 *                             CS_RENDER_FILL_HEAT_F32  fill_map fp32 [N][H][W] = p (4-byte aligned): h = p > threshold ?
 *                                                      (uint8)(255.0f * p) : 0, for p in [0, 1]
 *                             heat: k = colormap[invert ? 255 - h : h][channel] (colormap uint8 [256][3]), s = c + k,
 *                             c = (s >> 1) + ((s & 1) & ((s >> 1) & 1)): the mean rounded half to even
 *                       outlines  labels int32 [N][H][W] or NULL: a pixel whose id = max(label, 0) is positive and one of whose
 *                             four neighbours has another id (outside the image: id 0) -- the rule of cs_regions_edges_labels,
 *                             evaluated here from the labels -- gets outline_rgb = r | g << 8 | b << 16, or, with palette uint8
 *                             [palette_rows][3] (1 <= palette_rows <= 256, else NULL and 0), palette[(id - 1) % palette_rows].
 *                     The image reads are pointwise: out may be the images themselves (any other overlap is not allowed).
 * cs_render_points  : draws into canvas uint8 [N][H][W][3].  pts int64 [P][2], off int64 [N + 1] and limit int32 [N] or NULL are
 *                     the triple of cs_spatial_bin_counts: image n owns the rows [off[n], off[n + 1]) of pts, of which limit keeps
 *                     the first limit[n] (Python's [:c]); offsets that do not describe rows of the buffer own none.  flags:
 *                     CS_RENDER_POINTS_XY = the rows are (col, row) instead of (row, col); CS_RENDER_POINTS_TAIL = the rows
 *                     that limit does NOT keep are drawn instead (it needs limit).  With d2 = dr^2 + dc^2 from the point,
 *                     thickness < 0 writes the pixels with d2 <= radius^2, thickness = t in [1, 2 radius] those with
 *                     (2 radius - t)^2 <= 4 d2 <= (2 radius + t)^2; 0 <= radius <= 64.  Pixels outside the image are skipped and
 *                     a point may lie anywhere.  Every write of a call stores the same rgb = r | g << 8 | b << 16, so overlapping
 *                     marks do not depend on any order.  P == 0 launches nothing. */
#define CS_RENDER_FILL_NONE 0
#define CS_RENDER_FILL_MASK 1
#define CS_RENDER_FILL_HEAT_U8 2
#define CS_RENDER_FILL_HEAT_F32 3
#define CS_RENDER_POINTS_XY 1
#define CS_RENDER_POINTS_TAIL 2
int cs_render_compose(const uint8_t* images_hwc, int N, int H, int W, int fill, const void* fill_map, float threshold, int invert,
                      const uint8_t* colormap, const int32_t* labels, int outline_rgb, const uint8_t* palette, int palette_rows,
                      uint8_t* out, void* stream);
int cs_render_points(uint8_t* canvas_hwc, int N, int H, int W, const int64_t* pts, const int64_t* off, const int32_t* limit, long long P,
                     int radius, int thickness, int rgb, int flags, void* stream);

/* ---- polygons to pixels: label images and masks from vertex rings (csrc/polygons.hip) -----------------------------------------
 * The inverse of cs_regions_contour_labels, for any closed rings.  All arrays are DEVICE arrays, all arithmetic is integer.
 * Vertices are fixed-point: vertices int32 [V][2] = (row, col) in units of 1 / S pixel, S = 2^sub, 0 <= sub <= 8; sub = 0 is the
 * lattice of cs_regions_contour_labels.  Pixel (i, j) is the closed unit square with the corners (i, j) and (i + 1, j + 1); its
 * centre decides.  In units of 1 / (2 S) the centre is Y = (2 i + 1) S, X = (2 j + 1) S and a vertex (R, C) is y = 2 R, x = 2 C.
 * For every edge a -> b of every ring of a shape, the closing edge last -> first included, let d = yb - ya and
 * cross = (xb - xa)(Y - ya) - (X - xa) d in 64-bit integers.  The edge COUNTS for the pixel when (ya <= Y) != (yb <= Y) and
 * (d > 0 and cross <= 0, or d < 0 and cross >= 0): the ray from the centre towards smaller columns.  A counting edge weighs +1 if
 * d > 0, else -1; the winding number of the pixel is the sum over all rings of the shape.  rule CS_POLYGON_EVENODD takes the pixel
 * when the winding number is odd, CS_POLYGON_NONZERO when it is not 0.  A centre exactly on an edge or a vertex belongs to the side
 * towards larger columns or rows (top and left in, bottom and right out), so shapes that share an edge neither overlap nor leave
 * a gap; rings of fewer than 3 vertices, zero-area rings, repeated vertices and horizontal edges contribute nothing by the rule
 * itself; vertices may lie outside the image, only pixels of the image are written.
 * Layout: ring r is the rows ring_start[r] .. ring_start[r] + ring_count[r] of vertices (ring_start, ring_count int32 [R]; a count
 * <= 0, or a ring that does not lie within the V rows, draws nothing) -- a packed CSR table and the padded vertices of
 * cs_regions_contour_labels are both served.  Shape s owns the rings shape_rings[s] .. shape_rings[s + 1] (int32 [S + 1]); image n
 * owns the shapes image_shapes[n] .. image_shapes[n + 1] (int32 [N + 1], rising).  items int32 [I][3] = (shape, first row, rows):
 * one workgroup paints those rows of that shape; the items of a shape must cover every row it reaches.  items == NULL (I ignored):
 * one item per shape, and the workgroup works out the shape's rows itself.
 * Output: mode CS_POLYGON_LABELS: out int32 [N][H][W], shape s of image n RAISES the pixels it takes to s - image_shapes[n] + 1 by
 * an integer maximum -- the highest label wins, whatever the order of arrival, and what out held stays where it is larger;
 * mode CS_POLYGON_MASK: out uint8 [N][H][W], 1 is stored where any shape takes the pixel.  Other pixels are not written: the caller
 * clears out, or paints onto what it holds.
 * Need 0 < N <= 65535, 0 < H W < 2^31, max(H, W) << (sub + 1) < 2^30, every coordinate in [-2^28, 2^28] (not checked on the
 * device: every product then stays below 2^62), V, R, S, I < 2^31, vertices 8-byte aligned.  One launch whose grid depends on
 * I (or S) alone, no workspace, no environment, no host synchronisation: capturable. */
#define CS_POLYGON_EVENODD 0
#define CS_POLYGON_NONZERO 1
#define CS_POLYGON_LABELS 0
#define CS_POLYGON_MASK 1
int cs_polygons_rasterize(const int32_t* vertices, long long V, const int32_t* ring_start, const int32_t* ring_count, int R,
                          const int32_t* shape_rings, int S, const int32_t* image_shapes, const int32_t* items, long long I, int N,
                          int H, int W, int sub, int rule, int mode, void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CELLSEG_HIP_H_ */
