/*
 * adyolo_hip.h -- C ABI of libadyolo_hip.so: the MI355X (gfx950) hot path of AD-YOLO.
 *
 * The reference (sadPororo/AD-YOLO) has NO FFI: its plugin boundary is Python class dispatch
 * (src/wrapper.py:26-50, :70-85) and every arithmetic step is an implicit ATen / NumPy / librosa
 * call.  This header is therefore the boundary the build defines: each entry point replaces the
 * implicit library call(s) cited next to it.  All pointers are DEVICE pointers (HBM) unless a name
 * ends in _host; sizes are plain ints; `stream` is a hipStream_t passed as void* (NULL = default
 * stream).  Activations are float32, channels-last:  x[n][h][w][c]  with h = time frame, w = mel bin.
 * Every function returns 0 on success, a negative ADYOLO_E* code on bad arguments, or a positive
 * hipError_t; adyolo_last_error() returns a static description of the last failure on this thread.
 * No function allocates device memory or synchronises the device: workspaces are passed in.
 */
#ifndef ADYOLO_HIP_H
#define ADYOLO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADYOLO_ABI_VERSION 4
#define ADYOLO_EINVAL (-1)   /* bad shape / alignment / null pointer */
#define ADYOLO_ENOSUP (-2)   /* shape outside what the kernels are built for */

int         adyolo_abi_version(void);
const char *adyolo_last_error(void);
/* number of float32 words a workspace must hold, for the calls that take one */

/* ------------------------------------------------------------------------------------------------
 * K1  feature extraction: STFT(n_fft=1200, hop=600, periodic Hann, reflect-centre) -> log-mel (4 ch)
 *     + mel-scale FOA intensity vector (3 ch) -> z-score.
 *     replaces src/datasets.py:252-292 (librosa.core.stft :255, mel GEMM :264/:275, power_to_db :265,
 *     scaler :289-290) and the tensorise/concat step :158-160.
 *   audio   [B][n_samples][4] float32, already int16/32768 + 1e-8 (datasets.py:147), channels W,Y,Z,X
 *   clip_offset  NULL, or [B] int64 sample offsets into `audio`: "virtual clip" b is then the n_samples samples starting
 *           at clip_offset[b] -- the 20 s / 1 s-stride training chunks of src/preprocess.py:13-84 (chunking), computed
 *           from the whole recording in place; every virtual clip gets its own reflect padding (np.pad at the chunk
 *           start, preprocess.py writes the chunk as its own file) and its own top_db reference (chan_max row b)
 *   twiddle [2388][2]  rows 0..1199: tw[n] = exp(-2 pi i n/1200) (re,im) (the periodic Hann window is generated in the
 *           kernel); rows 1200 + (k-1) 120 + s = tw[(s k) mod 1200] and rows 2280 + (k-1) 12 + j = tw[10 j k] for k = 1..9,
 *           s < 120, j < 12: the same entries in the order the lanes of transform passes 1 and 2 read them
 *   mel_w   [n_mel_w <= 1200] float32 non-zero weights of the 64 (contiguous, triangular) mel filters, filter
 *           after filter; the filters are cut into n_chunks (<= 224) pieces of a few bins for load balance:
 *           chunk_mel[i] = filter index (non-decreasing, every filter 0..63 present), chunk_start[i] = first FFT bin, chunk_len[i], chunk_off[i] = offset in mel_w
 *   scaler_mean/scaler_rstd [7][64]: (x-mean)*rstd per (feature channel, mel bin)
 *   out     layout 0: [B][7][T][64]  (reference order, datasets.py:160)
 *           layout 1: [B][T][64][8]  (channels-last, 8th channel zero) -- what the encoder consumes
 *   chan_max [B][4] float32 workspace (per clip/channel max of the un-clipped log-mel, for top_db=80)
 *   T = n_samples / 600 (n_samples must be a multiple of 600).
 * Two launches: adyolo_feat_stft_mel (writes IV final, log-mel un-clipped + chan_max) then
 * adyolo_feat_finish (top_db clip relative to chan_max + z-score of the 4 log-mel channels).
 * ---------------------------------------------------------------------------------------------- */
int adyolo_feat_stft_mel(const float *audio, const int64_t *clip_offset, const float *twiddle,
                         const int32_t *chunk_mel, const int32_t *chunk_start, const int32_t *chunk_len,
                         const int32_t *chunk_off, const float *mel_w, int n_chunks, int n_mel_w,
                         const float *scaler_mean, const float *scaler_rstd, float *out, float *chan_max, int B,
                         int n_samples, int layout, void *stream);
int adyolo_feat_finish(float *out, const float *chan_max, const float *scaler_mean,
                       const float *scaler_rstd, int B, int T, int layout, void *stream);

/* K1m  GCC-PHAT features of 4-channel MIC-format audio (BASELINE config 5: "DCASE2022 MIC (GCC-PHAT features)").  NOT in
 *     the reference (FOA is hard-coded: src/datasets.py:36-37,55; the --feature switch is commented out, src/main.py:40):
 *     PARITY UNPINNED.  Definition: the DCASE2022 SELD baseline's (the repository README.md:156 credits for the metrics):
 *     per microphone pair m < n, R = conj(X_m) X_n, cc = irfft(exp(i angle(R))), feature = concat(cc[-32:], cc[:32]);
 *     X = the STFT of K1.  The four log-mel channels of the MIC feature set are adyolo_feat_stft_mel on the same audio.
 *   audio [B][n_samples][4] float32; out: channels-last pixels of pix_stride floats, [B][T][64 lag bins][pix_stride];
 *   the six pair channels (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) are written at ch0 .. ch0+5 as (cc - mean) * rstd with
 *   scaler_mean / scaler_rstd [6][64]. */
int adyolo_feat_gcc_phat(const float *audio, const int64_t *clip_offset /*or NULL*/, const float *twiddle,
                         const float *scaler_mean, const float *scaler_rstd, float *out, int B, int n_samples,
                         int pix_stride, int ch0, void *stream);
/* [B][C][H][W] (C<=8) -> [B][H][W][8] zero padded; entry of WrapperModel.forward (wrapper.py:52-57) */
int adyolo_nchw_to_nhwc8(const float *x, float *y, int B, int C, int H, int W, void *stream);

/* ------------------------------------------------------------------------------------------------
 * K2  3x3 convolution, stride 1, pad 1, as an fp32-MFMA implicit GEMM (v_mfma_f32_32x32x2_f32).
 *     replaces nn.Conv2d forward/backward at src/models/backbones/resnet.py:16,18,142.
 *   x [N][H][W][Cin]; y [N][H][W][Cout];  Cin in {8, multiples of 32}, Cout multiple of 32.
 *   wpk   packed weights [Cout][9][Cin]  (tap = ky*3+kx, Cin fastest) -- see adyolo_pack_w3x3
 *   bias  [Cout] or NULL;  addend [N][H][W][Cout] or NULL (added before the optional ReLU)
 *   y = relu?( conv(x', w) + bias + addend' )   with the optional fusions
 *     x' = x*in_scale[c] + in_shift[c] on in-image pixels (BatchNorm affine of the producer; zero padding stays 0)
 *     addend' = addend * (addend_mask > 0)  (residual gradient  de * (e > 0)  formed on the fly)
 *     mask_bits: bit 0 -- addend_mask points to ReLU-mask BITS (the uint64 words adyolo_se_tail_fwd writes, see K3b)
 *       instead of a float tensor; bit 1 -- the same for stat_mask.  Bits move 1/32 of the bytes.
 *     stats [2][tiles][Cout]: per 256-pixel patch, per channel sum of y and either sum of y^2 (stat_aux == NULL: the
 *       BatchNorm statistics / SE squeeze of the consumer, finished by adyolo_bn_stats_tiles) or sum of
 *       y * (stat_aux - stat_mean[c]) * stat_invstd[c] (y is a gradient, stat_aux the BatchNorm input at the same
 *       positions: the two sums of BatchNorm's backward, finished by adyolo_bn_bwd_tiles) -- no separate read pass.
 * data-gradient = the same call with the dgrad packing (wpk_dgrad, Cin<->Cout swapped).
 * weight-gradient: adyolo_conv3x3_wgrad accumulates into `slabs` ([n_slabs][Cout][9][CinP] float32,
 * n_slabs = adyolo_conv3x3_wgrad_slabs(...)) then reduces them into dw in the reference layout
 * [Cout][Cin_real][3][3] (Cin_real <= Cin: 7 for the stem whose activations are padded to 8).
 * ---------------------------------------------------------------------------------------------- */
int adyolo_pack_w3x3(const float *w /*[Cout][Cin_real][3][3]*/, float *wpk_fwd /*[Cout][9][Cin]*/,
                     float *wpk_dgrad /*[Cin][9][Cout] or NULL*/, int Cout, int Cin_real, int Cin,
                     void *stream);
int adyolo_conv3x3_tiles(int N, int H, int W);   /* number of 256-pixel patches = rows of `stats` */
int adyolo_conv3x3_fwd(const float *x, const float *wpk, const float *bias, const float *addend,
                       const float *addend_mask, const float *in_scale, const float *in_shift, float *y,
                       float *stats, const float *stat_aux, const float *stat_mean, const float *stat_invstd,
                       const float *stat_mask, int N, int H, int W, int Cin, int Cout, int relu, int mask_bits, void *stream);
/*   stat_mask (optional, needs stats): the two per-patch sums are taken of y * (stat_mask > 0) instead of y -- with
 *   stat_aux = c and stat_mask = e of the block BELOW, the data-gradient launch that produces de also produces the
 *   per-sample sums of the SE / BatchNorm-2 backward (finished by adyolo_se_tail_bwd_tiles), y itself is unaffected. */
/* K2w  the same operator as Winograd F(2x2,3x3) (2.25x fewer matrix FLOPs; fp32 throughout, results agree with the
 *      direct form to ~1e-6 relative).  u_fwd / u_dgrad: the transformed filters G g G^T in MFMA-fragment order
 *      [16][Cout/32][Cin/8][64][4] (forward) / [16][Cin/32][Cout/8][64][4] (data-gradient, taps flipped, channels
 *      transposed); Cin and Cout multiples of 32.  adyolo_wino_fwd takes the arguments of adyolo_conv3x3_fwd with
 *      `u` in place of `wpk`; its `stats` rows are 8x16-pixel patches: adyolo_wino_tiles(N,H,W) of them. */
int adyolo_wino_pack_w(const float *w /*[Cout][Cin_real][3][3]*/, float *u_fwd /*or NULL*/, float *u_dgrad /*or NULL*/,
                       int Cout, int Cin_real, int Cin, void *stream);
/* the same for EVERY 3x3 filter of a model in one launch (the packed filters change once per optimizer step, not per layer
 * call: 64 pack launches per SE-ResNet34 train step become one).  table (device) = n rows of 8 int64:
 * {w, u_fwd, u_dgrad or 0, Cout, Cin_real, Cin, unused, unused}; max_cout / max_cin = the largest channel counts in the table. */
int adyolo_wino_pack_many(const int64_t *table, int n, int max_cout, int max_cin, void *stream);
int adyolo_wino_tiles(int N, int H, int W);
int adyolo_wino_fwd(const float *x, const float *u, const float *bias, const float *addend,
                    const float *addend_mask, const float *in_scale, const float *in_shift, float *y, float *stats,
                    const float *stat_aux, const float *stat_mean, const float *stat_invstd, const float *stat_mask,
                    int N, int H, int W, int Cin, int Cout, int relu, int mask_bits, void *stream);
/* K2w4  the same operator as Winograd F(4x4,3x3) (csrc/wino4.hip; round 4): 36 multiplies per 4x4 output tile and channel pair,
 *      1.78x fewer matrix instructions than K2w, still on the exact-fp32 MFMA.  Interpolation points 0, +-3/4, +-3/2, infinity;
 *      error against a float64 convolution ~1e-6 of the output's absmax (K2w: 2e-7).  Replaces nn.Conv2d forward / data-gradient
 *      at src/models/backbones/resnet.py:16,18 for Cout a multiple of 64 and Cin a multiple of 32 (<= 512).
 *      u_fwd / u_dgrad: G g G^T in MFMA-fragment order [36][Cout/32][Cin/8][64][4] (forward) / [36][Cin/32][Cout/8][64][4]
 *      (data-gradient, taps flipped, channels transposed); position order: see csrc/wino4.hip.  adyolo_wino4_fwd takes the
 *      arguments of adyolo_conv3x3_fwd with `u` in place of `wpk`; its `stats` rows are 32x16-pixel (maps narrower than 32
 *      pixels) or 16x32-pixel patches: adyolo_wino4_tiles(N,H,W) of them.  adyolo_wino4_pack_many: the table of
 *      adyolo_wino_pack_many (columns 6, 7 unused). */
int adyolo_wino4_pack_w(const float *w /*[Cout][Cin_real][3][3]*/, float *u_fwd /*or NULL*/, float *u_dgrad /*or NULL*/,
                        int Cout, int Cin_real, int Cin, void *stream);
int adyolo_wino4_pack_many(const int64_t *table, int n, int max_cout, int max_cin, void *stream);
int adyolo_wino4_tiles(int N, int H, int W);
int adyolo_wino4_fwd(const float *x, const float *u, const float *bias, const float *addend, const float *addend_mask,
                     const float *in_scale, const float *in_shift, float *y, float *stats, const float *stat_aux,
                     const float *stat_mean, const float *stat_invstd, const float *stat_mask, int N, int H, int W, int Cin,
                     int Cout, int relu, int mask_bits, void *stream);
/*      adyolo_wino4_fwd launches the PERSISTENT form of the kernel (csrc/wino4p.hpp: one workgroup per CU walks the patches, the
 *      staging pipeline runs across patch boundaries, raw accumulators are exchanged and transformed on the reader side) or the
 *      one-patch-per-workgroup kernel; same results within fp32 rounding.  adyolo_wino4_fwd_form() is the ONE place that decides
 *      which (no device access): for Cout output channels, the operands present (the bits below) and mask_bits it returns
 *      2 persistent: Cout / 64 when that is whole, else Cout / 32, in {1, 2, 4, 8}; every mask operand given as bits; the persistent switch
 *        on, and an operand combination the kernel is built for (csrc/wino4p_launch.hpp: those of the SE-ResNet block; none has a bias);
 *      1 one-patch: otherwise, when Cout is a multiple of 64;
 *      0 none: adyolo_wino4_fwd returns ADYOLO_ENOSUP (so does a Cout that is not a positive multiple of 32).
 *      adyolo_wino4_fwd asks the same function; N, H, W, Cin and in_scale only set the patch shape inside the form.
 *      adyolo_wino4_last_form(): which one the last call launched (1 one-patch, 2 persistent, 0 none yet) -- for reporting. */
#define ADYOLO_W4_STATS 1        /* stats */
#define ADYOLO_W4_ADDEND 2       /* addend */
#define ADYOLO_W4_ADDEND_MASK 4  /* addend_mask (as bits: mask_bits & 1) */
#define ADYOLO_W4_STAT_AUX 8     /* stat_aux, stat_mean, stat_invstd */
#define ADYOLO_W4_STAT_MASK 16   /* stat_mask (as bits: mask_bits & 2) */
#define ADYOLO_W4_BIAS 32        /* bias */
int adyolo_wino4_fwd_form(int Cout, int operands, int mask_bits);
int adyolo_wino4_last_form(void);
/*      adyolo_set_switches(bits): the two on / off switches adyolo_wino4_fwd consults -- 1 persistent kernel, 2 patches one / two tiles
 *      wide on maps up to 8 pixels wide (plain launches on the persistent kernel).  Both are on until it is called; the library
 *      reads no environment variable (ops.reload_thresholds() pushes ADYOLO_W4_PERSIST / ADYOLO_W4_NARROW from the host's switch
 *      table, at load and on every reload).  Returns the bits now in effect. */
int adyolo_set_switches(int bits);
/* K2w4w (round 5, csrc/wino4w.hip): the weight gradient in the Winograd F(4x4,3x3) domain,
 *      dw = G^T [ sum over 4x4 output tiles (B^T d B) (.) (A e A^T) ] G  (36 multiplies per 16 outputs and channel pair: 9/36 of the
 *      direct form's matrix FLOPs, 1.78x fewer MFMAs than adyolo_wino_wgrad; interpolation points of K2w4; error against a float64
 *      weight gradient ~2e-6 of its absmax, tools/wino4w/numerics.py).  Same operator and argument meaning as adyolo_wino_wgrad
 *      (nn.Conv2d backward-weights, src/models/backbones/resnet.py:16,18; x optionally seen through a per-channel affine with
 *      zero padding).  Shapes: Cin % 32 == 0, Cout % 32 == 0, W % 16 == 0, H % 4 == 0, each tensor below 2 GiB --
 *      adyolo_wino4_wgrad_slabs returns the number of [36][Cin][Cout] float32 slabs the launch needs, or 0 when the shape is
 *      not supported (callers then use adyolo_wino_wgrad).  dw: reference layout [Cout][Cin_real][3][3]. */
int adyolo_wino4_wgrad_slabs(int N, int H, int W, int Cin, int Cout);
int adyolo_wino4_wgrad(const float *x, const float *dy, const float *in_scale /*or NULL*/, const float *in_shift /*or NULL*/,
                       float *slabs, float *du /*[36][Cin][Cout] scratch*/, float *dw, int N, int H, int W, int Cin, int Cin_real,
                       int Cout, void *stream);
/* Winograd weight-gradient: dw = G^T [ sum_tiles (B^T d B)(.)(A e A^T) ] G.  slabs: [n_slabs][16][Cin][Cout] float32 with
 * n_slabs = adyolo_wino_wgrad_slabs(...); du: [16][Cin][Cout] scratch; dw: reference layout [Cout][Cin_real][3][3]. */
int adyolo_wino_wgrad_slabs(int N, int H, int W, int Cin, int Cout);
int adyolo_wino_wgrad(const float *x, const float *dy, const float *in_scale, const float *in_shift, float *slabs,
                      float *du, float *dw, int N, int H, int W, int Cin, int Cin_real, int Cout, void *stream);
int adyolo_conv3x3_wgrad_slabs(int N, int H, int W, int Cin, int Cout);
int adyolo_conv3x3_wgrad(const float *x, const float *dy, const float *in_scale, const float *in_shift,
                         float *slabs, float *dw, int N, int H, int W, int Cin, int Cin_real, int Cout,
                         void *stream);
/* host only, no launch: the work split the weight-gradient launchers compute for a shape.  form 0: conv3x3_wgrad_kernel,
 * 1: stem_wgrad_kernel (Cin = 8, Cout = 32, no affine), 2: wino_wgrad_kernel, 3: wino4_wgrad_kernel.  out8 = {workgroups per channel
 * block (= slabs; the stem before its cap), work items (tiles | image rows | strip segments | run-pair segments), segments per
 * strip / pair, segment length (rows of a tile | rows per workgroup | tile rows | steps of one tile row), block width (NT | NB;
 * 1), tile / strip width in pixels, the stem's workgroups (min(slabs, 512)), 1 when the entry point takes the shape with that
 * kernel}; all zeros when it does not. */
int adyolo_wgrad_plan(int form, int N, int H, int W, int Cin, int Cout, int *out8);
/* host only, no launch (the CU count the F(4x4) launcher caches apart): what the forward / data-gradient entry points would
 * launch for a shape and operand set, through the functions their launchers call.  form 0: adyolo_conv3x3_fwd with
 * conv3x3_fwd_kernel, 1: the same entry point with stem_fwd_kernel, 2: adyolo_wino_fwd, 3: adyolo_wino4_fwd.  operands: the
 * ADYOLO_W4_* bits above; mask_bits as at the entry points; affine: in_scale / in_shift are given.  out24 =
 *   [0] kernel: 0 refused (forms 0 / 1: or the entry point takes its other kernel), 1 conv3x3_fwd_kernel, 2 stem_fwd_kernel,
 *       3 wino_fwd_kernel, 4 wino4_fwd_kernel, 5 wino4p_fwd_kernel (persistent)
 *   [1] [2] rows and columns of a patch,  [3] patchesH,  [4] patchesW,  [5] nsp = N * patchesH * patchesW
 *   [6] 32-channel output blocks per workgroup (BN / 32 | NT | NB),  [7] ncb channel blocks,  [8] xcd_div (0: no XCD dealing)
 *   [9] grid x,  [10] grid y,  [11] slots (persistent: workgroups per XCD, grid = 8 slots; else 0)
 *   [12] TC,  [13] AFF,  [14] ONE,  [15] KC,  [16] BN,  [17] TW,  [18] BRES,  [19] FULL,  [20] MKM,  [21] narrow,  [22] [23] 0
 * (template arguments of the kernel launched; 0 where the kernel has no such argument).  All zeros when refused. */
int adyolo_conv_fwd_plan(int form, int N, int H, int W, int Cin, int Cout, int operands, int mask_bits, int affine, int *out24);

/* ------------------------------------------------------------------------------------------------
 * K7  dense GEMM on fp32 MFMA:  C[m][n] = sum_k opA(m,k) * opB(n,k) (+ bias[n])
 *     opA(m,k) = transA ? A[k*lda+m] : A[m*lda+k];   opB(n,k) = transB ? B[k*ldb+n] : B[n*ldb+k]
 *     replaces nn.Linear (linearheads.py:95-98, resnet.py:96-98), the 1x1 downsample conv
 *     (resnet.py:160-162), the GRU input projections (resnet.py:153) and their backward passes.
 *   Leading dimensions must be multiples of 4, and so must each operand's contiguous axis (K for a
 *   k-major operand, M resp. N for a transposed one) -- 16-byte vector loads run along it.
 *   splits > 1: K is cut into `splits` ranges, partial products go to `slabs` ([splits][M][N]) and are
 *   summed deterministically into C (bias added once).  accumulate != 0: C += result.
 * ---------------------------------------------------------------------------------------------- */
int adyolo_gemm(const float *A, const float *B, const float *bias, float *C, float *slabs, int M,
                int N, int K, int lda, int ldb, int ldc, int transA, int transB, int splits,
                int accumulate, void *stream);
/* host only, no launch: what adyolo_gemm decides for these arguments -- klen: the K range of one split (whole K tiles of 32),
 * eff_splits: the splits that are not empty with it, fastg: bit 0 / 1 = operand A / B may go through a buffer descriptor
 * (taken by the kernel for k-major operands only). */
int adyolo_gemm_plan(int M, int N, int K, int lda, int ldb, int transA, int transB, int splits, int *klen,
                     int *eff_splits, int *fastg);
/* batched variant (attention, resnet_conformer.py:57-85): problem (o, i), o < outer, i < inner, uses the operand
 * bases A + o*oA + i*iA etc. (strides in floats, multiples of 4);  C = alpha * product (+ C when accumulate). */
int adyolo_gemm_batched(const float *A, const float *B, float *C, int M, int N, int K, int lda, int ldb, int ldc,
                        int transA, int transB, int outer, int inner, long oA, long iA, long oB, long iB, long oC,
                        long iC, float alpha, int accumulate, void *stream);
/* out[c] (+)= sum_r A[r*lda + c], deterministic two-stage; partial: [1024][C] workspace */
int adyolo_colsum(const float *A, float *out, float *partial, int R, int C, int lda, int accumulate,
                  void *stream);

/* ------------------------------------------------------------------------------------------------
 * K3  BatchNorm2d (train-mode batch statistics / eval-mode running statistics), channels-last.
 *     replaces nn.BatchNorm2d at resnet.py:17,19,144,163 (momentum 0.1, eps 1e-5).
 *   adyolo_bn_stats: per-sample channel sums  ssum[N][C]  (these are also the SE squeeze, K3b) and
 *     mean/invstd [C] of the whole batch; updates running_mean / running_var (unbiased) in place when
 *     they are non-NULL.  partial: workspace of 4*1024*C floats.
 *   adyolo_bn_scale_shift: scale = gamma*invstd, shift = beta - mean*scale   (train)
 *     or from running stats when mean == NULL is not allowed: pass running_mean/invstd computed by
 *     adyolo_bn_eval_stats.
 *   adyolo_affine_nhwc: y = x*scale[c] + shift[c]
 *   adyolo_bn_bwd_reduce: sdy[c] = sum dy, sdyx[c] = sum dy * xhat   (partial: 2*1024*C floats)
 *   adyolo_bn_bwd_apply:  dx = gamma*invstd*(dy - sdy/R - xhat*sdyx/R) [* (x > 0) when relu_mask]
 *     and dgamma += sdyx, dbeta += sdy when those pointers are non-NULL.
 * ---------------------------------------------------------------------------------------------- */
int adyolo_bn_stats(const float *x, float *ssum, float *mean, float *invstd, float *running_mean,
                    float *running_var, float *partial, int N, int HW, int C, float momentum,
                    float eps, void *stream);
/* same as adyolo_bn_stats but from the per-patch sums a convolution epilogue wrote (tiles = G*N, patch index
 * n*G + g); partial: workspace of 2*1024*C floats.  With gamma / beta / scale / shift (all or none) the same finishing
 * launch also writes scale = gamma*invstd, shift = beta - mean*scale (what adyolo_bn_scale_shift would compute). */
int adyolo_bn_stats_tiles(const float *tile_stats, float *ssum, float *mean, float *invstd, float *running_mean,
                          float *running_var, const float *gamma, const float *beta, float *scale, float *shift,
                          float *partial, int N, int G, int HW, int C, float momentum, float eps, void *stream);
/* the two halves of adyolo_bn_stats_tiles as separate calls (per-patch sums -> per-sample sums ps0 / ps1 [N][C];  per-sample
 * sums -> mean / invstd / running statistics / scale / shift over N samples of HW positions).  Exact data parallelism
 * all-gathers the per-sample sums of all ranks between the two, so N ranks compute the statistics of the concatenated
 * batch bit-identically to one device. */
int adyolo_bn_persample(const float *tile_stats, float *ps0, float *ps1, int N, int G, int C, void *stream);
int adyolo_bn_finish(const float *ps0, const float *ps1, float *mean, float *invstd, float *running_mean,
                     float *running_var, const float *gamma, const float *beta, float *scale, float *shift, int N,
                     int HW, int C, float momentum, float eps, void *stream);
int adyolo_bn_eval_stats(const float *running_mean, const float *running_var, float *mean,
                         float *invstd, int C, float eps, void *stream);
int adyolo_bn_scale_shift(const float *gamma, const float *beta, const float *mean,
                          const float *invstd, float *scale, float *shift, int C, void *stream);
int adyolo_affine_nhwc(const float *x, const float *scale, const float *shift, float *y, long rows,
                       int C, void *stream);
int adyolo_bn_bwd_reduce(const float *dy, const float *x, const float *mean, const float *invstd,
                         float *sdy, float *sdyx, float *partial, long rows, int C, void *stream);
/* sdy / sdyx from the per-patch sums a data-gradient convolution wrote (stat_aux mode) */
int adyolo_bn_bwd_tiles(const float *tile_stats, float *sdy, float *sdyx, float *partial /*[2][256][C]*/, int tiles, int C,
                        void *stream);
int adyolo_bn_bwd_apply(const float *dy, const float *x, const float *gamma, const float *mean,
                        const float *invstd, const float *sdy, const float *sdyx, float *dx,
                        float *dgamma, float *dbeta, float *dx_colsum /*or NULL: [C] channel sums of dx*/,
                        float *colsum_partial /*[8192][C] workspace when dx_colsum*/, long rows, int C, int relu_mask,
                        float count_scale /*1, or the number of equal data-parallel micro-batches sdy / sdyx were summed over*/,
                        void *stream);

/* ------------------------------------------------------------------------------------------------
 * K3b squeeze-excite + residual tail of SEBasicBlock (resnet.py:38-47, SELayer :91-106), fused:
 *     d = c*scale + shift (bn2);  s = sigmoid(W2 relu(W1 mean_hw(d) + b1) + b2);  e = relu(d*s + r)
 *   adyolo_se_fc_fwd: pooled[n][c] = scale*ssum/HW + shift;  hid = relu(W1 pooled + b1) [N][Cr];
 *                     s = sigmoid(W2 hid + b2) [N][C]
 *   adyolo_se_tail_fwd: e = relu((c*scale+shift)*s[n][c] + r)
 *   adyolo_se_tail_bwd_reduce: g = de*(e>0);  sg[n][c] = sum_hw g;  sgx[n][c] = sum_hw g*xhat
 *   adyolo_se_fc_bwd: from sg, sgx: dpool[n][c] and, packed as [db2 C | dW2 C*Cr | db1 Cr | dW1 Cr*C | sdd C | sddx C]
 *                     (P words, one workgroup per sample + a deterministic column sum over the batch), the FC
 *                     gradients and the batch sums bn2's backward needs: sdd[c] = sum dd (= dbeta2),
 *                     sddx[c] = sum dd*xhat (= dgamma2)
 *   adyolo_se_tail_bwd_apply: dc = scale*( g*s + dpool/HW - sdd/R - xhat*sddx/R ),  dr = g (dr may be NULL: the
 *                     identity-shortcut gradient is then formed inside the dgrad epilogue via addend_mask)
 * ---------------------------------------------------------------------------------------------- */
int adyolo_se_fc_fwd(const float *ssum, const float *scale, const float *shift, const float *w1,
                     const float *b1, const float *w2, const float *b2, float *pooled, float *hid,
                     float *s, int N, int HW, int C, int Cr, void *stream);
/* mask (optional): the ReLU mask (e > 0) as bits -- float4 i (4 consecutive channels) of the flattened tensor owns bit
 * (i & 63) of the 64-bit words mask[(i >> 6) * 4 + k], k = component; adyolo_relu_mask_words(N, HW, C) words (0 = shape
 * not supported: HW*C/4 must be a multiple of 64).  The backward passes then read the bits (1/32 of the bytes) instead
 * of e; with mask given, e may be NULL there. */
long adyolo_relu_mask_words(int N, int HW, int C);
/* r_scale / r_shift (both or neither): e = relu((c*scale+shift)*s + (r*r_scale + r_shift)) -- the downsample branch's
 * BatchNorm (resnet.py:160-163) applied while the shortcut is read, so bn(conv1x1(x)) is never written */
int adyolo_se_tail_fwd(const float *c, const float *r, const float *scale, const float *shift,
                       const float *s, const float *r_scale /*or NULL*/, const float *r_shift /*or NULL*/, float *e,
                       uint64_t *mask /*or NULL*/, int N, int HW, int C, void *stream);
/* The tail of the LAST block in front of a pooled stage boundary (the next SEBasicBlock starts with nn.AvgPool2d(2, 2):
 * resnet.py:29,40 / _make_layer :158-164): pooled [N][H/2][W/2][C] = avgpool2(e) and the ReLU-mask bits of e; e itself is not
 * written (only the pooling reads it in the forward pass, the backward passes read the bits).  adyolo_se_tail_fwd_pool_ok: 1
 * when the shape is taken (C/4 a power of two <= 32, H and W even, W*C/4 a multiple of 64), else use adyolo_se_tail_fwd +
 * adyolo_avgpool2_fwd.  Same values as those two calls, bit for bit. */
int adyolo_se_tail_fwd_pool_ok(int H, int W, int C);
int adyolo_se_tail_fwd_pool(const float *c, const float *r, const float *scale, const float *shift, const float *s,
                            const float *r_scale /*or NULL*/, const float *r_shift /*or NULL*/, float *pooled,
                            uint64_t *mask /*or NULL*/, int N, int H, int W, int C, void *stream);
int adyolo_se_tail_bwd_reduce(const float *de, const float *e, const uint64_t *mask /*or NULL*/, const float *c,
                              const float *mean, const float *invstd, float *sg, float *sgx, float *partial, int N,
                              int HW, int C, void *stream);
/* sg, sgx from per-patch sums [2][N*G][C] of a convolution epilogue run with stat_mask = e, stat_aux = c */
int adyolo_se_tail_bwd_tiles(const float *tile_stats, float *sg, float *sgx, int N, int G, int C, void *stream);
long adyolo_se_fc_bwd_words(int C, int Cr);   /* P = 2*C*Cr + Cr + 3*C */
int adyolo_se_fc_bwd(const float *sg, const float *sgx, const float *ssum, const float *gamma,
                     const float *beta, const float *mean, const float *invstd, const float *pooled,
                     const float *hid, const float *s, const float *w1, const float *w2, float *dpool,
                     float *part /*[N][P]*/, float *packed /*[P]*/, float *colsum_ws /*[1024][P]*/, int N,
                     int HW, int C, int Cr, void *stream);
/* The two passes for a block whose output was the pooled tensor (adyolo_se_tail_fwd_pool): dpooled [N][H/2][W/2][C] is the
 * gradient of avgpool2(e); de = 0.25 * dpooled spread over 2 x 2 pixels is formed on the fly (torch.nn.AvgPool2d's backward,
 * resnet.py:29) and written to de_out when given -- the identity shortcut's share of the gradient, read by conv1's
 * data-gradient epilogue -- so no adyolo_avgpool2_bwd launch and no full-size de is read by either pass.  Same values. */
int adyolo_se_tail_bwd_reduce_pooled(const float *dpooled, const uint64_t *mask, const float *c, const float *mean,
                                     const float *invstd, float *sg, float *sgx, float *partial, int N, int H, int W, int C,
                                     void *stream);
int adyolo_se_tail_bwd_apply_pooled(const float *dpooled, const uint64_t *mask, const float *c, const float *gamma,
                                    const float *mean, const float *invstd, const float *s, const float *dpool,
                                    const float *sdd, const float *sddx, float *dc, float *dr /*or NULL*/,
                                    float *de_out /*or NULL*/, int N, int H, int W, int C, float count_scale, void *stream);
int adyolo_se_tail_bwd_apply(const float *de, const float *e, const uint64_t *mask /*or NULL*/, const float *c,
                             const float *gamma, const float *mean, const float *invstd, const float *s,
                             const float *dpool, const float *sdd, const float *sddx, float *dc,
                             float *dr, int N, int HW, int C, float count_scale /*as in adyolo_bn_bwd_apply*/, void *stream);

/* K4  AvgPool2d(2,2) (resnet.py:13,27-29), channels-last; H and W even.  bwd: dx = dy/4 broadcast (+= if accumulate) */
int adyolo_avgpool2_fwd(const float *x, float *y, int N, int H, int W, int C, void *stream);
int adyolo_avgpool2_bwd(const float *dy, float *dx, int N, int H, int W, int C, void *stream);
/* y = a + b (elementwise, n float32);  adyolo_scale_dev: y = a * scalar_dev[0] (scalar read on device: no host sync) */
int adyolo_add(const float *a, const float *b, float *y, long n, void *stream);
int adyolo_scale_dev(const float *a, const float *scalar_dev, float *y, long n, void *stream);

/* ------------------------------------------------------------------------------------------------
 * K5  self-attention pooling over the 16 mel positions (resnet.py:109-123)
 *   x [R][F][C] (R = B*T'), w [C], b [1] -> y [R][C], attn [R][F]    (F <= 32, C == 256)
 *   bwd: dx [R][F][C]; dw_partial [nblk][C+1] workspace (last column = db), reduced into dw[C], db[1]
 * ---------------------------------------------------------------------------------------------- */
int adyolo_sap_fwd(const float *x, const float *w, const float *b, float *y, float *attn, int R,
                   int F, int C, void *stream);
int adyolo_sap_bwd(const float *dy, const float *x, const float *w, const float *attn, float *dx,
                   float *dw, float *db, float *partial, int R, int F, int C, void *stream);

/* ------------------------------------------------------------------------------------------------
 * K6  one bidirectional GRU layer, hidden 128 (nn.GRU at resnet.py:153,195; gate order r,z,n)
 *   gx  [B][T][2][384]  = x W_ih^T + b_ih for both directions (from adyolo_gemm)
 *   whh [2][384][128], bhh [2][384]
 *   out [B][T][256] (forward hidden | backward hidden);  gates [B][T][2][4][128] saves r,z,n,hn;
 *   hprev [B][T][2][128] saves the hidden state entering each step (gates/hprev may be NULL in eval)
 *   bwd: dout [B][T][256] -> dgx [B][T][2][384], dgh [B][T][2][384]
 *        (dW_ih = dgx^T x, dW_hh = dgh^T hprev, db = column sums, dx = dgx W_ih: adyolo_gemm/colsum)
 * K6b LayerNorm(256) + tanh (resnet.py:154,196-197): y = tanh(LN(x));
 *     bwd: dx, and dgamma/dbeta through `partial` ([nblk][2*C]) reduced into dgamma/dbeta (accumulated)
 * dropout mask for the inter-layer dropout (p = 0.3, train only): mask[i] = keep ? 1/(1-p) : 0 from a
 * counter-based generator (seed, offset); adyolo_mul applies it.
 * ---------------------------------------------------------------------------------------------- */
int adyolo_gru_fwd(const float *gx, const float *whh, const float *bhh, float *out, float *gates,
                   float *hprev, int B, int T, void *stream);
int adyolo_gru_bwd(const float *dout, const float *gates, const float *hprev, const float *whh,
                   float *dgx, float *dgh, int B, int T, void *stream);
int adyolo_ln_tanh_fwd(const float *x, const float *gamma, const float *beta, float *y, long R,
                       int C, float eps, void *stream);
int adyolo_ln_tanh_bwd(const float *dy, const float *x, const float *y, const float *gamma,
                       float *dx, float *dgamma, float *dbeta, float *partial, long R, int C,
                       float eps, void *stream);
int adyolo_dropout_mask(float *mask, long n, float p, uint64_t seed, uint64_t offset, void *stream);
/* y[i] = x[i] * mask[i] with the mask values adyolo_dropout_mask writes for (seed, offset), generated on the fly (forward:
 * x -> y; backward: the same call on the incoming gradient); n a multiple of 4.  Replaces nn.Dropout /
 * nn.GRU(dropout=) (reference resnet.py:153, resnet_conformer.py:46-47,199-206). */
int adyolo_dropout_apply(const float *x, float *y, long n, float p, uint64_t seed, uint64_t offset, void *stream);
/* same, with a device-side running offset added to `offset` (offset_dev may be NULL): a launch recorded in a hipGraph
 * draws a fresh part of the stream at every replay; adyolo_counter_add advances the counter at the end of a step. */
int adyolo_dropout_apply_dev(const float *x, float *y, long n, float p, uint64_t seed, uint64_t offset,
                             const uint64_t *offset_dev, void *stream);
int adyolo_counter_add(uint64_t *counter, uint64_t inc, void *stream);
int adyolo_mul(const float *a, const float *b, float *y, long n, void *stream);

/* ------------------------------------------------------------------------------------------------
 * K8  AD-YOLO loss, forward + backward in one pass over the logits (src/models/loss.py:189-251)
 *   logit  [B*T][Gaz*Gel][A][C+3]  (channel order obj, cls x C, u, v)
 *   target [M][7] float32 (b, frame, Gi, Gj, cls, U, V) -- datasets.py:164-184
 *   thr[3] responsibility thresholds in degrees (train_unify), gains[4] = angular, object, nonobj, class
 *   ws: workspace of adyolo_loss_workspace_words(...) 32-bit words (zeroed by the call itself)
 *   loss [1] float32;  dlogit same shape as logit or NULL (eval).  grad_scale multiplies dlogit.
 *   dist [M][A] (optional, may be NULL): angular distances D, for tests.
 * ---------------------------------------------------------------------------------------------- */
long adyolo_loss_workspace_words(int BT, int G, int A, int M);
int  adyolo_loss_fwd_bwd(const float *logit, const float *target, float *ws, float *loss,
                         float *dlogit, float *dist, int B, int T, int Gaz, int Gel, int A, int C,
                         int M, const float *thr_host, const float *gains_host, float grid_az,
                         float grid_el, float g_overlap, float grad_scale, void *stream);
/* the same in two phases (phases bit 0: workspace reset + assignment, bit 1: pass over the logits + final sum).  Exact data
 * parallelism all-reduces the first four 32-bit words of the workspace (distinct positives per threshold, responsible pairs)
 * between the phases and passes na_total = anchors of the whole batch (0: this call's own), so that every loss term is
 * normalised as on one device over the concatenated batch (loss.py:236-243). */
int  adyolo_loss_phase(const float *logit, const float *target, float *ws, float *loss,
                       float *dlogit, float *dist, int B, int T, int Gaz, int Gel, int A, int C,
                       int M, const float *thr_host, const float *gains_host, float grid_az,
                       float grid_el, float g_overlap, float grad_scale, int phases, long na_total, void *stream);

/* K8f per-clip AD-YOLO loss, forward only (evaluation: src/test.py:33-60 runs batch 1, every normaliser is per clip).
 *   logit     [B][T][Gaz*Gel][A][C+3]: B clips of one batched forward pass (each clip's logits 16-byte aligned)
 *   target    [cap][7] rows as above, the rows of clip b contiguous with b in column 0 (rows elsewhere, b = -1 padding
 *             included, are not read); row_start [B + 1] int32: clip b owns rows [row_start[b], row_start[b + 1])
 *   ws        adyolo_loss_per_clip_workspace_words(B, T, Gaz * Gel, A) 32-bit words (zeroed by the call itself)
 *   loss [B]  float32: loss[b] carries the bits adyolo_loss_fwd_bwd(dlogit = NULL) returns for clip b's logits and rows alone
 *             (0 for a clip without rows); valid [B] int32: 0 for a clip without rows, else 1
 *   acc       NULL, or the running accumulator of adyolo_loss_accumulate the valid losses are added to
 * Five launches whatever B is; no dlogit, no host synchronisation. */
long adyolo_loss_per_clip_workspace_words(int B, int T, int G, int A);
int  adyolo_loss_per_clip(const float *logit, const float *target, const int *row_start, float *ws, float *loss,
                          int *valid, float *acc, int B, int T, int Gaz, int Gel, int A, int C, long cap,
                          const float *thr_host, const float *gains_host, float grid_az, float grid_el,
                          float g_overlap, void *stream);
/* acc [2] float32 {sum, count} += the losses loss[i], i = 0 .. n - 1 with valid[i] != 0 (valid NULL: all), added one after the
 * other in float32 by one thread: the evaluation loop's ``total + loss`` on the device. */
int  adyolo_loss_accumulate(const float *loss, const int *valid, int n, float *acc, void *stream);

/* K8b inference decode (LabelPostProcessor.get_yolo_output, src/datasets.py:752-771): per anchor
 *   out = [sigmoid(obj), sigmoid(cls_c)*sigmoid(obj) x C, U deg in [-180,180), V deg in [-90, 90-1e-7]];
 *   by default thresholding and the (tiny, data-dependent) NMS stay on the host (ad-yolo_amd/postprocess.py);
 *   adyolo_yolo_select below runs them on the device. */
int adyolo_yolo_decode(const float *logit, float *out, long n_frames, int Gaz, int Gel, int A, int C,
                       float grid_az, float grid_el, float g_overlap, void *stream);

/* K8c inference selection (csrc/select.hip), opt-in: what postprocess.nms_decoded does on the host
 * (get_yolo_output thresholds + per-class NMS, src/datasets.py:773-855, helpers :858-919), on the decode above.
 *   dec   [n_frames][n_anchor = Gaz*Gel*A][C+3] from adyolo_yolo_decode; n_anchor <= ADYOLO_SELECT_MAX_N, else ENOSUP
 *   ws    adyolo_yolo_select_workspace_words(n_frames, n_anchor, C) words
 *   rows  capacity n_frames * C * n_anchor rows of [frame, class, x, y, z] float32; the first total rows are written:
 *         frames ascending, classes ascending, within a class the clusters in the order of their seeds
 *   frame_counts  [n_frames + 1] int32: rows per frame, then the total at [n_frames]
 *   a row passes with conf > conf_thresh and class_conf > clss_thresh (float32 compares: the caller rounds the
 *   thresholds the way its host comparison would); mode: ADYOLO_SELECT_CONN (connected components of
 *   dist < unify_thresh), ADYOLO_SELECT_SOFT (greedy, clusters of dist <= unify_thresh over all rows of the class) or
 *   ADYOLO_SELECT_PLAIN (greedy suppression, the seed alone).  Cluster vote: softmax(exp(conf^2 / vote_thresh)) weighted
 *   xyz, normalised; a class with one row and every PLAIN row keeps its unnormalised xyz. */
#define ADYOLO_SELECT_PLAIN 0
#define ADYOLO_SELECT_CONN  1
#define ADYOLO_SELECT_SOFT  2
#define ADYOLO_SELECT_MAX_N 1024
long adyolo_yolo_select_workspace_words(long n_frames, int n_anchor, int C);
int  adyolo_yolo_select(const float *dec, float *ws, float *rows, int *frame_counts, long n_frames, int n_anchor, int C,
                        float conf_thresh, float clss_thresh, float unify_thresh, float vote_thresh, int mode,
                        void *stream);

/* K8d SELD scoring (csrc/seld.hip), opt-in: what seld_metrics.SELDScorer.update adds for one recording (DCASE
 * location-sensitive detection and class-sensitive localisation over blocks of fpb frames, Hungarian association of the
 * predictions with the reference events per frame and class, 20-degree tracks), for rows already on the device.
 *   rows    [n_rows][5] [frame, class, x, y, z], float32 (rows_f64 = 0: what adyolo_yolo_select writes) or float64 (1); the
 *           frame column is not read: counts [n_clips * t_clip] int32 gives the rows of each frame, clip after clip, frames
 *           in order (a capacity n_rows beyond their sum is allowed).  Within a frame classes may come in any order; the
 *           order within a (frame, class) is kept (it decides the assignment under ties, as in scipy).
 *   file_ids [n_clips] int32: the reference file of each clip
 *   reference table, uploaded once (seld_metrics.DeviceSELDScorer):
 *     file_info [n_files][2] int32: first frame of the file in the table, number of blocks ceil(len / fpb), len = the
 *               largest frame index of its reference; frames >= blocks * fpb are not scored
 *     ref_off   [table frames * C + 1] int32: events of (frame, class) are ref_ev[ref_off[f * C + c] .. ref_off[f * C + c + 1])
 *               in reference order, at most ADYOLO_SELD_MAX_REF per (frame, class)
 *     ref_ev    [n_events][3] float64: azimuth in rad, sin and cos of the elevation
 *     keep      NULL, or [table frames] int32: only predictions of frames with keep != 0 are scored (overlap variants)
 *   acc     [n_files][9 * C + 3] float64, ADDED to: TP, FP, FP_spatial, FN, Nref, total_DE, DE_TP, DE_FP, DE_FN (each C
 *           classes wide), then S, D, I
 *   ws      adyolo_seld_score_workspace_words(n_clips, t_clip, max_blocks, C) words; max_blocks >= every blocks of file_info
 *   status  one int32 the kernels OR ADYOLO_SELD_* bits into; while it is nonzero (an error of this or an earlier call) acc
 *           is left as it is.  n_pred is only known on the device: more than ADYOLO_SELECT_MAX_N predictions of one
 *           (frame, class) set ADYOLO_SELD_PRED_OVERFLOW, which the caller reports as ENOSUP. */
#define ADYOLO_SELD_MAX_REF 8
#define ADYOLO_SELD_PRED_OVERFLOW 1   /* more than ADYOLO_SELECT_MAX_N predictions in one (frame, class) */
#define ADYOLO_SELD_REF_OVERFLOW  2   /* more than ADYOLO_SELD_MAX_REF reference events in one (frame, class) */
#define ADYOLO_SELD_BAD_ROWS      4   /* a negative count, or counts summing past n_rows */
#define ADYOLO_SELD_BAD_FILE      8   /* a file id outside [0, n_files) */
#define ADYOLO_SELD_NO_ASSIGNMENT 16  /* no finite assignment (a NaN coordinate) */
long adyolo_seld_score_workspace_words(long n_clips, int t_clip, int max_blocks, int C);
int  adyolo_seld_score(const void *rows, int rows_f64, long n_rows, const int *counts, long n_clips, int t_clip,
                       const int *file_ids, const int *file_info, const int *ref_off, const double *ref_ev, const int *keep,
                       int n_files, int C, int fpb, int max_blocks, double doa_thresh, float *ws, double *acc, int *status,
                       void *stream);
/* adyolo_seld_score_runs, opt-in: the same scores for the segments of ONE stitched run of frames (labelled evaluation through
 * windows: a pass begins in the middle of one recording and ends in the middle of another), against the same reference table.
 *   rows, rows_f64, n_rows  as above
 *   counts   [run_frames] int32: rows per frame of the run (what the selection writes for the run as one clip)
 *   segments DEVICE int32 [n_segments][ADYOLO_SELD_RUN_WORDS] = {file id, f0 = the segment's first frame on the file's own frame
 *            axis, r0 = its first frame in counts, n >= 0 = the frames of the run that belong to it, last = 1 for the file's
 *            final segment, 0, 0, 0}
 *   a segment covers the file's blocks [f0 / fpb, b1): b1 = min((f0 + n) / fpb, blocks) for a segment that is not the last,
 *   b1 = blocks of file_info for the last one, which so also accounts for the blocks past the audio that still hold reference
 *   events (FN); nothing at or past blocks * fpb is scored.  A prediction of file frame fr is read from counts[r0 + fr - f0],
 *   and only for f0 <= fr < f0 + n (and keep, where given).  A last segment with n = 0 is legal (a recording shorter than one
 *   frame that has a reference).
 *   acc      for every column the kernel reads acc[file][col], adds the segment's block records one at a time, left to right in
 *            float64 (S, D, I per block from its loc_fp / loc_fn), and writes it back; segments in table order; no float
 *            atomics.  A file scored in ordered segments into a zeroed row ends, in every column, with the bits one
 *            adyolo_seld_score call on the whole recording leaves (that call forms 0 + (r0 + r1 + ...) in the same order).
 *   seg_blocks >= the blocks every segment covers (it sizes the grid: one wave per (segment, block, class));
 *   ws       adyolo_seld_score_runs_workspace_words(n_segments, run_frames, seg_blocks, C) words
 *   status   as above, and ADYOLO_SELD_BAD_RUN for a segment with f0 % fpb != 0, (f0 + n) % fpb != 0 unless last, a negative
 *            f0, r0 or n, r0 + n > run_frames, or more blocks than seg_blocks; while the word is nonzero acc is left as it is. */
#define ADYOLO_SELD_RUN_WORDS 8
#define ADYOLO_SELD_BAD_RUN   32  /* a segment that breaks the contract above */
long adyolo_seld_score_runs_workspace_words(long n_segments, long run_frames, int seg_blocks, int C);
int  adyolo_seld_score_runs(const void *rows, int rows_f64, long n_rows, const int *counts, long run_frames,
                            const int *segments, long n_segments, const int *file_info, const int *ref_off,
                            const double *ref_ev, const int *keep, int n_files, int C, int fpb, int seg_blocks,
                            double doa_thresh, float *ws, double *acc, int *status, void *stream);

/* ------------------------------------------------------------------------------------------------
 * K10 the other heads / losses behind the reference's --loss switch (src/main.py:43)
 *   adyolo_act_fwd/bwd : y[r][c] = c < n_sigmoid_cols ? sigmoid(x) : tanh(x)   (linearheads.py:44-47,65,83)
 *   adyolo_seddoa_loss : w_bce * mean BCE(out[:, :nsed], tgt[:, :nsed]) + w_mse * mean((out[:, nsed:] * m - tgt[:, nsed:])^2),
 *                        m = tgt activity of the column's class when `masked` (SEDDOAloss loss.py:32-54: w = 1, 1000;
 *                        ACCDOAloss loss.py:57-67: nsed = 0, w_mse = 1).  partial: 2*1024 floats.  dout may be NULL.
 *   adyolo_adpit_loss  : ADPITloss (loss.py:70-153): out [rows][9][C], tgt [rows][6][4][C]; 13-permutation min-MSE.
 *                        partial: 1024 floats.
 * ---------------------------------------------------------------------------------------------- */
int adyolo_act_fwd(const float *x, float *y, long rows, int cols, int n_sigmoid_cols, void *stream);
int adyolo_act_bwd(const float *dy, const float *y, float *dx, long rows, int cols, int n_sigmoid_cols,
                   void *stream);
int adyolo_seddoa_loss(const float *out, const float *tgt, float *loss, float *dout, float *partial, long rows,
                       int cols, int nsed, int masked, float w_bce, float w_mse, void *stream);
int adyolo_adpit_loss(const float *out, const float *tgt, float *loss, float *dout, float *partial, long rows,
                      int C, void *stream);

/* Class-wise inference decode (LabelPostProcessor.get_seddoa_output / get_accdoa_output / get_adpit_output,
 * src/datasets.py:536-739), threshold-free: one record of ADYOLO_CLASSWISE_REC(mode) floats per (frame, class),
 * dec [n_frames][C][rec]; by default the conf threshold and the ADPIT unify decision stay on the host
 * (ad-yolo_amd/postprocess.py); adyolo_classwise_select below runs them on the device.
 *   SEDDOA  out [n_frames][4C]: [act = out[c], x, y, z = out[C+c], out[2C+c], out[3C+c]]
 *   ACCDOA  out [n_frames][3C]: [act = sqrt(x*x + y*y + z*z), x, y, z = out[c], out[C+c], out[2C+c]]
 *   ADPIT   out [n_frames][9C] (track k at 3kC): [act0, act1, act2, x0, y0, z0, x1, y1, z1, x2, y2, z2, d01, d12, d20, 0],
 *           d = angular distance in degrees between two tracks (utils/seld_metrics.py:97-114, fp32)
 * Activities are evaluated in that order without contraction (bit-equal to numpy's float32); xyz are copied.
 * dec must be 16-byte aligned.  EINVAL: bad arguments; ENOSUP: unknown mode. */
#define ADYOLO_CLASSWISE_SEDDOA 0
#define ADYOLO_CLASSWISE_ACCDOA 1
#define ADYOLO_CLASSWISE_ADPIT  2
#define ADYOLO_CLASSWISE_REC(mode) ((mode) == ADYOLO_CLASSWISE_ADPIT ? 16 : 4)
int adyolo_classwise_decode(const float *out, float *dec, long n_frames, int C, int mode, void *stream);

/* Class-wise inference selection (csrc/select.hip), opt-in: what postprocess.classwise_select does on the host (the
 * thresholds and, for ADPIT, the unification of get_seddoa_output / get_accdoa_output / get_adpit_output), on the decode
 * above, bit for bit.
 *   dec   [n_frames][C][ADYOLO_CLASSWISE_REC(mode)] from adyolo_classwise_decode, 16-byte aligned
 *   ws    adyolo_classwise_select_workspace_words(n_frames, C, mode) = 2 * n_frames * C words (counts and offsets)
 *   rows  capacity n_frames * C * (mode == ADYOLO_CLASSWISE_ADPIT ? 3 : 1) rows of [frame, class, x, y, z] float32; the
 *         first total rows are written: frames ascending, classes ascending, within a class the order below
 *   frame_counts  [n_frames + 1] int32: rows per frame, then the total at [n_frames] (as adyolo_yolo_select; what
 *         adyolo_seld_score takes)
 *   SEDDOA / ACCDOA: one row (xyz copied) where act > conf_thresh and 1.0f > conf_thresh (the reference tests the boolean
 *   against the threshold a second time).  ADPIT: sed_k = act_k > conf_thresh, q_k = sed_k and 1.0f > conf_thresh; the pairs
 *   (0,1), (1,2), (2,0) are one event when both are sed and d < unify_thresh; with n such pairs
 *     n == 0  the tracks with q_k, in track order
 *     n == 1  the third track if its q holds, then the mean of the pair: (a + b) / 2, (b + d) / 2 or (d + a) / 2
 *     n >= 2  ((a + b) + d) / 3
 *   in float32 with correctly rounded division (float32 compares: the caller rounds the thresholds the way its host
 *   comparison would; unify_thresh is not read for the other modes).  Deterministic: positions come from an exclusive scan
 *   of the per-(frame, class) counts, never from atomics.  No host synchronisation.
 * EINVAL: null pointer, n_frames or C <= 0, dec not 16-byte aligned; ENOSUP: unknown mode, or n_frames * C * 3 rows do not
 * fit 32-bit row counts. */
long adyolo_classwise_select_workspace_words(long n_frames, int C, int mode);
int  adyolo_classwise_select(const float *dec, float *ws, float *rows, int *frame_counts, long n_frames, int C, int mode,
                             float conf_thresh, float unify_thresh, void *stream);

/* Rotation test-time augmentation (csrc/select.hip), opt-in: what postprocess.merge_view_rows does on the host, bit for bit.
 * The same clips are selected under n_views symmetries of the array (augmentations.COMBINATIONS); adyolo_tta_collect parks
 * each view's rows, turned back into the recording's frame, and adyolo_tta_merge keeps what enough views agree on.
 *   pool         [n_views][n_frames][P][4] float32 {class, x, y, z}, 16-byte aligned; pool_counts [n_views][n_frames] int32
 *   ws           adyolo_tta_merge_workspace_words(n_frames, C) words: ONE workspace for the collects and the merge of a batch
 *   status       one int32 the kernels OR ADYOLO_TTA_* bits into
 * adyolo_tta_collect: one view's selection as adyolo_yolo_select / adyolo_classwise_select leave it -- rows (capacity n_rows,
 *   [frame, class, x, y, z]) and frame_counts [n_frames] (the total behind them is not read) -- into slot `view` of the pool.
 *   matrix: the view's signed permutation as a word, so that the call can be captured: component i of the turned-back vector
 *   is sign_i * xyz[src_i], src_i in bits [4 i, 4 i + 2), bit 4 i + 2 set for a negative sign (i.e. p = M^T xyz for the M that
 *   takes a direction to where the view puts it).  A frame with more than P rows keeps its first P (ADYOLO_TTA_ROWS_OVERFLOW);
 *   counts that are negative or run past n_rows, or a class outside [0, C): ADYOLO_TTA_BAD_ROWS.  The rows' positions come
 *   from a scan of the counts.
 * adyolo_tta_merge: per (frame, class) the candidates are the pool's rows of that class, views ascending and within a view in
 *   pool order; u = p / sqrt((px*px + py*py) + pz*pz), a candidate whose norm is zero or not finite is dropped
 *   (ADYOLO_TTA_BAD_VECTOR).  Two candidates are neighbours when (ua.x*ub.x + ua.y*ub.y) + ua.z*ub.z > cos_t; the clusters are
 *   the connected components, seeded at the lowest unassigned candidate, in seed order.  A cluster with members of at least
 *   min_views DISTINCT views gives the row [frame, class, s / |s|], s the sum of its members' u in candidate order, |s| by
 *   the expression above.  All float32, correctly rounded, no contraction.  More than ADYOLO_SELECT_MAX_N candidates in one
 *   (frame, class): that slot stays empty (ADYOLO_TTA_CAND_OVERFLOW).
 *   rows [capacity][5] and frame_counts [n_frames + 1] (the total last): the layout adyolo_yolo_select writes; capacity >=
 *   n_frames * (n_views * P / min_views), which no result exceeds.  Positions come from an exclusive scan, never from atomics;
 *   no host synchronisation.
 * EINVAL: null or misaligned pointer, n_views outside [1, ADYOLO_TTA_MAX_VIEWS], P outside [1, ADYOLO_SELECT_MAX_N], view or
 * min_views out of range, a matrix word that is no signed permutation, too small a capacity; ENOSUP: 32-bit counts overflow. */
#define ADYOLO_TTA_MAX_VIEWS     16
#define ADYOLO_TTA_ROWS_OVERFLOW 1    /* more than P rows of one view in one frame: the first P were kept */
#define ADYOLO_TTA_CAND_OVERFLOW 2    /* more than ADYOLO_SELECT_MAX_N candidates in one (frame, class): left empty */
#define ADYOLO_TTA_BAD_VECTOR    4    /* a row whose vector has a zero or non-finite norm: dropped */
#define ADYOLO_TTA_BAD_ROWS      8    /* frame counts negative or past the rows given, or a class outside [0, C) */
long adyolo_tta_merge_workspace_words(long n_frames, int C);
int  adyolo_tta_collect(const float *rows, long n_rows, const int *frame_counts, float *ws, float *pool, int *pool_counts,
                        int *status, long n_frames, int C, int n_views, int view, int P, unsigned matrix, void *stream);
int  adyolo_tta_merge(const float *pool, const int *pool_counts, float *ws, float *rows, long capacity, int *frame_counts,
                      int *status, long n_frames, int C, int n_views, int P, float cos_t, int min_views, void *stream);

/* Tracks (csrc/track.hip), opt-in: what postprocess.track_rows does on the host, bit for bit.  The rows a selection or
 * adyolo_tta_merge left are linked per (clip, class) into tracks across frames: directions smoothed, gaps of up to max_gap
 * frames filled, tracks of fewer than min_len hits dropped, tracks numbered; the result has the selection's layout.
 *   rows / frame_counts  a selection as adyolo_yolo_select / adyolo_classwise_select / adyolo_tta_merge leave it: rows (capacity
 *                n_rows, [frame, class, x, y, z]; the frame column is not read) and frame_counts [n_clips * t_clip], clip after
 *                clip (the total behind them is not read)
 *   ws           adyolo_track_workspace_words(n_clips * t_clip, C) words, 16-byte aligned; the caller initialises nothing
 *   out_rows [capacity][5], out_ids [capacity] int32, out_counts [n_clips * t_clip + 1] int32 (the total last): the layout
 *                adyolo_yolo_select writes, the frame column the index on the counts axis, and each row's track id;
 *                capacity >= n_clips * t_clip * C * ADYOLO_TRACK_SLOTS, which no result exceeds
 *   status       one int32 the kernels OR ADYOLO_TRACK_* bits into
 * Every (clip, class) on its own; ADYOLO_TRACK_SLOTS slots, each empty or a track {id, s, first, last, hits}; next_id = 0.
 * Per frame t of the clip: (1) the candidates are the class's rows of the frame in row order, the first ADYOLO_TRACK_MAX_DET of
 * them (ADYOLO_TRACK_DET_OVERFLOW), u = p / sqrt((px*px + py*py) + pz*pz), a zero or non-finite norm dropped
 * (ADYOLO_TRACK_BAD_VECTOR); (2) a slot with t - last - 1 > max_gap is closed, and closing a track with hits < min_len erases
 * its cells of frames first .. last; (3) greedy rounds match the unmatched slot and candidate with the largest
 * (s.x*u.x + s.y*u.y) + s.z*u.z > cos_gate (ties: the lowest slot, then the lowest candidate); (4) a matched slot gets
 * m = unit((s * b) + (u * a)), the frames of the gap behind it unit((s * (1 - w)) + (m * w)), w = g / (gap + 1), then s = m,
 * last = t, hits += 1; (5) the unmatched candidates in order open the lowest empty slots (s = u, id = next_id++), and one that
 * finds none is dropped (ADYOLO_TRACK_SLOT_OVERFLOW).  The clip's end closes every slot.  Rows: frames ascending, classes
 * ascending, slots ascending.  All float32, correctly rounded, no contraction.  cos_gate = cos of the gate angle, a the weight
 * of the new direction, b = 1 - a, all rounded by the caller.  A frame whose count is negative or runs past n_rows has no rows,
 * a row whose class is no integer in [0, C) is skipped: ADYOLO_TRACK_BAD_ROWS; nothing is read out of range.  Positions come
 * from exclusive scans, never from atomics; no host synchronisation.
 * EINVAL, before any launch: null or misaligned pointer, n_clips * t_clip < 1, C < 1, max_gap < 0, min_len < 1, cos_gate
 * outside (0, 1), a outside (0, 1], too small a capacity; ENOSUP: 32-bit counts overflow. */
#define ADYOLO_TRACK_SLOTS         8    /* concurrent tracks per clip and class */
#define ADYOLO_TRACK_MAX_DET       64   /* detections considered per frame and class */
#define ADYOLO_TRACK_DET_OVERFLOW  1    /* more than ADYOLO_TRACK_MAX_DET rows in one (frame, class): the first were taken */
#define ADYOLO_TRACK_SLOT_OVERFLOW 2    /* a detection found no empty slot: dropped */
#define ADYOLO_TRACK_BAD_VECTOR    4    /* a row whose vector has a zero or non-finite norm: dropped */
#define ADYOLO_TRACK_BAD_ROWS      8    /* frame counts negative or past the rows given, or a class outside [0, C) */
long adyolo_track_workspace_words(long n_frames, int C);
int  adyolo_track_rows(const float *rows, long n_rows, const int *frame_counts, long n_clips, int t_clip, int C,
                       float cos_gate, int max_gap, int min_len, float a, float b, float *ws, float *out_rows, int *out_ids,
                       long capacity, int *out_counts, int *status, void *stream);

/* Tracks through runs (csrc/track.hip), opt-in: what postprocess.track_run does on the host, bit for bit -- adyolo_track_rows
 * on a stream of recordings that arrives in runs of frames (the passes of a windowed evaluation), the state carried from one
 * call to the next.  A recording linked through any number of runs gives, concatenated, what adyolo_track_rows gives on it
 * whole (n_clips = 1): rows, counts, ids, status bits.
 *   rows / frame_counts [run_frames]  as adyolo_track_rows
 *   segments     [n_segments][4] int32 ON THE DEVICE, one row per recording the run holds frames of: {first frame in the run,
 *                frames (>= 1), continues, open}.  The rows tile the run in order.  continues (row 0 only): the recording's
 *                earlier frames were walked by the call that left `carry`; open (the last row only): it goes on in the next run
 *   hold         D >= H frames, H = max_gap for min_len 1, else (min_len - 1) * (max_gap + 1) + 1: how far behind the frame
 *                being walked a gap fill or the erasure of a short track can write (postprocess.track_hold)
 *   carry        adyolo_track_carry_words(C, hold) words, 16-byte aligned, all zero before a stream's first call, otherwise
 *                untouched by the caller: read when row 0 continues, written by every call (emptied when the last row is not open)
 *   ws           adyolo_track_run_workspace_words(run_frames, C, hold) words, 16-byte aligned; the caller initialises nothing
 *   out_rows [capacity][5], out_ids [capacity], capacity >= (hold + run_frames) * C * ADYOLO_TRACK_SLOTS
 *   out_counts   [hold + run_frames + 2] int32: the EMITTED frames' counts, zeros behind them, at [hold + run_frames] the row
 *                total, at [hold + run_frames + 1] the number of emitted frames
 * One wave per (segment, class).  A continuing segment starts from the carried slots and next_id, every other one empty.  A
 * segment that is not open closes every slot at its end, as a clip's end does.  An open one keeps its slots, next_id and the
 * cells of its last min(D, frames walked so far in the recording) frames -- the held frames -- in the carry.  Emitted: the
 * carried held frames first, then the run's frames without the newly held ones; the frame column is the index among them.
 * On the device, ADYOLO_TRACK_BAD_ROWS and nothing linked or emitted: a segment table that does not tile the run or carries a
 * flag on another row than stated, or (row 0 continuing) a carry no call leaves behind; nothing is read out of range.
 * EINVAL, before any launch: as adyolo_track_rows, and n_segments outside [1, run_frames], hold < H; ENOSUP: 32-bit counts. */
long adyolo_track_carry_words(int C, int hold);
long adyolo_track_run_workspace_words(long run_frames, int C, int hold);
int  adyolo_track_run(const float *rows, long n_rows, const int *frame_counts, long run_frames, const int *segments,
                      long n_segments, int C, float cos_gate, int max_gap, int min_len, float a, float b, int hold, float *carry,
                      float *ws, float *out_rows, int *out_ids, long capacity, int *out_counts, int *status, void *stream);

/* The detection CSV files as bytes (csrc/csv.hip, csrc/csv_format.hpp), opt-in: what postprocess.format_rows does on the
 * host, byte for byte -- the lines write_seld_output_file writes, "frame,class,id,x,y,z\n" with repr(float(float32)) floats, for
 * rows already on the device; all files of the call in one buffer.
 *   rows / frame_counts [n_frames]  a selection as adyolo_yolo_select / adyolo_classwise_select / adyolo_tta_merge /
 *                adyolo_track_rows / adyolo_track_run leave it (capacity n_rows; the frame column is not read; nothing behind
 *                the first sum(frame_counts) rows is read)
 *   ids          [n_rows] int32 track ids for the third column, or NULL: 0
 *   segments     [n_segments][2] int32 ON THE DEVICE: {first frame of the segment on the counts axis, the number that frame has
 *                in its file}; ascending, the first at frame 0.  A segment is one file's span.
 *   ws           ADYOLO_CSV_WORKSPACE_WORDS(n_frames, n_rows) 32-bit words, 16-byte aligned; the caller initialises nothing
 *   out          [capacity] bytes, 16-byte aligned: the lines, segment after segment
 *   seg_bytes    [n_segments + 1] int64: where each segment's bytes start in out, the total last
 *   status       one int32 the kernels OR ADYOLO_CSV_* bits into
 * A frame's number is seg.number + (frame - seg.first) of the last segment that starts at or before it.  class is the float
 * truncated; a class that is not finite or not within int32, or a negative id, is written as 0 and reported
 * (ADYOLO_CSV_BAD_VALUE).  A total above the capacity: ADYOLO_CSV_OVERFLOW, seg_bytes are the true offsets (the last is the
 * capacity to come back with) and NOTHING is written to out.  Frame counts that are negative or sum to more than n_rows
 * (ADYOLO_CSV_BAD_COUNTS), a table that is not as above (ADYOLO_CSV_BAD_TABLE): nothing is formatted, seg_bytes are zero.
 * Positions come from scans, never from atomics; nothing is written behind the total; no host synchronisation.
 * EINVAL, before any launch: null or misaligned pointer, n_frames < 1, n_segments < 1; ENOSUP: 32-bit counts overflow. */
#define ADYOLO_CSV_OVERFLOW    1    /* more bytes than the capacity: nothing was written, seg_bytes hold the need */
#define ADYOLO_CSV_BAD_COUNTS  2    /* frame counts negative or past the rows given */
#define ADYOLO_CSV_BAD_VALUE   4    /* a class not finite or outside int32, or a negative id: written as 0 */
#define ADYOLO_CSV_BAD_TABLE   8    /* a segment table not ascending from frame 0 within the frames */
#define ADYOLO_CSV_LINE_MAX    110  /* no line is longer */
#define ADYOLO_CSV_WORKSPACE_WORDS(n_frames, n_rows) (2 * (((n_rows) + 255) / 256) + 4 + (n_frames))
int  adyolo_csv_format(const float *rows, long n_rows, const int *frame_counts, long n_frames, const int *ids,
                       const int *segments, long n_segments, void *ws, unsigned char *out, long capacity, long long *seg_bytes,
                       int *status, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Input pipeline around K1.
 *   adyolo_pcm16_to_f32: staged WAV samples int16 -> float, x / 32768 + 1e-8 (src/datasets.py:105, src/preprocess.py:104)
 *   adyolo_mask_ranges:  SpecAug (src/utils/augmentations.py:6-33) on feat [B][T][F][C]: per sample zero frames [t0,t1) and
 *                        mel bins [f0,f1); ranges [B][4] int32 = {t0, t1, f0, f1}, an empty range masks nothing
 *   adyolo_mask_groups:  SpecAug per channel group (the reference masks MEL and IV each with its own draw, src/datasets.py:
 *                        158-159) on feat [B][T][F][C], C % 4 == 0: per sample b and group g zero frames [t0,t1) x all bins
 *                        and bins [f0,f1) x all frames of the group's float4 quads [q0,q1) (channels 4 q0 .. 4 q1 - 1).
 *                        ranges: DEVICE int32 [B][G][4] = {t0, t1, f0, f1}, clamped to [0,T] / [0,F] on the device (any value is
 *                        safe); group_quads: HOST int32 [G][2] = {q0, q1}, 0 <= q0 <= q1 <= C/4, G <= ADYOLO_MASK_MAX_GROUPS
 *                        (passed by value: capturable in a hipGraph).  Writes only the masked elements; no sync, no memset.
 *                        adyolo_mask_ranges is its one-group case (group_quads {0, C/4}).
 *   adyolo_feat_augment: frequency shift, the SpecAug stripes of adyolo_mask_groups and one cutout rectangle on feat
 *                        [B][T][64][C] in ONE launch, in place (no second feature-sized buffer).  table: DEVICE int32
 *                        [B][G + 2][4]; rows 0..G-1 = the ranges of adyolo_mask_groups, row G = the rectangle {t0, t1, f0, f1}
 *                        zeroed in ALL C channels (empty in either direction: nothing), row G + 1 = {s, 0, 0, 0}.  Per sample,
 *                        in this order: with s' = clamp(s, -63, 63) != 0 every quad of a group g with bit g of shift_mask set
 *                        moves along the bin axis, out[t][f] = in[t][src(f)], u = f - s', src = -u (u < 0), 126 - u (u > 63),
 *                        u otherwise (numpy.pad mode "reflect", cropped to 64 bins); then the stripes; then the rectangle.
 *                        Fill value 0.  Every table value is clamped on the device (any value is safe); a sample with s' = 0
 *                        is write-only (its masked elements), a masked element is never loaded.  group_quads as for
 *                        adyolo_mask_groups (host, by value).  No allocation, no sync: capturable.  EINVAL: null / misaligned
 *                        pointers, sizes as adyolo_mask_groups, shift_mask bits at or above G; ENOSUP: F != 64.
 *   adyolo_colstats:     per-column sum, sum of squares, max, min of a [rows][cols] fp32 matrix -> out [4][cols] float64
 *                        (train-set scaler statistics, src/preprocess.py:86-130); partial = [4][1024][cols] fp32 scratch
 * ---------------------------------------------------------------------------------------------- */
int adyolo_pcm16_to_f32(const int16_t *pcm, float *out, long n, void *stream);
int adyolo_mask_ranges(float *feat, const int32_t *ranges, int B, int T, int F, int C, void *stream);
#define ADYOLO_MASK_MAX_GROUPS 8
int adyolo_mask_groups(float *feat, const int32_t *ranges, int B, int G, int T, int F, int C, const int32_t *group_quads,
                       void *stream);
int adyolo_feat_augment(float *feat, const int32_t *table, int B, int G, int T, int F, int C, const int32_t *group_quads,
                        unsigned shift_mask, void *stream);
int adyolo_colstats(const float *a, float *partial, double *out, long rows, int cols, void *stream);

/* General strided convolution (channels-last) as an implicit GEMM on the fp32 MFMA, no column buffer (replaces nn.Conv2d
 * 7x7 s(1,2) at reference resnet_conformer.py:347 and torchvision BasicBlock's 3x3 / 1x1 s(1,2) at :353-393; forward,
 * data-gradient and weight-gradient).  Cin, Cout multiples of 4.  Kp = roundup4(KH*KW*Cin), Kq = roundup4(KH*KW*Cout).
 *   mode 0: src = x [N][H][W][Cin],     other = wk  [Cout][Kp] (k = (kh*KW+kw)*Cin + ci),  out = y  [N][Ho][Wo][Cout]
 *   mode 1: src = dy [N][Ho][Wo][Cout], other = wkT [Cin][Kq]  (k = (kh*KW+kw)*Cout + co), out = dx [N][H][W][Cin]
 *   mode 2: src = x,                    other = dy,                                         out = dwk [Cout][Kp]
 * splits (mode 2 only): split-K over the N*Ho*Wo output pixels, slabs = [splits][Cout][Kp] workspace (deterministic sum). */
int adyolo_conv_gemm(const float *src, const float *other, float *out, float *slabs, int mode, int N, int H, int W,
                     int Cin, int Cout, int KH, int KW, int SH, int SW, int PH, int PW, int splits, void *stream);
/* host only, no launch: what adyolo_conv_gemm decides for these arguments, refused with the same codes.  out8 =
 *   [0] M, [1] N, [2] K of the GEMM (mode 0: pixels of y x Cout x Kp; mode 1: pixels of dx x Cin x Kq; mode 2: Cout x Kp x pixels of y)
 *   [3] klen: the K range of one split (whole K tiles of 32),  [4] the splits that are not empty with it (1 in modes 0 / 1)
 *   [5] fastg: bit 0 / 1 = the plain operand A (mode 2: dy) / B (modes 0 / 1: the packed filter) may go through a buffer
 *       descriptor -- the kernel takes it for a k-major operand only, so never for mode 2's transposed dy; bit 2 = the gathered
 *       pixel operand of modes 0 / 1 goes through a descriptor (tap in the scalar offset)
 *   [6] fastk (modes 0 / 1): the (c, kh, kw) triple of a K tile is carried, not divided (source channels % 32 == 0)
 *   [7] fastp (mode 2): the pixel triple of a K row is carried (32 % Wo == 0 and Ho >= 32 / Wo) */
int adyolo_conv_gemm_plan(int mode, int N, int H, int W, int Cin, int Cout, int KH, int KW, int SH, int SW, int PH, int PW,
                          int splits, int *out8);

/* ------------------------------------------------------------------------------------------------
 * K9  ResNet-Conformer encoder pieces (src/models/backbones/resnet_conformer.py), channels-last fp32
 *   pack_wk : filter layout of adyolo_conv_gemm; rows of `wk` are (kh, kw, c)-ordered and padded to a multiple of 4 floats
 *       (Kp).  Used for the 7x7 s(1,2) stem (:347) and the torchvision BasicBlock 3x3 / 1x1 s(1,2) convolutions (:353-393).
 *   maxpool3 : MaxPool2d(3, stride (1,2), padding 1) (:350); arg = arg-max tap per output (uint8); bwd atomically
 *       adds into a ZEROED dx.
 *   affine_relu, relu_bwd, axpby : BN->ReLU of BasicBlock, residual mixing a*x + b*z (:98)
 *   swish (:142-150), glu over the channel axis (:167), dwconv3: depthwise Conv1d k=3, dilation d, padding d (:169)
 *       (flip = 1 gives the data gradient), softmax rows with a pre-scale (:73-76), avgpool1d(k) * fac (:288-294),
 *   ln : LayerNorm(256).
 * ---------------------------------------------------------------------------------------------- */
int adyolo_pack_wk(float *w, float *wk, int Cout, int Cin, int KH, int KW, int to_packed, void *stream);
int adyolo_maxpool3_fwd(const float *x, float *y, unsigned char *arg, int N, int H, int W, int C, void *stream);
int adyolo_maxpool3_bwd(const float *dy, const unsigned char *arg, float *dx_zeroed, int N, int H, int W, int C,
                        void *stream);
int adyolo_affine_relu_nhwc(const float *x, const float *scale, const float *shift, float *y, long rows, int C,
                            void *stream);
int adyolo_relu_bwd(const float *dy, const float *y, float *dx, long n, void *stream);
int adyolo_axpby(const float *x, const float *z, float *y, float a, float b, long n, void *stream);
/* y = a * dropout(x) + b * z in one pass (z NULL: y = a * dropout(x), the gradient w.r.t. x); mask = the stateless stream of
 * adyolo_dropout_apply(_dev) -- ResidualConnectionModule (resnet_conformer.py:98) on a sub-module that ends in nn.Dropout
 * (:209 FeedForwardModule, :178 ConformerConvModule, :272-274 attention branch); same rounding as the two separate calls. */
int adyolo_dropout_axpby(const float *x, const float *z /*or NULL*/, float *y, long n, float p, uint64_t seed, uint64_t offset,
                         const uint64_t *offset_dev /*or NULL*/, float a, float b, void *stream);
int adyolo_swish_fwd(const float *x, float *y, long n, void *stream);
int adyolo_swish_bwd(const float *dy, const float *x, float *dx, long n, void *stream);
int adyolo_glu_fwd(const float *x, float *y, long rows, int C, void *stream);
int adyolo_glu_bwd(const float *dy, const float *x, float *dx, long rows, int C, void *stream);
int adyolo_dwconv3_fwd(const float *x, const float *w, const float *bias, float *y, int B, int T, int C,
                       int dilation, int flip, void *stream);
int adyolo_dwconv3_wgrad(const float *dy, const float *x, float *dw, float *db, float *partial, float *colsum_ws,
                         int B, int T, int C, int dilation, void *stream);
int adyolo_softmax_fwd(const float *s, float *p, long rows, int L, float scale, void *stream);
int adyolo_softmax_bwd(const float *dp, const float *p, float *ds, long rows, int L, float scale, void *stream);
int adyolo_avgpool1d_fwd(const float *x, float *y, int B, int T, int C, int k, float fac, void *stream);
int adyolo_avgpool1d_bwd(const float *dy, float *dx, int B, int T, int C, int k, float fac, void *stream);

/* ------------------------------------------------------------------------------------------------
 * K9w  1-D Winograd F(4, 3) along the time axis for the stride-1 3x3 convolutions of the ResNet-Conformer's deep stages, whose
 *      maps are 1 bin wide (or 2 bins, folded into the channels): there torchvision BasicBlock's convolution (reference
 *      resnet_conformer.py:353-393) IS a 3 x 1 one.  H % 4 == 0, C % 4 == 0; T = H / 4 tiles per sample.
 *   wino1d_in     : x  [N][H][C] -> V [6][N T][C]  (B^T over the rows 4 t - 1 .. 4 t + 4; rows outside the sample are zeros)
 *   wino1d_out    : M  [6][N T][C] -> y [N][H][C]  (A^T)
 *   wino1d_dy     : dy [N][H][C] -> E [6][N T][C]  (A: the output gradient in the transform domain, for the weight gradient)
 *   wino1d_filter : mode 0  U[p][co][ci] = sum_k G[p][k] w[co][ci][k]        (forward)
 *                   mode 1  U[p][ci][co] = sum_k G[p][k] w[co][ci][2 - k]    (data gradient)
 *                   mode 2  w[co][ci][k] = sum_p G[p][k] U[p][co][ci]        (weight gradient from dU; writes w)
 *   The six position GEMMs between them are ONE adyolo_gemm_batched launch each way (M[p] = V[p] U[p]^T, dU[p] = E[p]^T V[p]).
 * ---------------------------------------------------------------------------------------------- */
int adyolo_wino1d_in(const float *x, float *V, int N, int H, int C, void *stream);
int adyolo_wino1d_out(const float *M, float *y, int N, int H, int C, void *stream);
int adyolo_wino1d_dy(const float *dy, float *E, int N, int H, int C, void *stream);
int adyolo_wino1d_filter(float *w, float *U, int Cout, int Cin, int mode, void *stream);
int adyolo_ln_fwd(const float *x, const float *gamma, const float *beta, float *y, long R, int C, float eps,
                  void *stream);
int adyolo_ln_bwd(const float *dy, const float *x, const float *gamma, float *dx, float *dgamma, float *dbeta,
                  float *partial, long R, int C, float eps, void *stream);

/* FOA rotation augmentation on raw audio (src/utils/augmentations.py:81-96): audio/out [B][n_samples][4] (W,Y,Z,X),
 * cfg [B][4] = {sign_y, sign_z, sign_x, swap_xy}.  Label angles are remapped on the host (augmentations.RotationAug). */
int adyolo_foa_rotate(const float *audio, float *out, const float *cfg, int B, long n_samples, void *stream);

/* FOA rotation followed by a yaw about the vertical axis (aug_config.yaw_rotation_augment, augmentations.rotate_audio_yaw; the
 * host-fed path): audio/out [B][n_samples][4] (W,Y,Z,X), 16-byte aligned; cfg DEVICE float [B][6] = {sign_y, sign_z, sign_x,
 * swap_xy, cos, sin} (augmentations.yaw_cos_sin).  Per frame the result (W, Y, Z, X) of adyolo_foa_rotate, then
 * Y' = fl(fl(Y c) + fl(X s)), X' = fl(fl(X c) - fl(Y s)): every product and sum rounded to float32, no FMA.  cos = 1, sin = 0
 * gives the bits of adyolo_foa_rotate (on frames without -0.0). */
int adyolo_foa_rotate_yaw(const float *audio, float *out, const float *cfg, int B, long n_samples, void *stream);

/* MIC channel-swap augmentation on raw audio (augmentations.swap_audio; the MIC-format counterpart of adyolo_foa_rotate):
 * audio/out [B][n_samples][4] (capsules M1..M4), 16-byte aligned, out-of-place only (out must not overlap audio);
 * src_dev DEVICE int32 [B][4]: out[b][i][j] = audio[b][i][src_dev[b][j] & 3] -- the selectors are masked in the kernel, so no
 * table value addresses outside the frame; the values are moved, not computed on (NaN payloads and -0.0 keep their bits).
 * Label angles are remapped on the host by the same combination (augmentations.rotate_labels). */
int adyolo_mic_swap(const float *audio, float *out, const int *src_dev, int B, long n_samples, void *stream);

/* Time-domain mixing on raw audio (aug_config.time_mix_augment, the host-fed path; the corpus paths mix inside
 * adyolo_corpus_gather): audio / mate / out [B][n_samples][4] float32, 16-byte aligned; gains DEVICE float [B]; mixed DEVICE
 * bytes [B] (0: the clip is not mixed).  out[b] = mixed[b] ? audio[b] + gains[b] * mate[b] : audio[b], the product rounded to
 * float32 before the sum (no FMA: the bits of ``audio + gain * mate`` on float32 tensors).  An unmixed clip is moved, not
 * computed on (NaN payloads and -0.0 keep their bits), and its mate and gain are not read.  out may be audio itself (in place)
 * or a buffer apart from it; it must not overlap mate. */
int adyolo_audio_mix(const float *audio, const float *mate, const float *gains, const unsigned char *mixed, float *out, int B,
                     long n_samples, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Training batches from an HBM-resident corpus (csrc/corpus.hip, ad-yolo_amd/corpus.py DeviceCorpus / ClasswiseDeviceCorpus),
 * opt-in: the host half of FoaDataset.__getitem__ + audio_collate_fn (src/datasets.py:93-184) on the device, from one small
 * per-batch item table.
 *   items    DEVICE int64 [B][ADYOLO_CORPUS_ITEM_WORDS] = {sample offset into pcm (frames), frame offset of the label window on
 *            its recording's frame axis, first event of the window in `events`, number of events, FOA combination (0..15, or -1:
 *            no rotation -- labels are then not wrapped either), recording, 0, 0}
 *   rot_host HOST float [16][ADYOLO_CORPUS_ROT_WORDS] = {sign_y, sign_z, sign_x, swap_xy, azimuth weight, azimuth offset,
 *            elevation weight, 0} per combination (augmentations.COMBINATIONS; passed by value: capturable)
 *   status   DEVICE int32 word the calls OR their ADYOLO_CORPUS_* bits into (never cleared by them)
 * Each stage has one entry point.  Two optional arguments, the same for every stage, select its form:
 *   mates    NULL: a plain batch.  Else time-domain mixing (aug_config.time_mix_augment: the audio of two chunks summed, their
 *            labels united): DEVICE int64 [B][ADYOLO_CORPUS_ITEM_WORDS], the chunk mixed into item b as an item row with its own
 *            combination; word 0 (sample offset) exactly -1: item b has no mate and the rest of the row is not read; any other
 *            offset outside pcm is a bad item; word 6: the bit pattern of the float32 gain g (zero-extended).  An item without a
 *            mate gets the plain form's bits.
 *   a yaw    (aug_config.yaw_rotation_augment, FOA only; gather: yaw_tab, AD-YOLO labels: the flag ``yaw``, class-wise labels:
 *            yaw_az + yaw_el) absent: word 7 of the rows is never read.  Else every source is turned about the vertical axis
 *            after its combination by its own yaw, word ADYOLO_CORPUS_YAW_WORD (7) of the item row and of the mate row (word 6
 *            of a mate stays the gain): WHOLE DEGREES as a signed integer, legal in [-180, 180); 0 turns nothing.  A row whose
 *            yaw is outside that range is a bad item, as a combination >= 16 is.
 * adyolo_corpus_gather: audio [B][n][4] float32 = the int16 frames pcm[off .. off + n) as x / 32768 + 1e-8, then
 *     mic_src_host NULL (the FOA form; rot_host required): channels (W,Y,Z,X) rotated like adyolo_foa_rotate -- bit for bit
 *       adyolo_pcm16_to_f32 followed by adyolo_foa_rotate;
 *     mic_src_host given (the MIC form; rot_host is not read): the capsules M1..M4 permuted by the item's combination -- bit for
 *       bit adyolo_pcm16_to_f32 followed by adyolo_mic_swap.  mic_src_host HOST uint32 [16], one word per combination: source
 *       channel s_j of output channel j in bits [8 j, 8 j + 2) (augmentations.mic_swap_source; passed by value: capturable), or
 *       ADYOLO_MIC_SWAP_NONE where the combination is no symmetry of the array, which makes the item a bad one.  comb < 0: no
 *       permutation (the bits of the FOA form with comb < 0).  The label calls are the same for both formats;
 *     yaw_tab given (FOA form only: with mic_src_host EINVAL -- there is no MIC yaw): each source's frames yawed after its
 *       combination -- bit for bit adyolo_pcm16_to_f32 -> adyolo_foa_rotate_yaw.  yaw_tab DEVICE float [360][2] = {cos, sin} of
 *       the yaws -180 .. 179 (augmentations.yaw_cos_sin), 8-byte aligned; entry yaw + 180 is read once per workgroup.  comb < 0:
 *       the yaw alone;
 *     mates given: audio [b] = a + g * m, where a is what the call writes for item b without mates and m what it would write
 *       for the mate row, each under its own combination (and yaw); the product is rounded to float32 before the sum (no FMA):
 *       bit for bit two gathers and ``a + g * m`` on float32 tensors.  An item without a mate costs the plain gather's bytes.
 *   pcm [n_total][4] int16, 16-byte aligned; an item (or its mate) outside it, a combination >= 16: zeros for the whole sample
 *   and ADYOLO_CORPUS_BAD_ITEM.  One pass; every parity of the two offsets and an odd n are legal.
 * adyolo_corpus_yolo_labels: the AD-YOLO rows of the batch (datasets.get_yolo_label + collate_fn): per item, per event
 *   [b, frame - frame offset, gi, gj, cls, U, V] for every responsible cell in (gi, gj) order, the rotation of
 *   augmentations.rotate_labels and the cell test of YoloLabelEncoder.encode_events in double, events whose relative frame is
 *   >= n_label_frames dropped.  events DEVICE double [n_events][4] = {frame, class, azimuth, elevation}; grid_bounds DEVICE
 *   double [2 Gaz + 2 Gel] = az_lb, az_ub, el_lb, el_ub (YoloLabelEncoder); target [cap][7] float32: the first count[0] rows
 *   written (at most cap; more sets ADYOLO_CORPUS_OVERFLOW, the rows past cap are dropped), b = -1 in the others (the loss
 *   skips them); ws adyolo_corpus_yolo_labels_workspace_words(B, max_events, mix) int32 words, mix = mates given: B (mix ? 2 :
 *   1) max(max_events, 1), -1 for B <= 0 or max_events < 0; max_events >= every item's (and mate's) event count (a larger count
 *   sets ADYOLO_CORPUS_BAD_ITEM and the item gets no rows).  Gaz, Gel <= 64, else ENOSUP.
 *     mates given: the rows of augmentations.merge_labels(item, mate) per item: frames ascending, the item's events before the
 *       mate's within a frame (both sources' events must be frame-sorted, as load_chunked_split leaves them), each event rotated
 *       by its own source's combination and counted from its own source's frame offset; column 0 is the item for both.  An
 *       item whose own row or mate row is bad gets no rows at all.  An all-unmixed batch equals the plain rows.
 *     yaw != 0: augmentations.yaw_labels after the combination's arithmetic: az = az + yaw, then < -180: += 360, > 180: -= 360,
 *       in double and uncontracted, before the 180 -> -180 rule of the encoder.  Any angles.
 * adyolo_corpus_classwise_labels: the dense SEDDOA / ACCDOA / ADPIT targets of the batch (augmentations.rotate_labels, then
 *   datasets.ClasswiseLabelEncoder, stacked over the batch), every element of target written exactly once, zeros included:
 *     format ADYOLO_CORPUS_SEDDOA  target [B][n_label_frames][4 C]        = [se, x, y, z], the last event of a class in a frame
 *     format ADYOLO_CORPUS_ACCDOA  target [B][n_label_frames][3 C]        = se * [x, y, z], the same event
 *     format ADYOLO_CORPUS_ADPIT   target [B][n_label_frames][6][4][C]    = {1, x, y, z} in slot 0 (one event of the class in
 *                                  the frame), 1-2 (two) or 3-5 (three or more: the first three in file order)
 *   C = n_classes.  events as above (only the frame and class columns are read; file order within a frame); xyz DEVICE float
 *   [n_events][ADYOLO_CORPUS_XYZ_SLOTS][3]: each event's direction vector built on the host (corpus.xyz_table), slot 0 without
 *   rotation (comb < 0), slot 1 + k under combination k.  Events whose relative frame is outside [0, n_label_frames) are
 *   dropped; an event whose class is outside [0, C) is dropped and sets ADYOLO_CORPUS_BAD_CLASS; an item outside the corpus
 *   (as for the rows, max_events included) gets an all-zero target and sets ADYOLO_CORPUS_BAD_ITEM.  No workspace, no
 *   atomics on the target: capturable, and the target may be a recorded step's static buffer.  C <= 256, else ENOSUP.
 *     mates given: the dense targets of the merged events: SEDDOA / ACCDOA take the last event of a class in a frame in
 *       item-then-mate order (the mate's wins a collision), ADPIT counts over both sources and keeps the first three in that
 *       order; each direction vector comes from the xyz slot of its own source's combination.  n_events < 2^30.  Bad items
 *       (either row) and bad classes as without mates.
 *     yaw_az and yaw_el given (together or not at all: one without the other is EINVAL; rot_host, as above, is then required
 *       and otherwise not read): z of an event is still read from its xyz slot; x = (float)(cos_az * cos_el) and y =
 *       (float)(sin_az * cos_el), one double product each, from yaw_az DEVICE double [361][2] = {cos, sin} of the azimuths
 *       -180 .. 180 and yaw_el DEVICE double [181] = cos of the elevations -90 .. 90, both 8-byte aligned, built on the host
 *       with the expressions of datasets._polar_to_xyz (ops.corpus_yaw_xyz_tables) and indexed by the event's moved angles (as
 *       in adyolo_corpus_yolo_labels with yaw).  The events' angles must be whole degrees (corpus.ClasswiseDeviceCorpus refuses
 *       any other split); an angle that is not indexes entry 0.
 * ---------------------------------------------------------------------------------------------- */
#define ADYOLO_CORPUS_ITEM_WORDS 8
#define ADYOLO_CORPUS_YAW_WORD   7   /* with a yaw: the row's yaw in whole degrees, [-180, 180) */
#define ADYOLO_CORPUS_ROT_WORDS  8
#define ADYOLO_CORPUS_OVERFLOW   1   /* more rows than the target capacity */
#define ADYOLO_CORPUS_BAD_ITEM   2   /* an item table entry outside the corpus */
#define ADYOLO_CORPUS_BAD_CLASS  4   /* an event class outside [0, n_classes) */
#define ADYOLO_CORPUS_XYZ_SLOTS  17  /* no rotation + the 16 FOA combinations */
#define ADYOLO_CORPUS_SEDDOA     0
#define ADYOLO_CORPUS_ACCDOA     1
#define ADYOLO_CORPUS_ADPIT      2
#define ADYOLO_MIC_SWAP_NONE     0xffffffffu  /* mic_src_host word of a combination that is no symmetry of the array */
int  adyolo_corpus_gather(const int16_t *pcm, long n_total, const int64_t *items, const int64_t *mates /* NULL: plain */,
                          int B, long n, const float *rot_host, const unsigned int *mic_src_host /* NULL: FOA form */,
                          const float *yaw_tab /* NULL: no yaw */, float *audio, int *status, void *stream);
long adyolo_corpus_yolo_labels_workspace_words(int B, int max_events, int mix);
int  adyolo_corpus_yolo_labels(const double *events, long n_events, const int64_t *items, const int64_t *mates /* NULL: plain */,
                               int B, int max_events, int n_label_frames, const double *grid_bounds, int Gaz, int Gel,
                               const float *rot_host, int yaw, int *ws, float *target, long cap, int *count, int *status,
                               void *stream);
int  adyolo_corpus_classwise_labels(const double *events, const float *xyz, long n_events, const int64_t *items,
                                    const int64_t *mates /* NULL: plain */, int B, int max_events, int n_label_frames,
                                    int n_classes, int format, const float *rot_host /* read with yaw only */,
                                    const double *yaw_az, const double *yaw_el /* both NULL: no yaw */, float *target,
                                    int *status, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Windowed inference (corpus.InferDeviceCorpus, test.infer_epoch_corpus): recordings of any length cut into overlapping
 * windows of ONE shape, each pass of W windows made and stitched on the device from a table uploaded once.
 *   windows  DEVICE int64 [W][ADYOLO_WINDOW_WORDS] = {sample offset into pcm (frames), valid samples, src_lo (first kept label
 *            frame, window-local), dst (its place on the frame axis of all recordings laid end to end), n (kept frames),
 *            recording, 0, 0}; an empty window (the filler of the last pass) has valid = 0 and n = 0
 * adyolo_corpus_gather_windows: audio [W][n][4] float32 = the int16 frames pcm[off .. off + valid) as x / 32768 + 1e-8 (the
 *   arithmetic of adyolo_corpus_gather with comb < 0, element for element), then n - valid frames of int16 zero, 1e-8f, which
 *   are not read from pcm (behind a recording lies the next one).  valid = 0: all 1e-8f, nothing else of the row is read.
 *   Offsets are whole label hops, so even: an odd or negative offset, valid outside [0, n] or off + valid > n_total gives
 *   zeros for that window and sets ADYOLO_CORPUS_BAD_ITEM.  pcm and audio 16-byte aligned; audio may be a recorded graph's
 *   static input.
 * adyolo_corpus_gather_windows_view: the same gather under ONE combination comb for the whole launch, passed by value (rotation
 *   test-time augmentation through windows: a further view of a pass, written into the same static input).  The two forms of
 *   adyolo_corpus_gather:
 *     mic_src_host NULL (rot_host, as above, required): FOA, bit for bit adyolo_corpus_gather_windows then adyolo_foa_rotate
 *       under comb -- the frames past valid included: the padding is the conversion of int16 zero under the same signs and
 *       swap (+-1e-8f), not a constant;
 *     mic_src_host given: MIC, bit for bit adyolo_corpus_gather_windows then adyolo_mic_swap; a combination whose word is
 *       ADYOLO_MIC_SWAP_NONE is what it is to adyolo_corpus_gather: zeros for every window and ADYOLO_CORPUS_BAD_ITEM.
 *   comb <= 0 (no view, or the identity): the bits of adyolo_corpus_gather_windows; comb >= 16: EINVAL.  Bad window rows and
 *   valid = 0 as above (the zeros of a bad window are +0).  The signs, the swap and the byte selectors are kernel arguments,
 *   worked out on the host: nothing is read per element but the stream.  Not for capture into a graph that is replayed under
 *   another combination: the call stays outside the recorded graph and writes its input.
 * adyolo_decode_stitch: for each window w, n frame records of rec floats from decoded[(w Wf + src_lo) ..] to
 *   out[(dst - pass_base) ..]: the pass's kept frames compacted into one run in window order.  decoded [W Wf][rec], out
 *   [out_frames][rec] (rec: whatever the decode writes per frame); 16-byte copies where rec % 4 == 0 (both buffers 16-byte
 *   aligned then), 4-byte copies otherwise.  A window with src_lo < 0, n < 0, src_lo + n > Wf or a destination outside
 *   [0, out_frames) is not copied and sets ADYOLO_CORPUS_BAD_ITEM.  The frames of out no window names are left as they are.
 * ---------------------------------------------------------------------------------------------- */
#define ADYOLO_WINDOW_WORDS 8
int  adyolo_corpus_gather_windows(const int16_t *pcm, long n_total, const int64_t *windows, int W, long n, float *audio,
                                  int *status, void *stream);
int  adyolo_corpus_gather_windows_view(const int16_t *pcm, long n_total, const int64_t *windows, int W, long n, int comb,
                                       const float *rot_host, const unsigned int *mic_src_host /* NULL: FOA form */,
                                       float *audio, int *status, void *stream);
int  adyolo_decode_stitch(const float *decoded, const int64_t *windows, int W, int Wf, long rec, long pass_base, float *out,
                          long out_frames, int *status, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Streaming inference (corpus.StreamDeviceCorpus, test.StreamInference): windows gathered out of a ring that holds the last
 * samples of ONE live stream.
 *   ring     DEVICE int16 [capacity][4]: absolute sample s of the stream (counted from its start) lives at ring[s % capacity];
 *            the caller copies pushed samples there (at most two copies per push, split at the seam)
 *   head     samples pushed so far, by value
 *   windows  as above, word 0 an ABSOLUTE sample offset of the stream
 * adyolo_stream_gather_windows: the bits of adyolo_corpus_gather_windows (comb <= 0) or adyolo_corpus_gather_windows_view
 *   (comb > 0; rot_host / mic_src_host as there, both may be NULL with comb <= 0) on the same stream laid out linearly with
 *   n_total = head: the conversion, the padding past valid, valid = 0 and both forms under a view.  One kernel body with the
 *   linear gathers, every index taken modulo the capacity; capacity and offsets are even, so the 16-byte two-frame loads never
 *   straddle the seam.  A bad window -- an odd or negative offset, valid outside [0, n], offset + valid > head (not pushed
 *   yet) or offset < head - capacity (already overwritten) -- gives zeros and ADYOLO_CORPUS_BAD_ITEM.  EINVAL before any
 *   launch: a null or misaligned pointer (ring / audio 16 bytes, windows 8), capacity odd or < n, comb >= 16.
 * ---------------------------------------------------------------------------------------------- */
int  adyolo_stream_gather_windows(const int16_t *ring, long capacity, long head, const int64_t *windows, int W, long n, int comb,
                                  const float *rot_host, const unsigned int *mic_src_host, float *audio, int *status,
                                  void *stream);

/* ------------------------------------------------------------------------------------------------
 * Sample-rate conversion of whole recordings (csrc/resample.hip; resample.plan builds the table, corpus.InferDeviceCorpus
 * and resample.resample_device call it): a polyphase FIR in integer arithmetic from a native four-channel stream into the
 * int16 stream the calls above read.  The result is defined bit for bit:
 *   source sample -> Q23 integer q    ADYOLO_RESAMPLE_INT16    q = x << 8
 *                                     ADYOLO_RESAMPLE_INT32    q = x >> 8, arithmetic (24-bit PCM left-justified in 32 bits)
 *                                     ADYOLO_RESAMPLE_FLOAT32  q = clamp(rint(x * 2^23), -2^23, 2^23 - 1), ties to even; Inf and
 *                                                              NaN count as 0 and set ADYOLO_CORPUS_NONFINITE
 *   output frame j of a recording of n frames (0 <= j < n_out = (n L + M - 1) / M), per channel:
 *     t = j M + centre,  p = t % L,  i0 = t / L
 *     acc = sum over k in [0, K) of q[i0 - k] * taps[p][k]        in int64; q is 0 outside [0, n)
 *     y = clamp((acc + 2^37 - 1 + ((acc >> 38) & 1)) >> 38, -32768, 32767)      round half even (38 = 30 + 23 - 15)
 *   taps  DEVICE int32 [L][K] in Q30 (n_taps = L K), every row summing to 2^30 and to at most 3 * 2^30 in magnitude (then acc
 *         cannot overflow); L / M is the rate ratio in lowest terms.  L = M = K = 1, centre = 0, taps = {2^30} only converts
 *         the sample format.
 *   recs  DEVICE int64 [R][ADYOLO_RESAMPLE_WORDS] = {src offset, src frames, dst offset, dst frames} in frames of 4 channels:
 *         one launch converts R recordings of one rate and kind.  A row that reaches outside src [src_frames][4] or dst
 *         [dst_frames][4], or whose dst frames are not n_out of its src frames, writes nothing and sets ADYOLO_CORPUS_BAD_ITEM.
 *         Only dst[dst offset .. + dst frames) of a good row is written.
 * src and dst 16-byte aligned; R < 65536; L, M, K < 65536.  A tile of ADYOLO_RESAMPLE_TILE output frames keeps its input span
 * (ceil((tile - 1) M / L) + K frames of 16 bytes) and its min(L, tile) phase rows in LDS: a plan that needs more than 160 KiB
 * there is ADYOLO_ENOSUP (every plan of resample.plan with M / L <= 15 fits; 192 kHz to 24 kHz is 8).  No allocation, no synchronisation, capturable.
 * ---------------------------------------------------------------------------------------------- */
#define ADYOLO_RESAMPLE_WORDS 4
#define ADYOLO_RESAMPLE_TILE 256
#define ADYOLO_RESAMPLE_INT16   0
#define ADYOLO_RESAMPLE_INT32   1
#define ADYOLO_RESAMPLE_FLOAT32 2
#define ADYOLO_CORPUS_NONFINITE 8   /* an Inf or NaN sample in a float32 recording (converted as 0) */
int  adyolo_resample_pcm(const void *src, int kind, long src_frames, const int64_t *recs, int R, const int32_t *taps,
                         long n_taps, int L, int M, int K, long centre, int16_t *dst, long dst_frames, int *status, void *stream);

/* K11 Adam, AdamW, SGD and gradient-norm clipping over one flat parameter buffer (csrc/optim.hip; the reference picks its
 * optimizer by name, src/train.py:29-37, and clips with clip_grad_norm_, src/train.py:54; no amsgrad).  The step counter is ON
 * THE DEVICE (one uint64): every call bumps step_dev itself and no argument changes from step to step, so the whole train step
 * can be recorded once in a hipGraph and replayed (train.TrainStep(graph=True)).  All float buffers (parameter, gradient and
 * state) must be 16-byte aligned (ADYOLO_EINVAL otherwise); n need not be a multiple of 4.
 *   st_dev    4 floats of scratch: {step size, 1/sqrt(bias correction 2)} (Adam / AdamW) or {first-step flag, 0} (SGD),
 *             total_norm (the pre-clip norm of grad * grad_scale, written when clipping is on), clip_coef
 *   partials  adyolo_grad_sumsq_parts(n) doubles of scratch, or NULL = no clipping (clip_coef = 1; max_norm ignored).
 *             With it: clip_coef = min(1, max_norm / (total_norm + 1e-6)) (torch.nn.utils.clip_grad_norm_), multiplied into
 *             grad_scale by the update.  The norm is summed in float64 in a fixed order: the same bits on every call.
 * The update kernels fix their own rounding (no compiler-chosen contraction): the n & 3 tail elements, a clip that does not
 * bind and the plain step all give the same bits. */
long adyolo_grad_sumsq_parts(long n);
/* partials[k] = float64 sum of (grad * grad_scale)^2 over the k-th workgroup's share */
int  adyolo_grad_sumsq(const float *grad, long n, float grad_scale, double *partials, void *stream);
/* grad_sumsq + the norm / coefficient part of the prep kernel alone: st_dev[2] = total_norm, st_dev[3] = clip_coef */
int  adyolo_grad_norm_dev(const float *grad, long n, float grad_scale, double *partials, float max_norm, float *st_dev,
                          void *stream);
/* decoupled == 0: torch.optim.Adam (weight decay added to the gradient).  decoupled != 0: torch.optim.AdamW:
 * p *= 1 - lr * weight_decay, then Adam's moments and update. */
int  adyolo_adam_step_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long n, float lr, float beta1,
                          float beta2, float eps, float weight_decay, int decoupled, uint64_t *step_dev, float *st_dev,
                          double *partials, float max_norm, float grad_scale, void *stream);
/* torch.optim.SGD: g' = grad * scale + wd * p; momentum != 0: buf = g' on the step that takes step_dev from 0 to 1, else
 * buf = momentum * buf + (1 - dampening) * g'; p -= lr * (nesterov ? g' + momentum * buf : buf).  momentum == 0: p -= lr * g',
 * momentum_buf may be NULL and is not touched. */
int  adyolo_sgd_step_dev(float *param, const float *grad, float *momentum_buf, long n, float lr, float weight_decay,
                         float momentum, float dampening, int nesterov, uint64_t *step_dev, float *st_dev, double *partials,
                         float max_norm, float grad_scale, void *stream);
/* The scheduled forms: the learning rate is computed ON THE DEVICE by the step's prep kernel, so that it can change from step
 * to step under a replayed hipGraph; lr is therefore no argument.  With t = *step_dev after its increment + table[18] and
 * e = floor((t - 1) / every):  lr(t) = base * warm(t) * main(e), evaluated in double and rounded to float ONCE; from there on
 * that float is used exactly as the plain entry points use their `lr` argument (a constant schedule gives their bits).
 *   warm(t) = s + (1 - s) * min(t - 1, W) / W   (W = 0: 1)
 *   main(e) = 1 | gamma^floor(e / step_size) | gamma^#{milestones <= e} | gamma^e |
 *             (eta_min + (base - eta_min) * (1 + cos(pi * min(e, T_max) / T_max)) / 2) / base
 *   sched_dev  adyolo_sched_table_doubles() (= 24) doubles, written by the host only, read by the prep kernel:
 *              [0] kind 0 constant, 1 step, 2 multistep, 3 exponential, 4 cosine; [1] base lr; [2] every; [3] W; [4] s;
 *              [5] gamma; [6] step_size; [7] T_max; [8] eta_min; [9] number of milestones (<= 8); [10..17] milestones;
 *              [18] step offset; [19] EMA decay; [20] EMA warm-up flag; [21] EMA offset (k = *step_dev after its increment
 *              - 1 + [21] = EMA updates so far); [22..23] reserved (0)
 *   sched_out  adyolo_sched_out_floats() (= 4) floats written every step: {lr of this step, AdamW's 1 - lr * weight_decay,
 *              EMA weight w of this step, EMA first-update flag}
 *   ema        NULL, or a buffer laid out like param (16-byte aligned): after param is formed, ema = param on the first update
 *              (k == 0; the old contents are not read), else ema = fma(param - ema, w, ema) with w = 1 - decay_eff,
 *              decay_eff = decay or, with the warm-up flag, min(decay, (1 + k) / (10 + k)). */
int  adyolo_sched_table_doubles(void);
int  adyolo_sched_out_floats(void);
int  adyolo_adam_step_sched_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long n, float beta1,
                                float beta2, float eps, float weight_decay, int decoupled, uint64_t *step_dev, float *st_dev,
                                double *partials, float max_norm, float grad_scale, const double *sched_dev, float *sched_out,
                                float *ema, void *stream);
int  adyolo_sgd_step_sched_dev(float *param, const float *grad, float *momentum_buf, long n, float weight_decay,
                               float momentum, float dampening, int nesterov, uint64_t *step_dev, float *st_dev,
                               double *partials, float max_norm, float grad_scale, const double *sched_dev, float *sched_out,
                               float *ema, void *stream);
/* The scheduled forms with parameter groups: a base rate and a weight decay per group of elements, everything else as above
 * (one counter, one set of bias corrections, ONE norm over the whole buffer and one clip coefficient, one EMA).
 *   groups_dev  n_groups x 2 doubles {base rate, weight_decay}, written by the host only (8-byte aligned); the weight decay
 *               is rounded to float first, as the float argument of the calls above is.  sched_dev[1] is not read.
 *   groups_out  n_groups x 4 floats written every step (16-byte aligned): {rate of this step (the closed form above with the
 *               group's base, rounded to float once; a base of exactly 0 gives 0 under every schedule), rate / (1 - beta1^t)
 *               (Adam / AdamW) or the rate again (SGD), AdamW's 1 - rate * weight_decay, weight_decay}
 *   group_map   n bytes (4-byte aligned): the group of every element; values are taken modulo 16
 *   n_groups    1 .. adyolo_optim_max_groups() (= 16)
 * st_dev[0] and sched_out keep group 0's values.  An element is updated exactly as the calls above update it when they are
 * given its group's base rate and weight decay: the same bits. */
int  adyolo_optim_max_groups(void);
int  adyolo_adam_step_groups_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long n, float beta1,
                                 float beta2, float eps, int decoupled, uint64_t *step_dev, float *st_dev, double *partials,
                                 float max_norm, float grad_scale, const double *sched_dev, float *sched_out, float *ema,
                                 const double *groups_dev, float *groups_out, int n_groups, const unsigned char *group_map,
                                 void *stream);
int  adyolo_sgd_step_groups_dev(float *param, const float *grad, float *momentum_buf, long n, float momentum, float dampening,
                                int nesterov, uint64_t *step_dev, float *st_dev, double *partials, float max_norm,
                                float grad_scale, const double *sched_dev, float *sched_out, float *ema,
                                const double *groups_dev, float *groups_out, int n_groups, const unsigned char *group_map,
                                void *stream);
/* The guarded steps: an optimizer step that does NOTHING when the gradient is not finite, decided on the device inside the
 * (recorded) step.  The test: the fp32 total norm -- the float of the square root of the float64 sum of (grad * grad_scale)^2 --
 * is not finite: a NaN or an infinity anywhere in the buffer, a product grad * grad_scale that overflows, a norm beyond fp32.
 * The sum of squares therefore always runs: partials is required, and max_norm < 0 means no clipping (clip_coef exactly 1);
 * st_dev[2] is written on every attempt.
 *   guard  adyolo_optim_guard_words() (= 4) int64, 8-byte aligned, written by the prep kernel only: {attempts, skipped,
 *          last attempt skipped (0 / 1), current run of consecutive skips}
 * A skipped attempt leaves param, the state, ema, *step_dev, st_dev[0..1], st_dev[3], sched_out and groups_out untouched and
 * writes st_dev[2] (the offending norm) and the record.  Because the counter does not tick, everything derived from it -- bias
 * corrections, the schedule's clock, the EMA's update count and first-copy flag, SGD's first-step flag -- continues as if the
 * attempt had never been made.  A taken step is the unguarded entry point's, bit for bit.
 * One entry point per rule carries the arguments of all three forms; the form is read from the pointers: groups_dev != NULL
 * grouped (lr and weight_decay ignored), else sched_dev != NULL scheduled (lr ignored), else plain (ema must be NULL). */
int  adyolo_optim_guard_words(void);
int  adyolo_adam_step_guard_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long n, float lr, float beta1,
                                float beta2, float eps, float weight_decay, int decoupled, uint64_t *step_dev, float *st_dev,
                                double *partials, float max_norm, float grad_scale, const double *sched_dev, float *sched_out,
                                float *ema, const double *groups_dev, float *groups_out, int n_groups,
                                const unsigned char *group_map, int64_t *guard, void *stream);
int  adyolo_sgd_step_guard_dev(float *param, const float *grad, float *momentum_buf, long n, float lr, float weight_decay,
                               float momentum, float dampening, int nesterov, uint64_t *step_dev, float *st_dev,
                               double *partials, float max_norm, float grad_scale, const double *sched_dev, float *sched_out,
                               float *ema, const double *groups_dev, float *groups_out, int n_groups,
                               const unsigned char *group_map, int64_t *guard, void *stream);
/* The accumulating steps: K micro-batches, one optimizer step, decided on the device inside the (recorded) step.  Every call
 * is a micro-step of a cycle of accum_steps calls; which one is read from the record, so the launches and their arguments
 * are the same for every call and one recording serves them all (accum_steps is a constant of a recorded step).
 *   accum      n floats laid out like grad, 16-byte aligned: the fp32 sum of the cycle's gradients so far, added left to
 *              right, ((g0 + g1) + g2) ...; the cycle's first call overwrites it without reading it
 *   accum_dev  adyolo_optim_accum_words() (= 4) int64, 8-byte aligned, written by the prep kernel only: {index of the next
 *              call inside its cycle, calls so far, cycles completed, the last call was a hold call (0 / 1)}.  Writing 0 to
 *              the first word between calls discards a partial cycle.
 * A hold call (not the last of its cycle) changes accum and the record and nothing else.  The cycle's last call adds its
 * gradient in and then takes the step the form's own entry point would take with grad = accum and
 * grad_scale = (float)((double)grad_scale / accum_steps), bit for bit: norm, clip coefficient, guard, counter, schedule and
 * EMA see one step per cycle.  The arguments are the guarded entry points' with guard optional: guard == NULL is the
 * unguarded step, and partials == NULL then means no clipping; with a guard a non-finite value in any micro-gradient of the
 * cycle makes the cycle's last call a skipped attempt. */
int  adyolo_optim_accum_words(void);
int  adyolo_adam_step_accum_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long n, float lr, float beta1,
                                float beta2, float eps, float weight_decay, int decoupled, uint64_t *step_dev, float *st_dev,
                                double *partials, float max_norm, float grad_scale, const double *sched_dev, float *sched_out,
                                float *ema, const double *groups_dev, float *groups_out, int n_groups,
                                const unsigned char *group_map, int64_t *guard, float *accum, int64_t *accum_dev,
                                int accum_steps, void *stream);
int  adyolo_sgd_step_accum_dev(float *param, const float *grad, float *momentum_buf, long n, float lr, float weight_decay,
                               float momentum, float dampening, int nesterov, uint64_t *step_dev, float *st_dev,
                               double *partials, float max_norm, float grad_scale, const double *sched_dev, float *sched_out,
                               float *ema, const double *groups_dev, float *groups_out, int n_groups,
                               const unsigned char *group_map, int64_t *guard, float *accum, int64_t *accum_dev,
                               int accum_steps, void *stream);

/* ------------------------------------------------------------------------------------------------
 * K9a multi-head self-attention core, flash style on the exact-fp32 matrix cores (csrc/attention.hip).
 *     replaces the energy / softmax / dropout / context products of MultiHeadAttention.forward
 *     (src/models/backbones/resnet_conformer.py:57-85); the (B, H, T, T) scores are never written to HBM.
 *   q, k, v, ctx, dq, dk, dv, dctx: [B][T][H*D] float32, head h in columns h*D .. h*D+D-1;  D must be 64
 *   ctx = dropout(softmax(scale * q k^T), p) v    per (batch, head);  dropout_p = 0: none (eval)
 *   lse2 [B][H][T]: per query row log2(sum_k exp(scale * q k)) (written by fwd when non-NULL, read by bwd)
 *   delta [B][H][T]: workspace of bwd (sum_dv dctx * ctx)
 *   seed: 32-bit seed of the stateless dropout hash keep(b, h, query, key); forward and backward of one call must use
 *         the same (dropout_p, seed).  adyolo_attn_dropout_mask writes that mask ([B][H][T][T], values 0 or 1/(1-p)).
 * ---------------------------------------------------------------------------------------------- */
/*   seed_dev (round 4; may be NULL): when non-NULL the kernels read the seed from this device word instead of `seed` -- a recorded
 *         step replays with a seed derived on the device by adyolo_seed32_dev(seed64, offset, offset_dev, out): out[0] = the 32-bit
 *         value the host-side stream (rng.DropoutStream.seed32) computes for (seed64, offset + *offset_dev). */
int adyolo_attn_fwd(const float *q, const float *k, const float *v, float *ctx, float *lse2, int B, int T, int H, int D,
                    float scale, float dropout_p, uint32_t seed, const uint32_t *seed_dev, void *stream);
int adyolo_attn_bwd(const float *q, const float *k, const float *v, const float *ctx, const float *dctx,
                    const float *lse2, float *delta, float *dq, float *dk, float *dv, int B, int T, int H, int D,
                    float scale, float dropout_p, uint32_t seed, const uint32_t *seed_dev, void *stream);
int adyolo_seed32_dev(uint64_t seed, uint64_t offset, const int64_t *offset_dev /*or NULL*/, uint32_t *out, void *stream);
int adyolo_attn_dropout_mask(float *mask, int B, int T, int H, float dropout_p, uint32_t seed, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ADYOLO_HIP_H */
