// Input-pipeline kernels around K1: PCM16 -> float conversion of staged WAV data, SpecAug
// masking on the channels-last feature tensor, and the train-set scaler statistics (mean / std / max / min per
// mel bin and channel).  References: /root/reference/src/datasets.py:101-162 (audio / 32768 + 1e-8, spec-augment call),
// /root/reference/src/utils/augmentations.py:6-33 (SpecAug), /root/reference/src/preprocess.py:86-130 (scaler).
#include <float.h>
#include "common.hpp"

namespace adyolo {

// int16 [n] -> float [n]:  x / 32768 + 1e-8   (datasets.py:105, preprocess.py:104); 8 samples per thread
__global__ __launch_bounds__(256) void pcm16_to_f32_kernel(const int16_t *__restrict__ pcm, float *__restrict__ out, long n8,
                                                           long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        const long b = i * 8;
        if (b + 8 <= n) {
            const int4 v = *reinterpret_cast<const int4 *>(pcm + b);          // 8 x int16
            const int w[4] = {v.x, v.y, v.z, v.w};
            float f[8];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                f[2 * k] = (float)(short)(w[k] & 0xffff) / 32768.0f + 1e-8f;
                f[2 * k + 1] = (float)(short)(w[k] >> 16) / 32768.0f + 1e-8f;
            }
            *reinterpret_cast<float4 *>(out + b) = make_float4(f[0], f[1], f[2], f[3]);
            *reinterpret_cast<float4 *>(out + b + 4) = make_float4(f[4], f[5], f[6], f[7]);
        } else {
            for (long j = b; j < n; ++j) out[j] = (float)pcm[j] / 32768.0f + 1e-8f;
        }
    }
}

// SpecAug on feat [B][T][F][C] (C4 = C / 4 float4 quads per pixel), per sample b and channel group g: zero frames [t0,t1) x
// all bins and bins [f0,f1) x all frames of the group's quads [q0,q1).  ranges int32 [B][G][4] = {t0, t1, f0, f1} (an empty
// range = no mask; every range clamped to [0,T] / [0,F] here, so no table value writes outside the tensor); mask value 0
// like torchaudio's default.  Write-only: one float4 store per masked element, nothing else is touched.  Work items of one
// (b, g) = the frame stripe (nt frames x F bins x nq quads) followed by the bin stripe without the frames already masked
// ((T - nt) frames x nf bins x nq quads); grid (blocks per group, B * G), grid-stride over the items.
struct MaskGroups {
    int q[ADYOLO_MASK_MAX_GROUPS][2];
};

__global__ __launch_bounds__(256) void mask_groups_kernel(float *__restrict__ feat, const int *__restrict__ rng,
                                                          MaskGroups groups, int G, int T, int F, int C4) {
    const int b = blockIdx.y / G, g = blockIdx.y - b * G;
    const int *r = rng + (size_t)blockIdx.y * 4;
    const int t0 = min(max(r[0], 0), T), t1 = min(max(r[1], t0), T);
    const int f0 = min(max(r[2], 0), F), f1 = min(max(r[3], f0), F);
    const int q0 = groups.q[g][0], nq = groups.q[g][1] - q0;
    const unsigned nt = t1 - t0, nf = f1 - f0;
    if ((nt == 0 && nf == 0) || nq <= 0) return;
    float4 *base = reinterpret_cast<float4 *>(feat) + (size_t)b * T * F * C4 + q0;
    const unsigned n_t = nt * F * nq, n_all = n_t + (T - nt) * nf * nq;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n_all; i += gridDim.x * blockDim.x) {
        unsigned t, f;
        const unsigned q = i % nq;
        if (i < n_t) {
            const unsigned k = i / nq;
            f = k % F;
            t = t0 + k / F;
        } else {
            const unsigned k = (i - n_t) / nq;
            f = f0 + k % nf;
            t = k / nf;
            t += t < (unsigned)t0 ? 0u : nt;
        }
        base[((size_t)t * F + f) * C4 + q] = z;
    }
}

// Frequency shift + SpecAug stripes + cutout on feat [B][T][64][C] in one pass, in place (adyolo_feat_augment).  table int32
// [B][G + 2][4]: rows 0..G-1 the SpecAug ranges of mask_groups_kernel, row G the cutout rectangle {t0, t1, f0, f1} over ALL quads,
// row G + 1 = {shift, -, -, -}.  Per sample, in this order: every quad of a group whose bit is set in shift_mask moves along the
// bin axis by s = clamp(shift, -63, 63), out[t][f] = in[t][src(f)] with the vacated bins reflected (u = f - s; src = -u below 0,
// 126 - u above 63); then the stripes; then the rectangle.  As all masks fill with 0 the result of an element is 0 where any mask
// covers it and in[src(f)] elsewhere: a masked element is stored as zero and not loaded, an unshifted quad is only stored to
// where it is masked (write-only, as mask_groups_kernel), and a sample with nothing to do costs no memory access.
// Every range and the shift are clamped here: no table value reaches outside the tensor.
// Work split: a row (b, t) of one quad is 64 float4, one per lane of a wave (F == 64 == the wave width).  One wave owns whole
// rows, FA_ROWS adjacent ones per pass (their loads issued together); grid (blocks per sample, B), 4 waves per block, the rows
// of [row_lo, row_hi) -- the frames any operation of this sample can touch -- dealt to the waves of the sample.
constexpr int FA_ROWS = 4;

__global__ __launch_bounds__(256) void feat_augment_kernel(float *feat, const int *__restrict__ table, MaskGroups groups, int G,
                                                           unsigned shift_mask, int T, int C4) {
    constexpr int F = 64;
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int *tb = table + (size_t)b * (G + 2) * 4;
    int gt0[ADYOLO_MASK_MAX_GROUPS], gt1[ADYOLO_MASK_MAX_GROUPS];
    unsigned fm = 0;                                  // per lane: bit g = this lane's bin is in group g's bin stripe
    unsigned live = 0;                                // bit g = group g has quads
    int row_lo = T, row_hi = 0;
#pragma unroll
    for (int g = 0; g < ADYOLO_MASK_MAX_GROUPS; ++g) {
        gt0[g] = gt1[g] = 0;
        if (g < G && groups.q[g][1] > groups.q[g][0]) {
            live |= 1u << g;
            const int t0 = min(max(tb[g * 4 + 0], 0), T), t1 = min(max(tb[g * 4 + 1], t0), T);
            const int f0 = min(max(tb[g * 4 + 2], 0), F), f1 = min(max(tb[g * 4 + 3], f0), F);
            gt0[g] = t0;
            gt1[g] = t1;
            fm |= (unsigned)(lane >= f0 && lane < f1) << g;
            if (f1 > f0) row_lo = 0, row_hi = T;                                  // a bin stripe crosses every frame
            if (t1 > t0) row_lo = min(row_lo, t0), row_hi = max(row_hi, t1);
        }
    }
    const int *cr = tb + G * 4;
    int ct0 = min(max(cr[0], 0), T), ct1 = min(max(cr[1], ct0), T);
    const int cf0 = min(max(cr[2], 0), F), cf1 = min(max(cr[3], cf0), F);
    if (cf1 == cf0) ct1 = ct0;                                                    // empty in either direction: no rectangle
    if (ct1 > ct0) row_lo = min(row_lo, ct0), row_hi = max(row_hi, ct1);
    const bool fc = lane >= cf0 && lane < cf1;
    const int s = min(max(tb[(G + 1) * 4], -(F - 1)), F - 1);
    const unsigned shifting = s != 0 ? shift_mask & live : 0u;                    // the groups that move in this sample
    if (shifting) row_lo = 0, row_hi = T;                                         // a moving quad: every frame of the sample
    const int u = lane - s;
    const int src = u < 0 ? -u : (u > F - 1 ? 2 * (F - 1) - u : u);               // in [0, 63] for |s| <= 63
    float4 *base = reinterpret_cast<float4 *>(feat) + (size_t)b * T * F * C4;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = gridDim.x * 4;
    for (int t = row_lo + wave * FA_ROWS; t < row_hi; t += n_waves * FA_ROWS) {
        unsigned tm[FA_ROWS];                                                     // bit g = row t + r is in group g's frame stripe
        bool cut[FA_ROWS];                                                        // this lane's element of row t + r is in the rectangle
#pragma unroll
        for (int r = 0; r < FA_ROWS; ++r) {
            tm[r] = 0;
#pragma unroll
            for (int g = 0; g < ADYOLO_MASK_MAX_GROUPS; ++g) tm[r] |= (unsigned)(t + r >= gt0[g] && t + r < gt1[g]) << g;
            cut[r] = fc && t + r >= ct0 && t + r < ct1;
        }
        for (int q = 0; q < C4; ++q) {
            unsigned gm = 0;                                                      // the groups this quad belongs to
#pragma unroll
            for (int g = 0; g < ADYOLO_MASK_MAX_GROUPS; ++g)
                gm |= (unsigned)(g < G && q >= groups.q[g][0] && q < groups.q[g][1]) << g;
            const bool in_bins = (fm & gm) != 0;
            if (gm & shifting) {
                // In place.  Rows t .. t + FA_ROWS - 1 belong to this wave alone (no other wave, of this or any other block,
                // loads or stores them), and a row of one quad is 64 float4, one per lane.  All 64 lanes load in[src(f)] of a
                // row in one wave-wide instruction BEFORE any lane stores to f: the stores take their data from the registers
                // the loads fill, so they wait for them, and the wave barrier keeps the compiler from moving the store of one
                // lane above the load of another.  A row is never split across waves, and the tensor is reached through this
                // one pointer only (no __restrict__ pair over the same buffer).
                float4 v[FA_ROWS];
#pragma unroll
                for (int r = 0; r < FA_ROWS; ++r) {
                    v[r] = z;
                    if (t + r < row_hi && !((tm[r] & gm) != 0 || in_bins || cut[r]))
                        v[r] = base[((size_t)(t + r) * F + src) * C4 + q];
                }
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int r = 0; r < FA_ROWS; ++r)
                    if (t + r < row_hi) base[((size_t)(t + r) * F + lane) * C4 + q] = v[r];
            } else {                                                              // write-only: the masked elements
#pragma unroll
                for (int r = 0; r < FA_ROWS; ++r)
                    if (t + r < row_hi && ((tm[r] & gm) != 0 || in_bins || cut[r]))
                        base[((size_t)(t + r) * F + lane) * C4 + q] = z;
            }
        }
    }
}

// per-column sum / sum of squares / max / min of a [rows][cols] matrix, stage 1: one partial row per workgroup
// part [4][nblk][cols]
__global__ __launch_bounds__(256) void colstats_partial_kernel(const float *__restrict__ a, float *__restrict__ part,
                                                               long rows, int cols) {
    const int nblk = gridDim.x;
    const long per = (rows + nblk - 1) / nblk;
    const long r0 = (long)blockIdx.x * per, r1 = r0 + per < rows ? r0 + per : rows;
    for (int c = threadIdx.x; c < cols; c += blockDim.x) {
        float s = 0.f, q = 0.f, mx = -FLT_MAX, mn = FLT_MAX;
        for (long r = r0; r < r1; ++r) {
            const float v = a[r * cols + c];
            s += v;
            q += v * v;
            mx = fmaxf(mx, v);
            mn = fminf(mn, v);
        }
        part[((size_t)0 * nblk + blockIdx.x) * cols + c] = s;
        part[((size_t)1 * nblk + blockIdx.x) * cols + c] = q;
        part[((size_t)2 * nblk + blockIdx.x) * cols + c] = mx;
        part[((size_t)3 * nblk + blockIdx.x) * cols + c] = mn;
    }
}
// stage 2: out [4][cols] doubles (sum, sumsq, max, min)
__global__ __launch_bounds__(256) void colstats_final_kernel(const float *__restrict__ part, double *__restrict__ out,
                                                             int nblk, int cols) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cols) return;
    double s = 0.0, q = 0.0, mx = -DBL_MAX, mn = DBL_MAX;
    for (int b = 0; b < nblk; ++b) {
        s += (double)part[((size_t)0 * nblk + b) * cols + c];
        q += (double)part[((size_t)1 * nblk + b) * cols + c];
        mx = fmax(mx, (double)part[((size_t)2 * nblk + b) * cols + c]);
        mn = fmin(mn, (double)part[((size_t)3 * nblk + b) * cols + c]);
    }
    out[0 * cols + c] = s;
    out[1 * cols + c] = q;
    out[2 * cols + c] = mx;
    out[3 * cols + c] = mn;
}

}  // namespace adyolo

using namespace adyolo;

extern "C" int adyolo_pcm16_to_f32(const int16_t *pcm, float *out, long n, void *stream) {
    ADYOLO_REQUIRE(pcm && out && n > 0, ADYOLO_EINVAL, "pcm16_to_f32: bad arguments");
    ADYOLO_REQUIRE(((uintptr_t)pcm & 15) == 0 && ((uintptr_t)out & 15) == 0, ADYOLO_EINVAL, "pcm16_to_f32: 16-byte aligned buffers");
    const long n8 = (n + 7) / 8;
    long g = (n8 + 255) / 256;
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(pcm16_to_f32_kernel, dim3((unsigned)g), dim3(256), 0, as_stream(stream), pcm, out, n8, n);
    return check_launch("pcm16_to_f32");
}

extern "C" int adyolo_mask_groups(float *feat, const int *ranges, int B, int G, int T, int F, int C, const int *group_quads,
                                  void *stream) {
    ADYOLO_REQUIRE(feat && ranges && group_quads && B > 0 && G > 0 && G <= ADYOLO_MASK_MAX_GROUPS && T > 0 && F > 0 && C > 0 &&
                   C % 4 == 0 && (long)T * F * (C / 4) < (1L << 31) && (long)B * G < 65536, ADYOLO_EINVAL,
                   "mask_groups: bad arguments");
    ADYOLO_REQUIRE(((uintptr_t)feat & 15) == 0 && ((uintptr_t)ranges & 3) == 0, ADYOLO_EINVAL, "mask_groups: misaligned buffers");
    const int C4 = C / 4;
    MaskGroups groups{};
    int nq_max = 0;
    for (int g = 0; g < G; ++g) {
        const int q0 = group_quads[2 * g], q1 = group_quads[2 * g + 1];
        ADYOLO_REQUIRE(0 <= q0 && q0 <= q1 && q1 <= C4, ADYOLO_EINVAL, "mask_groups: group %d quads [%d,%d) outside [0,%d]", g, q0,
                       q1, C4);
        groups.q[g][0] = q0;
        groups.q[g][1] = q1;
        nq_max = q1 - q0 > nq_max ? q1 - q0 : nq_max;
    }
    if (nq_max == 0) return 0;
    // the stripes of one group are at most ~T * 64 float4 at the usual mask widths: ~16 per thread, at most 32 blocks
    int gx = cdiv((long)T * F * nq_max, 256L * 16);
    gx = gx < 1 ? 1 : (gx > 32 ? 32 : gx);
    hipLaunchKernelGGL(mask_groups_kernel, dim3((unsigned)gx, (unsigned)(B * G)), dim3(256), 0, as_stream(stream), feat, ranges,
                       groups, G, T, F, C4);
    return check_launch("mask_groups");
}

// frequency shift + SpecAug stripes + cutout, in place: table [B][G + 2][4] on the device (feat_augment_kernel)
extern "C" int adyolo_feat_augment(float *feat, const int *table, int B, int G, int T, int F, int C, const int *group_quads,
                                   unsigned shift_mask, void *stream) {
    ADYOLO_REQUIRE(feat && table && group_quads && B > 0 && B < 65536 && G > 0 && G <= ADYOLO_MASK_MAX_GROUPS && T > 0 && F > 0 &&
                   C > 0 && C % 4 == 0 && (long)T * F * (C / 4) < (1L << 31), ADYOLO_EINVAL, "feat_augment: bad arguments");
    ADYOLO_REQUIRE(((uintptr_t)feat & 15) == 0 && ((uintptr_t)table & 3) == 0, ADYOLO_EINVAL, "feat_augment: misaligned buffers");
    ADYOLO_REQUIRE((shift_mask >> G) == 0, ADYOLO_EINVAL, "feat_augment: shift_mask 0x%x has bits above the %d groups", shift_mask, G);
    ADYOLO_REQUIRE(F == 64, ADYOLO_ENOSUP, "feat_augment: F = %d (a row of 64 mel bins is one wave; no other width)", F);
    const int C4 = C / 4;
    MaskGroups groups{};
    for (int g = 0; g < G; ++g) {
        const int q0 = group_quads[2 * g], q1 = group_quads[2 * g + 1];
        ADYOLO_REQUIRE(0 <= q0 && q0 <= q1 && q1 <= C4, ADYOLO_EINVAL, "feat_augment: group %d quads [%d,%d) outside [0,%d]", g, q0,
                       q1, C4);
        groups.q[g][0] = q0;
        groups.q[g][1] = q1;
    }
    // FA_ROWS rows per wave and pass, 4 waves per block: two passes per wave (75 blocks per sample at T = 2400), at most 128 blocks
    int gx = cdiv(T, 4L * FA_ROWS * 2);
    gx = gx < 1 ? 1 : (gx > 128 ? 128 : gx);
    hipLaunchKernelGGL(feat_augment_kernel, dim3((unsigned)gx, (unsigned)B), dim3(256), 0, as_stream(stream), feat, table, groups,
                       G, shift_mask, T, C4);
    return check_launch("feat_augment");
}

// one group over all quads: ranges [B][4] is the table [B][1][4]
extern "C" int adyolo_mask_ranges(float *feat, const int *ranges, int B, int T, int F, int C, void *stream) {
    ADYOLO_REQUIRE(feat && ranges && B > 0 && T > 0 && F > 0 && C > 0 && C % 4 == 0, ADYOLO_EINVAL, "mask_ranges: bad arguments");
    const int all[2] = {0, C / 4};
    return adyolo_mask_groups(feat, ranges, B, 1, T, F, C, all, stream);
}

extern "C" int adyolo_colstats(const float *a, float *partial, double *out, long rows, int cols, void *stream) {
    ADYOLO_REQUIRE(a && partial && out && rows > 0 && cols > 0, ADYOLO_EINVAL, "colstats: bad arguments");
    int nblk = (int)(rows < 1024 ? rows : 1024);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(colstats_partial_kernel, dim3(nblk), dim3(256), 0, st, a, partial, rows, cols);
    int rc = check_launch("colstats_partial");
    if (rc) return rc;
    hipLaunchKernelGGL(colstats_final_kernel, dim3(cdiv(cols, 256)), dim3(256), 0, st, partial, out, nblk, cols);
    return check_launch("colstats_final");
}

// ---- FOA rotation augmentation on raw audio (reference src/utils/augmentations.py:81-96): per clip a sign for each of
// the Y, Z, X channels and an optional X <-> Y swap;  audio [B][n][4] (W, Y, Z, X), cfg[b] = {sy, sz, sx, swap}
namespace adyolo {
__global__ __launch_bounds__(256) void foa_rotate_kernel(const float4 *__restrict__ x, float4 *__restrict__ y,
                                                         const float *__restrict__ cfg, long n_per_clip) {
    const int b = blockIdx.y;
    const float sy = cfg[b * 4 + 0], sz = cfg[b * 4 + 1], sx = cfg[b * 4 + 2];
    const bool swap = cfg[b * 4 + 3] != 0.f;
    const float4 *src = x + (size_t)b * n_per_clip;
    float4 *dst = y + (size_t)b * n_per_clip;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_per_clip; i += (long)gridDim.x * blockDim.x) {
        const float4 v = src[i];
        const float yy = v.y * sy, zz = v.z * sz, xx = v.w * sx;
        dst[i] = swap ? make_float4(v.x, xx, zz, yy) : make_float4(v.x, yy, zz, xx);
    }
}
}  // namespace adyolo

extern "C" int adyolo_foa_rotate(const float *audio, float *out, const float *cfg, int B, long n_samples, void *stream) {
    ADYOLO_REQUIRE(audio && out && cfg && B > 0 && n_samples > 0, ADYOLO_EINVAL, "foa_rotate: bad arguments");
    long g = (n_samples + 255) / 256;
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(adyolo::foa_rotate_kernel, dim3((unsigned)g, B), dim3(256), 0, adyolo::as_stream(stream),
                       (const float4 *)audio, (float4 *)out, cfg, n_samples);
    return adyolo::check_launch("foa_rotate");
}

// ---- FOA rotation followed by a yaw about the vertical axis (aug_config.yaw_rotation_augment, the host-fed path): the work of
// foa_rotate_kernel, then yaw_apply, per clip from cfg[b] = {sy, sz, sx, swap, cos, sin}
namespace adyolo {
__global__ __launch_bounds__(256) void foa_rotate_yaw_kernel(const float4 *__restrict__ x, float4 *__restrict__ y,
                                                             const float *__restrict__ cfg, long n_per_clip) {
    const int b = blockIdx.y;
    const float sy = cfg[b * 6 + 0], sz = cfg[b * 6 + 1], sx = cfg[b * 6 + 2];
    const bool swap = cfg[b * 6 + 3] != 0.f;
    const float c = cfg[b * 6 + 4], s = cfg[b * 6 + 5];
    const float4 *src = x + (size_t)b * n_per_clip;
    float4 *dst = y + (size_t)b * n_per_clip;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_per_clip; i += (long)gridDim.x * blockDim.x) {
        const float4 v = src[i];
        const float yy = v.y * sy, zz = v.z * sz, xx = v.w * sx;
        dst[i] = yaw_apply(swap ? make_float4(v.x, xx, zz, yy) : make_float4(v.x, yy, zz, xx), c, s);
    }
}
}  // namespace adyolo

extern "C" int adyolo_foa_rotate_yaw(const float *audio, float *out, const float *cfg, int B, long n_samples, void *stream) {
    ADYOLO_REQUIRE(audio && out && cfg && B > 0 && B < 65536 && n_samples > 0, ADYOLO_EINVAL, "foa_rotate_yaw: bad arguments");
    ADYOLO_REQUIRE(((uintptr_t)audio & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)cfg & 3) == 0, ADYOLO_EINVAL,
                   "foa_rotate_yaw: misaligned buffers (audio / out 16 bytes, cfg 4 bytes)");
    long g = (n_samples + 255) / 256;
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(adyolo::foa_rotate_yaw_kernel, dim3((unsigned)g, (unsigned)B), dim3(256), 0, adyolo::as_stream(stream),
                       (const float4 *)audio, (float4 *)out, cfg, n_samples);
    return adyolo::check_launch("foa_rotate_yaw");
}

// ---- MIC channel-swap augmentation on raw audio (augmentations.swap_audio): per clip a permutation of the four capsules,
// out[b][i][j] = audio[b][i][src[b][j] & 3].  One 16-byte load and one 16-byte store per frame; the clip's four selectors are
// uniform over the workgroup (blockIdx.y = clip: scalar loads, once), so each output word is three bit selects between the
// frame's registers.  The frame travels as four 32-bit integers: nothing is computed on the values, NaN payloads and -0.0 keep their bits.
namespace adyolo {
// word s of the frame through two all-ones / all-zeros masks of the selector's bits (and / or on scalar masks): no branch in the loop
__device__ __forceinline__ int mic_pick(const int4 &v, int s) {
    const int m0 = -(s & 1), m1 = -((s >> 1) & 1);
    const int lo = (v.y & m0) | (v.x & ~m0), hi = (v.w & m0) | (v.z & ~m0);
    return (hi & m1) | (lo & ~m1);
}

__global__ __launch_bounds__(256) void mic_swap_kernel(const int4 *__restrict__ x, int4 *__restrict__ y,
                                                       const int *__restrict__ sel, long n_per_clip) {
    const int b = blockIdx.y;
    const int s0 = sel[b * 4 + 0] & 3, s1 = sel[b * 4 + 1] & 3, s2 = sel[b * 4 + 2] & 3, s3 = sel[b * 4 + 3] & 3;
    const int4 *src = x + (size_t)b * n_per_clip;
    int4 *dst = y + (size_t)b * n_per_clip;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_per_clip; i += (long)gridDim.x * blockDim.x) {
        const int4 v = src[i];
        dst[i] = make_int4(mic_pick(v, s0), mic_pick(v, s1), mic_pick(v, s2), mic_pick(v, s3));
    }
}
}  // namespace adyolo

extern "C" int adyolo_mic_swap(const float *audio, float *out, const int *src_dev, int B, long n_samples, void *stream) {
    ADYOLO_REQUIRE(audio && out && src_dev && B > 0 && B < 65536 && n_samples > 0, ADYOLO_EINVAL, "mic_swap: bad arguments");
    ADYOLO_REQUIRE(((uintptr_t)audio & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)src_dev & 3) == 0, ADYOLO_EINVAL,
                   "mic_swap: misaligned buffers (audio / out 16 bytes, src 4 bytes)");
    const size_t words = (size_t)B * (size_t)n_samples * 4;
    ADYOLO_REQUIRE(out + words <= audio || audio + words <= out, ADYOLO_EINVAL, "mic_swap: out overlaps audio (out-of-place only)");
    long g = (n_samples + 255) / 256;
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(adyolo::mic_swap_kernel, dim3((unsigned)g, (unsigned)B), dim3(256), 0, adyolo::as_stream(stream),
                       (const int4 *)audio, (int4 *)out, src_dev, n_samples);
    return adyolo::check_launch("mic_swap");
}

// ---- Time-domain mixing on raw audio (aug_config.time_mix_augment, the host-fed path): per clip out = audio + gain * mate where
// the clip is mixed, the clip as it is where it is not.  One float4 per frame from each side; the clip's flag and gain are
// uniform over the workgroup (blockIdx.y = clip).  The product is rounded before the sum (mix_add), as in the corpus gather.  An
// unmixed clip travels as integers (its bits are kept) or, in place, is not touched at all.
namespace adyolo {
__global__ __launch_bounds__(256) void audio_mix_kernel(const float4 *x, const float4 *__restrict__ mate,
                                                        const float *__restrict__ gains,
                                                        const unsigned char *__restrict__ mixed, float4 *y, long n_per_clip) {
    const int b = blockIdx.y;
    const float4 *src = x + (size_t)b * n_per_clip;
    float4 *dst = y + (size_t)b * n_per_clip;
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
    if (!mixed[b]) {
        if (src == dst) return;
        const int4 *s = reinterpret_cast<const int4 *>(src);
        int4 *d = reinterpret_cast<int4 *>(dst);
        for (long i = tid; i < n_per_clip; i += nth) d[i] = s[i];
        return;
    }
    const float g = gains[b];
    const float4 *m = mate + (size_t)b * n_per_clip;
    for (long i = tid; i < n_per_clip; i += nth) dst[i] = mix_add(src[i], m[i], g);      // out == audio: read, then written
}
}  // namespace adyolo

extern "C" int adyolo_audio_mix(const float *audio, const float *mate, const float *gains, const unsigned char *mixed, float *out,
                                int B, long n_samples, void *stream) {
    ADYOLO_REQUIRE(audio && mate && gains && mixed && out && B > 0 && B < 65536 && n_samples > 0, ADYOLO_EINVAL,
                   "audio_mix: bad arguments");
    ADYOLO_REQUIRE(((uintptr_t)audio & 15) == 0 && ((uintptr_t)mate & 15) == 0 && ((uintptr_t)out & 15) == 0 &&
                       ((uintptr_t)gains & 3) == 0,
                   ADYOLO_EINVAL, "audio_mix: misaligned buffers (audio / mate / out 16 bytes, gains 4 bytes)");
    const size_t words = (size_t)B * (size_t)n_samples * 4;
    ADYOLO_REQUIRE(out == audio || out + words <= audio || audio + words <= out, ADYOLO_EINVAL,
                   "audio_mix: out overlaps audio without being audio (in place or apart)");
    ADYOLO_REQUIRE(out + words <= mate || mate + words <= out, ADYOLO_EINVAL, "audio_mix: out overlaps mate");
    long g = (n_samples + 255) / 256;
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(adyolo::audio_mix_kernel, dim3((unsigned)g, (unsigned)B), dim3(256), 0, adyolo::as_stream(stream),
                       (const float4 *)audio, (const float4 *)mate, gains, mixed, (float4 *)out, n_samples);
    return adyolo::check_launch("audio_mix");
}
