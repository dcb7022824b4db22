// K8: AD-YOLO angular-distance responsibility-assignment loss, forward + backward, no host syncs.
// Replaces ADYOLOloss.__call__ (/root/reference/src/models/loss.py:189-251): ~40 ATen kernels, three
// CPU-resident label tensors and six .item() syncs per call become three launches:
//   1. assign : one lane per target row -> decode its cell's anchors, great-circle distance D[m][a],
//               arg-min, threshold masks; marks anchors (bit sets), counts distinct positives per
//               threshold with the value returned by atomicOr, accumulates the angular term and its
//               (un-normalised) gradient on the u,v logits (fixed-point atomics: order-independent).
//   2. main   : ONE pass over the logits, one lane per logit (coalesced): BCE terms of the three
//               thresholds and dlogit written in the same pass (HBM traffic = read logits + write dlogits
//               + 6 words per anchor of assignment state).
//   3. final  : combines the per-workgroup partial sums in double into the (1,) loss.
// Each kernel is a template on GRAD: <true> is this training form, <false> the forward-only per-clip form (K8f, below).
#include "common.hpp"

namespace adyolo {

constexpr int LOSS_HDR = 64;        // counters: [0..2] Npos_i, [3] Npairs, [4] arrival counter of the assign workgroups
constexpr int LOSS_MAIN_BLOCKS = 2048, LOSS_ASSIGN_BLOCKS = 1024;

struct LossGeom {
    int B, T, Gaz, Gel, A, C, M;
    float thr[3];
    float gain_ang, gain_obj, gain_nonobj, gain_cls;
    float grid_az, grid_el, span;          // span = 0.5 + g_overlap
};

__device__ __forceinline__ float deg2rad_(float d) { return d * 0.017453292519943295f; }
__device__ __forceinline__ float rad2deg_(float r) { return r * 57.29577951308232f; }

// 32.32 fixed point for the order-independent accumulation of the angular gradient (|value| < 2^31, step 2.3e-10)
__device__ __forceinline__ unsigned long long to_fixed(float v) {
    const double c = fmin(fmax((double)v, -2147483000.0), 2147483000.0);
    return (unsigned long long)__double2ll_rn(c * 4294967296.0);
}
__device__ __forceinline__ float from_fixed(unsigned long long q) {
    return (float)((double)(long long)q * (1.0 / 4294967296.0));
}

// The normalisation unit: what one set of counts (distinct positives per threshold, responsible pairs, anchors) covers.  The
// three kernels below have two forms each.  GRAD, the training form (adyolo_loss_phase): the unit is the whole [B][T] batch
// on a one-dimensional grid; the counts go through the header and the gradient is formed.  !GRAD, the per-clip form
// (adyolo_loss_per_clip, K8f below): unit `idx` of `count` is one clip of a batched pass on a grid with a clip dimension; its
// rows are [row_start[idx], row_start[idx + 1]) of the target, clamped to its capacity, and its logits, bit sets and partial
// sums follow those of the clips before it.  With GRAD idx = 0 and count = 1 are constants and the offsets fold away.
struct LossUnit {
    int idx, count;
    int b0, b1;            // a row counts if its b column lies in [b0, b1)
    int r0, M, nang;       // first row, rows, assign workgroups (32 rows each per round: also the grid-stride over the rows)
};

template <bool GRAD>
__device__ __forceinline__ LossUnit loss_unit(const LossGeom &g, const int *__restrict__ row_start, long cap, int clip, int nang) {
    LossUnit u;
    if constexpr (GRAD) {
        u.idx = 0; u.count = 1; u.b0 = 0; u.b1 = g.B; u.r0 = 0; u.M = g.M; u.nang = nang;
    } else {
        long r0 = row_start[clip], r1 = row_start[clip + 1];
        r1 = r1 < 0 ? 0 : (r1 > cap ? cap : r1);
        r0 = r0 < 0 ? 0 : (r0 > r1 ? r1 : r0);
        u.idx = clip; u.count = g.B; u.b0 = clip; u.b1 = clip + 1; u.r0 = (int)r0; u.M = (int)(r1 - r0);
        u.nang = (u.M + 31) / 32;
        if (u.nang > LOSS_ASSIGN_BLOCKS) u.nang = LOSS_ASSIGN_BLOCKS;
    }
    return u;
}

// 8 lanes per target row: lane a of the octet owns anchor a (one decode + great-circle distance per lane instead of a
// serial loop over the anchors: 8x the parallelism of a one-lane-per-row kernel, which was latency-bound at 137 k rows);
// the arg-min is three shuffle steps inside the octet (ties -> the lowest anchor index, like the reference's argmin);
// distinct-positive counts are kept per wave (ballot + popcount) and leave once per workgroup.
// GRAD: grid (nang); hdr, ang_grad and dist (optional) are written.  !GRAD: grid (assign workgroups of the largest clip, B);
// workgroup (x, b) is workgroup x of clip b's own launch of nang workgroups (x >= nang: nothing to do); row_start and cap
// are read.  NA: anchors of all units (the stride of the cls_bits planes).
template <bool GRAD>
__global__ __launch_bounds__(256) void loss_assign_kernel(const float *__restrict__ logit,
                                                          const float *__restrict__ target, LossGeom g,
                                                          unsigned *__restrict__ hdr, unsigned *__restrict__ pos_bits,
                                                          unsigned *__restrict__ cls_bits,
                                                          unsigned long long *__restrict__ ang_grad,
                                                          float *__restrict__ ang_partial, float *__restrict__ dist,
                                                          long NA, const int *__restrict__ row_start, long cap) {
    __shared__ float red_sum[4];
    __shared__ int red_cnt[4][4];
    const LossUnit u = loss_unit<GRAD>(g, row_start, cap, blockIdx.y, gridDim.x);
    if (!GRAD && (int)blockIdx.x >= u.nang) return;
    const int a = threadIdx.x & 7;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float blk_sum = 0.f;                      // this thread's share of sum(D / 180) over responsible pairs
    int cnt0 = 0, cnt1 = 0, cnt2 = 0, cntp = 0;     // wave-uniform: distinct positives per threshold, responsible pairs
    const long nlanes = (long)u.M * 8;
    for (long gt = (long)blockIdx.x * blockDim.x + threadIdx.x; gt - threadIdx.x < nlanes; gt += (long)u.nang * blockDim.x) {
    const int m = (int)(gt >> 3);
    float my_sum = 0.f;
    int my_pairs = 0;
    float D = INFINITY, gu = 0.f, gv = 0.f;
    long cell = 0;
    int cl = 0;
    bool valid = false;
    if (m < u.M) {
        const float *tr = target + (size_t)(u.r0 + m) * 7;
        const int b = (int)tr[0], t = (int)tr[1], gi = (int)tr[2], gj = (int)tr[3];
        cl = (int)tr[4];
        const float U = tr[5], V = tr[6];
        if (b >= u.b0 && b < u.b1 && t >= 0 && t < g.T && gi >= 0 && gi < g.Gaz && gj >= 0 && gj < g.Gel && cl >= 0 &&
            cl < g.C) {
            valid = true;
            cell = (((long)b * g.T + t) * g.Gaz + gi) * g.Gel + gj;
            if (a < g.A) {
                const int CH = g.C + 3;
                const float off_u = gi * g.grid_az - 180.f + 0.5f * g.grid_az;
                const float off_v = gj * g.grid_el - 90.f + 0.5f * g.grid_el;
                const float u2 = deg2rad_(U), v2 = deg2rad_(V);
                const float sv2 = sinf(v2), cv2 = cosf(v2);
                const float *lp = logit + ((size_t)cell * g.A + a) * CH + g.C + 1;
                const float tu = tanhf(lp[0]), tv = tanhf(lp[1]);
                float ud = tu * g.span * g.grid_az + off_u;
                const float vraw = tv * g.span * g.grid_el + off_v;
                const float vd = fminf(fmaxf(vraw, -90.f), 90.f);
                if (ud >= 180.f) ud -= 360.f;
                if (ud < -180.f) ud += 360.f;
                const float u1 = deg2rad_(ud), v1 = deg2rad_(vd);
                const float sv1 = sinf(v1), cv1 = cosf(v1);
                const float du = u1 - u2, adu = fabsf(du);
                const float cs = sv1 * sv2 + cv1 * cv2 * cosf(adu);
                const float lo = -1.f + 1e-7f, hi = 1.f - 1e-7f;
                const float cc = fminf(fmaxf(cs, lo), hi);
                D = rad2deg_(acosf(cc));
                if constexpr (GRAD) {
                    float dD_dcs = 0.f;
                    if (cs >= lo && cs <= hi) dD_dcs = -57.29577951308232f / sqrtf(1.f - cc * cc);
                    const float sgn = du > 0.f ? 1.f : (du < 0.f ? -1.f : 0.f);
                    const float dcs_du1 = -cv1 * cv2 * sinf(adu) * sgn;
                    const float dcs_dv1 = cv1 * sv2 - sv1 * cv2 * cosf(adu);
                    const float dU_dl = (1.f - tu * tu) * g.span * g.grid_az;
                    const float dV_dl = (vraw >= -90.f && vraw <= 90.f) ? (1.f - tv * tv) * g.span * g.grid_el : 0.f;
                    gu = dD_dcs * dcs_du1 * 0.017453292519943295f * dU_dl;
                    gv = dD_dcs * dcs_dv1 * 0.017453292519943295f * dV_dl;
                    if (dist) dist[(size_t)m * g.A + a] = D;
                }
            }
        }
    }
    // first index of the minimum over the octet (all 64 lanes take part in the shuffles)
    float dmin = D;
    int amin = a;
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) {
        const float od = __shfl_xor(dmin, o, 64);
        const int oa = __shfl_xor(amin, o, 64);
        if (od < dmin || (od == dmin && oa < amin)) {
            dmin = od;
            amin = oa;
        }
    }
    unsigned bits = 0, fresh = 0;
    if (valid && a < g.A) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (D < g.thr[i] || a == amin) bits |= 1u << i;
    }
    if (bits) {
        const long anchor = cell * g.A + a;
        const unsigned old = atomicOr(&pos_bits[anchor], bits);
        fresh = bits & ~old;
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (bits & (1u << i)) atomicOr(&cls_bits[(size_t)i * NA + anchor], 1u << cl);
        if (bits & 1u) {          // angular term uses the first threshold only (loss.py:241-243)
            my_sum = D / 180.f;
            my_pairs = 1;
            if constexpr (GRAD) {
                // several targets can share an anchor: their gradients are summed in 32.32 fixed point, so the
                // result does not depend on the order the atomics land in (bit-reproducible training steps)
                atomicAdd(&ang_grad[anchor * 2 + 0], to_fixed(gu / 180.f));
                atomicAdd(&ang_grad[anchor * 2 + 1], to_fixed(gv / 180.f));
            }
        }
    }
    // distinct positives / pairs of this wave (same-address atomics are serialised by the memory system at ~12 ns each: one
    // per wave and counter cost 0.65 ms at 137 k rows -- the counts are kept in registers and leave once per workgroup)
    cnt0 += __popcll(__ballot(fresh & 1u));
    cnt1 += __popcll(__ballot((fresh >> 1) & 1u));
    cnt2 += __popcll(__ballot((fresh >> 2) & 1u));
    cntp += __popcll(__ballot(my_pairs != 0));
    blk_sum += my_sum;
    }
    blk_sum = wave_sum(blk_sum);
    if (lane == 0) {
        red_sum[wave] = blk_sum;
        red_cnt[wave][0] = cnt0;
        red_cnt[wave][1] = cnt1;
        red_cnt[wave][2] = cnt2;
        red_cnt[wave][3] = cntp;
    }
    __syncthreads();
    // per-workgroup results go to plain arrays, ang_partial [count][LOSS_ASSIGN_BLOCKS] and behind it the counts
    // [count][LOSS_ASSIGN_BLOCKS][4].  !GRAD: the final kernel adds the counts up.  GRAD: the main kernel needs them, so the LAST
    // workgroup to arrive (one atomic per workgroup) adds them up in a fixed order and publishes them in the header
    unsigned *cnt_partial = reinterpret_cast<unsigned *>(ang_partial + (size_t)u.count * LOSS_ASSIGN_BLOCKS) +
                            (size_t)u.idx * LOSS_ASSIGN_BLOCKS * 4;
    ang_partial += (size_t)u.idx * LOSS_ASSIGN_BLOCKS;
    if (threadIdx.x < 4)
        cnt_partial[blockIdx.x * 4 + threadIdx.x] = (unsigned)(red_cnt[0][threadIdx.x] + red_cnt[1][threadIdx.x] +
                                                                red_cnt[2][threadIdx.x] + red_cnt[3][threadIdx.x]);
    if (threadIdx.x == 0) ang_partial[blockIdx.x] = red_sum[0] + red_sum[1] + red_sum[2] + red_sum[3];
    if constexpr (GRAD) {
        __shared__ bool is_last;
        __syncthreads();
        if (threadIdx.x == 0) {        // ONE device-scope fence per workgroup (a fence costs 5-20 ns per wave on this multi-XCD part;
            __threadfence();           // release is cumulative over the barrier: it also covers the stores of threads 1-3)
            is_last = atomicAdd(&hdr[4], 1u) == gridDim.x - 1;
        }
        __syncthreads();
        if (is_last) {
            __threadfence();
            unsigned t4[4] = {0u, 0u, 0u, 0u};
            for (unsigned bk = threadIdx.x; bk < gridDim.x; bk += blockDim.x) {
#pragma unroll
                for (int i = 0; i < 4; ++i)        // (device-scope loads: the other workgroups' stores, not a stale L1 line)
                    t4[i] += __hip_atomic_load(cnt_partial + 4 * bk + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {                  // integer sums: any order gives the same result
                unsigned v = t4[i];
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                if (lane == 0) red_cnt[wave][i] = (int)v;
            }
            __syncthreads();
            if (threadIdx.x < 4)
                hdr[threadIdx.x] = (unsigned)(red_cnt[0][threadIdx.x] + red_cnt[1][threadIdx.x] + red_cnt[2][threadIdx.x] +
                                              red_cnt[3][threadIdx.x]);
        }
    }
}

__device__ __forceinline__ float bce_grad_logit(float s, float y) {
    // nn.BCELoss backward (s - y) / max(s (1 - s), 1e-12), chained with sigmoid' = s (1 - s)
    const float q = s * (1.f - s);
    return (s - y) / fmaxf(q, 1e-12f) * q;
}

// One pass over the logits, tile by tile (LM_TILE anchors = LM_TILE * (C + 3) consecutive floats): the tile is copied into
// LDS with coalesced 16-byte loads, one lane then owns one ANCHOR (row stride odd: conflict-free) -- a negative anchor costs
// one sigmoid / log pair (its class and angle gradients are zero), a positive one the C class terms and the angular
// gradient -- and the gradients leave through the same LDS tile with coalesced 16-byte stores.
// GRAD: grid (workgroups); the weights of the gradient come from the header's counts, dlogit (optional) is written.  !GRAD: grid
// (workgroups of one clip, B): the same pass over clip b's NA anchors without the gradient; a clip without rows is skipped (its
// loss is not formed).  Every clip's logits start on a 16-byte boundary (NA * CH % 4 == 0, checked by the caller).
constexpr int LM_TILE = 256;
template <bool PAD, bool GRAD>
__global__ __launch_bounds__(256) void loss_main_kernel(const float *__restrict__ logit, LossGeom g,
                                                        const unsigned *__restrict__ hdr,
                                                        const unsigned *__restrict__ pos_bits,
                                                        const unsigned *__restrict__ cls_bits,
                                                        const unsigned long long *__restrict__ ang_grad,
                                                        float *__restrict__ dlogit,
                                                        float *__restrict__ partial, long NA, long NA_total,
                                                        float grad_scale, const int *__restrict__ row_start, long cap) {
    // NA: anchors of one unit.  NA_total: anchors of the whole (data-parallel) batch the header's counts refer to (== NA on one device)
    extern __shared__ __attribute__((aligned(16))) float tile[];      // [LM_TILE][CHP]
    __shared__ float red[4][9];
    const LossUnit u = loss_unit<GRAD>(g, row_start, cap, blockIdx.y, 0);
    if (!GRAD && u.M == 0) return;
    const int CH = g.C + 3;
    const int CHP = PAD ? CH + 1 : CH;              // PAD: CH is even -> odd row stride
    const int tid = threadIdx.x;
    const long cls_plane = NA * u.count;
    logit += (size_t)u.idx * NA * CH;
    pos_bits += (size_t)u.idx * NA;
    cls_bits += (size_t)u.idx * NA;
    partial += (size_t)u.idx * LOSS_MAIN_BLOCKS * 9;
    float wpos[3] = {}, wneg[3] = {}, wcls[3] = {}, wang = 0.f;
    if constexpr (GRAD) {
        float npos[3], nneg[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            npos[i] = (float)hdr[i];
            nneg[i] = (float)(NA_total - (long)hdr[i]);
        }
        const float npairs = (float)hdr[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            wpos[i] = g.gain_obj / (3.f * npos[i]);
            wneg[i] = g.gain_nonobj / (3.f * nneg[i]);
            wcls[i] = g.gain_cls / (3.f * npos[i] * (float)g.C);
        }
        wang = g.gain_ang / npairs;
    }
    float acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = 0.f;
    const long ntiles = (NA + LM_TILE - 1) / LM_TILE;
    for (long tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const long a0 = tl * LM_TILE;
        const int na = (int)((NA - a0) < LM_TILE ? (NA - a0) : LM_TILE);
        const int nel = na * CH, n4 = nel >> 2;
        const float *src = logit + (size_t)a0 * CH;         // LM_TILE * CH * 4 bytes is a multiple of 16
        for (int i = tid; i < n4; i += 256) {
            const float4 v = reinterpret_cast<const float4 *>(src)[i];
            if (PAD) {
                const unsigned e = 4u * i, r = e / (unsigned)CH, c = e - r * (unsigned)CH;
                float *d = tile + r * CHP + c;               // CH even and e % 4 == 0: c is even, c + 3 may cross the row end
                const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned ck = c + k;
                    (ck < (unsigned)CH ? d + k : tile + (r + 1) * CHP + (ck - CH))[0] = vv[k];
                }
            } else {
                reinterpret_cast<float4 *>(tile)[i] = v;
            }
        }
        for (int e = 4 * n4 + tid; e < nel; e += 256) {
            const int r = e / CH;
            tile[r * CHP + (e - r * CH)] = src[e];
        }
        __syncthreads();
        if (tid < na) {
            const long anchor = a0 + tid;
            float *x = tile + tid * CHP;
            const unsigned pb = pos_bits[anchor];
            {
                const float s = sigmoidf_(x[0]);
                const float lp = -fmaxf(logf(s), -100.f);           // -log(s), clamped like nn.BCELoss
                const float lq = -fmaxf(logf(1.f - s), -100.f);     // -log(1-s)
                const float g1 = GRAD ? bce_grad_logit(s, 1.f) : 0.f, g0 = GRAD ? bce_grad_logit(s, 0.f) : 0.f;
                float grad = 0.f;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    if (pb & (1u << i)) {
                        acc[i] += lp;
                        grad += wpos[i] * g1;
                    } else {
                        acc[3 + i] += lq;
                        grad += wneg[i] * g0;
                    }
                }
                if constexpr (GRAD) x[0] = grad * grad_scale;
            }
            if (pb) {
                unsigned cb[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) cb[i] = (pb & (1u << i)) ? cls_bits[(size_t)i * cls_plane + anchor] : 0u;
                for (int ch = 1; ch <= g.C; ++ch) {
                    const float s = sigmoidf_(x[ch]);
                    const float lp = -fmaxf(logf(s), -100.f);
                    const float lq = -fmaxf(logf(1.f - s), -100.f);
                    const float g1 = GRAD ? bce_grad_logit(s, 1.f) : 0.f, g0 = GRAD ? bce_grad_logit(s, 0.f) : 0.f;
                    float grad = 0.f;
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        if (pb & (1u << i)) {
                            const unsigned yb = (cb[i] >> (ch - 1)) & 1u;
                            acc[6 + i] += yb ? lp : lq;
                            grad += wcls[i] * (yb ? g1 : g0);
                        }
                    }
                    if constexpr (GRAD) x[ch] = grad * grad_scale;
                }
                if constexpr (GRAD) {
                    // (only anchors responsible at the first threshold ever received an angular gradient)
                    const ulonglong2 ag = (pb & 1u) ? *reinterpret_cast<const ulonglong2 *>(ang_grad + anchor * 2)
                                                    : make_ulonglong2(0ull, 0ull);
                    x[g.C + 1] = wang * from_fixed(ag.x) * grad_scale;
                    x[g.C + 2] = wang * from_fixed(ag.y) * grad_scale;
                }
            } else if constexpr (GRAD) {
                for (int ch = 1; ch < CH; ++ch) x[ch] = 0.f;
            }
        }
        __syncthreads();
        if (GRAD && dlogit) {
            float *dst = dlogit + (size_t)a0 * CH;
            for (int i = tid; i < n4; i += 256) {
                float4 v;
                if (PAD) {
                    const unsigned e = 4u * i, r = e / (unsigned)CH, c = e - r * (unsigned)CH;
                    float vv[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const unsigned ck = c + k;
                        vv[k] = (ck < (unsigned)CH ? tile + r * CHP + ck : tile + (r + 1) * CHP + (ck - CH))[0];
                    }
                    v = make_float4(vv[0], vv[1], vv[2], vv[3]);
                } else {
                    v = reinterpret_cast<const float4 *>(tile)[i];
                }
                reinterpret_cast<float4 *>(dst)[i] = v;
            }
            for (int e = 4 * n4 + tid; e < nel; e += 256) {
                const int r = e / CH;
                dst[e] = tile[r * CHP + (e - r * CH)];
            }
        }
        if constexpr (GRAD) __syncthreads();        // (the stage-out reads other lanes' rows of the tile)
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const float v = wave_sum(acc[i]);
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    if (tid < 9)
        partial[(size_t)blockIdx.x * 9 + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// One workgroup per unit combines its partial sums in double.  GRAD: grid (1); the four counts are the header's, NA is the batch
// total and nang the assign grid.  !GRAD: grid (B); the counts of clip b are added up here from its assign workgroups' partials
// (integers), NA is the clip's anchors, loss[b] and valid[b] are written (a clip without rows: 0 and 0).
template <bool GRAD>
__global__ __launch_bounds__(256) void loss_final_kernel(const float *__restrict__ partial, int nblk,
                                                         const float *__restrict__ ang_partial, int nang,
                                                         const unsigned *__restrict__ hdr, LossGeom g, long NA,
                                                         float *__restrict__ loss, int *__restrict__ valid,
                                                         const int *__restrict__ row_start, long cap) {
    __shared__ double red[256];
    __shared__ double tot[10];
    const LossUnit u = loss_unit<GRAD>(g, row_start, cap, blockIdx.x, nang);
    const unsigned *cnt = hdr;
    if constexpr (!GRAD) {
        __shared__ unsigned cred[4][4];
        __shared__ unsigned csum[4];
        if (u.M == 0) {
            if (threadIdx.x == 0) {
                loss[u.idx] = 0.f;
                valid[u.idx] = 0;
            }
            return;
        }
        const unsigned *cnt_partial = reinterpret_cast<const unsigned *>(ang_partial + (size_t)u.count * LOSS_ASSIGN_BLOCKS) +
                                      (size_t)u.idx * LOSS_ASSIGN_BLOCKS * 4;
        ang_partial += (size_t)u.idx * LOSS_ASSIGN_BLOCKS;
        partial += (size_t)u.idx * LOSS_MAIN_BLOCKS * 9;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        unsigned t4[4] = {0u, 0u, 0u, 0u};
        for (int bk = threadIdx.x; bk < u.nang; bk += 256) {
#pragma unroll
            for (int i = 0; i < 4; ++i) t4[i] += cnt_partial[4 * bk + i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned v = t4[i];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0) cred[wave][i] = v;
        }
        __syncthreads();
        if (threadIdx.x < 4) csum[threadIdx.x] = cred[0][threadIdx.x] + cred[1][threadIdx.x] + cred[2][threadIdx.x] + cred[3][threadIdx.x];
        cnt = csum;
    }
    const double s = block_colsum32(partial, nblk, 9, 0, 9, red);        // 9 BCE sums
    if ((threadIdx.x >> 5) == 0 && (threadIdx.x & 31) < 9) tot[threadIdx.x & 31] = s;
    double a = 0.0;
    for (int b = threadIdx.x; b < u.nang; b += 256) a += (double)ang_partial[b];
    red[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double ang = 0.0;
        for (int k = 0; k < 256; ++k) ang += red[k];
        double total = (double)g.gain_ang * ang / (double)cnt[3];
        for (int i = 0; i < 3; ++i) {
            const double np_ = (double)cnt[i], nn_ = (double)(NA - (long)cnt[i]);
            total += ((double)g.gain_obj * tot[i] / np_ + (double)g.gain_nonobj * tot[3 + i] / nn_ +
                      (double)g.gain_cls * tot[6 + i] / (np_ * (double)g.C)) / 3.0;
        }
        loss[u.idx] = (float)total;
        if constexpr (!GRAD) valid[u.idx] = 1;
    }
}

static LossGeom make_geom(int B, int T, int Gaz, int Gel, int A, int C, int M, const float *thr_host, const float *gains_host,
                          float grid_az, float grid_el, float g_overlap) {
    LossGeom g;
    g.B = B; g.T = T; g.Gaz = Gaz; g.Gel = Gel; g.A = A; g.C = C; g.M = M;
    for (int i = 0; i < 3; ++i) g.thr[i] = thr_host[i];
    g.gain_ang = gains_host[0]; g.gain_obj = gains_host[1]; g.gain_nonobj = gains_host[2]; g.gain_cls = gains_host[3];
    g.grid_az = grid_az; g.grid_el = grid_el; g.span = 0.5f + g_overlap;
    return g;
}

// main workgroups of one unit of NA anchors
static int main_blocks(long NA) {
    const long nb = (NA + LM_TILE - 1) / LM_TILE;
    return (int)(nb > LOSS_MAIN_BLOCKS ? LOSS_MAIN_BLOCKS : nb);
}

// loss_main_kernel<PAD, GRAD> on `grid`: an even C + 3 takes the PAD form (one more float per LDS row, one more row)
template <bool GRAD>
static void launch_loss_main(dim3 grid, hipStream_t st, const float *logit, const LossGeom &g, const unsigned *hdr,
                             const unsigned *pos_bits, const unsigned *cls_bits, const unsigned long long *ang_grad,
                             float *dlogit, float *partial, long NA, long na_total, float grad_scale, const int *row_start,
                             long cap) {
    const int CH = g.C + 3;
    if (CH & 1)
        hipLaunchKernelGGL((loss_main_kernel<false, GRAD>), grid, dim3(256), (size_t)LM_TILE * CH * 4, st, logit, g, hdr, pos_bits,
                           cls_bits, ang_grad, dlogit, partial, NA, na_total, grad_scale, row_start, cap);
    else
        hipLaunchKernelGGL((loss_main_kernel<true, GRAD>), grid, dim3(256), (size_t)(LM_TILE + 1) * (CH + 1) * 4, st, logit, g, hdr,
                           pos_bits, cls_bits, ang_grad, dlogit, partial, NA, na_total, grad_scale, row_start, cap);
}

}  // namespace adyolo

using namespace adyolo;

// workspace (32-bit words): [hdr 64][pos_bits NA][cls_bits 3*NA][ang_grad 2*NA x int64][ang_partial 1024][cnt_partial 4*1024][partial 9*2048]
extern "C" long adyolo_loss_workspace_words(int BT, int G, int A, int M) {
    const long NA = (long)BT * G * A;
    return LOSS_HDR + 8 * NA + 5L * LOSS_ASSIGN_BLOCKS + 9L * LOSS_MAIN_BLOCKS + 64;
}

// phases: 1 = workspace reset + assignment (fills the header's counts), 2 = the pass over the logits + the final sum.  One
// device runs both back to back (adyolo_loss_fwd_bwd).  Under EXACT data parallelism the header's four counts (distinct
// positives per threshold, responsible pairs) are all-reduced between the phases and phase 2 gets the anchor count of the
// whole batch (na_total): every term is then normalised like the single-device loss on the concatenated batch
// (loss.py:236-243), and the per-rank loss values add up to it.
extern "C" int adyolo_loss_phase(const float *logit, const float *target, float *ws, float *loss, float *dlogit,
                                 float *dist, int B, int T, int Gaz, int Gel, int A, int C, int M,
                                 const float *thr_host, const float *gains_host, float grid_az, float grid_el,
                                 float g_overlap, float grad_scale, int phases, long na_total, void *stream) {
    ADYOLO_REQUIRE(logit && target && ws && loss && thr_host && gains_host, ADYOLO_EINVAL, "loss: null pointer");
    ADYOLO_REQUIRE(B > 0 && T > 0 && Gaz > 0 && Gel > 0 && A > 0 && A <= 8 && C > 0 && C <= 32, ADYOLO_ENOSUP,
                   "loss: unsupported geometry A=%d (<=8) C=%d (<=32)", A, C);
    ADYOLO_REQUIRE(M > 0, ADYOLO_EINVAL, "loss: M == 0 (the reference fails on an empty target too, loss.py:224)");
    hipStream_t st = as_stream(stream);
    const long NA = (long)B * T * Gaz * Gel * A;
    ADYOLO_REQUIRE((phases & ~3) == 0 && phases != 0 && (na_total == 0 || na_total >= NA), ADYOLO_EINVAL, "loss: bad phases / na_total");
    if (na_total == 0) na_total = NA;
    const LossGeom g = make_geom(B, T, Gaz, Gel, A, C, M, thr_host, gains_host, grid_az, grid_el, g_overlap);

    unsigned *hdr = reinterpret_cast<unsigned *>(ws);
    unsigned *pos_bits = hdr + LOSS_HDR;
    unsigned *cls_bits = pos_bits + NA;
    unsigned long long *ang_grad = reinterpret_cast<unsigned long long *>(cls_bits + 3 * NA);   // 8-byte aligned: 64 + 4 NA words
    float *ang_partial = reinterpret_cast<float *>(ang_grad + 2 * NA);
    int nang = cdiv(M, 32);                 // 8 lanes per target row: 32 rows per workgroup and round
    if (nang > LOSS_ASSIGN_BLOCKS) nang = LOSS_ASSIGN_BLOCKS;
    float *partial = ang_partial + 5 * LOSS_ASSIGN_BLOCKS;
    int rc = 0;
    if (phases & 1) {
        rc = fill32(ws, 0u, (size_t)(LOSS_HDR + 8 * NA), st);             // (a kernel, not a memset node: see common.hpp)
        if (rc) return rc;
        hipLaunchKernelGGL(loss_assign_kernel<true>, dim3(nang), dim3(256), 0, st, logit, target, g, hdr, pos_bits, cls_bits,
                           ang_grad, ang_partial, dist, NA, nullptr, 0);
        rc = check_launch("loss_assign");
        if (rc) return rc;
    }
    if (phases & 2) {
        const int nb = main_blocks(NA);
        launch_loss_main<true>(dim3((unsigned)nb), st, logit, g, hdr, pos_bits, cls_bits, ang_grad, dlogit, partial, NA, na_total,
                               grad_scale, nullptr, 0);
        rc = check_launch("loss_main");
        if (rc) return rc;
        hipLaunchKernelGGL(loss_final_kernel<true>, dim3(1), dim3(256), 0, st, partial, nb, ang_partial, nang, hdr, g, na_total,
                           loss, nullptr, nullptr, 0);
        rc = check_launch("loss_final");
    }
    return rc;
}

extern "C" int adyolo_loss_fwd_bwd(const float *logit, const float *target, float *ws, float *loss, float *dlogit,
                                   float *dist, int B, int T, int Gaz, int Gel, int A, int C, int M,
                                   const float *thr_host, const float *gains_host, float grid_az, float grid_el,
                                   float g_overlap, float grad_scale, void *stream) {
    return adyolo_loss_phase(logit, target, ws, loss, dlogit, dist, B, T, Gaz, Gel, A, C, M, thr_host, gains_host, grid_az,
                             grid_el, g_overlap, grad_scale, 3, 0, stream);
}

// ---- K8b: AD-YOLO decode for inference (reference datasets.py:752-771, LabelPostProcessor.get_yolo_output) ----
// out[anchor][0] = sigmoid(obj); out[anchor][1..C] = sigmoid(cls) * sigmoid(obj) (class-confidence score);
// out[anchor][C+1] = U (deg, wrapped to [-180,180)), out[anchor][C+2] = V (deg, clamped to [-90, 90 - 1e-7])
namespace adyolo {
__global__ __launch_bounds__(256) void yolo_decode_kernel(const float *__restrict__ logit, float *__restrict__ out,
                                                          long n_anchor, int Gaz, int Gel, int A, int C, float grid_az,
                                                          float grid_el, float span) {
    const int CH = C + 3;
    for (long a = (long)blockIdx.x * blockDim.x + threadIdx.x; a < n_anchor; a += (long)gridDim.x * blockDim.x) {
        const long cell = a / A;
        const int gj = (int)(cell % Gel), gi = (int)((cell / Gel) % Gaz);
        const float *lp = logit + (size_t)a * CH;
        float *op = out + (size_t)a * CH;
        const float conf = sigmoidf_(lp[0]);
        op[0] = conf;
        for (int c = 1; c <= C; ++c) op[c] = sigmoidf_(lp[c]) * conf;
        float u = tanhf(lp[C + 1]) * span * grid_az + (gi * grid_az - 180.f + 0.5f * grid_az);
        float v = tanhf(lp[C + 2]) * span * grid_el + (gj * grid_el - 90.f + 0.5f * grid_el);
        v = fminf(fmaxf(v, -90.f), 90.f - 1e-7f);
        if (u >= 180.f) u -= 360.f;
        if (u < -180.f) u += 360.f;
        op[C + 1] = u;
        op[C + 2] = v;
    }
}
}  // namespace adyolo

extern "C" int adyolo_yolo_decode(const float *logit, float *out, long n_frames, int Gaz, int Gel, int A, int C,
                                  float grid_az, float grid_el, float g_overlap, void *stream) {
    ADYOLO_REQUIRE(logit && out && n_frames > 0 && Gaz > 0 && Gel > 0 && A > 0 && C > 0, ADYOLO_EINVAL, "yolo_decode: bad arguments");
    const long n_anchor = n_frames * Gaz * Gel * A;
    long g = (n_anchor + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(adyolo::yolo_decode_kernel, dim3((unsigned)g), dim3(256), 0, adyolo::as_stream(stream), logit, out,
                       n_anchor, Gaz, Gel, A, C, grid_az, grid_el, 0.5f + g_overlap);
    return adyolo::check_launch("yolo_decode");
}

// ---- K8f: per-clip AD-YOLO loss, forward only (evaluation: reference src/test.py:33-60 runs batch 1, so every normaliser of
// ADYOLOloss is per clip) ----
// B clips of one batched forward pass in one assignment launch, one pass over the logits and one finalisation.  loss[b] carries
// the bits adyolo_loss_fwd_bwd returns for clip b alone (its logits, its rows with b = 0, no dlogit).  The kernels are the !GRAD
// instantiations of the training kernels above -- loss_assign_kernel<false>, loss_main_kernel<PAD, false>,
// loss_final_kernel<false> against that call's loss_assign_kernel<true>, loss_main_kernel<PAD, true>, loss_final_kernel<true>
// -- so one body holds the row decode and distance, the arg-min and threshold bits, the tile staging, the nine BCE sums, the
// workgroup reductions and the combination in double.  What the two forms do not share is the normalisation unit (LossUnit: the
// grid has a clip dimension, and inside a clip the rows and the anchor tiles are dealt to workgroups exactly as that call deals
// them, 32 rows per assign workgroup up to LOSS_ASSIGN_BLOCKS, LM_TILE anchors per main workgroup up to LOSS_MAIN_BLOCKS) and
// what GRAD switches on: the derivative chain, the dist store, the fixed-point gradient atomics, the arrival counter and the
// header in the assignment; the weights, the gradient written into the tile and its stage-out to dlogit in the main pass; the
// header as the source of the counts in the finalisation.  Without a gradient nothing needs the counts before the final sum:
// they leave as per-workgroup partials and are added there.  A row counts only if its b column names the clip its range
// belongs to.
namespace adyolo {

// one thread: acc[0] += loss[i] for the valid i in order, in float32 (the host loop's ``total + loss``); acc[1] += their count
__global__ void loss_accumulate_kernel(const float *__restrict__ loss, const int *__restrict__ valid, int n,
                                       float *__restrict__ acc) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    float sum = acc[0], cnt = acc[1];
    for (int i = 0; i < n; ++i) {
        if (valid && !valid[i]) continue;
        sum = sum + loss[i];
        cnt = cnt + 1.f;
    }
    acc[0] = sum;
    acc[1] = cnt;
}

}  // namespace adyolo

// workspace (32-bit words): [pos_bits B*NA][cls_bits 3*B*NA][ang_partial B*1024][cnt_partial B*4*1024][partial B*9*2048]
extern "C" long adyolo_loss_per_clip_workspace_words(int B, int T, int G, int A) {
    if (B <= 0 || T <= 0 || G <= 0 || A <= 0) return -1;
    const long NA = (long)T * G * A;
    return (long)B * (4 * NA + 5L * LOSS_ASSIGN_BLOCKS + 9L * LOSS_MAIN_BLOCKS) + 64;
}

extern "C" int adyolo_loss_accumulate(const float *loss, const int *valid, int n, float *acc, void *stream) {
    ADYOLO_REQUIRE(loss && acc && n > 0, ADYOLO_EINVAL, "loss_accumulate: bad arguments");
    hipLaunchKernelGGL(loss_accumulate_kernel, dim3(1), dim3(64), 0, as_stream(stream), loss, valid, n, acc);
    return check_launch("loss_accumulate");
}

extern "C" int adyolo_loss_per_clip(const float *logit, const float *target, const int *row_start, float *ws, float *loss,
                                    int *valid, float *acc, int B, int T, int Gaz, int Gel, int A, int C, long cap,
                                    const float *thr_host, const float *gains_host, float grid_az, float grid_el,
                                    float g_overlap, void *stream) {
    ADYOLO_REQUIRE(logit && target && row_start && ws && loss && valid && thr_host && gains_host, ADYOLO_EINVAL,
                   "loss_per_clip: null pointer");
    ADYOLO_REQUIRE(B > 0 && B < 65536 && T > 0 && Gaz > 0 && Gel > 0 && A > 0 && A <= 8 && C > 0 && C <= 32, ADYOLO_ENOSUP,
                   "loss_per_clip: unsupported geometry B=%d A=%d (<=8) C=%d (<=32)", B, A, C);
    ADYOLO_REQUIRE(cap > 0 && cap < (1L << 31), ADYOLO_EINVAL, "loss_per_clip: bad target capacity %ld", cap);
    const long NA = (long)T * Gaz * Gel * A, NA_all = NA * B;
    const int CH = C + 3;
    // every clip's logits start on a 16-byte boundary, as its own call's would (the tile loads are 16 bytes wide)
    ADYOLO_REQUIRE(((uintptr_t)logit & 15) == 0 && (B == 1 || (NA * CH) % 4 == 0), ADYOLO_ENOSUP,
                   "loss_per_clip: a clip of %ld x %d logits does not start on a 16-byte boundary", NA, CH);
    hipStream_t st = as_stream(stream);
    const LossGeom g = make_geom(B, T, Gaz, Gel, A, C, 0, thr_host, gains_host, grid_az, grid_el, g_overlap);

    unsigned *pos_bits = reinterpret_cast<unsigned *>(ws);
    unsigned *cls_bits = pos_bits + NA_all;
    float *ang_partial = reinterpret_cast<float *>(cls_bits + 3 * NA_all);        // (cnt_partial follows it: 4 B words more per slot)
    float *partial = ang_partial + (size_t)B * 5 * LOSS_ASSIGN_BLOCKS;
    int rc = fill32(ws, 0u, (size_t)(4 * NA_all), st);
    if (rc) return rc;
    int gx = cdiv(cap, 32);
    if (gx > LOSS_ASSIGN_BLOCKS) gx = LOSS_ASSIGN_BLOCKS;
    hipLaunchKernelGGL(loss_assign_kernel<false>, dim3((unsigned)gx, (unsigned)B), dim3(256), 0, st, logit, target, g, nullptr,
                       pos_bits, cls_bits, nullptr, ang_partial, nullptr, NA_all, row_start, cap);
    rc = check_launch("loss_assign_clip");
    if (rc) return rc;
    const int nb = main_blocks(NA);
    launch_loss_main<false>(dim3((unsigned)nb, (unsigned)B), st, logit, g, nullptr, pos_bits, cls_bits, nullptr, nullptr, partial,
                            NA, 0, 0.f, row_start, cap);
    rc = check_launch("loss_main_clip");
    if (rc) return rc;
    hipLaunchKernelGGL(loss_final_kernel<false>, dim3((unsigned)B), dim3(256), 0, st, partial, nb, ang_partial, 0, nullptr, g, NA,
                       loss, valid, row_start, cap);
    rc = check_launch("loss_final_clip");
    if (rc) return rc;
    if (acc) {
        hipLaunchKernelGGL(loss_accumulate_kernel, dim3(1), dim3(64), 0, st, loss, valid, B, acc);
        rc = check_launch("loss_accumulate");
    }
    return rc;
}
