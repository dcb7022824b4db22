// AD-YOLO detection selection on the GPU: the confidence / class thresholds and the per-class NMS of
// LabelPostProcessor.get_yolo_output (src/datasets.py:773-855, helpers :858-919), i.e. postprocess.nms_decoded, on a
// decoded tensor [frames][N = Gaz*Gel*A][C+3] (csrc/loss.hip yolo_decode_kernel).
//
// Three launches:
//   1. yolo_select_kernel, one wave per (frame, class): filter conf > conf_t and class_conf > clss_t; stable rank by
//      descending class_conf (ties: anchor order, what argsort(kind="stable") does on the np.nonzero order); the sorted
//      rows' angles, xyz and vote exponents go to LDS; then the clusters, seeded in rank order:
//        conn-merge  connected components of dist < unify, grown breadth first from the lowest unassigned rank
//        soft-merge  greedy: the seed's cluster is every row of the class with dist <= unify (removed ones too); the
//                    rows within dist <= unify of the seed leave the remaining set
//        plain       the same greedy suppression, each seed written alone, xyz not normalised
//      and the vote of each cluster (postprocess._voted: softmax of exp(conf^2 / t), weighted xyz, normalised).  A class
//      with one surviving row is written alone (postprocess._single).  Rows go to a per-(frame, class) slot of the workspace.
//      Every pair distance is evaluated at most once per seed (greedy) or once per frontier row (components), so the cost
//      grows with the surviving candidates K (K^2 at worst), not with N^2.
//   2. select_scan_kernel (one workgroup): exclusive scan of the slot counts, per-frame row counts and the total.
//   3. select_compact_kernel: slot rows -> compacted [frame, class, x, y, z].
// Angular distances use the float32 formula of postprocess._ang_dist_deg evaluated in its order without contraction.
// The class-wise heads (seddoa / accdoa / adpit) select with adyolo_classwise_select further down; behind it, the rows that
// several views of a clip select are merged by adyolo_tta_collect / adyolo_tta_merge (rotation test-time augmentation).
#include "common.hpp"

namespace adyolo {

constexpr int SEL_WAVE = 64;
constexpr int SEL_WORDS = ADYOLO_SELECT_MAX_N / SEL_WAVE;   // rows per lane: row j = lane + 64 k, bit k of a lane mask
static_assert(SEL_WORDS <= 32, "lane masks are 32-bit");

// numpy's float32 constants: np.deg2rad multiplies by (float)(pi / 180), np.rad2deg by 180.f / (float)pi
#define SEL_D2R 0.017453292f
#define SEL_R2D 57.295776f

__device__ __forceinline__ float sel_dist(float ru_a, float sv_a, float cv_a, float ru_b, float sv_b, float cv_b) {
#pragma clang fp contract(off)
    float d = sv_a * sv_b + cv_a * cv_b * cosf(fabsf(ru_a - ru_b));
    d = fminf(fmaxf(d, -1.f), 1.f);
    return acosf(d) * SEL_R2D;
}

// lowest row index whose bit is set in some lane's mask, or -1 (wave-uniform)
__device__ __forceinline__ int sel_first(uint32_t bits, int kw) {
    for (int k = 0; k < kw; ++k) {
        const unsigned long long b = __ballot((bits >> k) & 1u);
        if (b) return k * SEL_WAVE + (int)__builtin_ctzll(b);
    }
    return -1;
}

// One connected component of the relation near(f, j), grown breadth first from `seed` (already taken out of `left`) over the
// rows still in `left`; the rows that join leave `left`.  -> the component as lane masks.  front: two lists of K ints in LDS.
template <class Near>
__device__ __forceinline__ uint32_t sel_grow(int seed, uint32_t &left, int kw, int lane, int *const *front, Near near) {
    uint32_t memb = lane == (seed & (SEL_WAVE - 1)) ? 1u << (seed / SEL_WAVE) : 0u;
    int cur = 0, fsz = 1;
    if (lane == 0) front[0][0] = seed;
    __syncthreads();
    while (fsz > 0) {
        uint32_t fresh = 0;
        for (int k = 0; k < kw; ++k) {
            if (!((left >> k) & 1u)) continue;
            const int j = lane + k * SEL_WAVE;
            for (int q = 0; q < fsz; ++q)
                if (near(front[cur][q], j)) {
                    fresh |= 1u << k;
                    break;
                }
        }
        int n = 0;
        for (int k = 0; k < kw; ++k) {
            const unsigned long long b = __ballot((fresh >> k) & 1u);
            if ((fresh >> k) & 1u) front[cur ^ 1][n + __popcll(b & ((1ull << lane) - 1ull))] = lane + k * SEL_WAVE;
            n += __popcll(b);
        }
        left &= ~fresh;
        memb |= fresh;
        __syncthreads();
        cur ^= 1;
        fsz = n;
    }
    return memb;
}

struct SelRows {
    float *ru, *sv, *cv, *x, *y, *z, *e;   // sorted by rank: u (rad), sin v, cos v, unit vector, exp(conf^2 / t)
};

// postprocess._voted over the rows whose bits are set in `memb` (wave-wide; every lane returns the result)
__device__ void sel_vote(const SelRows &r, uint32_t memb, int kw, int lane, float &ox, float &oy, float &oz) {
#pragma clang fp contract(off)
    float m = -INFINITY;
    for (int k = 0; k < kw; ++k)
        if ((memb >> k) & 1u) m = fmaxf(m, r.e[lane + k * SEL_WAVE]);
    m = wave_max(m);
    float sw = 0.f;
    for (int k = 0; k < kw; ++k)
        if ((memb >> k) & 1u) sw += expf(r.e[lane + k * SEL_WAVE] - m);
    sw = wave_sum(sw);
    float vx = 0.f, vy = 0.f, vz = 0.f;
    for (int k = 0; k < kw; ++k)
        if ((memb >> k) & 1u) {
            const int j = lane + k * SEL_WAVE;
            const float w = expf(r.e[j] - m) / sw;
            vx += r.x[j] * w;
            vy += r.y[j] * w;
            vz += r.z[j] * w;
        }
    vx = wave_sum(vx);
    vy = wave_sum(vy);
    vz = wave_sum(vz);
    const float n = sqrtf(vx * vx + vy * vy + vz * vz);
    ox = vx / n;
    oy = vy / n;
    oz = vz / n;
}

// grid: one 64-lane workgroup per (frame, class) slot; dynamic LDS: 9 arrays of npad = N rounded up to 64 words
__global__ __launch_bounds__(64) void yolo_select_kernel(const float *__restrict__ dec, float *__restrict__ slot_xyz,
                                                         int *__restrict__ slot_count, int N, int C, float conf_t,
                                                         float clss_t, float unify_t, float vote_t, int mode) {
#pragma clang fp contract(off)
    extern __shared__ float sel_lds[];
    const int npad = (N + SEL_WAVE - 1) / SEL_WAVE * SEL_WAVE;
    float *s_key = sel_lds;                                       // class conf of the survivors, anchor order
    int *s_anchor = reinterpret_cast<int *>(sel_lds + npad);      // their anchor index
    int *s_front[2] = {reinterpret_cast<int *>(s_key), s_anchor}; // conn-merge frontier lists (after the sort)
    SelRows r{sel_lds + 2 * npad, sel_lds + 3 * npad, sel_lds + 4 * npad, sel_lds + 5 * npad,
              sel_lds + 6 * npad, sel_lds + 7 * npad, sel_lds + 8 * npad};
    const long slot = blockIdx.x;
    const long frame = slot / C;
    const int cls = (int)(slot - frame * C);
    const int lane = threadIdx.x;
    const int CH = C + 3;
    const float *fd = dec + (size_t)frame * N * CH;
    float *out = slot_xyz + (size_t)slot * N * 3;

    // 1. filter, compacted in anchor order
    int K = 0;
    for (int n0 = 0; n0 < N; n0 += SEL_WAVE) {
        const int n = n0 + lane;
        float cc = 0.f;
        bool pass = false;
        if (n < N) {
            const float *p = fd + (size_t)n * CH;
            cc = p[1 + cls];
            pass = p[0] > conf_t && cc > clss_t;
        }
        const unsigned long long b = __ballot(pass);
        if (pass) {
            const int at = K + __popcll(b & ((1ull << lane) - 1ull));
            s_key[at] = cc;
            s_anchor[at] = n;
        }
        K += __popcll(b);
    }
    if (K == 0) {
        if (lane == 0) slot_count[slot] = 0;
        return;
    }
    __syncthreads();
    // 2. stable rank by descending class conf; the sorted rows' angles, unit vectors and vote exponents
    for (int i = lane; i < K; i += SEL_WAVE) {
        const float ki = s_key[i];
        int rank = 0;
        for (int j = 0; j < K; ++j) {
            const float kj = s_key[j];
            rank += (kj > ki) || (kj == ki && j < i);
        }
        const float *p = fd + (size_t)s_anchor[i] * CH;
        const float ru = p[C + 1] * SEL_D2R, rv = p[C + 2] * SEL_D2R;
        const float sv = sinf(rv), cv = cosf(rv);
        r.ru[rank] = ru;
        r.sv[rank] = sv;
        r.cv[rank] = cv;
        r.x[rank] = cosf(ru) * cv;
        r.y[rank] = sinf(ru) * cv;
        r.z[rank] = sv;
        r.e[rank] = expf(ki * ki / vote_t);
    }
    __syncthreads();
    if (K == 1) {                                                 // _single: not normalised
        if (lane == 0) {
            out[0] = r.x[0];
            out[1] = r.y[0];
            out[2] = r.z[0];
            slot_count[slot] = 1;
        }
        return;
    }
    const int kw = (K + SEL_WAVE - 1) / SEL_WAVE;
    uint32_t left = 0;                                            // rows not yet removed / assigned
    for (int k = 0; k < kw; ++k)
        if (lane + k * SEL_WAVE < K) left |= 1u << k;
    int S = 0;
    for (int seed = sel_first(left, kw); seed >= 0; seed = sel_first(left, kw), ++S) {
        if (lane == (seed & (SEL_WAVE - 1))) left &= ~(1u << (seed / SEL_WAVE));
        float ox, oy, oz;
        if (mode == ADYOLO_SELECT_CONN) {
            const uint32_t memb = sel_grow(seed, left, kw, lane, s_front, [&](int f, int j) {
                return sel_dist(r.ru[f], r.sv[f], r.cv[f], r.ru[j], r.sv[j], r.cv[j]) < unify_t;
            });
            sel_vote(r, memb, kw, lane, ox, oy, oz);
        } else {
            const float ru = r.ru[seed], sv = r.sv[seed], cv = r.cv[seed];
            uint32_t memb = 0;
            for (int k = 0; k < kw; ++k) {
                const int j = lane + k * SEL_WAVE;
                if (j >= K || (mode != ADYOLO_SELECT_SOFT && !((left >> k) & 1u))) continue;
                const bool near = !(sel_dist(ru, sv, cv, r.ru[j], r.sv[j], r.cv[j]) > unify_t);
                if (near) {
                    memb |= 1u << k;
                    left &= ~(1u << k);
                }
            }
            if (mode == ADYOLO_SELECT_SOFT) {
                sel_vote(r, memb, kw, lane, ox, oy, oz);
            } else {
                ox = r.x[seed];
                oy = r.y[seed];
                oz = r.z[seed];
            }
        }
        if (lane == 0) {
            out[3 * S + 0] = ox;
            out[3 * S + 1] = oy;
            out[3 * S + 2] = oz;
        }
    }
    if (lane == 0) slot_count[slot] = S;
}

constexpr int SCAN_THREADS = 1024;

// counts [n_slots] -> offsets [n_slots] (exclusive), frame_counts [n_frames] (+ the total at [n_frames])
__global__ __launch_bounds__(SCAN_THREADS) void select_scan_kernel(const int *__restrict__ count, int *__restrict__ offs,
                                                                   int *__restrict__ frame_counts, long n_frames, int C) {
    __shared__ int part[SCAN_THREADS];
    const int t = threadIdx.x;
    const long n_slots = n_frames * C;
    const long chunk = (n_slots + SCAN_THREADS - 1) / SCAN_THREADS;
    const long s0 = t * chunk, s1 = s0 + chunk < n_slots ? s0 + chunk : n_slots;
    int sum = 0;
    for (long s = s0; s < s1; ++s) sum += count[s];
    part[t] = sum;
    __syncthreads();
    for (int o = 1; o < SCAN_THREADS; o <<= 1) {                 // inclusive Hillis-Steele scan of the chunk sums
        const int v = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - sum;
    for (long s = s0; s < s1; ++s) {
        offs[s] = run;
        run += count[s];
    }
    for (long f = t; f < n_frames; f += SCAN_THREADS) {
        int c = 0;
        for (int k = 0; k < C; ++k) c += count[f * C + k];
        frame_counts[f] = c;
    }
    if (t == SCAN_THREADS - 1) frame_counts[n_frames] = part[t];
}

__global__ __launch_bounds__(64) void select_compact_kernel(const float *__restrict__ slot_xyz, const int *__restrict__ count,
                                                            const int *__restrict__ offs, float *__restrict__ rows,
                                                            long n_slots, int N, int C) {
    for (long slot = blockIdx.x; slot < n_slots; slot += gridDim.x) {
        const int cnt = count[slot];
        const float *src = slot_xyz + (size_t)slot * N * 3;
        float *dst = rows + (size_t)offs[slot] * 5;
        const float fr = (float)(slot / C), cl = (float)(slot % C);
        for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
            dst[5 * i + 0] = fr;
            dst[5 * i + 1] = cl;
            dst[5 * i + 2] = src[3 * i + 0];
            dst[5 * i + 3] = src[3 * i + 1];
            dst[5 * i + 4] = src[3 * i + 2];
        }
    }
}

// ---------------------------------------------------------------------------------------------- class-wise heads
// postprocess.classwise_select (get_seddoa_output / get_accdoa_output / get_adpit_output, src/datasets.py:536-739) on the
// records of adyolo_classwise_decode (csrc/losses.hip): up to three rows per (frame, class).  Three launches: the counts of
// every (frame, class), select_scan_kernel above, and a pass that evaluates the slots again and stores them at the scanned
// offsets -- the rows are a pure function of one 16- or 64-byte record, so evaluating twice is cheaper than parking them.
// All float32, the sums in the host's operand order.

// the rows of one (frame, class) in the reference's order, each handed to emit(x, y, z)
template <int MODE, class Emit>
__device__ __forceinline__ void classwise_slots(const float *__restrict__ dec, long slot, float conf_t, float unify_t,
                                                Emit emit) {
#pragma clang fp contract(off)                                   // nothing here multiplies today; kept so that it stays exact
    const bool one_above = 1.0f > conf_t;                        // the reference's second test, on the boolean (_above)
    if (MODE != ADYOLO_CLASSWISE_ADPIT) {
        const f32x4 r = reinterpret_cast<const f32x4 *>(dec)[slot];
        if (r[0] > conf_t && one_above) emit(r[1], r[2], r[3]);
        return;
    }
    const f32x4 *p = reinterpret_cast<const f32x4 *>(dec) + slot * 4;
    const f32x4 r0 = p[0], r1 = p[1], r2 = p[2], r3 = p[3];
    const float ax = r0[3], ay = r1[0], az = r1[1], bx = r1[2], by = r1[3], bz = r2[0], dx = r2[1], dy = r2[2], dz = r2[3];
    const bool s0 = r0[0] > conf_t, s1 = r0[1] > conf_t, s2 = r0[2] > conf_t;
    const bool q0 = s0 && one_above, q1 = s1 && one_above, q2 = s2 && one_above;
    const bool p01 = s0 && s1 && r3[0] < unify_t, p12 = s1 && s2 && r3[1] < unify_t, p20 = s2 && s0 && r3[2] < unify_t;
    const int n = (int)p01 + (int)p12 + (int)p20;
    if (n == 0) {                                                 // every active track, in track order
        if (q0) emit(ax, ay, az);
        if (q1) emit(bx, by, bz);
        if (q2) emit(dx, dy, dz);
    } else if (n >= 2) {                                          // one event: the mean of all three
        emit(((ax + bx) + dx) / 3.f, ((ay + by) + dy) / 3.f, ((az + bz) + dz) / 3.f);
    } else if (p01) {                                             // one pair: the third track, then the mean of the pair
        if (q2) emit(dx, dy, dz);
        emit((ax + bx) / 2.f, (ay + by) / 2.f, (az + bz) / 2.f);
    } else if (p12) {
        if (q0) emit(ax, ay, az);
        emit((bx + dx) / 2.f, (by + dy) / 2.f, (bz + dz) / 2.f);
    } else {
        if (q1) emit(bx, by, bz);
        emit((dx + ax) / 2.f, (dy + ay) / 2.f, (dz + az) / 2.f);
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void classwise_count_kernel(const float *__restrict__ dec, int *__restrict__ count,
                                                              long n_slots, float conf_t, float unify_t) {
    const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n_slots) return;
    int n = 0;
    classwise_slots<MODE>(dec, slot, conf_t, unify_t, [&](float, float, float) { ++n; });
    count[slot] = n;
}

template <int MODE>
__global__ __launch_bounds__(256) void classwise_write_kernel(const float *__restrict__ dec, const int *__restrict__ offs,
                                                              float *__restrict__ rows, long n_slots, int C, float conf_t,
                                                              float unify_t) {
    const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n_slots) return;
    const float fr = (float)(slot / C), cl = (float)(slot % C);
    float *dst = rows + (size_t)offs[slot] * 5;
    classwise_slots<MODE>(dec, slot, conf_t, unify_t, [&](float x, float y, float z) {
        dst[0] = fr, dst[1] = cl, dst[2] = x, dst[3] = y, dst[4] = z;
        dst += 5;
    });
}

template <int MODE>
static int classwise_select_launch(const float *dec, int *count, int *offs, float *rows, int *frame_counts, long n_frames,
                                   int C, float conf_t, float unify_t, hipStream_t st) {
    const long n_slots = n_frames * C;
    const dim3 grid(cdiv(n_slots, 256)), block(256);
    hipLaunchKernelGGL(classwise_count_kernel<MODE>, grid, block, 0, st, dec, count, n_slots, conf_t, unify_t);
    int rc = check_launch("classwise_select_count");
    if (rc) return rc;
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, count, offs, frame_counts, n_frames, C);
    rc = check_launch("classwise_select_scan");
    if (rc) return rc;
    hipLaunchKernelGGL(classwise_write_kernel<MODE>, grid, block, 0, st, dec, offs, rows, n_slots, C, conf_t, unify_t);
    return check_launch("classwise_select_write");
}

// ------------------------------------------------------------------------------------ rotation test-time augmentation
// postprocess.merge_view_rows on the device.  adyolo_tta_collect turns one view's selected rows back into the recording's frame
// and parks them, frame by frame, in a pool [V][frames][P] of {class, x, y, z}; adyolo_tta_merge clusters the pool's rows per
// (frame, class) -- connected components of dot > cos_t over unit vectors, seeded in candidate order (views ascending, a
// view's rows in the order its selection wrote them) -- keeps the clusters that at least min_views DISTINCT views support and
// writes [frame, class, s / |s|], s the sum of the members' unit vectors in candidate order.  Every operation is a correctly
// rounded float32 one evaluated in the host's order without contraction: the rows are the host's bit for bit.
// Merge launches: the kept clusters of every (frame, class) counted, select_scan_kernel, and a pass that forms them again and
// stores them at the scanned offsets (as the class-wise selection: cheaper than parking up to 1024 rows per slot).

// view matrix as a word: component i of the turned-back vector is sign_i * xyz[src_i]; src_i in bits [4 i, 4 i + 2), bit
// 4 i + 2 set for a negative sign (the product with +-1 is exact, and a zero keeps the sign the host's product gives it)
__device__ __forceinline__ float tta_pick(uint32_t m, int i, float x, float y, float z) {
    const uint32_t f = m >> (4 * i);
    const float v = (f & 3u) == 0 ? x : (f & 3u) == 1 ? y : z;
    return v * ((f & 4u) ? -1.f : 1.f);
}

__device__ __forceinline__ float tta_dot(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    return (ax * bx + ay * by) + az * bz;
}

// one thread per (frame, pool position); offs: exclusive scan of counts
__global__ __launch_bounds__(256) void tta_collect_kernel(const float *__restrict__ rows, long n_rows,
                                                          const int *__restrict__ counts, const int *__restrict__ offs,
                                                          f32x4 *__restrict__ pool, int *__restrict__ pool_counts,
                                                          long n_frames, int P, int C, uint32_t mat, int *__restrict__ status) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long f = t / P;
    const int i = (int)(t - f * P);
    if (f >= n_frames) return;
    int cnt = counts[f], bits = 0;
    const long off = offs[f];
    if (cnt < 0 || off < 0 || off + cnt > n_rows) {
        cnt = 0;
        bits |= ADYOLO_TTA_BAD_ROWS;
    }
    if (cnt > P) {
        cnt = P;
        bits |= ADYOLO_TTA_ROWS_OVERFLOW;
    }
    if (i < cnt) {
        const float *r = rows + (size_t)(off + i) * 5;
        const float c = r[1], x = r[2], y = r[3], z = r[4];
        f32x4 o;
        o[0] = c;
        o[1] = tta_pick(mat, 0, x, y, z);
        o[2] = tta_pick(mat, 1, x, y, z);
        o[3] = tta_pick(mat, 2, x, y, z);
        pool[f * P + i] = o;
        if (!(c >= 0.f && c < (float)C)) atomicOr(status, ADYOLO_TTA_BAD_ROWS);   // no (frame, class) would own the row
    }
    if (i == 0) {
        pool_counts[f] = cnt;
        if (bits) atomicOr(status, bits);
    }
}

// grid: one 64-lane workgroup per (frame, class); dynamic LDS: 7 arrays of kmax words (kmax a multiple of 64).  WRITE = false:
// count[slot] = kept clusters; WRITE = true: the rows of a slot with count[slot] > 0 at offs[slot].
template <bool WRITE>
__global__ __launch_bounds__(64) void tta_merge_kernel(const f32x4 *__restrict__ pool, const int *__restrict__ pool_counts,
                                                       int *__restrict__ count, const int *__restrict__ offs,
                                                       float *__restrict__ rows, long n_frames, int C, int V, int P, int kmax,
                                                       float cos_t, int min_views, int *__restrict__ status) {
#pragma clang fp contract(off)
    extern __shared__ float sel_lds[];
    float *ux = sel_lds, *uy = sel_lds + kmax, *uz = sel_lds + 2 * kmax;
    int *s_view = reinterpret_cast<int *>(sel_lds + 3 * kmax), *s_cl = s_view + kmax;
    int *s_front[2] = {s_cl + kmax, s_cl + 2 * kmax};
    const long slot = blockIdx.x;
    const long frame = slot / C;
    const int cls = (int)(slot - frame * C);
    const int lane = threadIdx.x;
    if (WRITE && count[slot] == 0) return;
    // 1. the candidates of this class: views ascending, a view's rows in pool order; unit vectors
    int K = 0;
    bool bad = false;
    for (int v = 0; v < V; ++v) {
        const int n = min(max(pool_counts[v * n_frames + frame], 0), P);
        const f32x4 *src = pool + ((size_t)v * n_frames + frame) * P;
        for (int i0 = 0; i0 < n; i0 += SEL_WAVE) {
            const int i = i0 + lane;
            bool good = false;
            float x = 0.f, y = 0.f, z = 0.f, nrm = 1.f;
            if (i < n) {
                const f32x4 r = src[i];
                if (r[0] == (float)cls) {
                    x = r[1], y = r[2], z = r[3];
                    nrm = sqrtf((x * x + y * y) + z * z);
                    good = nrm > 0.f && nrm < INFINITY;           // a zero, infinite or NaN norm: dropped and reported
                    bad |= !good;
                }
            }
            const unsigned long long b = __ballot(good);
            const int at = K + __popcll(b & ((1ull << lane) - 1ull));
            if (good && at < kmax) {
                ux[at] = x / nrm;
                uy[at] = y / nrm;
                uz[at] = z / nrm;
                s_view[at] = v;
            }
            K += __popcll(b);
        }
    }
    if (!WRITE && bad) atomicOr(status, ADYOLO_TTA_BAD_VECTOR);
    if (K == 0 || K > ADYOLO_SELECT_MAX_N || K > kmax) {          // (kmax >= min(V * P, ADYOLO_SELECT_MAX_N): one condition)
        if (!WRITE && lane == 0) {
            count[slot] = 0;
            if (K) atomicOr(status, ADYOLO_TTA_CAND_OVERFLOW);
        }
        return;
    }
    __syncthreads();
    // 2. connected components, seeded at the lowest unassigned candidate
    const int kw = (K + SEL_WAVE - 1) / SEL_WAVE;
    uint32_t left = 0;
    for (int k = 0; k < kw; ++k)
        if (lane + k * SEL_WAVE < K) left |= 1u << k;
    int S = 0;
    for (int seed = sel_first(left, kw); seed >= 0; seed = sel_first(left, kw), ++S) {
        if (lane == (seed & (SEL_WAVE - 1))) left &= ~(1u << (seed / SEL_WAVE));
        const uint32_t memb = sel_grow(seed, left, kw, lane, s_front, [&](int f, int j) {
            return tta_dot(ux[f], uy[f], uz[f], ux[j], uy[j], uz[j]) > cos_t;
        });
        for (int k = 0; k < kw; ++k)
            if ((memb >> k) & 1u) s_cl[lane + k * SEL_WAVE] = S;
    }
    __syncthreads();
    // 3. one lane per cluster: the views that support it and the sum of its members in candidate order
    int kept = 0;
    float *dst = WRITE ? rows + (size_t)offs[slot] * 5 : nullptr;
    for (int c0 = 0; c0 < S; c0 += SEL_WAVE) {
        const int c = c0 + lane;
        float sx = 0.f, sy = 0.f, sz = 0.f;
        uint32_t views = 0;
        if (c < S)
            for (int j = 0; j < K; ++j)
                if (s_cl[j] == c) {                               // the sum starts AT the first member: a lone -0 stays -0
                    sx = views ? sx + ux[j] : ux[j];
                    sy = views ? sy + uy[j] : uy[j];
                    sz = views ? sz + uz[j] : uz[j];
                    views |= 1u << s_view[j];
                }
        const bool keep = c < S && __popc(views) >= min_views;
        const unsigned long long b = __ballot(keep);
        if (WRITE && keep) {
            float *d = dst + (size_t)(kept + __popcll(b & ((1ull << lane) - 1ull))) * 5;
            const float nrm = sqrtf((sx * sx + sy * sy) + sz * sz);
            d[0] = (float)frame, d[1] = (float)cls, d[2] = sx / nrm, d[3] = sy / nrm, d[4] = sz / nrm;
        }
        kept += __popcll(b);
    }
    if (!WRITE && lane == 0) count[slot] = kept;
}

// the matrix word of adyolo_tta_collect: three sources that are a permutation of the axes
static inline bool tta_matrix_ok(unsigned m) {
    const unsigned a = m & 3u, b = (m >> 4) & 3u, c = (m >> 8) & 3u;
    return (m >> 11) == 0 && !(m & 0x88u) && a < 3 && b < 3 && c < 3 && a != b && b != c && a != c;
}

}  // namespace adyolo

using namespace adyolo;

extern "C" long adyolo_yolo_select_workspace_words(long n_frames, int n_anchor, int C) {
    if (n_frames <= 0 || n_anchor <= 0 || C <= 0) return 0;
    return n_frames * C * (3L * n_anchor + 2);
}

extern "C" int adyolo_yolo_select(const float *dec, float *ws, float *rows, int *frame_counts, long n_frames, int n_anchor,
                                  int C, float conf_thresh, float clss_thresh, float unify_thresh, float vote_thresh,
                                  int mode, void *stream) {
    ADYOLO_REQUIRE(dec && ws && rows && frame_counts && n_frames > 0 && n_anchor > 0 && C > 0, ADYOLO_EINVAL,
                   "yolo_select: bad arguments");
    ADYOLO_REQUIRE(mode == ADYOLO_SELECT_PLAIN || mode == ADYOLO_SELECT_CONN || mode == ADYOLO_SELECT_SOFT, ADYOLO_EINVAL,
                   "yolo_select: unknown mode %d", mode);
    ADYOLO_REQUIRE(n_anchor <= ADYOLO_SELECT_MAX_N, ADYOLO_ENOSUP, "yolo_select: %d candidates per frame and class, at most %d",
                   n_anchor, ADYOLO_SELECT_MAX_N);
    const long n_slots = n_frames * C;
    ADYOLO_REQUIRE(n_slots * n_anchor < (1L << 31) && n_slots < (1L << 31), ADYOLO_ENOSUP,
                   "yolo_select: %ld frames x %d classes x %d candidates do not fit 32-bit row counts", n_frames, C, n_anchor);
    float *slot_xyz = ws;
    int *count = reinterpret_cast<int *>(ws + (size_t)n_slots * n_anchor * 3);
    int *offs = count + n_slots;
    hipStream_t st = as_stream(stream);
    const int npad = (n_anchor + SEL_WAVE - 1) / SEL_WAVE * SEL_WAVE;
    hipLaunchKernelGGL(yolo_select_kernel, dim3((unsigned)n_slots), dim3(SEL_WAVE), (size_t)9 * npad * sizeof(float), st,
                       dec, slot_xyz, count, n_anchor, C, conf_thresh, clss_thresh, unify_thresh, vote_thresh, mode);
    int rc = check_launch("yolo_select");
    if (rc) return rc;
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, count, offs, frame_counts, n_frames, C);
    rc = check_launch("yolo_select_scan");
    if (rc) return rc;
    const long g = n_slots < 4096 ? n_slots : 4096;
    hipLaunchKernelGGL(select_compact_kernel, dim3((unsigned)g), dim3(64), 0, st, slot_xyz, count, offs, rows, n_slots,
                       n_anchor, C);
    return check_launch("yolo_select_compact");
}

static inline bool classwise_mode_ok(int mode) {
    return mode == ADYOLO_CLASSWISE_SEDDOA || mode == ADYOLO_CLASSWISE_ACCDOA || mode == ADYOLO_CLASSWISE_ADPIT;
}

extern "C" long adyolo_classwise_select_workspace_words(long n_frames, int C, int mode) {
    if (n_frames <= 0 || C <= 0 || !classwise_mode_ok(mode)) return 0;
    return 2 * n_frames * C;
}

extern "C" int adyolo_classwise_select(const float *dec, float *ws, float *rows, int *frame_counts, long n_frames, int C,
                                       int mode, float conf_thresh, float unify_thresh, void *stream) {
    ADYOLO_REQUIRE(dec && ws && rows && frame_counts, ADYOLO_EINVAL, "classwise_select: null pointer");
    ADYOLO_REQUIRE(n_frames > 0 && C > 0, ADYOLO_EINVAL, "classwise_select: %ld frames x %d classes", n_frames, C);
    ADYOLO_REQUIRE(((uintptr_t)dec & 15) == 0, ADYOLO_EINVAL, "classwise_select: dec is not 16-byte aligned");
    ADYOLO_REQUIRE(classwise_mode_ok(mode), ADYOLO_ENOSUP, "classwise_select: unknown mode %d", mode);
    ADYOLO_REQUIRE(n_frames < (1L << 31) / (3L * C), ADYOLO_ENOSUP,
                   "classwise_select: %ld frames x %d classes x 3 rows do not fit 32-bit row counts", n_frames, C);
    int *count = reinterpret_cast<int *>(ws);
    int *offs = count + n_frames * C;
    hipStream_t st = as_stream(stream);
    if (mode == ADYOLO_CLASSWISE_ADPIT)
        return classwise_select_launch<ADYOLO_CLASSWISE_ADPIT>(dec, count, offs, rows, frame_counts, n_frames, C, conf_thresh,
                                                               unify_thresh, st);
    return classwise_select_launch<ADYOLO_CLASSWISE_SEDDOA>(dec, count, offs, rows, frame_counts, n_frames, C, conf_thresh,
                                                            unify_thresh, st);
}

extern "C" long adyolo_tta_merge_workspace_words(long n_frames, int C) {
    if (n_frames <= 0 || C <= 0) return 0;
    return 2 * n_frames * C + 2 * n_frames + 1;
}

static int tta_shape_ok(const char *who, long n_frames, int C, int n_views, int P) {
    ADYOLO_REQUIRE(n_frames > 0 && C > 0, ADYOLO_EINVAL, "%s: %ld frames x %d classes", who, n_frames, C);
    ADYOLO_REQUIRE(n_views >= 1 && n_views <= ADYOLO_TTA_MAX_VIEWS, ADYOLO_EINVAL, "%s: %d views, 1 to %d are taken", who,
                   n_views, ADYOLO_TTA_MAX_VIEWS);
    ADYOLO_REQUIRE(P >= 1 && P <= ADYOLO_SELECT_MAX_N, ADYOLO_EINVAL, "%s: %d rows per view and frame, 1 to %d are taken", who, P,
                   ADYOLO_SELECT_MAX_N);
    ADYOLO_REQUIRE(n_frames * C < (1L << 31) && n_frames * n_views * P < (1L << 31), ADYOLO_ENOSUP,
                   "%s: %ld frames x %d classes, %d views x %d rows do not fit 32-bit row counts", who, n_frames, C, n_views, P);
    return 0;
}

extern "C" int adyolo_tta_collect(const float *rows, long n_rows, const int *frame_counts, float *ws, float *pool,
                                  int *pool_counts, int *status, long n_frames, int C, int n_views, int view, int P,
                                  unsigned matrix, void *stream) {
    ADYOLO_REQUIRE(rows && frame_counts && ws && pool && pool_counts && status && n_rows >= 0, ADYOLO_EINVAL,
                   "tta_collect: null pointer");
    int rc = tta_shape_ok("tta_collect", n_frames, C, n_views, P);
    if (rc) return rc;
    ADYOLO_REQUIRE(view >= 0 && view < n_views, ADYOLO_EINVAL, "tta_collect: view %d of %d", view, n_views);
    ADYOLO_REQUIRE(tta_matrix_ok(matrix), ADYOLO_EINVAL, "tta_collect: 0x%x is no signed permutation of the axes", matrix);
    ADYOLO_REQUIRE(((uintptr_t)pool & 15) == 0, ADYOLO_EINVAL, "tta_collect: pool is not 16-byte aligned");
    // the tail of the merge workspace: the exclusive scan of the frame counts, and the copy of them the scan also writes
    int *offs = reinterpret_cast<int *>(ws) + 2 * n_frames * C;
    int *copy = offs + n_frames;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, frame_counts, offs, copy, n_frames, 1);
    rc = check_launch("tta_collect_scan");
    if (rc) return rc;
    hipLaunchKernelGGL(tta_collect_kernel, dim3(cdiv(n_frames * P, 256)), dim3(256), 0, st, rows, n_rows, frame_counts, offs,
                       reinterpret_cast<f32x4 *>(pool) + (size_t)view * n_frames * P, pool_counts + (size_t)view * n_frames,
                       n_frames, P, C, (uint32_t)matrix, status);
    return check_launch("tta_collect");
}

extern "C" int adyolo_tta_merge(const float *pool, const int *pool_counts, float *ws, float *rows, long capacity,
                                int *frame_counts, int *status, long n_frames, int C, int n_views, int P, float cos_t,
                                int min_views, void *stream) {
    ADYOLO_REQUIRE(pool && pool_counts && ws && rows && frame_counts && status, ADYOLO_EINVAL, "tta_merge: null pointer");
    int rc = tta_shape_ok("tta_merge", n_frames, C, n_views, P);
    if (rc) return rc;
    ADYOLO_REQUIRE(min_views >= 1 && min_views <= n_views, ADYOLO_EINVAL, "tta_merge: min_views %d with %d views", min_views,
                   n_views);
    ADYOLO_REQUIRE(((uintptr_t)pool & 15) == 0, ADYOLO_EINVAL, "tta_merge: pool is not 16-byte aligned");
    // a kept cluster has rows of min_views views, so a frame gives at most V * P / min_views of them
    const long per_frame = (long)n_views * P / min_views;
    ADYOLO_REQUIRE(capacity >= n_frames * per_frame, ADYOLO_EINVAL, "tta_merge: %ld rows of capacity, %ld frames x %ld are needed",
                   capacity, n_frames, per_frame);
    const long n_slots = n_frames * C;
    int *count = reinterpret_cast<int *>(ws);
    int *offs = count + n_slots;
    const long most = (long)n_views * P < ADYOLO_SELECT_MAX_N ? (long)n_views * P : ADYOLO_SELECT_MAX_N;
    const int kmax = (int)((most + SEL_WAVE - 1) / SEL_WAVE * SEL_WAVE);
    const size_t lds = (size_t)7 * kmax * sizeof(float);
    const f32x4 *pl = reinterpret_cast<const f32x4 *>(pool);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(tta_merge_kernel<false>, dim3((unsigned)n_slots), dim3(SEL_WAVE), lds, st, pl, pool_counts, count, offs,
                       rows, n_frames, C, n_views, P, kmax, cos_t, min_views, status);
    rc = check_launch("tta_merge_count");
    if (rc) return rc;
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, count, offs, frame_counts, n_frames, C);
    rc = check_launch("tta_merge_scan");
    if (rc) return rc;
    hipLaunchKernelGGL(tta_merge_kernel<true>, dim3((unsigned)n_slots), dim3(SEL_WAVE), lds, st, pl, pool_counts, count, offs,
                       rows, n_frames, C, n_views, P, kmax, cos_t, min_views, status);
    return check_launch("tta_merge_write");
}
