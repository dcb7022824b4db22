// Tracks: postprocess.track_rows on the device.  The rows a selection (or the test-time-augmentation merge) left, frame by
// frame, are linked per (clip, class) into tracks across frames: directions smoothed, short gaps filled, short tracks dropped,
// tracks numbered.  The result has the selection's own layout, so the scorer and the CSV writer take it unchanged.
//
// A sequential recurrence per (clip, class) -- nothing like the per-(frame, class) kernels of select.hip -- in three stages on
// one stream, no host read between them:
//   bin   track_scan_kernel (the rows' offsets from the frame counts, validated) and track_bin_kernel, one wave per (frame,
//         class): the class's rows in row order, the first ADYOLO_TRACK_MAX_DET of them, normalised, into a candidate list
//         [frame][class][3][64] with its length in ncand [class][frame].
//   link  track_link_kernel, one wave per (clip, class), walks the clip's frames in order.  Lane k < 8 holds slot k's track
//         {id, s, first, last, hits}; lane j holds candidate j.  The candidates do not depend on the state, so they are
//         fetched ahead of the recurrence: the lengths 64 frames at a time (one load per lane), the vectors one frame ahead;
//         a block of 64 frames without a candidate, entered with no track open, is cleared by all lanes and stepped over.
//         Every greedy round is one wave arg-max over the 8 x 64 dots (ties: lowest slot, then lowest candidate).  Lane k
//         writes slot k's cell {x, y, z, id} of EVERY frame into a dense grid [frame][class][8] (id -1: empty), the gap fills
//         behind it, and the erasure of a track that closes short: one lane writes all of a slot's cells, so their order is
//         program order, and the caller initialises nothing.
//   emit  track_emit_kernel<false> counts the valid cells per frame, track_scan_kernel turns the counts into offsets, and
//         track_emit_kernel<true> compacts the cells into rows [frame, class, x, y, z] and ids; grid order is output order.
// Every float operation is a correctly rounded float32 one in the host's order without contraction (the division and the
// square root as adyolo_tta_merge writes them): rows, counts, ids and status are the host's bit for bit.
#include "common.hpp"

namespace adyolo {

constexpr int TRK_WAVE = 64;
constexpr int TRK_SLOTS = ADYOLO_TRACK_SLOTS;
constexpr int TRK_DET = ADYOLO_TRACK_MAX_DET;
constexpr int TRK_CAND_WORDS = 3 * TRK_DET;                     // per (frame, class): x[64], y[64], z[64]
constexpr int TRK_SCAN_THREADS = 1024;
static_assert(TRK_DET == TRK_WAVE, "lane j holds candidate j");
static_assert(TRK_SLOTS == 8, "the arg-max key packs the slot into 3 bits");

__device__ __forceinline__ unsigned long long trk_below(int lane) { return (1ull << lane) - 1ull; }

// count [n] -> offs [n] (exclusive scan, sums in 64 bits).  IN = true, the selection's frame counts: a frame whose count is
// negative or whose rows would start before row 0 or end past n_rows gets offs = -1 (it has no rows) and sets
// ADYOLO_TRACK_BAD_ROWS.  IN = false, the emitted counts: they are also copied to totals [n], the sum to totals [n].
template <bool IN>
__global__ __launch_bounds__(TRK_SCAN_THREADS) void track_scan_kernel(const int *__restrict__ count, int *__restrict__ offs,
                                                                      int *__restrict__ totals, long n, long n_rows,
                                                                      int *__restrict__ status) {
    __shared__ long part[TRK_SCAN_THREADS];
    const int t = threadIdx.x;
    const long chunk = (n + TRK_SCAN_THREADS - 1) / TRK_SCAN_THREADS;
    const long s0 = t * chunk < n ? t * chunk : n, s1 = s0 + chunk < n ? s0 + chunk : n;
    long sum = 0;
    for (long s = s0; s < s1; ++s) sum += count[s];
    part[t] = sum;
    __syncthreads();
    for (int o = 1; o < TRK_SCAN_THREADS; o <<= 1) {             // inclusive Hillis-Steele scan of the chunk sums
        const long v = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    long run = part[t] - sum;
    bool bad = false;
    for (long s = s0; s < s1; ++s) {
        const int c = count[s];
        if (IN) {
            const bool b = c < 0 || run < 0 || run + c > n_rows;
            offs[s] = b ? -1 : (int)run;
            bad |= b;
        } else {
            offs[s] = (int)run;
            totals[s] = c;
        }
        run += c;
    }
    if (IN && bad) atomicOr(status, ADYOLO_TRACK_BAD_ROWS);
    if (!IN && t == TRK_SCAN_THREADS - 1) totals[n] = (int)part[t];
}

// grid: one wave per (frame, class).  cand [slot][3][64], ncand [class][frame]
__global__ __launch_bounds__(TRK_WAVE) void track_bin_kernel(const float *__restrict__ rows, const int *__restrict__ counts,
                                                            const int *__restrict__ offs, float *__restrict__ cand,
                                                            int *__restrict__ ncand, long n_frames, int C,
                                                            int *__restrict__ status) {
#pragma clang fp contract(off)
    const long slot = blockIdx.x;
    const long frame = slot / C;
    const int cls = (int)(slot - frame * C);
    const int lane = threadIdx.x;
    const int off = offs[frame];
    const int cnt = off < 0 ? 0 : counts[frame];
    float *dst = cand + (size_t)slot * TRK_CAND_WORDS;
    int raw = 0, K = 0, bits = 0;
    for (int i0 = 0; i0 < cnt; i0 += TRK_WAVE) {
        if (cls != 0 && raw > TRK_DET) break;                    // (class 0's wave reads on: it checks every row's class)
        const int i = i0 + lane;
        bool mine = false;
        float x = 0.f, y = 0.f, z = 0.f;
        if (i < cnt) {
            const float *r = rows + (size_t)(off + i) * 5;
            const float c = r[1];
            if (cls == 0 && !(c >= 0.f && c < (float)C && c == floorf(c))) bits |= ADYOLO_TRACK_BAD_ROWS;
            mine = c == (float)cls;
            if (mine) x = r[2], y = r[3], z = r[4];
        }
        const unsigned long long bm = __ballot(mine);
        const bool taken = mine && raw + __popcll(bm & trk_below(lane)) < TRK_DET;   // the first 64 rows of the class
        const float nrm = sqrtf((x * x + y * y) + z * z);
        const bool good = taken && nrm > 0.f && nrm < INFINITY;   // a zero, infinite or NaN norm: dropped and reported
        if (taken && !good) bits |= ADYOLO_TRACK_BAD_VECTOR;
        const unsigned long long bg = __ballot(good);
        if (good) {
            const int at = K + __popcll(bg & trk_below(lane));
            dst[at] = x / nrm;
            dst[TRK_DET + at] = y / nrm;
            dst[2 * TRK_DET + at] = z / nrm;
        }
        raw += __popcll(bm);
        K += __popcll(bg);
    }
    if (raw > TRK_DET) bits |= ADYOLO_TRACK_DET_OVERFLOW;
    int all = 0;
    for (int b = 1; b <= ADYOLO_TRACK_BAD_ROWS; b <<= 1)
        if (__ballot(bits & b)) all |= b;
    if (lane == 0) {
        ncand[(size_t)cls * n_frames + frame] = K;
        if (all) atomicOr(status, all);
    }
}

// The recurrence waits on its cross-lane steps, so they stay in the vector unit instead of crossing the LDS network:
// a wave-uniform lane is read with v_readlane, and the arg-max reduces with DPP moves.
__device__ __forceinline__ int trk_lane(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float trk_lane(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// old = 0 is the identity: a lane whose DPP source does not exist, or whose row is masked off, keeps its value
template <int CTRL, int ROWS>
__device__ __forceinline__ unsigned trk_max_dpp(unsigned v) {
    const unsigned w = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xf, false);
    return w > v ? w : v;
}

// the maximum over the wave, in every lane (all 64 lanes active): the running maximum along each row of 16 lanes
// (row_shr 1, 2, 4, 8), lane 15 of rows 0 and 2 into rows 1 and 3 (row_bcast 15), lane 31 into rows 2 and 3 (row_bcast 31);
// lane 63 then holds it
__device__ __forceinline__ unsigned trk_wave_max(unsigned v) {
    v = trk_max_dpp<0x111, 0xf>(v);
    v = trk_max_dpp<0x112, 0xf>(v);
    v = trk_max_dpp<0x114, 0xf>(v);
    v = trk_max_dpp<0x118, 0xf>(v);
    v = trk_max_dpp<0x142, 0xa>(v);
    v = trk_max_dpp<0x143, 0xc>(v);
    return (unsigned)trk_lane((int)v, 63);
}

__device__ __forceinline__ f32x4 trk_cell(float x, float y, float z, int id) {
    f32x4 v;
    v[0] = x, v[1] = y, v[2] = z, v[3] = __int_as_float(id);
    return v;
}

// grid: one wave per (clip, class)
__global__ __launch_bounds__(TRK_WAVE) void track_link_kernel(const float *__restrict__ cand, const int *__restrict__ ncand,
                                                             f32x4 *__restrict__ grid, long n_frames, int t_clip, int C,
                                                             float cos_g, int max_gap, int min_len, float a, float b,
                                                             int *__restrict__ status) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    const long clip = blockIdx.x / C;
    const int c = (int)(blockIdx.x - clip * C);
    const long f0 = clip * t_clip;
    const int *nc = ncand + (size_t)c * n_frames + f0;
    const float *cd = cand + ((size_t)f0 * C + c) * TRK_CAND_WORDS;           // frame t: + t * C * TRK_CAND_WORDS
    f32x4 *cells = grid + ((size_t)f0 * C + c) * TRK_SLOTS + (lane & (TRK_SLOTS - 1));   // frame t: + t * C * TRK_SLOTS
    const size_t cand_step = (size_t)C * TRK_CAND_WORDS, cell_step = (size_t)C * TRK_SLOTS;
    const f32x4 empty = trk_cell(0.f, 0.f, 0.f, -1);
    // slot k's track, in lane k
    bool occ = false;
    int id = 0, first = 0, last = 0, hits = 0;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    int next_id = 0, bits = 0;
    // the candidates fetched ahead: the lengths of this block of 64 frames and of the next, the vectors of the next frame
    int len_blk = 0, len_nxt = lane < t_clip ? nc[lane] : 0;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (lane < trk_lane(len_nxt, 0)) px = cd[lane], py = cd[TRK_DET + lane], pz = cd[2 * TRK_DET + lane];
    for (int t = 0; t < t_clip; ++t) {
        if ((t & (TRK_WAVE - 1)) == 0) {
            len_blk = len_nxt;
            len_nxt = t + TRK_WAVE + lane < t_clip ? nc[t + TRK_WAVE + lane] : 0;
            if (__ballot(len_blk != 0) == 0 && __ballot(occ) == 0) {
                // silence: nothing arrives in these 64 frames and nothing is open.  All lanes clear the block's cells (no
                // later write reaches back into it) and the walk goes on behind it, the first frame there fetched
#pragma unroll
                for (int i = 0; i < TRK_WAVE / TRK_SLOTS; ++i) {
                    const int f = t + (lane >> 3) + TRK_SLOTS * i;
                    if (f < t_clip) cells[(size_t)f * cell_step] = empty;
                }
                const int t1 = t + TRK_WAVE;
                if (t1 < t_clip && lane < trk_lane(len_nxt, 0)) {
                    const float *p = cd + (size_t)t1 * cand_step;
                    px = p[lane], py = p[TRK_DET + lane], pz = p[2 * TRK_DET + lane];
                }
                t += TRK_WAVE - 1;
                continue;
            }
        }
        const int n = trk_lane(len_blk, t & (TRK_WAVE - 1));
        const float ux = px, uy = py, uz = pz;
        const int t1 = t + 1;
        const int n1 = t1 >= t_clip ? 0 : (t1 & (TRK_WAVE - 1)) ? trk_lane(len_blk, t1 & (TRK_WAVE - 1)) : trk_lane(len_nxt, 0);
        if (lane < n1) {
            const float *p = cd + (size_t)t1 * cand_step;
            px = p[lane], py = p[TRK_DET + lane], pz = p[2 * TRK_DET + lane];
        }
        f32x4 *cell = cells + (size_t)t * cell_step;
        if (n == 0 && __ballot(occ) == 0) {                      // nothing arrives and nothing is open
            if (lane < TRK_SLOTS) *cell = empty;
            continue;
        }
        // 2. expire
        if (occ && t - last - 1 > max_gap) {
            if (hits < min_len)
                for (int f = first; f <= last; ++f) cells[(size_t)f * cell_step] = empty;
            occ = false;
        }
        bool hit = false;
        unsigned long long cand_free = n >= TRK_WAVE ? ~0ull : trk_below(n);
        const unsigned occ_mask = (unsigned)__ballot(occ);
        if (n > 0 && occ_mask) {
            // 3. associate: the eligible dots of candidate `lane` with every slot, as ordered keys (dot > cos_g > 0)
            unsigned key[TRK_SLOTS];
#pragma unroll
            for (int k = 0; k < TRK_SLOTS; ++k) {
                const float kx = trk_lane(sx, k), ky = trk_lane(sy, k), kz = trk_lane(sz, k);
                const float d = (kx * ux + ky * uy) + kz * uz;
                key[k] = (lane < n && ((occ_mask >> k) & 1u) && d > cos_g) ? __float_as_uint(d) : 0u;
            }
            for (;;) {
                unsigned bv = 0;
                int bk = 0;
#pragma unroll
                for (int k = 0; k < TRK_SLOTS; ++k)
                    if (key[k] > bv) bv = key[k], bk = k;        // strictly larger: the lowest slot keeps a tie
                const unsigned m = trk_wave_max(bv);
                if (m == 0) break;
                const unsigned who = trk_wave_max(bv == m ? (((unsigned)(TRK_SLOTS - 1 - bk) << 6) | (unsigned)(63 - lane)) + 1u : 0u) - 1u;
                const int ks = TRK_SLOTS - 1 - (int)(who >> 6), js = 63 - (int)(who & 63u);
#pragma unroll
                for (int k = 0; k < TRK_SLOTS; ++k)
                    if (k == ks || lane == js) key[k] = 0u;
                cand_free &= ~(1ull << js);
                // 4. update slot ks with candidate js (every lane forms m; lane ks keeps it)
                const float kx = trk_lane(sx, ks), ky = trk_lane(sy, ks), kz = trk_lane(sz, ks);
                const float vx = trk_lane(ux, js), vy = trk_lane(uy, js), vz = trk_lane(uz, js);
                float mx = (kx * b) + (vx * a), my = (ky * b) + (vy * a), mz = (kz * b) + (vz * a);
                const float nrm = sqrtf((mx * mx + my * my) + mz * mz);
                mx = mx / nrm, my = my / nrm, mz = mz / nrm;
                if (lane == ks) {
                    const int gap = t - last - 1;
                    for (int g = 1; g <= gap; ++g) {
                        const float w = (float)g / (float)(gap + 1);
                        const float w1 = 1.f - w;
                        const float gx = (sx * w1) + (mx * w), gy = (sy * w1) + (my * w), gz = (sz * w1) + (mz * w);
                        const float gn = sqrtf((gx * gx + gy * gy) + gz * gz);
                        cells[(size_t)(last + g) * cell_step] = trk_cell(gx / gn, gy / gn, gz / gn, id);
                    }
                    sx = mx, sy = my, sz = mz;
                    last = t;
                    ++hits;
                    hit = true;
                }
            }
        }
        // 5. open: the r-th unmatched candidate takes the r-th empty slot
        if (cand_free) {
            const unsigned free_slots = ~(unsigned)__ballot(occ) & ((1u << TRK_SLOTS) - 1u);
            const int n_new = __popcll(cand_free), n_free = __popc(free_slots);
            if (n_new > n_free) bits |= ADYOLO_TRACK_SLOT_OVERFLOW;
            const int n_open = n_new < n_free ? n_new : n_free;
            const int r = __popc(free_slots & ((1u << (lane & 31)) - 1u));
            const bool opens = lane < TRK_SLOTS && !occ && r < n_open;
            unsigned long long rest = cand_free;
            for (int i = 0; i < TRK_SLOTS - 1; ++i)
                if (i < r && opens) rest &= rest - 1ull;
            const int j = opens ? (int)__builtin_ctzll(rest) : 0;
            const float vx = __shfl(ux, j), vy = __shfl(uy, j), vz = __shfl(uz, j);
            if (opens) {
                occ = true;
                id = next_id + r;
                sx = vx, sy = vy, sz = vz;
                first = last = t;
                hits = 1;
                hit = true;
            }
            next_id += n_open;
        }
        if (lane < TRK_SLOTS) *cell = hit ? trk_cell(sx, sy, sz, id) : empty;
    }
    // the clip's end closes every slot
    if (occ && hits < min_len)
        for (int f = first; f <= last; ++f) cells[(size_t)f * cell_step] = empty;
    if (__ballot(bits != 0) && lane == 0) atomicOr(status, ADYOLO_TRACK_SLOT_OVERFLOW);
}

// grid: one wave per frame.  WRITE = false: cell_count[frame] = its valid cells; WRITE = true: they go to rows / ids at
// cell_offs[frame], classes ascending, slots ascending.
template <bool WRITE>
__global__ __launch_bounds__(TRK_WAVE) void track_emit_kernel(const f32x4 *__restrict__ grid, int *__restrict__ cell_count,
                                                             const int *__restrict__ cell_offs, float *__restrict__ rows,
                                                             int *__restrict__ ids, long n_frames, int C) {
    const int lane = threadIdx.x;
    const int n_cells = C * TRK_SLOTS;
    for (long frame = blockIdx.x; frame < n_frames; frame += gridDim.x) {
        const f32x4 *src = grid + (size_t)frame * n_cells;
        int run = 0;
        const long at0 = WRITE ? cell_offs[frame] : 0;
        for (int i0 = 0; i0 < n_cells; i0 += TRK_WAVE) {
            const int i = i0 + lane;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            bool valid = false;
            if (i < n_cells) {
                v = src[i];
                valid = __float_as_int(v[3]) >= 0;
            }
            const unsigned long long bm = __ballot(valid);
            if (WRITE && valid) {
                const long at = at0 + run + __popcll(bm & trk_below(lane));
                float *d = rows + (size_t)at * 5;
                d[0] = (float)frame, d[1] = (float)(i / TRK_SLOTS), d[2] = v[0], d[3] = v[1], d[4] = v[2];
                ids[at] = __float_as_int(v[3]);
            }
            run += __popcll(bm);
        }
        if (!WRITE && lane == 0) cell_count[frame] = run;
    }
}

}  // namespace adyolo

using namespace adyolo;

extern "C" long adyolo_track_workspace_words(long n_frames, int C) {
    if (n_frames <= 0 || C <= 0) return 0;
    return n_frames * C * (4L * TRK_SLOTS + TRK_CAND_WORDS + 1) + 3 * n_frames;
}

extern "C" int adyolo_track_rows(const float *rows, long n_rows, const int *frame_counts, long n_clips, int t_clip, int C,
                                 float cos_gate, int max_gap, int min_len, float a, float b, float *ws, float *out_rows,
                                 int *out_ids, long capacity, int *out_counts, int *status, void *stream) {
    ADYOLO_REQUIRE(rows && frame_counts && ws && out_rows && out_ids && out_counts && status, ADYOLO_EINVAL,
                   "track_rows: null pointer");
    ADYOLO_REQUIRE((((uintptr_t)rows | (uintptr_t)frame_counts | (uintptr_t)out_rows | (uintptr_t)out_ids |
                     (uintptr_t)out_counts | (uintptr_t)status) & 3) == 0 && ((uintptr_t)ws & 15) == 0, ADYOLO_EINVAL,
                   "track_rows: a pointer is not 4-byte aligned, or ws not 16-byte aligned");
    ADYOLO_REQUIRE(n_rows >= 0 && n_clips >= 1 && t_clip >= 1 && C >= 1, ADYOLO_EINVAL,
                   "track_rows: %ld rows, %ld clips x %d frames x %d classes", n_rows, n_clips, t_clip, C);
    ADYOLO_REQUIRE(max_gap >= 0 && min_len >= 1, ADYOLO_EINVAL, "track_rows: max_gap %d, min_len %d", max_gap, min_len);
    ADYOLO_REQUIRE(cos_gate > 0.f && cos_gate < 1.f, ADYOLO_EINVAL, "track_rows: cos_gate %g outside (0, 1)", (double)cos_gate);
    ADYOLO_REQUIRE(a > 0.f && a <= 1.f, ADYOLO_EINVAL, "track_rows: smoothing weight %g outside (0, 1]", (double)a);
    ADYOLO_REQUIRE(n_clips < (1L << 31) / t_clip, ADYOLO_ENOSUP, "track_rows: %ld clips x %d frames", n_clips, t_clip);
    const long n_frames = n_clips * t_clip;
    ADYOLO_REQUIRE(n_frames < (1L << 31) / ((long)C * TRK_SLOTS) && n_rows < (1L << 31), ADYOLO_ENOSUP,
                   "track_rows: %ld frames x %d classes x %d tracks or %ld rows do not fit 32-bit row counts", n_frames, C,
                   TRK_SLOTS, n_rows);
    const long n_slots = n_frames * C;
    ADYOLO_REQUIRE(capacity >= n_slots * TRK_SLOTS, ADYOLO_EINVAL, "track_rows: %ld rows of capacity, %ld are needed", capacity,
                   n_slots * TRK_SLOTS);
    f32x4 *grid = reinterpret_cast<f32x4 *>(ws);
    float *cand = ws + (size_t)n_slots * 4 * TRK_SLOTS;
    int *ncand = reinterpret_cast<int *>(cand + (size_t)n_slots * TRK_CAND_WORDS);
    int *in_offs = ncand + n_slots;
    int *cell_count = in_offs + n_frames;
    int *cell_offs = cell_count + n_frames;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(track_scan_kernel<true>, dim3(1), dim3(TRK_SCAN_THREADS), 0, st, frame_counts, in_offs,
                       static_cast<int *>(nullptr), n_frames, n_rows, status);
    int rc = check_launch("track_scan_rows");
    if (rc) return rc;
    hipLaunchKernelGGL(track_bin_kernel, dim3((unsigned)n_slots), dim3(TRK_WAVE), 0, st, rows, frame_counts, in_offs, cand, ncand,
                       n_frames, C, status);
    rc = check_launch("track_bin");
    if (rc) return rc;
    hipLaunchKernelGGL(track_link_kernel, dim3((unsigned)(n_clips * C)), dim3(TRK_WAVE), 0, st, cand, ncand, grid, n_frames, t_clip,
                       C, cos_gate, max_gap, min_len, a, b, status);
    rc = check_launch("track_link");
    if (rc) return rc;
    const dim3 eg((unsigned)(n_frames < 65536 ? n_frames : 65536));
    hipLaunchKernelGGL(track_emit_kernel<false>, eg, dim3(TRK_WAVE), 0, st, grid, cell_count, cell_offs, out_rows, out_ids,
                       n_frames, C);
    rc = check_launch("track_emit_count");
    if (rc) return rc;
    hipLaunchKernelGGL(track_scan_kernel<false>, dim3(1), dim3(TRK_SCAN_THREADS), 0, st, cell_count, cell_offs, out_counts,
                       n_frames, 0L, status);
    rc = check_launch("track_emit_scan");
    if (rc) return rc;
    hipLaunchKernelGGL(track_emit_kernel<true>, eg, dim3(TRK_WAVE), 0, st, grid, cell_count, cell_offs, out_rows, out_ids,
                       n_frames, C);
    return check_launch("track_emit_write");
}
