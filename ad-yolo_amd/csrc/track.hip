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
// The carried form, adyolo_track_run (postprocess.track_run on the device), links one run of a stream of recordings -- a pass of
// a windowed evaluation -- and carries the state to the next call: track_run_plan_kernel first (the carry copied, the segment
// table checked, the emitted window), then the same bin, the link as track_link_run_kernel with one wave per (segment, class),
// and the emit over the emitted frames only.  Both link kernels are one text, track_link.hpp, compiled twice.  What makes it
// exact: a fill reaches max_gap frames back and an erasure (min_len - 1) * (max_gap + 1) + 1, so a recording's frames further
// back than the hold are final and can be emitted.
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

// The carry of the carried form (adyolo_track_run), all of one recording that goes on in the next run, per class so that a
// class's wave reads and writes words of its own only:
//   head  [C][4] int        {next_id, walked: the recording's frames walked so far, held = min(hold, walked), 0}
//   slot  [C][8][8]         {occupied, id, first, last (on the recording's own frame axis), hits, s.x, s.y, s.z}
//   cells [hold][C][8] f32x4  the held frames' cells, the last frame walked at hold - 1 (the first hold - held are not read)
constexpr int TRK_HEAD_WORDS = 4, TRK_SLOT_WORDS = 8, TRK_WIN_WORDS = 4;
__host__ __device__ inline long trk_carry_words(int C, int hold) {
    return (long)C * (TRK_HEAD_WORDS + TRK_SLOTS * TRK_SLOT_WORDS) + (long)hold * C * TRK_SLOTS * 4;
}

#define TRK_CARRY 0
#include "track_link.hpp"
#undef TRK_CARRY
#define TRK_CARRY 1
#include "track_link.hpp"
#undef TRK_CARRY

// The carried form's first kernel, one block: the carry is copied to `snap` (the link kernel reads the copy and writes the
// carry, so a run whose first segment continues and whose last is open needs no second buffer), the segment table and -- when
// row 0 continues -- the carry's heads are checked, and win = {the grid frame the emitted frames start at, their number, 1 (0:
// refused, ADYOLO_TRACK_BAD_ROWS, nothing is linked or emitted), 0}; the number also goes to n_emit [0].
__global__ __launch_bounds__(TRK_SCAN_THREADS) void track_run_plan_kernel(const int *__restrict__ segs, int S, long run_frames,
                                                                          int C, int hold, const float *__restrict__ carry,
                                                                          float *__restrict__ snap, int *__restrict__ win,
                                                                          int *__restrict__ n_emit, int *__restrict__ status) {
    __shared__ int bad;
    const int t = threadIdx.x;
    if (t == 0) bad = 0;
    const long words = trk_carry_words(C, hold);
    for (long i = t; i < words; i += TRK_SCAN_THREADS) snap[i] = carry[i];
    __syncthreads();
    bool b = false;
    for (int s = t; s < S; s += TRK_SCAN_THREADS) {
        const long r0 = segs[4 * s], n = segs[4 * s + 1], cont = segs[4 * s + 2], open = segs[4 * s + 3];
        const long before = s ? (long)segs[4 * s - 4] + segs[4 * s - 3] : 0;
        b |= r0 != before || n < 1 || r0 < 0 || r0 + n > run_frames || (s == S - 1 && r0 + n != run_frames) ||
             (cont != 0 && (cont != 1 || s != 0)) || (open != 0 && (open != 1 || s != S - 1));
    }
    const int *head = reinterpret_cast<const int *>(snap);
    const bool cont = segs[2] == 1;
    if (cont)
        for (int c = t; c < C; c += TRK_SCAN_THREADS) {
            const int next_id = head[4 * c], walked = head[4 * c + 1], held = head[4 * c + 2];
            b |= next_id < 0 || walked < 0 || walked > (1 << 30) || held != (walked < hold ? walked : hold) || walked != head[1];
        }
    if (b) atomicOr(&bad, 1);
    __syncthreads();
    if (t == 0) {
        if (bad) {
            win[0] = hold, win[1] = 0, win[2] = 0, win[3] = 0;
            n_emit[0] = 0;
            atomicOr(status, ADYOLO_TRACK_BAD_ROWS);
        } else {
            const int held_in = cont ? head[2] : 0;
            const long walked = (S == 1 && cont ? (long)head[1] : 0L) + segs[4 * (S - 1) + 1];
            const int held_out = segs[4 * (S - 1) + 3] ? (int)(walked < hold ? walked : hold) : 0;
            win[0] = hold - held_in, win[1] = (int)(held_in + run_frames - held_out), win[2] = 1, win[3] = 0;
            n_emit[0] = win[1];
        }
    }
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

// The carried form's emit (track_emit_kernel's frame loop with the frame's place and number given): one frame's cells `src`
// [C][8], by one wave.  WRITE = false: -> the number of valid ones; WRITE = true: they go to rows / ids
// from row at0 on, classes ascending, slots ascending, with `frame` in the frame column.
template <bool WRITE>
__device__ __forceinline__ int trk_emit_frame(const f32x4 *__restrict__ src, long at0, long frame, int n_cells,
                                              float *__restrict__ rows, int *__restrict__ ids) {
    const int lane = threadIdx.x;
    int run = 0;
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
    return run;
}

// The carried form: emitted frame e is grid frame win[0] + e for e < win[1]; the frames behind them (n_out = hold + run_frames
// in all) count no cell.
template <bool WRITE>
__global__ __launch_bounds__(TRK_WAVE) void track_emit_run_kernel(const f32x4 *__restrict__ grid, int *__restrict__ cell_count,
                                                                 const int *__restrict__ cell_offs, float *__restrict__ rows,
                                                                 int *__restrict__ ids, long n_out, int C,
                                                                 const int *__restrict__ win) {
    const int n_cells = C * TRK_SLOTS;
    const long lo = win[0], n_emit = win[1];
    for (long e = blockIdx.x; e < n_out; e += gridDim.x) {
        int run = 0;
        if (e < n_emit) run = trk_emit_frame<WRITE>(grid + (size_t)(lo + e) * n_cells, WRITE ? cell_offs[e] : 0, e, n_cells, rows, ids);
        if (!WRITE && threadIdx.x == 0) cell_count[e] = run;
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

extern "C" long adyolo_track_carry_words(int C, int hold) {
    if (C <= 0 || hold < 0) return 0;
    return trk_carry_words(C, hold);
}

extern "C" long adyolo_track_run_workspace_words(long run_frames, int C, int hold) {
    if (run_frames <= 0 || C <= 0 || hold < 0) return 0;
    const long n_out = run_frames + hold;
    return n_out * C * 4L * TRK_SLOTS + trk_carry_words(C, hold) + run_frames * C * (TRK_CAND_WORDS + 1) + run_frames + 2 * n_out +
           TRK_WIN_WORDS;
}

extern "C" int adyolo_track_run(const float *rows, long n_rows, const int *frame_counts, long run_frames, const int *segments,
                                long n_segments, int C, float cos_gate, int max_gap, int min_len, float a, float b, int hold,
                                float *carry, float *ws, float *out_rows, int *out_ids, long capacity, int *out_counts,
                                int *status, void *stream) {
    ADYOLO_REQUIRE(rows && frame_counts && segments && carry && ws && out_rows && out_ids && out_counts && status, ADYOLO_EINVAL,
                   "track_run: null pointer");
    ADYOLO_REQUIRE((((uintptr_t)rows | (uintptr_t)frame_counts | (uintptr_t)segments | (uintptr_t)out_rows | (uintptr_t)out_ids |
                     (uintptr_t)out_counts | (uintptr_t)status) & 3) == 0 && (((uintptr_t)ws | (uintptr_t)carry) & 15) == 0,
                   ADYOLO_EINVAL, "track_run: a pointer is not 4-byte aligned, or ws or carry not 16-byte aligned");
    ADYOLO_REQUIRE(n_rows >= 0 && run_frames >= 1 && C >= 1 && n_segments >= 1 && n_segments <= run_frames, ADYOLO_EINVAL,
                   "track_run: %ld rows, %ld frames x %d classes in %ld segments", n_rows, run_frames, C, n_segments);
    ADYOLO_REQUIRE(max_gap >= 0 && min_len >= 1, ADYOLO_EINVAL, "track_run: max_gap %d, min_len %d", max_gap, min_len);
    ADYOLO_REQUIRE(cos_gate > 0.f && cos_gate < 1.f, ADYOLO_EINVAL, "track_run: cos_gate %g outside (0, 1)", (double)cos_gate);
    ADYOLO_REQUIRE(a > 0.f && a <= 1.f, ADYOLO_EINVAL, "track_run: smoothing weight %g outside (0, 1]", (double)a);
    // what a write can reach back: a fill max_gap frames, the erasure of a track of min_len - 1 hits (postprocess.track_hold)
    const long reach = min_len == 1 ? (long)max_gap : ((long)min_len - 1) * ((long)max_gap + 1) + 1;
    ADYOLO_REQUIRE(hold >= reach, ADYOLO_EINVAL, "track_run: a hold of %d frames, max_gap %d and min_len %d reach back %ld", hold,
                   max_gap, min_len, reach);
    const long n_out = run_frames + hold;
    ADYOLO_REQUIRE(n_out < (1L << 31) / ((long)C * TRK_SLOTS) && n_rows < (1L << 31) && n_segments < (1L << 31) / C, ADYOLO_ENOSUP,
                   "track_run: %ld frames x %d classes x %d tracks or %ld rows do not fit 32-bit row counts", n_out, C, TRK_SLOTS,
                   n_rows);
    ADYOLO_REQUIRE(capacity >= n_out * C * TRK_SLOTS, ADYOLO_EINVAL, "track_run: %ld rows of capacity, %ld are needed", capacity,
                   n_out * C * TRK_SLOTS);
    const long n_slots = run_frames * C;
    f32x4 *grid = reinterpret_cast<f32x4 *>(ws);
    float *snap = ws + (size_t)n_out * C * 4 * TRK_SLOTS;
    float *cand = snap + trk_carry_words(C, hold);
    int *ncand = reinterpret_cast<int *>(cand + (size_t)n_slots * TRK_CAND_WORDS);
    int *in_offs = ncand + n_slots;
    int *cell_count = in_offs + run_frames;
    int *cell_offs = cell_count + n_out;
    int *win = cell_offs + n_out;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(track_run_plan_kernel, dim3(1), dim3(TRK_SCAN_THREADS), 0, st, segments, (int)n_segments, run_frames, C, hold,
                       carry, snap, win, out_counts + n_out + 1, status);
    int rc = check_launch("track_run_plan");
    if (rc) return rc;
    hipLaunchKernelGGL(track_scan_kernel<true>, dim3(1), dim3(TRK_SCAN_THREADS), 0, st, frame_counts, in_offs,
                       static_cast<int *>(nullptr), run_frames, n_rows, status);
    rc = check_launch("track_scan_rows");
    if (rc) return rc;
    hipLaunchKernelGGL(track_bin_kernel, dim3((unsigned)n_slots), dim3(TRK_WAVE), 0, st, rows, frame_counts, in_offs, cand, ncand,
                       run_frames, C, status);
    rc = check_launch("track_bin");
    if (rc) return rc;
    hipLaunchKernelGGL(track_link_run_kernel, dim3((unsigned)(n_segments * C)), dim3(TRK_WAVE), 0, st, cand, ncand, grid, run_frames,
                       C, cos_gate, max_gap, min_len, a, b, status, segments, win, snap, carry, hold);
    rc = check_launch("track_link_run");
    if (rc) return rc;
    const dim3 eg((unsigned)(n_out < 65536 ? n_out : 65536));
    hipLaunchKernelGGL(track_emit_run_kernel<false>, eg, dim3(TRK_WAVE), 0, st, grid, cell_count, cell_offs, out_rows, out_ids,
                       n_out, C, win);
    rc = check_launch("track_emit_count");
    if (rc) return rc;
    hipLaunchKernelGGL(track_scan_kernel<false>, dim3(1), dim3(TRK_SCAN_THREADS), 0, st, cell_count, cell_offs, out_counts, n_out,
                       0L, status);
    rc = check_launch("track_emit_scan");
    if (rc) return rc;
    hipLaunchKernelGGL(track_emit_run_kernel<true>, eg, dim3(TRK_WAVE), 0, st, grid, cell_count, cell_offs, out_rows, out_ids,
                       n_out, C, win);
    return check_launch("track_emit_write");
}
