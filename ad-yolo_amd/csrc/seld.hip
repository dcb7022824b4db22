// SELD scoring on the GPU: the per-recording accumulators of seld_metrics.SELDScorer.update (DCASE location-sensitive
// detection and class-sensitive localisation over 1-second blocks, Hungarian track association) for rows selected on the
// device (adyolo_yolo_select) or uploaded from the host, against a reference table packed once per split.
//
// Four launches:
//   1. seld_scan_kernel (one workgroup): exclusive scan of the per-frame row counts -> row offsets; checks them against the
//      row capacity.
//   2. seld_block_kernel, one wave per (clip, block, class): the per-frame maxima n_ref / n_pred, then for every frame of
//      the block with events on both sides the assignment of lsap.hpp (scipy's, ties included) with the lanes over the
//      columns; the per-track average distances, and the block's TP / FP / FP_spatial / FN / Nref / total_DE / DE_TP / DE_FP /
//      DE_FN and loc_fp / loc_fn go to a workspace record.
//   3. seld_clip_kernel, one workgroup per clip: the records summed in block order; S / D / I from each block's loc_fp / loc_fn.
//   4. seld_file_kernel (one workgroup): the clip sums added to the per-file accumulators in clip order, unless the status
//      word is set.  No float atomics anywhere: the result is the same from run to run.
// adyolo_seld_score_runs scores the segments of one stitched run of frames (windowed evaluation) instead of whole clips: the
// scan, then seld_run_block_kernel, one wave per (segment, block, class) -- the same body as seld_block_kernel under the
// segment's frame mapping (seld_block_body, SeldSpan) -- then seld_run_sum_kernel (one workgroup): the segments in table order,
// each block record added to the file's accumulators one at a time, which leaves the bits of a whole-clip call.
// Distances are float64 in the host's order (cartesian_to_polar, then * pi / 180, then _great_circle_deg) without
// contraction; only OCML's atan2 / sin / cos / acos may differ from the host's libm by an ulp.
#include "common.hpp"
#include "lsap.hpp"

namespace adyolo {

constexpr int SELD_WAVE = 64;
constexpr int SELD_REC = 11;              // TP FP FP_spatial FN Nref total_DE DE_TP DE_FP DE_FN loc_fp loc_fn
constexpr int SELD_FIELDS = 9;

__device__ __forceinline__ double seld_dist(double az1, double s1, double c1, double az2, double s2, double c2) {
#pragma clang fp contract(off)
    double d = s1 * s2 + c1 * c2 * cos(fabs(az1 - az2));
    d = fmin(fmax(d, -1.0), 1.0);
    return acos(d) * 180.0 / M_PI;
}

struct SeldWave {
    const double *ra, *rs, *rc, *ca, *cs, *cc;   // row / column objects: azimuth (rad), sin and cos of the elevation
    int lane_;
    __device__ int lane() const { return lane_; }
    __device__ int width() const { return SELD_WAVE; }
    __device__ void sync() const { __syncthreads(); }
    __device__ double cost(int i, int j) const { return seld_dist(ra[i], rs[i], rc[i], ca[j], cs[j], cc[j]); }
    __device__ void reduce(double &v, int &r) const {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(v, o, SELD_WAVE);
            const int orank = __shfl_xor(r, o, SELD_WAVE);
            if (lsap::better(ov, orank, v, r)) {
                v = ov;
                r = orank;
            }
        }
    }
};

template <typename T>
__device__ __forceinline__ int row_class(const T *rows, long i) {
    return (int)rows[i * 5 + 1];
}

// rows of class c among rows [off, off + cnt) of one frame, counted wave-wide (every lane returns the count)
template <typename T>
__device__ int seld_count_class(const T *rows, long off, int cnt, int c, int lane) {
    int n = 0;
    for (int k0 = 0; k0 < cnt; k0 += SELD_WAVE) {
        const int k = k0 + lane;
        n += __popcll(__ballot(k < cnt && row_class(rows, off + k) == c));
    }
    return n;
}

// The frames of one file that a launch holds predictions for: file frame fr, lo <= fr < hi, is frame first + (fr - lo) of
// counts / offs.  The clip form: lo = 0, hi = t_clip, first = clip * t_clip; a segment of a run: lo = f0, hi = f0 + n, first = r0.
struct SeldSpan {
    long first;
    int lo, hi;
    __device__ bool holds(int fr) const { return fr >= lo && fr < hi; }
    __device__ long at(int fr) const { return first + (fr - lo); }
};

// One wave: block b, class c of the file whose table frames start at base, the predictions of its frames in span -> the record
// rec (zeroed by the caller).  Both kernels below are this body under their own frame mapping.
template <typename T>
__device__ __forceinline__ void seld_block_body(const T *__restrict__ rows, const int *__restrict__ counts,
                                                const int *__restrict__ offs, const int *__restrict__ ref_off,
                                                const double *__restrict__ ref_ev, const int *__restrict__ keep, long base,
                                                SeldSpan span, int b, int c, int C, int fpb, double doa_thresh,
                                                double *__restrict__ rec, int *__restrict__ status) {
#pragma clang fp contract(off)
    __shared__ double p_az[ADYOLO_SELECT_MAX_N], p_s[ADYOLO_SELECT_MAX_N], p_c[ADYOLO_SELECT_MAX_N];
    __shared__ double l_v[ADYOLO_SELECT_MAX_N], l_spc[ADYOLO_SELECT_MAX_N];
    __shared__ int l_path[ADYOLO_SELECT_MAX_N], l_r4c[ADYOLO_SELECT_MAX_N], l_rem[ADYOLO_SELECT_MAX_N];
    __shared__ unsigned char l_sc[ADYOLO_SELECT_MAX_N];
    __shared__ double r_az[ADYOLO_SELD_MAX_REF], r_s[ADYOLO_SELD_MAX_REF], r_c[ADYOLO_SELD_MAX_REF], l_u[ADYOLO_SELD_MAX_REF];
    __shared__ int l_c4r[ADYOLO_SELD_MAX_REF];
    __shared__ double t_sum[ADYOLO_SELD_MAX_REF];
    __shared__ int t_cnt[ADYOLO_SELD_MAX_REF], t_order[ADYOLO_SELD_MAX_REF];
    __shared__ int f_nref[64], f_npred[64];
    const int lane = threadIdx.x;

    // per-frame event counts of class c on both sides
    int n_ref = 0, n_pred = 0;
    for (int q = 0; q < fpb; ++q) {
        const int fr = b * fpb + q;
        const long cell = (base + fr) * C + c;
        const int nr = ref_off[cell + 1] - ref_off[cell];
        int np = 0;
        if (span.holds(fr) && (keep == nullptr || keep[base + fr])) {
            const long f = span.at(fr);
            np = seld_count_class(rows, (long)offs[f], counts[f], c, lane);
        }
        if (lane == 0) {
            f_nref[q] = nr;
            f_npred[q] = np;
        }
        n_ref = max(n_ref, nr);
        n_pred = max(n_pred, np);
    }
    if (n_pred > ADYOLO_SELECT_MAX_N || n_ref > ADYOLO_SELD_MAX_REF) {
        if (lane == 0) atomicOr(status, n_pred > ADYOLO_SELECT_MAX_N ? ADYOLO_SELD_PRED_OVERFLOW : ADYOLO_SELD_REF_OVERFLOW);
        return;
    }
    if (n_ref == 0 && n_pred == 0) return;
    __syncthreads();

    double tp = 0, fp = 0, fps = 0, fn = 0, tde = 0, de_tp = 0, de_fp = 0, de_fn = 0, loc_fp = 0, loc_fn = 0;
    if (n_ref > 0 && n_pred > 0) {
        if (lane < ADYOLO_SELD_MAX_REF) {
            t_sum[lane] = 0.0;
            t_cnt[lane] = 0;
        }
        int n_tracks = 0;
        for (int q = 0; q < fpb; ++q) {
            const int nr = f_nref[q], np = f_npred[q];
            if (nr == 0 || np == 0) continue;
            const int fr = b * fpb + q;
            const long f = span.at(fr);
            // the reference events of this frame (CSV order) and the predictions of class c (row order)
            const long e0 = ref_off[(base + fr) * C + c];
            if (lane < nr) {
                r_az[lane] = ref_ev[(e0 + lane) * 3 + 0];
                r_s[lane] = ref_ev[(e0 + lane) * 3 + 1];
                r_c[lane] = ref_ev[(e0 + lane) * 3 + 2];
            }
            const long off = offs[f];
            const int cnt = counts[f];
            int n = 0;
            for (int k0 = 0; k0 < cnt; k0 += SELD_WAVE) {
                const int k = k0 + lane;
                const bool hit = k < cnt && row_class(rows, off + k) == c;
                const unsigned long long m = __ballot(hit);
                if (hit) {
                    const int at = n + __popcll(m & ((1ull << lane) - 1ull));
                    const T *p = rows + (off + k) * 5;
                    const double x = (double)p[2], y = (double)p[3], z = (double)p[4];
                    const double az = atan2(y, x) * 180.0 / M_PI;
                    const double el = atan2(z, sqrt(x * x + y * y)) * 180.0 / M_PI;
                    const double elr = el * M_PI / 180.0;
                    p_az[at] = az * M_PI / 180.0;
                    p_s[at] = sin(elr);
                    p_c[at] = cos(elr);
                }
                n += __popcll(m);
            }
            __syncthreads();
            // scipy solves with rows <= columns: refs x preds, or preds x refs when there are fewer predictions
            const bool tr = np < nr;
            SeldWave cx;
            cx.lane_ = lane;
            if (tr) {
                cx.ra = p_az; cx.rs = p_s; cx.rc = p_c;
                cx.ca = r_az; cx.cs = r_s; cx.cc = r_c;
            } else {
                cx.ra = r_az; cx.rs = r_s; cx.rc = r_c;
                cx.ca = p_az; cx.cs = p_s; cx.cc = p_c;
            }
            const lsap::State st{l_u, l_v, l_spc, l_path, l_c4r, l_r4c, l_rem, l_sc};
            if (lsap::solve(cx, tr ? np : nr, tr ? nr : np, st) != 0) {
                if (lane == 0) atomicOr(status, ADYOLO_SELD_NO_ASSIGNMENT);
                return;
            }
            if (lane == 0) {
                for (int r = 0; r < nr; ++r) {                   // tracks keyed by the reference row, first seen first
                    const int m = lsap::match_of_row(st, tr, r);
                    if (m < 0) continue;
                    if (t_cnt[r] == 0) t_order[n_tracks++] = r;
                    t_sum[r] += seld_dist(r_az[r], r_s[r], r_c[r], p_az[m], p_s[m], p_c[m]);
                    t_cnt[r] += 1;
                }
            }
            n_tracks = __shfl(n_tracks, 0, SELD_WAVE);
            __syncthreads();
        }
        if (n_tracks == 0) {                                     // no common frame: n_pred false negatives
            loc_fn += n_pred;
            fn += n_pred;
            de_fn += n_pred;
        } else {
            for (int k = 0; k < n_tracks; ++k) {
                const int r = t_order[k];
                const double avg = t_sum[r] / (double)t_cnt[r];
                tde += avg;
                de_tp += 1;
                if (avg <= doa_thresh) {
                    tp += 1;
                } else {
                    loc_fp += 1;
                    fps += 1;
                }
            }
            if (n_pred > n_ref) {
                loc_fp += n_pred - n_ref;
                fp += n_pred - n_ref;
                de_fp += n_pred - n_ref;
            } else if (n_pred < n_ref) {
                loc_fn += n_ref - n_pred;
                fn += n_ref - n_pred;
                de_fn += n_ref - n_pred;
            }
        }
    } else if (n_ref > 0) {
        loc_fn += n_ref;
        fn += n_ref;
        de_fn += n_ref;
    } else {
        loc_fp += n_pred;
        fp += n_pred;
        de_fp += n_pred;
    }
    if (lane == 0) {
        rec[0] = tp;
        rec[1] = fp;
        rec[2] = fps;
        rec[3] = fn;
        rec[4] = n_ref;
        rec[5] = tde;
        rec[6] = de_tp;
        rec[7] = de_fp;
        rec[8] = de_fn;
        rec[9] = loc_fp;
        rec[10] = loc_fn;
    }
}

// grid: n_clips * max_blocks * C workgroups of one wave: whole clips of t_clip frames, each from frame 0 of its file
template <typename T>
__global__ __launch_bounds__(SELD_WAVE) void seld_block_kernel(
    const T *__restrict__ rows, const int *__restrict__ counts, const int *__restrict__ offs, const int *__restrict__ file_ids,
    const int *__restrict__ file_info, const int *__restrict__ ref_off, const double *__restrict__ ref_ev,
    const int *__restrict__ keep, int n_files, int t_clip, int C, int fpb, int max_blocks, double doa_thresh,
    double *__restrict__ rec_out, int *__restrict__ status) {
    const int lane = threadIdx.x;
    const long g = blockIdx.x;
    const int c = (int)(g % C);
    const int b = (int)((g / C) % max_blocks);
    const long clip = g / ((long)C * max_blocks);
    double *rec = rec_out + g * SELD_REC;
    if (lane < SELD_REC) rec[lane] = 0.0;
    if (*status != 0) return;                                   // bad rows, or an error of an earlier call: nothing is added
    const int fid = file_ids[clip];
    if (fid < 0 || fid >= n_files) {
        if (lane == 0 && b == 0 && c == 0) atomicOr(status, ADYOLO_SELD_BAD_FILE);
        return;
    }
    if (b >= file_info[2 * fid + 1]) return;
    const SeldSpan span{clip * t_clip, 0, t_clip};
    seld_block_body(rows, counts, offs, ref_off, ref_ev, keep, (long)file_info[2 * fid], span, b, c, C, fpb, doa_thresh, rec,
                    status);
}

// A segment row {file, f0, r0, n, last, 0, 0, 0} -> the file's blocks [b0, b1) it covers; false for a row that breaks the
// contract of adyolo_seld_score_runs (the caller has checked the file id).
__device__ __forceinline__ bool seld_segment_blocks(const int *__restrict__ sg, int file_blocks, int fpb, int run_frames,
                                                    int seg_blocks, int &b0, int &b1) {
    const int f0 = sg[1], r0 = sg[2], n = sg[3], last = sg[4];
    b0 = b1 = 0;
    if (f0 < 0 || r0 < 0 || n < 0 || f0 % fpb != 0 || n > run_frames || r0 > run_frames - n || f0 > INT_MAX - n) return false;
    if (!last && (f0 + n) % fpb != 0) return false;
    b0 = f0 / fpb;
    b1 = last ? file_blocks : min((f0 + n) / fpb, file_blocks);
    if (b1 < b0) b1 = b0;
    return b1 - b0 <= seg_blocks;
}

// grid: n_segments * seg_blocks * C workgroups of one wave: the segments of one stitched run
template <typename T>
__global__ __launch_bounds__(SELD_WAVE) void seld_run_block_kernel(
    const T *__restrict__ rows, const int *__restrict__ counts, const int *__restrict__ offs, const int *__restrict__ segments,
    const int *__restrict__ file_info, const int *__restrict__ ref_off, const double *__restrict__ ref_ev,
    const int *__restrict__ keep, int n_files, int run_frames, int C, int fpb, int seg_blocks, double doa_thresh,
    double *__restrict__ rec_out, int *__restrict__ status) {
    const int lane = threadIdx.x;
    const long g = blockIdx.x;
    const int c = (int)(g % C);
    const int k = (int)((g / C) % seg_blocks);
    const long seg = g / ((long)C * seg_blocks);
    double *rec = rec_out + g * SELD_REC;
    if (lane < SELD_REC) rec[lane] = 0.0;
    if (*status != 0) return;
    const int *sg = segments + seg * ADYOLO_SELD_RUN_WORDS;
    const int fid = sg[0];
    if (fid < 0 || fid >= n_files) {
        if (lane == 0 && k == 0 && c == 0) atomicOr(status, ADYOLO_SELD_BAD_FILE);
        return;
    }
    int b0, b1;
    if (!seld_segment_blocks(sg, file_info[2 * fid + 1], fpb, run_frames, seg_blocks, b0, b1)) {
        if (lane == 0 && k == 0 && c == 0) atomicOr(status, ADYOLO_SELD_BAD_RUN);
        return;
    }
    if (b0 + k >= b1) return;
    const SeldSpan span{(long)sg[2], sg[1], sg[1] + sg[3]};
    seld_block_body(rows, counts, offs, ref_off, ref_ev, keep, (long)file_info[2 * fid], span, b0 + k, c, C, fpb, doa_thresh, rec,
                    status);
}

// One workgroup, a thread per accumulator column: the segments in table order, each one's block records added to acc[file]
// one at a time from left to right (S / D / I per block from its loc_fp / loc_fn, as seld_clip_kernel forms them).  A file
// scored in ordered segments into a zeroed row therefore ends with the bits of one whole-clip call: 0 + r0 + r1 + ...
__global__ __launch_bounds__(128) void seld_run_sum_kernel(const double *__restrict__ rec, const int *__restrict__ segments,
                                                           const int *__restrict__ file_info, int n_segments, int run_frames,
                                                           int C, int fpb, int seg_blocks, double *__restrict__ acc,
                                                           const int *__restrict__ status) {
    if (*status != 0) return;
    const int ncol = SELD_FIELDS * C + 3;
    for (int col = threadIdx.x; col < ncol; col += blockDim.x) {
        for (int seg = 0; seg < n_segments; ++seg) {
            const int *sg = segments + (long)seg * ADYOLO_SELD_RUN_WORDS;
            const int fid = sg[0];
            int b0, b1;
            seld_segment_blocks(sg, file_info[2 * fid + 1], fpb, run_frames, seg_blocks, b0, b1);   // (status is 0: legal)
            const int nb = b1 - b0;
            if (nb <= 0) continue;
            const double *r0 = rec + (long)seg * seg_blocks * C * SELD_REC;
            double s = acc[(long)fid * ncol + col];
            if (col < SELD_FIELDS * C) {
                const int f = col / C, c = col % C;
                for (int b = 0; b < nb; ++b) s += r0[((long)b * C + c) * SELD_REC + f];
            } else {
                const int which = col - SELD_FIELDS * C;         // 0 S, 1 D, 2 I
                for (int b = 0; b < nb; ++b) {
                    double lfp = 0.0, lfn = 0.0;
                    for (int c = 0; c < C; ++c) {
                        lfp += r0[((long)b * C + c) * SELD_REC + 9];
                        lfn += r0[((long)b * C + c) * SELD_REC + 10];
                    }
                    s += which == 0 ? fmin(lfp, lfn) : which == 1 ? fmax(0.0, lfn - lfp) : fmax(0.0, lfp - lfn);
                }
            }
            acc[(long)fid * ncol + col] = s;
        }
    }
}

constexpr int SCAN_THREADS = 1024;

// counts [n_frames] -> offs [n_frames] (exclusive); flags a negative count or a total beyond n_rows
__global__ __launch_bounds__(SCAN_THREADS) void seld_scan_kernel(const int *__restrict__ count, int *__restrict__ offs,
                                                                 long n_frames, long n_rows, int *__restrict__ status) {
    __shared__ long part[SCAN_THREADS];
    const int t = threadIdx.x;
    const long chunk = (n_frames + SCAN_THREADS - 1) / SCAN_THREADS;
    const long s0 = t * chunk, s1 = s0 + chunk < n_frames ? s0 + chunk : n_frames;
    long sum = 0;
    bool bad = false;
    for (long s = s0; s < s1; ++s) {
        bad |= count[s] < 0;
        sum += count[s];
    }
    part[t] = sum;
    __syncthreads();
    for (int o = 1; o < SCAN_THREADS; o <<= 1) {                 // inclusive Hillis-Steele scan of the chunk sums
        const long v = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    long run = part[t] - sum;
    for (long s = s0; s < s1; ++s) {
        offs[s] = (int)(run < INT_MAX ? run : INT_MAX);
        run += count[s];
    }
    if (bad || (t == SCAN_THREADS - 1 && part[t] > n_rows)) atomicOr(status, ADYOLO_SELD_BAD_ROWS);
}

// one workgroup per clip: thread per accumulator column, the blocks in order
__global__ __launch_bounds__(128) void seld_clip_kernel(const double *__restrict__ rec, const int *__restrict__ file_ids,
                                                        const int *__restrict__ file_info, int n_files, int C,
                                                        int max_blocks, double *__restrict__ clip_sum) {
    const long clip = blockIdx.x;
    const int ncol = SELD_FIELDS * C + 3;
    const int fid = file_ids[clip];
    const int nb = fid >= 0 && fid < n_files ? file_info[2 * fid + 1] : 0;
    const double *r0 = rec + clip * max_blocks * C * SELD_REC;
    for (int col = threadIdx.x; col < ncol; col += blockDim.x) {
        double s = 0.0;
        if (col < SELD_FIELDS * C) {
            const int k = col / C, c = col % C;
            for (int b = 0; b < nb; ++b) s += r0[((long)b * C + c) * SELD_REC + k];
        } else {
            const int which = col - SELD_FIELDS * C;             // 0 S, 1 D, 2 I
            for (int b = 0; b < nb; ++b) {
                double lfp = 0.0, lfn = 0.0;
                for (int c = 0; c < C; ++c) {
                    lfp += r0[((long)b * C + c) * SELD_REC + 9];
                    lfn += r0[((long)b * C + c) * SELD_REC + 10];
                }
                s += which == 0 ? fmin(lfp, lfn) : which == 1 ? fmax(0.0, lfn - lfp) : fmax(0.0, lfp - lfn);
            }
        }
        clip_sum[clip * ncol + col] = s;
    }
}

// the clip sums added to acc[file] in clip order (a file named twice in one call gets both, in order)
__global__ __launch_bounds__(256) void seld_file_kernel(const double *__restrict__ clip_sum, const int *__restrict__ file_ids,
                                                        long n_clips, int ncol, double *__restrict__ acc,
                                                        const int *__restrict__ status) {
    if (*status != 0) return;
    for (int col = threadIdx.x; col < ncol; col += blockDim.x)
        for (long k = 0; k < n_clips; ++k) acc[(long)file_ids[k] * ncol + col] += clip_sum[k * ncol + col];
}

}  // namespace adyolo

using namespace adyolo;

static long seld_rec_doubles(long n_clips, int max_blocks, int C) { return n_clips * max_blocks * C * SELD_REC; }

extern "C" long adyolo_seld_score_workspace_words(long n_clips, int t_clip, int max_blocks, int C) {
    if (n_clips <= 0 || t_clip <= 0 || max_blocks <= 0 || C <= 0) return 0;
    return 2 * (seld_rec_doubles(n_clips, max_blocks, C) + n_clips * (SELD_FIELDS * C + 3)) + n_clips * t_clip;
}

extern "C" int adyolo_seld_score(const void *rows, int rows_f64, long n_rows, const int *counts, long n_clips, int t_clip,
                                 const int *file_ids, const int *file_info, const int *ref_off, const double *ref_ev,
                                 const int *keep, int n_files, int C, int fpb, int max_blocks, double doa_thresh,
                                 float *ws, double *acc, int *status, void *stream) {
    ADYOLO_REQUIRE(counts && file_ids && file_info && ref_off && ref_ev && ws && acc && status && (rows || n_rows == 0) &&
                       n_rows >= 0 && n_clips > 0 && t_clip > 0 && n_files > 0 && C > 0 && fpb > 0 && fpb <= 64 &&
                       max_blocks > 0 && (rows_f64 == 0 || rows_f64 == 1) && doa_thresh == doa_thresh,
                   ADYOLO_EINVAL, "seld_score: bad arguments");
    const long n_frames = n_clips * (long)t_clip;
    ADYOLO_REQUIRE(n_clips * max_blocks * C < (1L << 31) && n_frames < (1L << 31) && n_rows < (1L << 31), ADYOLO_ENOSUP,
                   "seld_score: %ld clips x %d blocks x %d classes, %ld frames, %ld rows do not fit 32-bit indices", n_clips,
                   max_blocks, C, n_frames, n_rows);
    double *rec = reinterpret_cast<double *>(ws);
    double *clip_sum = rec + seld_rec_doubles(n_clips, max_blocks, C);
    int *offs = reinterpret_cast<int *>(clip_sum + n_clips * (SELD_FIELDS * C + 3));
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(seld_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, counts, offs, n_frames, n_rows, status);
    int rc = check_launch("seld_score_scan");
    if (rc) return rc;
    const dim3 grid((unsigned)(n_clips * max_blocks * C));
    if (rows_f64)
        hipLaunchKernelGGL(seld_block_kernel<double>, grid, dim3(SELD_WAVE), 0, st, static_cast<const double *>(rows), counts,
                           offs, file_ids, file_info, ref_off, ref_ev, keep, n_files, t_clip, C, fpb, max_blocks, doa_thresh,
                           rec, status);
    else
        hipLaunchKernelGGL(seld_block_kernel<float>, grid, dim3(SELD_WAVE), 0, st, static_cast<const float *>(rows), counts,
                           offs, file_ids, file_info, ref_off, ref_ev, keep, n_files, t_clip, C, fpb, max_blocks, doa_thresh,
                           rec, status);
    rc = check_launch("seld_score_block");
    if (rc) return rc;
    hipLaunchKernelGGL(seld_clip_kernel, dim3((unsigned)n_clips), dim3(128), 0, st, rec, file_ids, file_info, n_files, C,
                       max_blocks, clip_sum);
    rc = check_launch("seld_score_clip");
    if (rc) return rc;
    hipLaunchKernelGGL(seld_file_kernel, dim3(1), dim3(256), 0, st, clip_sum, file_ids, n_clips, SELD_FIELDS * C + 3, acc,
                       status);
    return check_launch("seld_score_file");
}

extern "C" long adyolo_seld_score_runs_workspace_words(long n_segments, long run_frames, int seg_blocks, int C) {
    if (n_segments <= 0 || run_frames <= 0 || seg_blocks <= 0 || C <= 0) return 0;
    return 2 * seld_rec_doubles(n_segments, seg_blocks, C) + run_frames;
}

extern "C" int adyolo_seld_score_runs(const void *rows, int rows_f64, long n_rows, const int *counts, long run_frames,
                                      const int *segments, long n_segments, const int *file_info, const int *ref_off,
                                      const double *ref_ev, const int *keep, int n_files, int C, int fpb, int seg_blocks,
                                      double doa_thresh, float *ws, double *acc, int *status, void *stream) {
    ADYOLO_REQUIRE(counts && segments && file_info && ref_off && ref_ev && ws && acc && status && (rows || n_rows == 0) &&
                       n_rows >= 0 && run_frames > 0 && n_segments > 0 && n_files > 0 && C > 0 && fpb > 0 && fpb <= 64 &&
                       seg_blocks > 0 && (rows_f64 == 0 || rows_f64 == 1) && doa_thresh == doa_thresh,
                   ADYOLO_EINVAL, "seld_score_runs: bad arguments");
    ADYOLO_REQUIRE(n_segments * seg_blocks * C < (1L << 31) && run_frames < (1L << 31) && n_rows < (1L << 31), ADYOLO_ENOSUP,
                   "seld_score_runs: %ld segments x %d blocks x %d classes, %ld frames, %ld rows do not fit 32-bit indices",
                   n_segments, seg_blocks, C, run_frames, n_rows);
    double *rec = reinterpret_cast<double *>(ws);
    int *offs = reinterpret_cast<int *>(rec + seld_rec_doubles(n_segments, seg_blocks, C));
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(seld_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, counts, offs, run_frames, n_rows, status);
    int rc = check_launch("seld_score_runs_scan");
    if (rc) return rc;
    const dim3 grid((unsigned)(n_segments * seg_blocks * C));
    if (rows_f64)
        hipLaunchKernelGGL(seld_run_block_kernel<double>, grid, dim3(SELD_WAVE), 0, st, static_cast<const double *>(rows),
                           counts, offs, segments, file_info, ref_off, ref_ev, keep, n_files, (int)run_frames, C, fpb, seg_blocks,
                           doa_thresh, rec, status);
    else
        hipLaunchKernelGGL(seld_run_block_kernel<float>, grid, dim3(SELD_WAVE), 0, st, static_cast<const float *>(rows), counts,
                           offs, segments, file_info, ref_off, ref_ev, keep, n_files, (int)run_frames, C, fpb, seg_blocks,
                           doa_thresh, rec, status);
    rc = check_launch("seld_score_runs_block");
    if (rc) return rc;
    hipLaunchKernelGGL(seld_run_sum_kernel, dim3(1), dim3(128), 0, st, rec, segments, file_info, (int)n_segments,
                       (int)run_frames, C, fpb, seg_blocks, acc, status);
    return check_launch("seld_score_runs_sum");
}
