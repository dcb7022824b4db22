// The detection CSV files as bytes: postprocess.format_rows on the device.  The rows a selection, the view merge or a tracker
// left -- rows [capacity][5] and per-frame counts, trimmed or not -- become the very bytes write_seld_output_file writes,
// all files of the call in one buffer, with the byte offset at which each file's span starts.  The text of a line is
// csv_format.hpp, the header the host test compiles too.
//
// Count / scan / write, as the selection kernels do it, on one stream with no host read in between:
//   csv_plan_kernel   (one workgroup) the inclusive scan of the frame counts (row_end), the counts and the segment table
//                     validated; a refused call formats nothing and leaves seg_bytes zero.
//   csv_len_kernel    one lane per row, 256 rows per tile: the row's frame from its POSITION (a binary search in row_end),
//                     the frame's number in its file from the segment table, the line's LENGTH only; summed per tile.
//   csv_scan_kernel   (one workgroup) the exclusive scan of the tile sums in 64 bits, the total, the capacity check, and
//                     seg_bytes of the segments that start behind the last row.
//   csv_write_kernel  the same lanes format again, now into LDS at the tile-relative offset a workgroup scan of the lengths
//                     gives -- a line is written byte by byte, but into LDS -- and the workgroup then copies the tile's
//                     contiguous span out in aligned 16-byte stores (the LDS image is shifted so that 16-byte chunks of LDS
//                     are 16-byte chunks of the output; only the first and the last chunk of a tile go out byte by byte).
//                     The lane that holds a segment's first row stores its offset to seg_bytes.
// No atomic decides a position (the status word alone is ORed into); nothing behind row counts.sum() is read; nothing is
// written behind the total, and with a total above the capacity nothing is written at all.
#include "common.hpp"
#include "csv_format.hpp"

namespace adyolo {

constexpr int CSV_TILE = 256;                                    // rows per tile = lanes per workgroup
constexpr int CSV_SCAN_THREADS = 1024;
constexpr int CSV_LDS_BYTES = 16 + CSV_TILE * CSVF_LINE_MAX;     // the shifted image of one tile
static_assert(CSV_LDS_BYTES % 16 == 0, "the tile image is read in 16-byte chunks");

// ws, in 32-bit words: [tiles] int64 tile sums / offsets, then the head {valid, total rows, total bytes (2 words)}, then row_end [frames]
struct CsvHead {
    int valid;                                                   // 0 refused, 1 format, 2 lengths only (over the capacity)
    int total_rows;
    long long total_bytes;
};

__device__ __forceinline__ long csv_tiles(long n_rows) { return (n_rows + CSV_TILE - 1) / CSV_TILE; }

__global__ __launch_bounds__(CSV_SCAN_THREADS) void csv_plan_kernel(const int *__restrict__ count, long n_frames, long n_rows,
                                                                    const int *__restrict__ seg, long n_seg,
                                                                    int *__restrict__ row_end, CsvHead *__restrict__ head,
                                                                    long long *__restrict__ seg_bytes, int *__restrict__ status) {
    __shared__ long part[CSV_SCAN_THREADS];
    __shared__ int bad_counts, bad_table;
    const int t = threadIdx.x;
    if (t == 0) bad_counts = 0, bad_table = 0;
    __syncthreads();
    const long chunk = (n_frames + CSV_SCAN_THREADS - 1) / CSV_SCAN_THREADS;
    const long s0 = t * chunk < n_frames ? t * chunk : n_frames, s1 = s0 + chunk < n_frames ? s0 + chunk : n_frames;
    long sum = 0;
    bool neg = false;
    for (long s = s0; s < s1; ++s) {
        const int c = count[s];
        neg |= c < 0;
        sum += c < 0 ? 0 : c;
    }
    if (neg) bad_counts = 1;
    part[t] = sum;
    __syncthreads();
    for (int o = 1; o < CSV_SCAN_THREADS; o <<= 1) {             // inclusive Hillis-Steele scan of the chunk sums
        const long v = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    const long total = part[CSV_SCAN_THREADS - 1];
    const bool counts_ok = !bad_counts && total <= n_rows;       // (n_rows < 2^31: the entry checked)
    // the table: the first segment at frame 0, starts ascending and within the frames, numbers not negative and, counted on to
    // the last frame, within int32
    for (long k = t; k < n_seg; k += CSV_SCAN_THREADS) {
        const int first = seg[2 * k], number = seg[2 * k + 1];
        const int before = k ? seg[2 * (k - 1)] : 0;
        if ((k == 0 && first != 0) || first < before || first > n_frames || number < 0 ||
            (long)number + (n_frames - first) - 1 > 0x7fffffffL)
            bad_table = 1;
    }
    __syncthreads();
    const bool ok = counts_ok && !bad_table;
    if (ok) {
        long run = part[t] - sum;
        for (long s = s0; s < s1; ++s) {
            run += count[s];
            row_end[s] = (int)run;
        }
    }
    for (long k = t; k <= n_seg; k += CSV_SCAN_THREADS) seg_bytes[k] = 0;
    if (t == 0) {
        head->valid = ok ? 1 : 0;
        head->total_rows = ok ? (int)total : 0;
        head->total_bytes = 0;
        const int bits = (counts_ok ? 0 : ADYOLO_CSV_BAD_COUNTS) | (bad_table ? ADYOLO_CSV_BAD_TABLE : 0);
        if (bits) atomicOr(status, bits);
    }
}

// the first frame f with row_end[f] > n (n < the total, so there is one)
__device__ __forceinline__ int csv_frame_of(const int *__restrict__ row_end, int n_frames, int n) {
    int lo = 0, hi = n_frames - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (row_end[mid] > n) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// the last segment k with seg[k].first <= f (segment 0 starts at frame 0)
__device__ __forceinline__ int csv_segment_of(const int *__restrict__ seg, int n_seg, int f) {
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[2 * mid] <= f) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

struct CsvLine {
    long long frame, cls, id;
    uint32_t x, y, z;
    int k;                                                       // the row's segment
    bool bad;
};

__device__ __forceinline__ CsvLine csv_line_of(const float *__restrict__ rows, const int *__restrict__ ids,
                                               const int *__restrict__ row_end, int n_frames, const int *__restrict__ seg,
                                               int n_seg, int n) {
    CsvLine l;
    const int f = csv_frame_of(row_end, n_frames, n);
    l.k = csv_segment_of(seg, n_seg, f);
    l.frame = (long long)seg[2 * l.k + 1] + (f - seg[2 * l.k]);
    const float *r = rows + (size_t)n * 5;
    const float c = r[1];
    l.x = __float_as_uint(r[2]), l.y = __float_as_uint(r[3]), l.z = __float_as_uint(r[4]);
    const bool c_ok = fabsf(c) < 2147483648.f;                   // false for a NaN and for +-inf: what int() refuses
    l.cls = c_ok ? (long long)c : 0;                             // (the conversion truncates, as int() does)
    const int id = ids ? ids[n] : 0;
    l.id = id < 0 ? 0 : id;
    l.bad = !c_ok || id < 0;
    return l;
}

__global__ __launch_bounds__(CSV_TILE) void csv_len_kernel(const float *__restrict__ rows, const int *__restrict__ ids,
                                                           const int *__restrict__ row_end, int n_frames,
                                                           const int *__restrict__ seg, int n_seg,
                                                           const CsvHead *__restrict__ head, long long *__restrict__ tile_sum,
                                                           int *__restrict__ status) {
    if (head->valid == 0) return;
    __shared__ int wave_sum[CSV_TILE / 64];
    const int total = head->total_rows;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long tile = blockIdx.x; tile * CSV_TILE < total; tile += gridDim.x) {
        const long row = tile * CSV_TILE + threadIdx.x;          // (in 64 bits: the last tile may reach past 2^31)
        const int n = row < total ? (int)row : total;            // total: no row
        int len = 0;
        if (n < total) {
            const CsvLine l = csv_line_of(rows, ids, row_end, n_frames, seg, n_seg, n);
            len = csvf::line_len(l.frame, l.cls, l.id, l.x, l.y, l.z);
            if (l.bad) atomicOr(status, ADYOLO_CSV_BAD_VALUE);
        }
        for (int o = 32; o > 0; o >>= 1) len += __shfl_down(len, o, 64);
        if (lane == 0) wave_sum[wave] = len;
        __syncthreads();
        if (threadIdx.x == 0) {
            int s = 0;
            for (int w = 0; w < CSV_TILE / 64; ++w) s += wave_sum[w];
            tile_sum[tile] = s;
        }
        __syncthreads();
    }
}

// the first row at or behind segment k's start
__device__ __forceinline__ int csv_first_row(const int *__restrict__ seg, const int *__restrict__ row_end, int k) {
    const int first = seg[2 * k];
    return first == 0 ? 0 : row_end[first - 1];
}

__global__ __launch_bounds__(CSV_SCAN_THREADS) void csv_scan_kernel(long long *__restrict__ tile, CsvHead *__restrict__ head,
                                                                    const int *__restrict__ seg, long n_seg,
                                                                    const int *__restrict__ row_end, long capacity,
                                                                    long long *__restrict__ seg_bytes, int *__restrict__ status) {
    if (head->valid == 0) return;
    __shared__ long long part[CSV_SCAN_THREADS];
    const int t = threadIdx.x;
    const int total_rows = head->total_rows;
    const long n = ((long)total_rows + CSV_TILE - 1) / CSV_TILE;
    const long chunk = (n + CSV_SCAN_THREADS - 1) / CSV_SCAN_THREADS;
    const long s0 = t * chunk < n ? t * chunk : n, s1 = s0 + chunk < n ? s0 + chunk : n;
    long long sum = 0;
    for (long s = s0; s < s1; ++s) sum += tile[s];
    part[t] = sum;
    __syncthreads();
    for (int o = 1; o < CSV_SCAN_THREADS; o <<= 1) {
        const long long v = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    long long run = part[t] - sum;
    for (long s = s0; s < s1; ++s) {                             // in place: the sums become the tiles' offsets
        const long long c = tile[s];
        tile[s] = run;
        run += c;
    }
    const long long total = part[CSV_SCAN_THREADS - 1];
    for (long k = t; k <= n_seg; k += CSV_SCAN_THREADS)
        if (k == n_seg || csv_first_row(seg, row_end, (int)k) == total_rows) seg_bytes[k] = total;
    if (t == 0) {
        head->total_bytes = total;
        if (total > capacity) {
            head->valid = 2;
            atomicOr(status, ADYOLO_CSV_OVERFLOW);
        }
    }
}

__global__ __launch_bounds__(CSV_TILE) void csv_write_kernel(const float *__restrict__ rows, const int *__restrict__ ids,
                                                             const int *__restrict__ row_end, int n_frames,
                                                             const int *__restrict__ seg, int n_seg,
                                                             const CsvHead *__restrict__ head,
                                                             const long long *__restrict__ tile_off,
                                                             unsigned char *__restrict__ out, long long *__restrict__ seg_bytes) {
    const int valid = head->valid;
    if (valid == 0) return;
    __shared__ __attribute__((aligned(16))) char image[CSV_LDS_BYTES];
    __shared__ int wave_sum[CSV_TILE / 64];
    const int total = head->total_rows;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long tile = blockIdx.x; tile * CSV_TILE < total; tile += gridDim.x) {
        const long row = tile * CSV_TILE + threadIdx.x;          // (in 64 bits: the last tile may reach past 2^31)
        const int n = row < total ? (int)row : total;            // total: no row
        const long long base = tile_off[tile];
        const int shift = (int)(base & 15);                      // image[shift + i] is out[base + i]
        CsvLine l = {};
        int len = 0;
        if (n < total) {
            l = csv_line_of(rows, ids, row_end, n_frames, seg, n_seg, n);
            len = csvf::line_len(l.frame, l.cls, l.id, l.x, l.y, l.z);
        }
        int incl = len;                                          // the workgroup's exclusive scan of the lengths
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int at = incl - len, bytes = 0;
        for (int w = 0; w < CSV_TILE / 64; ++w) {
            if (w < wave) at += wave_sum[w];
            bytes += wave_sum[w];
        }
        if (n < total) {
            if (valid == 1) csvf::line_put(image + shift + at, l.frame, l.cls, l.id, l.x, l.y, l.z);
            // this row opens every segment that starts between the row before it and itself
            for (int k = l.k; k >= 0 && csv_first_row(seg, row_end, k) == n; --k) seg_bytes[k] = base + at;
        }
        __syncthreads();
        if (valid == 1) {
            unsigned char *dst = out + (base - shift);           // 16-byte aligned (the entry checked `out`)
            const int end = shift + bytes;
            for (int c = threadIdx.x; 16 * c < end; c += CSV_TILE) {
                const int b0 = 16 * c;
                if (b0 >= shift && b0 + 16 <= end) {
                    *reinterpret_cast<uint4 *>(dst + b0) = *reinterpret_cast<const uint4 *>(image + b0);
                } else {                                         // a chunk shared with the tile before or behind
                    const int lo = b0 > shift ? b0 : shift, hi = b0 + 16 < end ? b0 + 16 : end;
                    for (int b = lo; b < hi; ++b) dst[b] = (unsigned char)image[b];
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace adyolo

using namespace adyolo;

extern "C" int adyolo_csv_format(const float *rows, long n_rows, const int *frame_counts, long n_frames, const int *ids,
                                 const int *segments, long n_segments, void *ws, unsigned char *out, long capacity,
                                 long long *seg_bytes, int *status, void *stream) {
    ADYOLO_REQUIRE(rows && frame_counts && segments && ws && out && seg_bytes && status, ADYOLO_EINVAL,
                   "csv_format: null pointer");
    ADYOLO_REQUIRE(n_rows >= 0 && n_frames >= 1 && n_segments >= 1 && capacity >= 0, ADYOLO_EINVAL,
                   "csv_format: %ld rows, %ld frames, %ld segments, %ld bytes", n_rows, n_frames, n_segments, capacity);
    ADYOLO_REQUIRE(n_rows < (1L << 31) && n_frames < (1L << 31) && n_segments < (1L << 31), ADYOLO_ENOSUP,
                   "csv_format: %ld rows, %ld frames, %ld segments do not fit 32-bit counts", n_rows, n_frames, n_segments);
    ADYOLO_REQUIRE(((uintptr_t)out & 15) == 0 && ((uintptr_t)ws & 15) == 0 && ((uintptr_t)seg_bytes & 7) == 0, ADYOLO_EINVAL,
                   "csv_format: out / ws not 16-byte or seg_bytes not 8-byte aligned");
    const long tiles = (n_rows + CSV_TILE - 1) / CSV_TILE;
    long long *tile = reinterpret_cast<long long *>(ws);
    CsvHead *head = reinterpret_cast<CsvHead *>(tile + tiles);
    int *row_end = reinterpret_cast<int *>(head + 1);
    static_assert(sizeof(CsvHead) == 16, "ADYOLO_CSV_WORKSPACE_WORDS counts four words for the head");
    const unsigned grid = (unsigned)(tiles < 1 ? 1 : (tiles < 1024 ? tiles : 1024));
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(csv_plan_kernel, dim3(1), dim3(CSV_SCAN_THREADS), 0, st, frame_counts, n_frames, n_rows, segments,
                       n_segments, row_end, head, seg_bytes, status);
    int rc = check_launch("csv_plan");
    if (rc) return rc;
    hipLaunchKernelGGL(csv_len_kernel, dim3(grid), dim3(CSV_TILE), 0, st, rows, ids, row_end, (int)n_frames, segments,
                       (int)n_segments, head, tile, status);
    rc = check_launch("csv_len");
    if (rc) return rc;
    hipLaunchKernelGGL(csv_scan_kernel, dim3(1), dim3(CSV_SCAN_THREADS), 0, st, tile, head, segments, n_segments, row_end,
                       capacity, seg_bytes, status);
    rc = check_launch("csv_scan");
    if (rc) return rc;
    hipLaunchKernelGGL(csv_write_kernel, dim3(grid), dim3(CSV_TILE), 0, st, rows, ids, row_end, (int)n_frames, segments,
                       (int)n_segments, head, tile, out, seg_bytes);
    return check_launch("csv_write");
}
