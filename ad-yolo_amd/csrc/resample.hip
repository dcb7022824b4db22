// Sample-rate conversion of whole recordings on the device (ad-yolo_amd/resample.py, corpus.py InferDeviceCorpus): a polyphase FIR
// in integer arithmetic from a native stream (int16, left-justified int32 or float32, four channels) into the int16 stream the
// rest of the inference path reads.  The arithmetic is defined bit for bit (adyolo_hip.h ``adyolo_resample_pcm``, DESIGN
// section 5 "Sample-rate conversion"): Q23 samples times Q30 taps summed in int64, rounded half-even to int16.  Integer sums
// are associative, so the order of the taps here is free.
//   resample_pcm_kernel<KIND>  grid (tiles, R), ADYOLO_RESAMPLE_TILE threads.  A tile is ADYOLO_RESAMPLE_TILE consecutive output
//                              frames of one recording, one frame (four channels, one 8-byte store) per thread.  Per tile the
//                              workgroup stages in LDS (a) the input span the tile reads, already converted to Q23, one int4 per
//                              frame, zero outside the recording, and (b) the phase rows the tile touches, transposed: slot r of
//                              row k holds tap k of output j0 + r's phase, so that the lanes of a wave read consecutive banks (one
//                              broadcast address when L = 1).  min(L, tile) slots: output j0 + u has the phase of slot u % L.
//                              The slot stride is odd, so the transposing writes spread over the banks as well.
#include "common.hpp"

namespace adyolo {

constexpr int RS_TILE = ADYOLO_RESAMPLE_TILE;
constexpr long RS_LDS_MAX = 160 * 1024;               // one workgroup may hold the whole LDS of a CU
constexpr int RS_GRID_X = 1024;                       // workgroups per recording at most; longer recordings loop

__device__ __forceinline__ int rs_q23(float x, bool &bad) {
    if ((__float_as_uint(x) & 0x7f800000u) == 0x7f800000u) {   // Inf / NaN: counts as 0, told through the status word
        bad = true;
        return 0;
    }
    const float y = rintf(x * 8388608.0f);                     // a power of two: exact (or +-Inf, which the clamp takes)
    return (int)fminf(fmaxf(y, -8388608.0f), 8388607.0f);
}

template <int KIND>
__device__ __forceinline__ int4 rs_load(const void *__restrict__ src, int64_t frame, bool &bad) {
    if (KIND == ADYOLO_RESAMPLE_INT16) {
        const int2 v = reinterpret_cast<const int2 *>(src)[frame];
        return make_int4((int)(short)(v.x & 0xffff) << 8, (v.x >> 16) << 8, (int)(short)(v.y & 0xffff) << 8, (v.y >> 16) << 8);
    } else if (KIND == ADYOLO_RESAMPLE_INT32) {
        const int4 v = reinterpret_cast<const int4 *>(src)[frame];
        return make_int4(v.x >> 8, v.y >> 8, v.z >> 8, v.w >> 8);
    } else {
        const float4 v = reinterpret_cast<const float4 *>(src)[frame];
        return make_int4(rs_q23(v.x, bad), rs_q23(v.y, bad), rs_q23(v.z, bad), rs_q23(v.w, bad));
    }
}

__device__ __forceinline__ int rs_round16(int64_t acc) {       // round half even at bit 38, then the int16 clamp
    const int64_t y = (acc + ((int64_t)1 << 37) - 1 + ((acc >> 38) & 1)) >> 38;
    return (int)(y < -32768 ? -32768 : (y > 32767 ? 32767 : y));
}

// span_cap = ceil((RS_TILE - 1) M / L) + K frames: floor(a + b) - floor(a) <= ceil(b), so no tile's span is longer.
template <int KIND>
__global__ __launch_bounds__(RS_TILE) void resample_pcm_kernel(const void *__restrict__ src, long src_frames,
                                                               const int64_t *__restrict__ recs,
                                                               const int32_t *__restrict__ taps, int L, int M, int K, long centre,
                                                               int span_cap, int16_t *__restrict__ dst, long dst_frames,
                                                               int *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) int rs_lds[];
    int4 *span = reinterpret_cast<int4 *>(rs_lds);             // [span_cap] Q23 frames
    int *tp = rs_lds + 4 * (size_t)span_cap;                   // [K][ldr] taps, slot-minor
    const int64_t *row = recs + (size_t)blockIdx.y * ADYOLO_RESAMPLE_WORDS;
    const int64_t s_off = row[0], s_n = row[1], d_off = row[2], d_n = row[3];
    const bool ok = s_off >= 0 && s_n >= 0 && s_off <= src_frames && s_n <= src_frames - s_off && d_off >= 0 && d_n >= 0 &&
                    d_off <= dst_frames && d_n <= dst_frames - d_off && d_n == (s_n * L + M - 1) / M;
    if (!ok) {                                                 // uniform over the workgroup: nothing of the row is written
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, ADYOLO_CORPUS_BAD_ITEM);
        return;
    }
    const int rows = L < RS_TILE ? L : RS_TILE, ldr = rows | 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const void *rec_src = (const char *)src + (size_t)s_off * (KIND == ADYOLO_RESAMPLE_INT16 ? 8 : 16);
    int2 *rec_dst = reinterpret_cast<int2 *>(dst) + d_off;
    bool bad = false;
    unsigned staged_p0 = 0xffffffffu;                          // no p0 (p0 < L < 65536): nothing staged yet
    for (int64_t j0 = (int64_t)blockIdx.x * RS_TILE; j0 < d_n; j0 += (int64_t)gridDim.x * RS_TILE) {
        const int64_t t0 = j0 * M + centre;                    // output j0 + u: t = t0 + u M, and u M < 2^24 (M < 65536)
        const int64_t i00 = t0 / L;
        const unsigned p0 = (unsigned)(t0 - i00 * L);
        const int64_t i_lo = i00 - (K - 1);
        const int u_last = (int)((d_n - j0 < RS_TILE ? d_n - j0 : RS_TILE) - 1);
        const int span_n = (int)((p0 + (unsigned)u_last * (unsigned)M) / (unsigned)L) + K;
        for (int s = tid; s < span_n; s += RS_TILE) {
            const int64_t i = i_lo + s;
            int4 q = make_int4(0, 0, 0, 0);
            if (i >= 0 && i < s_n) q = rs_load<KIND>(rec_src, i, bad);
            span[s] = q;
        }
        if (p0 != staged_p0) {                                 // slot r holds phase (p0 + r M) % L: the slots depend on p0 alone,
            staged_p0 = p0;                                    // so a later tile of the stride loop with the same p0 keeps them
            for (int r = wave; r < rows; r += RS_TILE / 64) {  // (always when L = 1)
                const unsigned p = (p0 + (unsigned)r * (unsigned)M) % (unsigned)L;
                const int32_t *g = taps + (size_t)p * K;
                for (int k = lane; k < K; k += 64) tp[k * ldr + r] = g[k];
            }
        }
        __syncthreads();
        if (tid <= u_last) {
            const int base = (int)((p0 + (unsigned)tid * (unsigned)M) / (unsigned)L) + K - 1;     // i0 - i_lo
            const int4 *x = span + base;
            const int *h = tp + tid % rows;
            int64_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll 4
            for (int k = 0; k < K; ++k) {
                const int4 q = x[-k];
                const int c = h[k * ldr];                      // 32 x 32 + 64: one multiply-add per channel
                a0 += (int64_t)q.x * c;
                a1 += (int64_t)q.y * c;
                a2 += (int64_t)q.z * c;
                a3 += (int64_t)q.w * c;
            }
            const unsigned y0 = (unsigned)rs_round16(a0), y1 = (unsigned)rs_round16(a1), y2 = (unsigned)rs_round16(a2),
                           y3 = (unsigned)rs_round16(a3);
            rec_dst[j0 + tid] = make_int2((int)((y0 & 0xffffu) | (y1 << 16)), (int)((y2 & 0xffffu) | (y3 << 16)));
        }
        __syncthreads();
    }
    if (bad) atomicOr(status, ADYOLO_CORPUS_NONFINITE);
}

template <int KIND>
static int resample_launch(const void *src, long src_frames, const int64_t *recs, int R, const int32_t *taps, int L, int M, int K,
                           long centre, int span_cap, size_t lds, int16_t *dst, long dst_frames, int *status, void *stream) {
    if (lds > 64 * 1024) {                                     // above the default limit of a launch: asked for by name
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(resample_pcm_kernel<KIND>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        ADYOLO_REQUIRE(e == hipSuccess, ADYOLO_ENOSUP, "resample_pcm: %zu bytes of LDS refused: %s", lds, hipGetErrorString(e));
    }
    const long tiles = (dst_frames + RS_TILE - 1) / RS_TILE;   // in long: dst_frames may be up to 2^40
    const int gx = tiles < 1 ? 1 : (tiles > RS_GRID_X ? RS_GRID_X : (int)tiles);
    hipLaunchKernelGGL(resample_pcm_kernel<KIND>, dim3((unsigned)gx, (unsigned)R), dim3(RS_TILE), lds, as_stream(stream), src,
                       src_frames, recs, taps, L, M, K, centre, span_cap, dst, dst_frames, status);
    return check_launch("resample_pcm");
}

}  // namespace adyolo

using namespace adyolo;

extern "C" int adyolo_resample_pcm(const void *src, int kind, long src_frames, const int64_t *recs, int R, const int32_t *taps,
                                   long n_taps, int L, int M, int K, long centre, int16_t *dst, long dst_frames, int *status,
                                   void *stream) {
    ADYOLO_REQUIRE(src && recs && taps && dst && status, ADYOLO_EINVAL, "resample_pcm: null pointer");
    ADYOLO_REQUIRE(kind >= ADYOLO_RESAMPLE_INT16 && kind <= ADYOLO_RESAMPLE_FLOAT32, ADYOLO_EINVAL, "resample_pcm: kind %d", kind);
    ADYOLO_REQUIRE(R > 0 && R < 65536 && src_frames >= 0 && dst_frames >= 0 && src_frames < (1L << 40) && dst_frames < (1L << 40),
                   ADYOLO_EINVAL, "resample_pcm: bad shape R=%d src_frames=%ld dst_frames=%ld", R, src_frames, dst_frames);
    ADYOLO_REQUIRE(L > 0 && M > 0 && K > 0 && L < 65536 && M < 65536 && K < 65536 && centre >= 0 && centre < (1L << 31) &&
                       n_taps == (long)L * K,
                   ADYOLO_EINVAL, "resample_pcm: L=%d M=%d K=%d centre=%ld do not describe a table of %ld taps", L, M, K, centre,
                   n_taps);
    ADYOLO_REQUIRE(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0 && ((uintptr_t)recs & 7) == 0 &&
                       ((uintptr_t)taps & 3) == 0 && ((uintptr_t)status & 3) == 0,
                   ADYOLO_EINVAL, "resample_pcm: misaligned buffers (src / dst 16 bytes, recs 8 bytes, taps / status 4 bytes)");
    const long span_cap = ((long)(RS_TILE - 1) * M + L - 1) / L + K;
    const long ldr = (L < RS_TILE ? L : RS_TILE) | 1;
    const long lds = 16 * span_cap + 4 * (long)K * ldr;
    ADYOLO_REQUIRE(lds <= RS_LDS_MAX, ADYOLO_ENOSUP,
                   "resample_pcm: L=%d M=%d K=%d needs %ld bytes of LDS per tile (at most %ld)", L, M, K, lds, RS_LDS_MAX);
    switch (kind) {
    case ADYOLO_RESAMPLE_INT16:
        return resample_launch<ADYOLO_RESAMPLE_INT16>(src, src_frames, recs, R, taps, L, M, K, centre, (int)span_cap, (size_t)lds,
                                                      dst, dst_frames, status, stream);
    case ADYOLO_RESAMPLE_INT32:
        return resample_launch<ADYOLO_RESAMPLE_INT32>(src, src_frames, recs, R, taps, L, M, K, centre, (int)span_cap, (size_t)lds,
                                                      dst, dst_frames, status, stream);
    default:
        return resample_launch<ADYOLO_RESAMPLE_FLOAT32>(src, src_frames, recs, R, taps, L, M, K, centre, (int)span_cap,
                                                        (size_t)lds, dst, dst_frames, status, stream);
    }
}
