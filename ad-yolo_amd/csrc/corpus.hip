// Training batches from an HBM-resident corpus (ad-yolo_amd/corpus.py DeviceCorpus, ClasswiseDeviceCorpus): the chunk gather of
// the audio and the label encoding (AD-YOLO rows or dense class-wise targets), both from a per-batch item table, so that no
// training chunk crosses PCIe.  What they replace is the host half of FoaDataset.__getitem__ + audio_collate_fn (reference
// src/datasets.py:93-184: the WAV read, ``audio / 32768 + 1e-8``, RotationAug, get_yolo_label or the class-wise encoders,
// collate_fn) followed by AudioStager, adyolo_pcm16_to_f32 and adyolo_foa_rotate.
//
// Every stage has one kernel body with a compile-time MIX parameter.  MIX false is the plain batch: the item table alone, and
// nothing of a second source in its lanes, LDS or registers.  MIX true is time-domain mixing (aug_config.time_mix_augment: the
// audio of two chunks summed, their labels united): a second table of mates beside the items, and an item without a mate gets
// the plain form's bits.  Each stage has ONE entry point (adyolo_corpus_gather, adyolo_corpus_yolo_labels,
// adyolo_corpus_classwise_labels): the table of mates and the yaw are optional arguments, and the entry point picks the kernel
// instance from which of them it was given.
//   corpus_gather_kernel<Tab, MIX>   one pass int16 window -> float32 ``x / 32768 + 1e-8``, two frames per iteration from one
//                                    16-byte load (two 8-byte loads when the window starts on an odd frame), two 16-byte stores.
//                                    Tab = CorpusRot: FOA channels rotated; CorpusMicSrc: the four MIC capsules permuted
//                                    (channel swap); CorpusYaw: CorpusRot, then a yaw about the vertical axis by the whole angle
//                                    in word 7 of the row.  MIX: the mate's window, under its own combination (and yaw), added
//                                    as a + g * m
//   corpus_count_scan_kernel<MIX, YAW>  one workgroup: rows per lane -- (item, event), or (item, source, event) in merged order
//                                    -- exclusive scan, the total and the overflow bit
//   corpus_rows_kernel<MIX, YAW>     the rows [b, t, gi, gj, cls, U, V] at their scanned offsets, b = -1 in the rest of the
//                                    capacity
//   corpus_classwise_kernel<MIX, YAW>  the dense SEDDOA / ACCDOA / ADPIT targets (datasets.ClasswiseLabelEncoder): per tile of
//                                    label frames, each frame's event range per source, the event each (frame, class) output
//                                    takes, then every output element written once
// The label kernels have a second compile-time parameter YAW (aug_config.yaw_rotation_augment): each row's azimuths moved by its
// word 7 after the combination (augmentations.yaw_labels); YAW false is the code without it.
// Windowed inference (corpus.py InferDeviceCorpus, test.py infer_epoch_corpus) reads the same stream through a window table:
//   corpus_gather_windows_kernel<FORM>  the gather without rotation, the frames past a window's valid count int16 zero, never
//                                 read; or (rotation test-time augmentation) under one combination for the whole launch
//   decode_stitch_kernel          each window's kept decoded frames copied into one contiguous run per pass
// Streaming inference (corpus.py StreamDeviceCorpus, test.py StreamInference) reads windows out of a ring of the live stream:
//   corpus_gather_windows_kernel<FORM, WindowRing>  the same kernel body with every index taken modulo the ring's capacity
// The AD-YOLO label arithmetic is done in double, as the host does it (augmentations.rotate_labels on Python floats,
// datasets.YoloLabelEncoder.encode_events in float64); only the written row is rounded to float32.  The class-wise kernel does
// no arithmetic at all: the direction vectors come from a table the host builds with its own functions (corpus.xyz_table); with
// YAW x and y are one double product of two host-built table entries each (CorpusYawXyz), z still the table's.
#include "common.hpp"

namespace adyolo {

struct CorpusRot {                     // ADYOLO_CORPUS_ROT_WORDS floats per combination, passed by value (capturable)
    float c[16][ADYOLO_CORPUS_ROT_WORDS];
};

struct CorpusMicSrc {                  // one word per combination (adyolo_hip.h), passed by value (capturable)
    unsigned w[16];
};

// FOA rotation followed by a yaw (aug_config.yaw_rotation_augment): the combinations of CorpusRot, and the device table
// [360][2] = {cos, sin} of the whole-degree yaws -180 .. 179 (ops.corpus_yaw_table: augmentations.yaw_cos_sin); a row's yaw is
// its word ADYOLO_CORPUS_YAW_WORD, in whole degrees
struct CorpusYaw {
    CorpusRot rot;
    const float2 *cs;
};

// a row's yaw is legal: whole degrees in [-180, 180)
__device__ __forceinline__ bool corpus_yaw_ok(int64_t phi) { return phi >= -180 && phi < 180; }

__device__ __forceinline__ float4 pcm_rot(int lo, int hi, float sy, float sz, float sx, bool swap) {
    // the arithmetic of pcm16_to_f32_kernel (csrc/aug.hip) then foa_rotate_kernel (csrc/aug.hip), element for element
    const float w = (float)(short)(lo & 0xffff) / 32768.0f + 1e-8f;
    const float y = (float)(short)(lo >> 16) / 32768.0f + 1e-8f;
    const float z = (float)(short)(hi & 0xffff) / 32768.0f + 1e-8f;
    const float x = (float)(short)(hi >> 16) / 32768.0f + 1e-8f;
    const float yy = y * sy, zz = z * sz, xx = x * sx;
    return swap ? make_float4(w, xx, zz, yy) : make_float4(w, yy, zz, xx);
}

// The MIC form: a permutation of the four capsules instead of signs (augmentations.mic_swap_source).  The int16 halves of a
// frame are moved to their output places before the conversion: two v_perm_b32 per frame, then the arithmetic of
// pcm16_to_f32_kernel, element for element.
// frame bytes 0..7 = {lo, hi}; selector byte k of v_perm_b32(hi, lo, sel) names the frame byte that lands in byte k
__device__ __forceinline__ float4 pcm_swap(int lo, int hi, unsigned sel_lo, unsigned sel_hi) {
    const int a = (int)__builtin_amdgcn_perm((unsigned)hi, (unsigned)lo, sel_lo);
    const int c = (int)__builtin_amdgcn_perm((unsigned)hi, (unsigned)lo, sel_hi);
    return make_float4((float)(short)(a & 0xffff) / 32768.0f + 1e-8f, (float)(short)(a >> 16) / 32768.0f + 1e-8f,
                       (float)(short)(c & 0xffff) / 32768.0f + 1e-8f, (float)(short)(c >> 16) / 32768.0f + 1e-8f);
}

// One source's conversion, uniform over the workgroup (blockIdx.y = item), so held in scalar registers: the signs and the swap
// of pcm_rot, or the two byte selectors of pcm_swap.  gather_source returns false for a combination that is no symmetry of the
// array (MIC table only); comb < 0: the frame as it is.  The two table forms also run on the host: a window gather under one
// combination for the whole launch takes its CorpusSrc as a kernel argument.
struct CorpusSrc {
    float sy, sz, sx;
    bool swap;
    unsigned sel_lo, sel_hi;
    float c, s;                        // CorpusYaw only: the cosine and sine of the row's yaw
};

__host__ __device__ __forceinline__ bool gather_source(const CorpusRot &rot, int64_t comb, CorpusSrc &s) {
    s.sy = 1.f; s.sz = 1.f; s.sx = 1.f; s.swap = false; s.sel_lo = 0u; s.sel_hi = 0u;
    if (comb >= 0) {
        s.sy = rot.c[comb][0]; s.sz = rot.c[comb][1]; s.sx = rot.c[comb][2]; s.swap = rot.c[comb][3] != 0.f;
    }
    return true;
}

__host__ __device__ __forceinline__ bool gather_source(const CorpusMicSrc &tab, int64_t comb, CorpusSrc &s) {
    unsigned w = 0x03020100u;                               // identity: channel j from channel j
    if (comb >= 0) w = tab.w[comb];
    // channel c = frame bytes {2 c, 2 c + 1}: the byte pair c * 0x0202 + 0x0100; & 3 keeps every selector inside the frame
    const unsigned s0 = w & 3u, s1 = (w >> 8) & 3u, s2 = (w >> 16) & 3u, s3 = (w >> 24) & 3u;
    s.sy = 1.f; s.sz = 1.f; s.sx = 1.f; s.swap = false;
    s.sel_lo = (s0 * 0x0202u + 0x0100u) | ((s1 * 0x0202u + 0x0100u) << 16);
    s.sel_hi = (s2 * 0x0202u + 0x0100u) | ((s3 * 0x0202u + 0x0100u) << 16);
    return w != ADYOLO_MIC_SWAP_NONE;
}

__device__ __forceinline__ bool gather_source(const CorpusYaw &tab, int64_t comb, CorpusSrc &s) {
    return gather_source(tab.rot, comb, s);
}

// the part of a source's conversion that comes from the rest of its row: the yaw (CorpusYaw; false outside [-180, 180))
__device__ __forceinline__ bool gather_row(const CorpusRot &, const int64_t *__restrict__, CorpusSrc &) { return true; }
__device__ __forceinline__ bool gather_row(const CorpusMicSrc &, const int64_t *__restrict__, CorpusSrc &) { return true; }
__device__ __forceinline__ bool gather_row(const CorpusYaw &tab, const int64_t *__restrict__ row, CorpusSrc &s) {
    const int64_t phi = row[ADYOLO_CORPUS_YAW_WORD];
    if (!corpus_yaw_ok(phi)) return false;
    const float2 cs = tab.cs[phi + 180];
    s.c = cs.x;
    s.s = cs.y;
    return true;
}

__device__ __forceinline__ float4 gather_conv(const CorpusRot &, int lo, int hi, const CorpusSrc &s) {
    return pcm_rot(lo, hi, s.sy, s.sz, s.sx, s.swap);
}
__device__ __forceinline__ float4 gather_conv(const CorpusMicSrc &, int lo, int hi, const CorpusSrc &s) {
    return pcm_swap(lo, hi, s.sel_lo, s.sel_hi);
}
__device__ __forceinline__ float4 gather_conv(const CorpusYaw &, int lo, int hi, const CorpusSrc &s) {
    return yaw_apply(pcm_rot(lo, hi, s.sy, s.sz, s.sx, s.swap), s.c, s.s);
}

// an item or mate row as a window of the stream: false when its offset or combination is outside the corpus
template <class Tab>
__device__ __forceinline__ bool gather_window(const int64_t *__restrict__ row, long n_total, long n, const Tab &tab,
                                              CorpusSrc &s) {
    const int64_t off = row[0], comb = row[4];
    return off >= 0 && off <= n_total - n && comb < 16 && gather_source(tab, comb, s) && gather_row(tab, row, s);
}

// frames 2 i and 2 i + 1 of a window: one 16-byte load where the window starts on an even frame, two 8-byte loads where not
template <bool EVEN>
__device__ __forceinline__ int4 gather_load2(const int16_t *__restrict__ src, long i) {
    if (EVEN) return reinterpret_cast<const int4 *>(src)[i];
    const int2 *s2 = reinterpret_cast<const int2 *>(src);
    const int2 a = s2[2 * i], c = s2[2 * i + 1];
    return make_int4(a.x, a.y, c.x, c.y);
}

// the streaming loop for one parity of the item's and of the mate's offset; MIXED false: the mate is not read at all
template <class Tab, bool A_EVEN, bool M_EVEN, bool MIXED>
__device__ __forceinline__ void gather_loop(const Tab &tab, const int16_t *__restrict__ sa, const int16_t *__restrict__ sm,
                                            long n, const CorpusSrc &ca, const CorpusSrc &cm, float g, float4 *__restrict__ dst,
                                            long tid, long nth) {
    const long n2 = n >> 1;
    for (long i = tid; i < n2; i += nth) {
        const int4 va = gather_load2<A_EVEN>(sa, i);
        float4 o0 = gather_conv(tab, va.x, va.y, ca), o1 = gather_conv(tab, va.z, va.w, ca);
        if (MIXED) {
            const int4 vm = gather_load2<M_EVEN>(sm, i);
            o0 = mix_add(o0, gather_conv(tab, vm.x, vm.y, cm), g);
            o1 = mix_add(o1, gather_conv(tab, vm.z, vm.w, cm), g);
        }
        dst[2 * i] = o0;
        dst[2 * i + 1] = o1;
    }
    if ((n & 1) && tid == 0) {
        const int2 va = reinterpret_cast<const int2 *>(sa)[n - 1];
        float4 o = gather_conv(tab, va.x, va.y, ca);
        if (MIXED) {
            const int2 vm = reinterpret_cast<const int2 *>(sm)[n - 1];
            o = mix_add(o, gather_conv(tab, vm.x, vm.y, cm), g);
        }
        dst[n - 1] = o;
    }
}

// grid (blocks per item, B).  An item whose window is outside the corpus -- with MIX, or whose mate's is -- gets zeros for the
// whole sample and sets status bit 2.  A mate row has the layout of an item row; offset (word 0) == -1: the item has no mate,
// and nothing else of that row is read; word 6: the float32 bits of the gain.  MIX false: ``mates`` is not read.
template <class Tab, bool MIX>
__global__ __launch_bounds__(256) void corpus_gather_kernel(const int16_t *__restrict__ pcm, long n_total,
                                                            const int64_t *__restrict__ items,
                                                            const int64_t *__restrict__ mates, long n, Tab tab,
                                                            float4 *__restrict__ out, int *__restrict__ status) {
    const int b = blockIdx.y;
    const int64_t *it = items + (size_t)b * ADYOLO_CORPUS_ITEM_WORDS, *mt = it;
    bool mixed = false;
    if (MIX) {
        mt = mates + (size_t)b * ADYOLO_CORPUS_ITEM_WORDS;
        mixed = mt[0] != -1;
    }
    float4 *dst = out + (size_t)b * n;
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
    CorpusSrc ca, cm = {1.f, 1.f, 1.f, false, 0u, 0u, 1.f, 0.f};
    float g = 0.f;
    bool ok = gather_window(it, n_total, n, tab, ca);
    if (ok && mixed) {
        ok = gather_window(mt, n_total, n, tab, cm);
        g = __int_as_float((int)mt[6]);
    }
    if (!ok) {
        if (tid == 0 && status) atomicOr(status, ADYOLO_CORPUS_BAD_ITEM);
        for (long i = tid; i < n; i += nth) dst[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const int64_t off = it[0];
    const int16_t *sa = pcm + (size_t)off * 4;
    if (!mixed) {
        if ((off & 1) == 0)
            gather_loop<Tab, true, true, false>(tab, sa, sa, n, ca, cm, g, dst, tid, nth);
        else
            gather_loop<Tab, false, true, false>(tab, sa, sa, n, ca, cm, g, dst, tid, nth);
        return;
    }
    const int64_t moff = mt[0];
    const int16_t *sm = pcm + (size_t)moff * 4;
    switch ((int)(off & 1) | ((int)(moff & 1) << 1)) {           // uniform over the workgroup
    case 0: gather_loop<Tab, true, true, true>(tab, sa, sm, n, ca, cm, g, dst, tid, nth); break;
    case 1: gather_loop<Tab, false, true, true>(tab, sa, sm, n, ca, cm, g, dst, tid, nth); break;
    case 2: gather_loop<Tab, true, false, true>(tab, sa, sm, n, ca, cm, g, dst, tid, nth); break;
    default: gather_loop<Tab, false, false, true>(tab, sa, sm, n, ca, cm, g, dst, tid, nth); break;
    }
}

struct CorpusLabelGeom {
    int B, max_events, n_label_frames, Gaz, Gel;
    long n_events, cap;
};

// an item or mate row as a range of the event table: true when the range or the combination -- with YAW, or the yaw -- is
// outside the corpus
template <bool YAW = false>
__device__ __forceinline__ bool corpus_row_bad(const int64_t *__restrict__ row, int max_events, long n_events) {
    const int64_t ev_lo = row[2], ev_n = row[3], comb = row[4];
    if (YAW && !corpus_yaw_ok(row[ADYOLO_CORPUS_YAW_WORD])) return true;
    return ev_lo < 0 || ev_n < 0 || ev_n > max_events || ev_lo > n_events - ev_n || comb >= 16;
}

// An event's angles as the host moves them: augmentations.rotate_labels under the row's combination (comb < 0: none), then
// with YAW augmentations.yaw_labels by the row's yaw (whole degrees, legal: corpus_row_bad), all in double, nothing contracted.
template <bool YAW>
__device__ __forceinline__ void corpus_move_angles(const CorpusRot &rot, const int64_t *__restrict__ row, double &a, double &v) {
#pragma clang fp contract(off)
    const int64_t comb = row[4];
    if (comb >= 0) {                                              // augmentations.rotate_labels
        a = a * (double)rot.c[comb][4] + (double)rot.c[comb][5];
        if (a < -180.0)
            a += 360.0;
        else if (a > 180.0)
            a -= 360.0;
        v = v * (double)rot.c[comb][6];
    }
    if (YAW) {                                                    // augmentations.yaw_labels
        a = a + (double)row[ADYOLO_CORPUS_YAW_WORD];
        if (a < -180.0)
            a += 360.0;
        else if (a > 180.0)
            a -= 360.0;
    }
}

// Event e of the item (or mate) row ``it``: its frame relative to the row's window, the rotated angles and its az / el cell
// masks.  Returns the number of rows it produces (0: no event, or its frame is past the label frames).
template <bool YAW>
__device__ int corpus_event_at(const double *__restrict__ events, const int64_t *__restrict__ it,
                               const double *__restrict__ bounds, const CorpusRot &rot, const CorpusLabelGeom &g, int e,
                               int &frame, int &cls, double &az, double &el, unsigned long long &az_bits,
                               unsigned long long &el_bits, bool &bad) {
    const int64_t frame_off = it[1], ev_lo = it[2], ev_n = it[3];
    bad = corpus_row_bad<YAW>(it, g.max_events, g.n_events);
    if (bad || e >= ev_n) return 0;
    const double *ev = events + (size_t)(ev_lo + e) * 4;
    const int64_t fr = (int64_t)ev[0] - frame_off;
    if (fr < 0 || fr >= g.n_label_frames) return 0;              // get_yolo_label: frame_idx < nb_label_frames
    frame = (int)fr;
    cls = (int)ev[1];
    double a = ev[2], v = ev[3];
    corpus_move_angles<YAW>(rot, it, a, v);
    if (a == 180.0) a = -180.0;                                  // YoloLabelEncoder.encode_events
    const double *az_lb = bounds, *az_ub = bounds + g.Gaz, *el_lb = bounds + 2 * g.Gaz, *el_ub = el_lb + g.Gel;
    az_bits = 0ull;
    el_bits = 0ull;
    int naz = 0, nel = 0;
    for (int i = 0; i < g.Gaz; ++i) {
        const bool ok = (az_lb[i] <= a && a < az_ub[i]) || (a + 360.0 < az_ub[i]) || (az_lb[i] < a - 360.0);
        if (ok) { az_bits |= 1ull << i; ++naz; }
    }
    for (int j = 0; j < g.Gel; ++j) {
        const bool ok = el_lb[j] <= v && v < el_ub[j];
        if (ok) { el_bits |= 1ull << j; ++nel; }
    }
    az = a;
    el = v;
    return naz * nel;
}

// The lane decoder of both AD-YOLO kernels -> rows of the lane (as corpus_event_at); b: its item; at: the word of ws that holds
// its count, then its scanned offset: the item's first word plus the lane's place among the item's lanes.
// Plain: lanes are (item, event), max_events per item, and a lane's place is the lane itself.
// MIX: lanes are (item, source, event), 2 max_events per item, the item's events first.  Both sources' events are frame-sorted
// (corpus.load_chunked_split), so the place of an event in the merged order of augmentations.merge_labels -- frames ascending,
// the item's events before the mate's within a frame -- is its own index plus the number of the other source's events before
// it: those with a smaller window-relative frame for an item lane, a smaller or equal one for a mate lane (a binary search).
// The lanes without an event take the places behind the events, so that every place of the item's 2 max_events is written
// once.  An item whose own row or whose mate row is bad has no rows at all.
template <bool MIX, bool YAW>
__device__ int corpus_lane(const double *__restrict__ events, const int64_t *__restrict__ items,
                           const int64_t *__restrict__ mates, const double *__restrict__ bounds, const CorpusRot &rot,
                           const CorpusLabelGeom &g, long lane, int &b, long &at, int &frame, int &cls, double &az, double &el,
                           unsigned long long &az_bits, unsigned long long &el_bits, bool &bad) {
    const int me = g.max_events, per = MIX ? 2 * me : me;
    b = (int)(lane / per);
    const int r = (int)(lane - (long)b * per);
    const int64_t *it = items + (size_t)b * ADYOLO_CORPUS_ITEM_WORDS;
    if (!MIX) {
        at = lane;
        return corpus_event_at<YAW>(events, it, bounds, rot, g, r, frame, cls, az, el, az_bits, el_bits, bad);
    }
    const int src = r >= me ? 1 : 0, e = r - src * me;
    const int64_t *mt = mates + (size_t)b * ADYOLO_CORPUS_ITEM_WORDS;
    const bool has_mate = mt[0] != -1;
    bad = corpus_row_bad<YAW>(it, me, g.n_events) || (has_mate && corpus_row_bad<YAW>(mt, me, g.n_events));
    const int n_a = bad ? 0 : (int)it[3], n_m = bad || !has_mate ? 0 : (int)mt[3];
    if (e >= (src ? n_m : n_a)) {
        at = lane - r + (src ? me + e : n_m + e);
        return 0;
    }
    const int64_t *own = src ? mt : it, *other = src ? it : mt;
    const int64_t f = (int64_t)events[(size_t)(own[2] + e) * 4] - own[1];
    const double *oev = events + (size_t)other[2] * 4;
    const int64_t ooff = other[1];
    int lo = 0, hi = src ? n_a : n_m;
    while (lo < hi) {                                            // the other source's events that come first
        const int mid = (lo + hi) >> 1;
        const int64_t fo = (int64_t)oev[(size_t)mid * 4] - ooff;
        if (src ? fo <= f : fo < f)
            lo = mid + 1;
        else
            hi = mid;
    }
    at = lane - r + e + lo;
    bool own_bad;
    return corpus_event_at<YAW>(events, own, bounds, rot, g, e, frame, cls, az, el, az_bits, el_bits, own_bad);
}

constexpr int CORPUS_SCAN_THREADS = 1024;

// one workgroup: ws[at] = exclusive offset of the rows of the lane decoded to ``at``; count[0] = total rows; status |= overflow /
// bad item
template <bool MIX, bool YAW>
__global__ __launch_bounds__(CORPUS_SCAN_THREADS) void corpus_count_scan_kernel(
    const double *__restrict__ events, const int64_t *__restrict__ items, const int64_t *__restrict__ mates,
    const double *__restrict__ bounds, CorpusRot rot, CorpusLabelGeom g, int *ws, int *__restrict__ count,
    int *__restrict__ status) {
    __shared__ int part[CORPUS_SCAN_THREADS];
    __shared__ int any_bad;
    const int t = threadIdx.x;
    if (t == 0) any_bad = 0;
    __syncthreads();
    const long lanes = (long)g.B * (MIX ? 2 : 1) * g.max_events;
    const long chunk = (lanes + CORPUS_SCAN_THREADS - 1) / CORPUS_SCAN_THREADS;
    const long s0 = t * chunk, s1 = s0 + chunk < lanes ? s0 + chunk : lanes;
    int sum = 0;
    bool bad_here = false;
    for (long s = s0; s < s1; ++s) {                             // every lane's row count, at its word
        int b, frame, cls;
        long at;
        double az, el;
        unsigned long long ab, eb;
        bool bad;
        const int c = corpus_lane<MIX, YAW>(events, items, mates, bounds, rot, g, s, b, at, frame, cls, az, el, ab, eb, bad);
        bad_here |= bad;
        ws[at] = c;
        sum += c;                                                // plain: at == s, so this is the chunk's sum
    }
    if (bad_here) any_bad = 1;
    if (MIX) {                                                   // the chunk's words were written from other threads' lanes
        __threadfence_block();
        __syncthreads();
        sum = 0;
        for (long s = s0; s < s1; ++s) sum += ws[s];
    }
    part[t] = sum;
    __syncthreads();
    for (int o = 1; o < CORPUS_SCAN_THREADS; o <<= 1) {          // inclusive Hillis-Steele scan of the chunk sums
        const int v = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - sum;
    for (long s = s0; s < s1; ++s) {
        const int c = ws[s];
        ws[s] = run;
        run += c;
    }
    if (t == CORPUS_SCAN_THREADS - 1) {
        const int total = part[t];
        count[0] = total;
        int bits = any_bad ? ADYOLO_CORPUS_BAD_ITEM : 0;
        if ((long)total > g.cap) bits |= ADYOLO_CORPUS_OVERFLOW;
        if (bits && status) atomicOr(status, bits);
    }
}

// grid-stride over the lanes (rows of each event, cells in (gi, gj) order) and over the capacity (b = -1 past the total);
// column 0 of a row is the item, whichever source the event comes from
template <bool MIX, bool YAW>
__global__ __launch_bounds__(256) void corpus_rows_kernel(const double *__restrict__ events, const int64_t *__restrict__ items,
                                                          const int64_t *__restrict__ mates,
                                                          const double *__restrict__ bounds, CorpusRot rot, CorpusLabelGeom g,
                                                          const int *__restrict__ ws, const int *__restrict__ count,
                                                          float *__restrict__ target) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
    const long lanes = (long)g.B * (MIX ? 2 : 1) * g.max_events;
    for (long s = tid; s < lanes; s += nth) {
        int b, frame, cls;
        long at;
        double az, el;
        unsigned long long ab, eb;
        bool bad;
        const int c = corpus_lane<MIX, YAW>(events, items, mates, bounds, rot, g, s, b, at, frame, cls, az, el, ab, eb, bad);
        if (c == 0) continue;
        long r = ws[at];
        const float fb = (float)b, ft = (float)frame, fc = (float)cls, fu = (float)az, fv = (float)el;
        for (int i = 0; i < g.Gaz; ++i) {
            if (!((ab >> i) & 1ull)) continue;
            for (int j = 0; j < g.Gel; ++j) {
                if (!((eb >> j) & 1ull)) continue;
                if (r < g.cap) {
                    float *row = target + (size_t)r * 7;
                    row[0] = fb; row[1] = ft; row[2] = (float)i; row[3] = (float)j; row[4] = fc; row[5] = fu; row[6] = fv;
                }
                ++r;
            }
        }
    }
    const long total = count[0];
    for (long r = total + tid; r < g.cap; r += nth) {
        float *row = target + (size_t)r * 7;
        row[0] = -1.f; row[1] = 0.f; row[2] = 0.f; row[3] = 0.f; row[4] = 0.f; row[5] = 0.f; row[6] = 0.f;
    }
}

constexpr int CW_THREADS = 256;
constexpr int CW_FRAMES = 8;                   // label frames per workgroup
constexpr int CW_MAX_CLASSES = 256;
constexpr int CW_EV_CACHE = 512;               // classes of a tile's events held in LDS per source (the rest are read from memory)
constexpr int CW_SRC_BIT = 30;                 // MIX: a picked event carries its source in this bit of its index (n_events < 2^30)

struct CorpusClasswiseGeom {
    int B, max_events, n_label_frames, C, format, row;   // row: floats per label frame (4 C, 3 C or 24 C)
    long n_events;
};

// grid (label-frame tiles, B).  NS sources: the item, and with MIX its mate when it has one.  LDS: lb[s][i] = the first event
// of source s at or after frame t0 + i; cls[s][] = the classes of the tile's events (-1: outside [0, C)); pick[i][c] = {count of
// class c in frame t0 + i, its first three events} (ADPIT) or {its last event, ...} (SEDDOA / ACCDOA), -1 where there is none.
// A (frame, class) output picks over the item's range, then the mate's (the order of merge_labels); every picked event carries
// its source, because its direction vector is read from the xyz slot of its own source's combination.
//
// YAW (aug_config.yaw_rotation_augment): z still comes from the xyz slot (a yaw does not move it), x and y from two host-built
// double tables indexed by the moved whole-degree angles (corpus_move_angles): yaw.az [361][2] = {cos, sin} of azimuth -180 ..
// 180, yaw.el [181] = cos of elevation -90 .. 90; x = (float)(cos_az * cos_el), y = (float)(sin_az * cos_el), one double
// product each, rounded once -- what the host encoder's float64 arrays give as float32.  YAW false: ``yaw`` is not read.
struct CorpusYawXyz {
    CorpusRot rot;
    const double *az, *el;
};
struct CorpusNoYawXyz {};              // what the kernel takes in its place without YAW: nothing
template <bool YAW> struct CorpusYawXyzArg { typedef CorpusNoYawXyz type; };
template <> struct CorpusYawXyzArg<true> { typedef CorpusYawXyz type; };

__device__ __forceinline__ float corpus_yaw_xy(const CorpusNoYawXyz &, const double *__restrict__, const int64_t *__restrict__,
                                               int) {
    return 0.f;
}

__device__ __forceinline__ float corpus_yaw_xy(const CorpusYawXyz &yaw, const double *__restrict__ ev,
                                               const int64_t *__restrict__ row, int k) {
#pragma clang fp contract(off)
    double a = ev[2], v = ev[3];
    corpus_move_angles<true>(yaw.rot, row, a, v);
    // whole degrees inside the tables (the host corpus refuses a split with any other angle); anything else reads entry 0
    const int ia = a >= -180.0 && a <= 180.0 ? (int)a + 180 : 0, ie = v >= -90.0 && v <= 90.0 ? (int)v + 90 : 0;
    return (float)(yaw.az[2 * ia + k] * yaw.el[ie]);
}

template <bool MIX, bool YAW>
__global__ __launch_bounds__(CW_THREADS) void corpus_classwise_kernel(const double *__restrict__ events,
                                                                      const float *__restrict__ xyz,
                                                                      const int64_t *__restrict__ items,
                                                                      const int64_t *__restrict__ mates, CorpusClasswiseGeom g,
                                                                      typename CorpusYawXyzArg<YAW>::type yaw,
                                                                      float *__restrict__ target, int *__restrict__ status) {
    constexpr int NS = MIX ? 2 : 1;
    extern __shared__ int pick[];                // [CW_FRAMES][C][4]
    __shared__ int lb[NS][CW_FRAMES + 1];
    __shared__ int cls[NS][CW_EV_CACHE];
    const int b = blockIdx.y, t0 = blockIdx.x * CW_FRAMES, tid = threadIdx.x;
    const int nf = g.n_label_frames - t0 < CW_FRAMES ? g.n_label_frames - t0 : CW_FRAMES;
    const int64_t *rows[NS];
    rows[0] = items + (size_t)b * ADYOLO_CORPUS_ITEM_WORDS;
    if (MIX) rows[NS - 1] = mates + (size_t)b * ADYOLO_CORPUS_ITEM_WORDS;
    const int ns = MIX && rows[NS - 1][0] != -1 ? 2 : 1;
    float *dst = target + ((size_t)b * g.n_label_frames + t0) * g.row;
    const int n_out = nf * g.row;
    int64_t frame_off[NS] = {}, ev_lo[NS] = {};
    int n[NS] = {};
    size_t slot[NS] = {};
    bool bad = false;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (s >= ns) break;
        bad |= corpus_row_bad<YAW>(rows[s], g.max_events, g.n_events);
        const int64_t comb = rows[s][4];
        frame_off[s] = rows[s][1];
        ev_lo[s] = rows[s][2];
        n[s] = (int)rows[s][3];
        slot[s] = comb < 0 ? 0 : (size_t)comb + 1;
    }
    if (bad) {
        if (blockIdx.x == 0 && tid == 0) atomicOr(status, ADYOLO_CORPUS_BAD_ITEM);
        for (int p = tid; p < n_out; p += CW_THREADS) dst[p] = 0.f;
        return;
    }
    if (tid <= nf) {
#pragma unroll
        for (int s = 0; s < NS; ++s) lb[s][tid] = n[s];
    }
    __syncthreads();
    // a source's events are frame-sorted: lb[s][i] is written by the one event whose frame is the first to reach t0 + i (one
    // round of independent loads, no binary search); it stays n[s] where none does.  Unsorted input can leave lb out of order:
    // every range below is then empty or still inside [0, n[s]).
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (s >= ns) break;
        const double *ev = events + (size_t)ev_lo[s] * 4;
        const double base = (double)(frame_off[s] + t0);
        for (int e = tid; e < n[s]; e += CW_THREADS) {
            const double fe = ev[(size_t)e * 4] - base;
            const double fp = e > 0 ? ev[(size_t)(e - 1) * 4] - base : -1.0;
            const double lo = fp < 0.0 ? 0.0 : floor(fp) + 1.0, hi = fe > (double)nf ? (double)nf : floor(fe);
            if (lo <= hi)
                for (int i = (int)lo; i <= (int)hi; ++i) lb[s][i] = e;
        }
    }
    __syncthreads();
    const int C = g.C;
    int e0[NS] = {}, e1[NS] = {};                                 // the tile's events of each source
#pragma unroll
    for (int s = 0; s < NS; ++s) {                                // their classes checked, the first ones cached
        if (s >= ns) break;
        const double *ev = events + (size_t)ev_lo[s] * 4;
        e0[s] = lb[s][0];
        e1[s] = lb[s][nf];
        for (int e = e0[s] + tid; e < e1[s]; e += CW_THREADS) {
            const double cd = ev[(size_t)e * 4 + 1];
            const bool ok = cd >= 0.0 && cd < (double)C;
            if (!ok) atomicOr(status, ADYOLO_CORPUS_BAD_CLASS);
            if (e - e0[s] < CW_EV_CACHE) cls[s][e - e0[s]] = ok ? (int)cd : -1;
        }
    }
    __syncthreads();
    const bool adpit = g.format == ADYOLO_CORPUS_ADPIT;
    for (int p = tid; p < nf * C; p += CW_THREADS) {
        const int i = p / C, c = p - i * C;
        int cnt = 0, last = -1, first[3] = {-1, -1, -1};
#pragma unroll
        for (int s = 0; s < NS; ++s) {                            // the item's events of the frame, then the mate's
            if (s >= ns) break;
            const double *ev = events + (size_t)ev_lo[s] * 4;
            for (int e = lb[s][i]; e < lb[s][i + 1]; ++e) {       // file order within the frame
                int ce;
                if (e < e1[s] && (unsigned)(e - e0[s]) < (unsigned)CW_EV_CACHE) {
                    ce = cls[s][e - e0[s]];
                } else {
                    const double cd = ev[(size_t)e * 4 + 1];
                    ce = cd >= 0.0 && cd < (double)C ? (int)cd : -1;
                }
                if (ce == c) {
                    const int idx = ((int)ev_lo[s] + e) | (s << CW_SRC_BIT);
                    if (cnt < 3) first[cnt] = idx;
                    last = idx;
                    ++cnt;
                }
            }
        }
        int *q = pick + p * 4;
        q[0] = adpit ? cnt : last;
        q[1] = first[0];
        q[2] = first[1];
        q[3] = first[2];
    }
    __syncthreads();
    // every position r of a frame's row is owned by one thread, its class / component / track slot worked out once (no
    // division per element); the frames of the tile are written one after the other, each row by consecutive threads
    for (int r = tid; r < g.row; r += CW_THREADS) {
        int c, k, s = 0;                       // class, component (-1: the activity 1.0, else x / y / z), ADPIT track slot
        if (adpit) {
            s = r / (4 * C);
            const int rr = r - s * 4 * C;
            k = rr / C - 1;
            c = rr - (k + 1) * C;
        } else {
            const int part = r / C;
            c = r - part * C;
            k = g.format == ADYOLO_CORPUS_SEDDOA ? part - 1 : part;
        }
        // ADPIT: slot 0 takes the class's event when it has one, slots 1-2 its two, slots 3-5 the first three of three or more
        const int lo_cnt = s == 0 ? 1 : s <= 2 ? 2 : 3, hi_cnt = s == 0 ? 1 : s <= 2 ? 2 : 0x7fffffff;
        const int j = s == 0 ? 0 : s <= 2 ? s - 1 : s - 3;
        for (int i = 0; i < nf; ++i) {
            const int *q = pick + (i * C + c) * 4;
            const int e = adpit ? (q[0] >= lo_cnt && q[0] <= hi_cnt ? q[1 + j] : -1) : q[0];
            const size_t sl = MIX && ((e >> CW_SRC_BIT) & 1) ? slot[NS - 1] : slot[0];
            const size_t idx = MIX ? (size_t)(e & ((1 << CW_SRC_BIT) - 1)) : (size_t)e;
            if (YAW && e >= 0 && (k == 0 || k == 1)) {            // x, y of a yawed event: from its moved angles
                const bool mate = MIX && ((e >> CW_SRC_BIT) & 1);
                dst[(size_t)i * g.row + r] = corpus_yaw_xy(yaw, events + idx * 4, mate ? rows[NS - 1] : rows[0], k);
                continue;
            }
            dst[(size_t)i * g.row + r] = e < 0 ? 0.f : k < 0 ? 1.f : xyz[(idx * ADYOLO_CORPUS_XYZ_SLOTS + sl) * 3 + k];
        }
    }
}

// ================================================================================================ windowed inference
// A window row: {offset, valid, src_lo, dst, n, recording, 0, 0} (adyolo_hip.h).  Both kernels stream: every output element is
// written once by the thread that read its source, in the access shapes of corpus_gather_kernel.

// The conversion of a window gather, one kernel instance each: the frame as it is (adyolo_corpus_gather_windows), or one
// combination for the whole launch (adyolo_corpus_gather_windows_view: rotation test-time augmentation), FOA signs and swap or
// the MIC byte selectors.  The combination's CorpusSrc is worked out on the host and passed by value, so the signs, the swap
// and the selectors are kernel arguments: scalar registers, no table read at all.
enum { WINDOW_PLAIN, WINDOW_FOA, WINDOW_MIC };

template <int FORM>
__device__ __forceinline__ float4 window_conv(int lo, int hi, const CorpusSrc &s) {
    if (FORM == WINDOW_MIC) return pcm_swap(lo, hi, s.sel_lo, s.sel_hi);
    if (FORM == WINDOW_FOA) return pcm_rot(lo, hi, s.sy, s.sz, s.sx, s.swap);
    return pcm_rot(lo, hi, 1.f, 1.f, 1.f, false);
}

// Where a window's frames lie.  WindowLinear: a linear stream of n_total frames, window frame f at pcm[off + f] (nothing to
// carry: no kernel argument).  WindowRing: ``pcm`` is a ring of ``capacity`` frames that holds the last ones of a live stream
// of n_total (the head) frames so far, absolute frame s at pcm[s % capacity] (adyolo_stream_gather_windows).  Capacity and
// offsets are even, so a two-frame 16-byte load never straddles the seam; a window is at most ``capacity`` long, so one
// conditional subtraction wraps an index.  head % capacity comes from the host (head_mod): no division on the device.
struct WindowLinear {
    __device__ __forceinline__ bool bad(int64_t off, int64_t valid, long n_total) const { return off > n_total - valid; }
    __device__ __forceinline__ int64_t seek(int64_t off, long) { return off; }      // -> the frame the reads are counted from
    __device__ __forceinline__ long pair(long i) const { return i; }
    __device__ __forceinline__ long frame(long f) const { return f; }
};

struct WindowRing {
    long capacity, head_mod;
    long pos;                                                     // the window's first frame in the ring (after seek)
    __device__ __forceinline__ bool bad(int64_t off, int64_t valid, long head) const {
        return off > head - valid || off < head - capacity;      // not pushed yet, or already overwritten
    }
    __device__ __forceinline__ int64_t seek(int64_t off, long head) {               // 0 <= head - off <= capacity
        pos = head_mod - (long)(head - off);
        if (pos < 0) pos += capacity;
        return 0;
    }
    __device__ __forceinline__ long pair(long i) const {
        const long j = (pos >> 1) + i;
        return j >= (capacity >> 1) ? j - (capacity >> 1) : j;
    }
    __device__ __forceinline__ long frame(long f) const {
        const long j = pos + f;
        return j >= capacity ? j - capacity : j;
    }
};

template <class... Ring> struct WindowOf { typedef WindowLinear type; };
template <> struct WindowOf<WindowRing> { typedef WindowRing type; };

// Both window gathers, grid (blocks per window, W).  Ring: nothing (the linear gathers: the kernel has the arguments it always
// had), or one WindowRing (the streaming gather: the same body with every index taken through the ring).  Frames at or past
// ``valid`` are the conversion of int16 zero and are not read from the stream: under a view the padding is turned like every
// other frame (1e-8f under the signs and the swap).  comb_ok false (a MIC combination that is no symmetry of the array): every
// window is a bad item.
template <int FORM, class... Ring>
__global__ __launch_bounds__(256) void corpus_gather_windows_kernel(const int16_t *__restrict__ pcm, long n_total,
                                                                    const int64_t *__restrict__ windows, long n, CorpusSrc cs,
                                                                    int comb_ok, float4 *__restrict__ out,
                                                                    int *__restrict__ status, Ring... ring) {
    typename WindowOf<Ring...>::type geom{ring...};
    const int w = blockIdx.y;
    const int64_t off = windows[(size_t)w * ADYOLO_WINDOW_WORDS + 0];
    const int64_t valid = windows[(size_t)w * ADYOLO_WINDOW_WORDS + 1];
    float4 *dst = out + (size_t)w * n;
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
    const float4 pad = window_conv<FORM>(0, 0, cs);               // int16 zero: what the zero padding of a training chunk becomes
    if (valid == 0 && comb_ok) {                                  // an empty window: nothing else of the row is looked at
        for (long i = tid; i < n; i += nth) dst[i] = pad;
        return;
    }
    if (!comb_ok || off < 0 || (off & 1) || valid < 0 || valid > n || geom.bad(off, valid, n_total)) {
        if (tid == 0 && status) atomicOr(status, ADYOLO_CORPUS_BAD_ITEM);
        for (long i = tid; i < n; i += nth) dst[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const int16_t *src = pcm + (size_t)geom.seek(off, n_total) * 4;       // even offset: two frames per 16-byte load
    const long n2 = n >> 1;
    const int4 *s4 = reinterpret_cast<const int4 *>(src);
    const int2 *s2 = reinterpret_cast<const int2 *>(src);
    for (long i = tid; i < n2; i += nth) {
        float4 o0 = pad, o1 = pad;
        if (2 * i + 1 < valid) {
            const int4 v = s4[geom.pair(i)];
            o0 = window_conv<FORM>(v.x, v.y, cs);
            o1 = window_conv<FORM>(v.z, v.w, cs);
        } else if (2 * i < valid) {                               // the last frame of an odd count
            const int2 v = s2[geom.frame(2 * i)];
            o0 = window_conv<FORM>(v.x, v.y, cs);
        }
        dst[2 * i] = o0;
        dst[2 * i + 1] = o1;
    }
    if ((n & 1) && tid == 0) {
        float4 o = pad;
        if (n - 1 < valid) {
            const int2 v = s2[geom.frame(n - 1)];
            o = window_conv<FORM>(v.x, v.y, cs);
        }
        dst[n - 1] = o;
    }
}

// grid (blocks per window, W).  A window's kept frames are one contiguous run of n * rec floats on both sides.  VEC: rec % 4
// == 0, so that every run starts and ends on a 16-byte boundary of its buffer.
template <bool VEC>
__global__ __launch_bounds__(256) void decode_stitch_kernel(const float *__restrict__ decoded,
                                                            const int64_t *__restrict__ windows, int Wf, long rec,
                                                            long pass_base, float *__restrict__ out, long out_frames,
                                                            int *__restrict__ status) {
    const int w = blockIdx.y;
    const int64_t *row = windows + (size_t)w * ADYOLO_WINDOW_WORDS;
    const int64_t src_lo = row[2], n = row[4];
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
    if (n == 0) return;
    const int64_t d0 = row[3] - pass_base;
    if (src_lo < 0 || n < 0 || n > Wf || src_lo > Wf - n || d0 < 0 || d0 > out_frames - n) {
        if (tid == 0 && status) atomicOr(status, ADYOLO_CORPUS_BAD_ITEM);
        return;
    }
    const float *s = decoded + ((size_t)w * Wf + (size_t)src_lo) * rec;
    float *d = out + (size_t)d0 * rec;
    const long len = (long)n * rec;
    if (VEC) {
        const float4 *s4 = reinterpret_cast<const float4 *>(s);
        float4 *d4 = reinterpret_cast<float4 *>(d);
        for (long i = tid; i < (len >> 2); i += nth) d4[i] = s4[i];
    } else {
        for (long i = tid; i < len; i += nth) d[i] = s[i];
    }
}

static void corpus_rot(const float *rot_host, CorpusRot &rot) {
    for (int c = 0; c < 16; ++c)
        for (int k = 0; k < ADYOLO_CORPUS_ROT_WORDS; ++k) rot.c[c][k] = rot_host[c * ADYOLO_CORPUS_ROT_WORDS + k];
}

static void corpus_mic(const unsigned int *src_host, CorpusMicSrc &tab) {
    for (int c = 0; c < 16; ++c) tab.w[c] = src_host[c];
}

// The launchers of each stage, one per kernel instance; ``name`` is the entry point, for its messages; MIX false takes mates ==
// nullptr.  Each entry point below picks its instance in one place: mates given -> MIX, a yaw given -> CorpusYaw / YAW.
template <class Tab, bool MIX>
static int corpus_gather_launch(const char *name, const int16_t *pcm, long n_total, const int64_t *items, const int64_t *mates,
                                int B, long n, const Tab &tab, float *audio, int *status, void *stream) {
    ADYOLO_REQUIRE(pcm && items && (mates || !MIX) && audio, ADYOLO_EINVAL, "%s: null pointer", name);
    ADYOLO_REQUIRE(B > 0 && B < 65536 && n > 0 && n_total >= n, ADYOLO_EINVAL, "%s: bad shape B=%d n=%ld n_total=%ld", name, B, n,
                   n_total);
    ADYOLO_REQUIRE(((uintptr_t)pcm & 15) == 0 && ((uintptr_t)audio & 15) == 0 && ((uintptr_t)items & 7) == 0 &&
                       ((uintptr_t)mates & 7) == 0,
                   ADYOLO_EINVAL, "%s: misaligned buffers (pcm / audio 16 bytes, items / mates 8 bytes)", name);
    // ~16 frames per thread: at 20 s (480000 frames) 118 blocks per item, 1888 for a batch of 16
    int gx = cdiv(n, 256L * 16);
    gx = gx < 1 ? 1 : (gx > 4096 ? 4096 : gx);
    hipLaunchKernelGGL((corpus_gather_kernel<Tab, MIX>), dim3((unsigned)gx, (unsigned)B), dim3(256), 0, as_stream(stream), pcm,
                       n_total, items, mates, n, tab, (float4 *)audio, status);
    return check_launch(name);
}

template <bool MIX, bool YAW>
static int corpus_yolo_labels_launch(const char *name, const double *events, long n_events, const int64_t *items,
                                     const int64_t *mates, int B, int max_events, int n_label_frames, const double *grid_bounds,
                                     int Gaz, int Gel, const float *rot_host, int *ws, float *target, long cap, int *count,
                                     int *status, void *stream) {
    ADYOLO_REQUIRE(events && items && (mates || !MIX) && grid_bounds && rot_host && ws && target && count && status, ADYOLO_EINVAL,
                   "%s: null pointer", name);
    const long lanes = (long)B * (MIX ? 2 : 1) * max_events;
    ADYOLO_REQUIRE(B > 0 && max_events >= 0 && n_events >= 0 && n_label_frames > 0 && cap > 0 && cap < (1L << 31) &&
                       lanes < (1L << 31),
                   ADYOLO_EINVAL, "%s: bad shape B=%d max_events=%d cap=%ld", name, B, max_events, cap);
    ADYOLO_REQUIRE(Gaz > 0 && Gaz <= 64 && Gel > 0 && Gel <= 64, ADYOLO_ENOSUP, "%s: grid %d x %d (at most 64 x 64 cells)", name,
                   Gaz, Gel);
    ADYOLO_REQUIRE(((uintptr_t)events & 7) == 0 && ((uintptr_t)items & 7) == 0 && ((uintptr_t)mates & 7) == 0 &&
                       ((uintptr_t)grid_bounds & 7) == 0 && ((uintptr_t)target & 3) == 0,
                   ADYOLO_EINVAL, "%s: misaligned buffers", name);
    CorpusRot rot;
    corpus_rot(rot_host, rot);
    CorpusLabelGeom g;
    g.B = B; g.max_events = max_events; g.n_label_frames = n_label_frames; g.Gaz = Gaz; g.Gel = Gel;
    g.n_events = n_events; g.cap = cap;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL((corpus_count_scan_kernel<MIX, YAW>), dim3(1), dim3(CORPUS_SCAN_THREADS), 0, st, events, items, mates,
                       grid_bounds, rot, g, ws, count, status);
    int rc = check_launch(name);
    if (rc) return rc;
    long work = cap > lanes ? cap : lanes;
    int gx = cdiv(work, 256L * 4);
    gx = gx < 1 ? 1 : (gx > 1024 ? 1024 : gx);
    hipLaunchKernelGGL((corpus_rows_kernel<MIX, YAW>), dim3((unsigned)gx), dim3(256), 0, st, events, items, mates, grid_bounds, rot, g,
                       ws, count, target);
    return check_launch(name);
}

template <bool MIX, bool YAW>
static int corpus_classwise_launch(const char *name, const double *events, const float *xyz, long n_events, const int64_t *items,
                                   const int64_t *mates, int B, int max_events, int n_label_frames, int n_classes, int format,
                                   float *target, int *status, void *stream, typename CorpusYawXyzArg<YAW>::type yaw) {
    ADYOLO_REQUIRE(events && xyz && items && (mates || !MIX) && target && status, ADYOLO_EINVAL, "%s: null pointer", name);
    ADYOLO_REQUIRE(B > 0 && B < 65536 && max_events >= 0 && n_events >= 0 && n_events < (1L << (MIX ? CW_SRC_BIT : 31)) &&
                       n_label_frames > 0 && n_classes > 0,
                   ADYOLO_EINVAL, "%s: bad shape B=%d max_events=%d n_events=%ld n_label_frames=%d C=%d", name, B, max_events,
                   n_events, n_label_frames, n_classes);
    ADYOLO_REQUIRE(format == ADYOLO_CORPUS_SEDDOA || format == ADYOLO_CORPUS_ACCDOA || format == ADYOLO_CORPUS_ADPIT,
                   ADYOLO_EINVAL, "%s: unknown format %d", name, format);
    ADYOLO_REQUIRE(n_classes <= CW_MAX_CLASSES, ADYOLO_ENOSUP, "%s: %d classes (at most %d)", name, n_classes, CW_MAX_CLASSES);
    ADYOLO_REQUIRE(((uintptr_t)events & 7) == 0 && ((uintptr_t)items & 7) == 0 && ((uintptr_t)mates & 7) == 0 &&
                       ((uintptr_t)xyz & 3) == 0 && ((uintptr_t)target & 3) == 0 && ((uintptr_t)status & 3) == 0,
                   ADYOLO_EINVAL, "%s: misaligned buffers", name);
    CorpusClasswiseGeom g;
    g.B = B; g.max_events = max_events; g.n_label_frames = n_label_frames; g.C = n_classes; g.format = format;
    g.row = (format == ADYOLO_CORPUS_SEDDOA ? 4 : format == ADYOLO_CORPUS_ACCDOA ? 3 : 24) * n_classes;
    g.n_events = n_events;
    const size_t lds = (size_t)CW_FRAMES * n_classes * 4 * sizeof(int);
    hipLaunchKernelGGL((corpus_classwise_kernel<MIX, YAW>), dim3((unsigned)cdiv(n_label_frames, CW_FRAMES), (unsigned)B),
                       dim3(CW_THREADS), lds, as_stream(stream), events, xyz, items, mates, g, yaw, target, status);
    return check_launch(name);
}

}  // namespace adyolo

using namespace adyolo;

extern "C" int adyolo_corpus_gather(const int16_t *pcm, long n_total, const int64_t *items, const int64_t *mates, int B, long n,
                                    const float *rot_host, const unsigned int *mic_src_host, const float *yaw_tab, float *audio,
                                    int *status, void *stream) {
    const char *name = "corpus_gather";
    ADYOLO_REQUIRE(rot_host || mic_src_host, ADYOLO_EINVAL, "%s: null pointer", name);
    if (mic_src_host) {
        ADYOLO_REQUIRE(!yaw_tab, ADYOLO_EINVAL, "%s: a yaw table with the MIC form (there is no MIC yaw)", name);
        CorpusMicSrc tab;
        corpus_mic(mic_src_host, tab);
        return (mates ? corpus_gather_launch<CorpusMicSrc, true> : corpus_gather_launch<CorpusMicSrc, false>)(
            name, pcm, n_total, items, mates, B, n, tab, audio, status, stream);
    }
    if (yaw_tab) {
        ADYOLO_REQUIRE(((uintptr_t)yaw_tab & 7) == 0, ADYOLO_EINVAL, "%s: misaligned yaw table (8 bytes)", name);
        CorpusYaw tab;
        corpus_rot(rot_host, tab.rot);
        tab.cs = reinterpret_cast<const float2 *>(yaw_tab);
        return (mates ? corpus_gather_launch<CorpusYaw, true> : corpus_gather_launch<CorpusYaw, false>)(
            name, pcm, n_total, items, mates, B, n, tab, audio, status, stream);
    }
    CorpusRot rot;
    corpus_rot(rot_host, rot);
    return (mates ? corpus_gather_launch<CorpusRot, true> : corpus_gather_launch<CorpusRot, false>)(
        name, pcm, n_total, items, mates, B, n, rot, audio, status, stream);
}

extern "C" long adyolo_corpus_yolo_labels_workspace_words(int B, int max_events, int mix) {
    if (B <= 0 || max_events < 0) return -1;
    return (long)B * (mix ? 2 : 1) * (max_events > 0 ? max_events : 1);
}

extern "C" int adyolo_corpus_yolo_labels(const double *events, long n_events, const int64_t *items, const int64_t *mates, int B,
                                         int max_events, int n_label_frames, const double *grid_bounds, int Gaz, int Gel,
                                         const float *rot_host, int yaw, int *ws, float *target, long cap, int *count,
                                         int *status, void *stream) {
    return (mates ? (yaw ? corpus_yolo_labels_launch<true, true> : corpus_yolo_labels_launch<true, false>)
                  : (yaw ? corpus_yolo_labels_launch<false, true> : corpus_yolo_labels_launch<false, false>))(
        "corpus_yolo_labels", events, n_events, items, mates, B, max_events, n_label_frames, grid_bounds, Gaz, Gel, rot_host, ws,
        target, cap, count, status, stream);
}

extern "C" int adyolo_corpus_classwise_labels(const double *events, const float *xyz, long n_events, const int64_t *items,
                                              const int64_t *mates, int B, int max_events, int n_label_frames, int n_classes,
                                              int format, const float *rot_host, const double *yaw_az, const double *yaw_el,
                                              float *target, int *status, void *stream) {
    const char *name = "corpus_classwise_labels";
    if (!yaw_az && !yaw_el)
        return (mates ? corpus_classwise_launch<true, false> : corpus_classwise_launch<false, false>)(
            name, events, xyz, n_events, items, mates, B, max_events, n_label_frames, n_classes, format, target, status, stream,
            CorpusNoYawXyz());
    ADYOLO_REQUIRE(rot_host && yaw_az && yaw_el, ADYOLO_EINVAL, "%s: null pointer", name);
    ADYOLO_REQUIRE(((uintptr_t)yaw_az & 7) == 0 && ((uintptr_t)yaw_el & 7) == 0, ADYOLO_EINVAL, "%s: misaligned yaw tables", name);
    CorpusYawXyz yaw;
    corpus_rot(rot_host, yaw.rot);
    yaw.az = yaw_az;
    yaw.el = yaw_el;
    return (mates ? corpus_classwise_launch<true, true> : corpus_classwise_launch<false, true>)(
        name, events, xyz, n_events, items, mates, B, max_events, n_label_frames, n_classes, format, target, status, stream, yaw);
}

// ------------------------------------------------------------------------------------------------ windowed inference
namespace adyolo {
// the window gathers: the checks, the grid of adyolo_corpus_gather and the instance of the form.  RING: ``pcm`` is the ring of
// adyolo_stream_gather_windows, n_total its head, capacity its length
template <int FORM, bool RING = false>
static int corpus_gather_windows_launch(const char *name, const int16_t *pcm, long n_total, const int64_t *windows, int W, long n,
                                        const CorpusSrc &cs, bool comb_ok, float *audio, int *status, void *stream,
                                        long capacity = 0) {
    ADYOLO_REQUIRE(pcm && windows && audio, ADYOLO_EINVAL, "%s: null pointer", name);
    ADYOLO_REQUIRE(W > 0 && W < 65536 && n > 0 && n_total >= 0, ADYOLO_EINVAL, "%s: bad shape W=%d n=%ld n_total=%ld", name, W, n,
                   n_total);
    ADYOLO_REQUIRE(((uintptr_t)pcm & 15) == 0 && ((uintptr_t)audio & 15) == 0 && ((uintptr_t)windows & 7) == 0, ADYOLO_EINVAL,
                   "%s: misaligned buffers (pcm / audio 16 bytes, windows 8 bytes)", name);
    int gx = cdiv(n, 256L * 16);                            // the grid of adyolo_corpus_gather
    gx = gx < 1 ? 1 : (gx > 4096 ? 4096 : gx);
    if constexpr (RING) {
        ADYOLO_REQUIRE(capacity >= n && !(capacity & 1), ADYOLO_EINVAL, "%s: a ring of %ld frames for windows of %ld (even, >= n)",
                       name, capacity, n);
        hipLaunchKernelGGL((corpus_gather_windows_kernel<FORM, WindowRing>), dim3((unsigned)gx, (unsigned)W), dim3(256), 0,
                           as_stream(stream), pcm, n_total, windows, n, cs, comb_ok ? 1 : 0, (float4 *)audio, status,
                           WindowRing{capacity, n_total % capacity, 0});
        return check_launch(name);
    }
    hipLaunchKernelGGL(corpus_gather_windows_kernel<FORM>, dim3((unsigned)gx, (unsigned)W), dim3(256), 0, as_stream(stream), pcm,
                       n_total, windows, n, cs, comb_ok ? 1 : 0, (float4 *)audio, status);
    return check_launch(name);
}
}  // namespace adyolo

extern "C" int adyolo_corpus_gather_windows(const int16_t *pcm, long n_total, const int64_t *windows, int W, long n,
                                            float *audio, int *status, void *stream) {
    const CorpusSrc cs = {1.f, 1.f, 1.f, false, 0u, 0u, 1.f, 0.f};
    return corpus_gather_windows_launch<WINDOW_PLAIN>("corpus_gather_windows", pcm, n_total, windows, W, n, cs, true, audio,
                                                      status, stream);
}

extern "C" int adyolo_corpus_gather_windows_view(const int16_t *pcm, long n_total, const int64_t *windows, int W, long n,
                                                 int comb, const float *rot_host, const unsigned int *mic_src_host,
                                                 float *audio, int *status, void *stream) {
    const char *name = "corpus_gather_windows_view";
    ADYOLO_REQUIRE(rot_host || mic_src_host, ADYOLO_EINVAL, "%s: null pointer", name);
    ADYOLO_REQUIRE(comb < 16, ADYOLO_EINVAL, "%s: combination %d (at most 15)", name, comb);
    CorpusSrc cs = {1.f, 1.f, 1.f, false, 0u, 0u, 1.f, 0.f};
    if (comb <= 0)                                          // no view, or the identity: the plain gather's instance and bits
        return corpus_gather_windows_launch<WINDOW_PLAIN>(name, pcm, n_total, windows, W, n, cs, true, audio, status, stream);
    if (mic_src_host) {
        CorpusMicSrc tab;
        corpus_mic(mic_src_host, tab);
        const bool ok = gather_source(tab, comb, cs);
        return corpus_gather_windows_launch<WINDOW_MIC>(name, pcm, n_total, windows, W, n, cs, ok, audio, status, stream);
    }
    CorpusRot rot;
    corpus_rot(rot_host, rot);
    gather_source(rot, comb, cs);
    return corpus_gather_windows_launch<WINDOW_FOA>(name, pcm, n_total, windows, W, n, cs, true, audio, status, stream);
}

extern "C" int adyolo_stream_gather_windows(const int16_t *ring, long capacity, long head, const int64_t *windows, int W, long n,
                                            int comb, const float *rot_host, const unsigned int *mic_src_host, float *audio,
                                            int *status, void *stream) {
    const char *name = "stream_gather_windows";
    ADYOLO_REQUIRE(comb < 16, ADYOLO_EINVAL, "%s: combination %d (at most 15)", name, comb);
    ADYOLO_REQUIRE(comb <= 0 || rot_host || mic_src_host, ADYOLO_EINVAL, "%s: null pointer", name);
    CorpusSrc cs = {1.f, 1.f, 1.f, false, 0u, 0u, 1.f, 0.f};
    if (comb <= 0)                                          // no view, or the identity
        return corpus_gather_windows_launch<WINDOW_PLAIN, true>(name, ring, head, windows, W, n, cs, true, audio, status, stream,
                                                                capacity);
    if (mic_src_host) {
        CorpusMicSrc tab;
        corpus_mic(mic_src_host, tab);
        const bool ok = gather_source(tab, comb, cs);
        return corpus_gather_windows_launch<WINDOW_MIC, true>(name, ring, head, windows, W, n, cs, ok, audio, status, stream,
                                                              capacity);
    }
    CorpusRot rot;
    corpus_rot(rot_host, rot);
    gather_source(rot, comb, cs);
    return corpus_gather_windows_launch<WINDOW_FOA, true>(name, ring, head, windows, W, n, cs, true, audio, status, stream, capacity);
}

extern "C" int adyolo_decode_stitch(const float *decoded, const int64_t *windows, int W, int Wf, long rec, long pass_base,
                                    float *out, long out_frames, int *status, void *stream) {
    ADYOLO_REQUIRE(decoded && windows && out, ADYOLO_EINVAL, "decode_stitch: null pointer");
    ADYOLO_REQUIRE(W > 0 && W < 65536 && Wf > 0 && rec > 0 && out_frames > 0, ADYOLO_EINVAL,
                   "decode_stitch: bad shape W=%d Wf=%d rec=%ld out_frames=%ld", W, Wf, rec, out_frames);
    const bool vec = (rec & 3) == 0;
    ADYOLO_REQUIRE(((uintptr_t)decoded & (vec ? 15 : 3)) == 0 && ((uintptr_t)out & (vec ? 15 : 3)) == 0 &&
                       ((uintptr_t)windows & 7) == 0,
                   ADYOLO_EINVAL, "decode_stitch: misaligned buffers (decoded / out %d bytes, windows 8 bytes)", vec ? 16 : 4);
    // ~16 bytes x 4 per thread over one window's frames
    int gx = cdiv((long)Wf * rec, 256L * 16);
    gx = gx < 1 ? 1 : (gx > 1024 ? 1024 : gx);
    const dim3 grid((unsigned)gx, (unsigned)W);
    if (vec)
        hipLaunchKernelGGL(decode_stitch_kernel<true>, grid, dim3(256), 0, as_stream(stream), decoded, windows, Wf, rec, pass_base,
                           out, out_frames, status);
    else
        hipLaunchKernelGGL(decode_stitch_kernel<false>, grid, dim3(256), 0, as_stream(stream), decoded, windows, Wf, rec, pass_base,
                           out, out_frames, status);
    return check_launch("decode_stitch");
}
