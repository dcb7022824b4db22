// The link stage's kernel, written once and compiled twice by track.hip: TRK_CARRY 0 is track_link_kernel (adyolo_track_rows:
// one wave per (clip, class), the text and the code of the whole-clip form as they were); TRK_CARRY 1 is track_link_run_kernel
// (adyolo_track_run: one wave per (segment, class)).  The carried form takes row blockIdx.x / C of the segment table {first
// frame in the run, frames, continues, open} (checked by track_run_plan_kernel: win[2]), and its grid has `hold` frames in
// front of the run's.  A continuing segment starts from the carry (`cin`, the plan kernel's copy): lane k loads slot k's track
// and writes slot k's held cells in front of the segment's frames, at t < 0 -- an index that wraps as (size_t) and lands
// where the signed one would -- where the gap fill and the erasure then reach them like any other cell.  An open segment ends by
// storing its slots, next_id and its last held frames' cells into `cout` instead of closing.
#if TRK_CARRY
// grid: one wave per (segment, class); grid has hold + run_frames frames, ncand's rows n_frames = run_frames
__global__ __launch_bounds__(TRK_WAVE) void track_link_run_kernel(const float *__restrict__ cand, const int *__restrict__ ncand,
                                                                 f32x4 *__restrict__ grid, long n_frames, int C, float cos_g,
                                                                 int max_gap, int min_len, float a, float b,
                                                                 int *__restrict__ status, const int *__restrict__ segs,
                                                                 const int *__restrict__ win, const float *__restrict__ cin,
                                                                 float *__restrict__ cout, int hold) {
#else
// grid: one wave per (clip, class)
__global__ __launch_bounds__(TRK_WAVE) void track_link_kernel(const float *__restrict__ cand, const int *__restrict__ ncand,
                                                             f32x4 *__restrict__ grid, long n_frames, int t_clip, int C,
                                                             float cos_g, int max_gap, int min_len, float a, float b,
                                                             int *__restrict__ status) {
#endif
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    const long clip = blockIdx.x / C;
    const int c = (int)(blockIdx.x - clip * C);
#if TRK_CARRY
    if (win[2] == 0) return;                                     // a refused table or carry: nothing is linked or emitted
    const int *sg = segs + clip * 4;
    const long f0 = sg[0];
    const int t_clip = sg[1];
    const bool cont = sg[2] != 0, open = sg[3] != 0;
    grid += (size_t)hold * C * TRK_SLOTS;                        // the held frames lie in front of the run's: frames t < 0
#else
    const long f0 = clip * t_clip;
#endif
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
#if TRK_CARRY
    int walked = 0;                                               // the recording's frames before t = 0
    bool bad = false;
    if (cont) {
        const int *head = reinterpret_cast<const int *>(cin) + c * TRK_HEAD_WORDS;
        next_id = head[0], walked = head[1];
        const int held = head[2];                                 // (the plan kernel checked: min(hold, walked))
        if (lane < TRK_SLOTS) {
            const int *sl = reinterpret_cast<const int *>(cin) + C * TRK_HEAD_WORDS + (c * TRK_SLOTS + lane) * TRK_SLOT_WORDS;
            occ = sl[0] != 0, id = sl[1], first = sl[2] - walked, last = sl[3] - walked, hits = sl[4];
            sx = __int_as_float(sl[5]), sy = __int_as_float(sl[6]), sz = __int_as_float(sl[7]);
            // a track no run leaves behind (it would write in front of the held frames) is dropped and reported
            if (occ && !(first <= last && last < 0 && first >= -walked && hits >= 1 && (hits >= min_len || first >= -held)))
                occ = false, bad = true;
            const f32x4 *src = reinterpret_cast<const f32x4 *>(cin + (size_t)C * (TRK_HEAD_WORDS + TRK_SLOTS * TRK_SLOT_WORDS)) +
                               (size_t)c * TRK_SLOTS + lane;
            for (int j = hold - held; j < hold; ++j) cells[(size_t)(j - hold) * cell_step] = src[(size_t)j * cell_step];
        }
    }
#endif
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
#if TRK_CARRY
    if (__ballot(bad) && lane == 0) atomicOr(status, ADYOLO_TRACK_BAD_ROWS);
    if (open) {
        // the recording goes on: the slots, next_id and the held frames' cells are the carry.  (The cells of a silent block
        // were written by other lanes than the slot's own: the fence orders those stores before this lane reads them back.)
        __threadfence_block();
        walked += t_clip;
        const int held = walked < hold ? walked : hold;
        if (lane < TRK_SLOTS) {
            int *sl = reinterpret_cast<int *>(cout) + C * TRK_HEAD_WORDS + (c * TRK_SLOTS + lane) * TRK_SLOT_WORDS;
            sl[0] = occ, sl[1] = id, sl[2] = first + (walked - t_clip), sl[3] = last + (walked - t_clip), sl[4] = hits;
            sl[5] = __float_as_int(sx), sl[6] = __float_as_int(sy), sl[7] = __float_as_int(sz);
            f32x4 *dst = reinterpret_cast<f32x4 *>(cout + (size_t)C * (TRK_HEAD_WORDS + TRK_SLOTS * TRK_SLOT_WORDS)) +
                         (size_t)c * TRK_SLOTS + lane;
            for (int j = hold - held; j < hold; ++j) dst[(size_t)j * cell_step] = cells[(size_t)(t_clip - hold + j) * cell_step];
        }
        if (lane == 0) {
            int *head = reinterpret_cast<int *>(cout) + c * TRK_HEAD_WORDS;
            head[0] = next_id, head[1] = walked, head[2] = held, head[3] = 0;
        }
        occ = false;                                              // nothing is closed below
    } else if (clip == gridDim.x / C - 1) {                       // the run ends with its last recording: an empty carry
        int *w = reinterpret_cast<int *>(cout);
        if (lane < TRK_SLOTS) w[C * TRK_HEAD_WORDS + (c * TRK_SLOTS + lane) * TRK_SLOT_WORDS] = 0;
        if (lane < TRK_HEAD_WORDS) w[c * TRK_HEAD_WORDS + lane] = 0;
    }
#endif
    // the clip's end closes every slot
    if (occ && hits < min_len)
        for (int f = first; f <= last; ++f) cells[(size_t)f * cell_step] = empty;
    if (__ballot(bits != 0) && lane == 0) atomicOr(status, ADYOLO_TRACK_SLOT_OVERFLOW);
}
