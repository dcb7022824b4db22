// K11: Adam, AdamW, SGD and gradient-norm clipping over one flat parameter buffer (all 6.68 M parameters live in one
// allocation, so one launch updates the whole model and one RCCL all-reduce covers all gradients).  The reference picks its
// optimizer by name (src/train.py:29-37) and clips with clip_grad_norm_(max_norm) (src/train.py:54); the arithmetic follows
// torch.optim's single-tensor paths.
//
// One optimizer step = up to three launches whose arguments never change from step to step (hipGraph-replayable):
//   grad_sumsq_kernel   (clipping only) partial sums of (g * grad_scale)^2 in float64, one per workgroup, fixed grid and order
//   optim_prep_kernel   one workgroup: step counter += 1; st[0..1] = bias corrections (Adam / AdamW) or the "first step" flag
//                       (SGD); st[2] = total_norm (fp32); st[3] = clip_coef = min(1, max_norm / (total_norm + 1e-6)) -- 1 when off
//   *_update_kernel     the update, grad_scale * st[3] folded into the gradient (exact when st[3] = 1: the unclipped step is
//                       the same kernel)
// There is one update kernel per rule, adam_update_kernel<DECOUPLED, FORM, EMA> and sgd_update_kernel<MOM, FORM, EMA>.  FORM
// says where an element's constants {rate, step size, decay, weight decay} come from, and nothing else differs between the
// forms -- the walk, the per-element arithmetic and the EMA are one piece of source, so the forms agree bit for bit:
//   FORM_ARG     the plain entry points: from the arguments
//   FORM_SCHED   the *_sched entry points: the rate from the device.  The prep kernel evaluates a closed-form schedule in double
//                from the counter and a host-written table (SCHED_* below), rounds it to float ONCE and from there treats it
//                exactly as the plain entry points treat their `lr` argument: a constant schedule gives the plain step's bits
//   FORM_GROUPS  the *_groups entry points: a scheduled form with a rate and a weight decay per parameter group, from a table in
//                LDS through a byte map of the buffer; a group's elements get the bits of FORM_SCHED run on them alone
// The scheduled forms can also keep an exponential moving average of the parameters in the update launch (template flag EMA:
// two more streams, none without it).
// The guarded steps (adyolo_*_step_guard_dev) always run the sum of squares; their prep kernel takes the step only if the fp32
// norm is finite and otherwise leaves the counter, st[0..1], sched_out and groups_out alone and says so in the guard record,
// which makes every workgroup of the update kernel return before its first access: a skipped attempt changes nothing, and
// since the counter did not tick, the next attempt is the step the skipped one would have been.
// The accumulating steps (adyolo_*_step_accum_dev; K micro-batches, one step): every call is a micro-step.  grad_accum_kernel
// adds the gradient into an accumulator laid out like it (the cycle's first call overwrites it), the prep kernel keeps the
// accumulation record and, on all but the cycle's last call, stops there and tells the update kernel to do the same; the last
// call is the step above with the accumulator as its gradient and grad_scale / K as its scale.  Which call of the cycle this
// is, is read from the record on the device: the launches and their arguments are the same for every micro-step.
// st is 4 floats of device scratch.  All streams move 16 bytes per lane per access (pointers 16-byte aligned, the n & 3 tail
// elements are done by workgroup 0); grids are capped and grid-stride.  Elements that are zero in parameter, gradient and state
// (the padding of dist.FlatParameters) stay zero in every kernel.
//
// Rounding is written in the source: adam_one and sgd_one switch floating-point contraction off and spell out every fused
// multiply-add they want, so the float4 body, the tail, and every (DECOUPLED, clipped or not) form round alike whatever the
// vectoriser does.
#include <math.h>
#include "common.hpp"

namespace adyolo {

constexpr int OX_THREADS = 256;
constexpr int OX_MAX_BLOCKS = 2048;      // update kernels: 8 workgroups per CU, grid-stride beyond
constexpr int OX_SUMSQ_BLOCKS = 1024;    // = the largest number of partials (8 KB of float64)

// sched_dev: the schedule table, float64, written by the host only (construction, load_state_dict, set_lr)
enum {
    SCHED_KIND = 0,         // SCHED_CONSTANT ... SCHED_COSINE
    SCHED_BASE = 1,         // base learning rate
    SCHED_EVERY = 2,        // steps per schedule unit: e = floor((t - 1) / every)
    SCHED_WARMUP = 3,       // W warm-up STEPS (0 = none)
    SCHED_START = 4,        // s: warm(t) = s + (1 - s) * min(t - 1, W) / W
    SCHED_GAMMA = 5,        // step / multistep / exponential
    SCHED_STEP_SIZE = 6,    // step
    SCHED_T_MAX = 7,        // cosine
    SCHED_ETA_MIN = 8,      // cosine
    SCHED_N_MILESTONES = 9, // multistep: how many of the 8 slots are used
    SCHED_MILESTONE0 = 10,  // .. 17
    SCHED_OFFSET = 18,      // t = device counter (after its increment) + this: the schedule's clock survives a resume
    SCHED_EMA_DECAY = 19,
    SCHED_EMA_WARMUP = 20,  // != 0: decay_eff = min(decay, (1 + k) / (10 + k))
    SCHED_EMA_OFFSET = 21,  // k = device counter (after its increment) - 1 + this: EMA updates so far
    SCHED_TABLE_DOUBLES = 24
};
enum { SCHED_CONSTANT = 0, SCHED_STEP = 1, SCHED_MULTISTEP = 2, SCHED_EXPONENTIAL = 3, SCHED_COSINE = 4 };
// sched_out: what the prep kernel derives for this step, float32
enum { SOUT_LR = 0, SOUT_DECAY = 1, SOUT_EMA_W = 2, SOUT_EMA_FIRST = 3, SCHED_OUT_FLOATS = 4 };
// Parameter groups (the *_groups entry points).  groups_dev: float64 (G, 2) {base rate, weight_decay}, written by the host
// only.  groups_out: float32 (G, 4), what the prep kernel derives per group for this step.  The group map holds one byte per
// element of the buffer: the element's group.
enum { GOUT_LR = 0, GOUT_STEP = 1, GOUT_DECAY = 2, GOUT_WD = 3, GROUP_OUT_FLOATS = 4 };
constexpr int OX_MAX_GROUPS = 16;

static inline int update_grid(long n) {
    long g = ((n >> 2) + OX_THREADS - 1) / OX_THREADS;
    return (int)(g < 1 ? 1 : (g > OX_MAX_BLOCKS ? OX_MAX_BLOCKS : g));
}

static inline int sumsq_grid(long n) {
    long g = ((n >> 2) + OX_THREADS - 1) / OX_THREADS;
    return (int)(g < 1 ? 1 : (g > OX_SUMSQ_BLOCKS ? OX_SUMSQ_BLOCKS : g));
}

static inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---------------------------------------------------------------------------------------------- gradient norm
__global__ __launch_bounds__(OX_THREADS) void grad_sumsq_kernel(const float *__restrict__ g, long n, float grad_scale,
                                                                double *__restrict__ partials) {
    __shared__ double red[OX_THREADS / 64];
    const long n4 = n >> 2;
    const float4 *g4 = reinterpret_cast<const float4 *>(g);
    double s = 0.0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const float4 v = g4[i];
        const double a = (double)(v.x * grad_scale), b = (double)(v.y * grad_scale);
        const double c = (double)(v.z * grad_scale), d = (double)(v.w * grad_scale);
        s += (a * a + b * b) + (c * c + d * d);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const double a = (double)(g[n4 * 4 + threadIdx.x] * grad_scale);
        s += a * a;
    }
    // fixed order: butterfly inside the wave, then the four waves one after the other
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ---------------------------------------------------------------------------------------------- gradient accumulation
// The accumulation record (the *_accum entry points): four int64 written only by the prep kernel, by one lane.  ACC_MICRO is
// the index inside its cycle of the NEXT call (0 .. accum_steps - 1); ACC_HOLD says that the last call was not its cycle's last.
enum { ACC_MICRO = 0, ACC_CALLS = 1, ACC_CYCLES = 2, ACC_HOLD = 3, ACC_WORDS = 4 };

// accum = g on a cycle's first micro-step (accum is not read: whatever a discarded cycle left there is gone), else accum + g.
// On the cycle's last micro-step, with partials != nullptr, also the partial sums of (accum * grad_scale)^2 that
// grad_sumsq_kernel would give on the finished accumulator: it is launched on that kernel's grid, a lane walks the same
// vectors and sums the same expressions in the same order, and the reduction is the same.  The micro index is grid-uniform
// and read before the first load; the prep kernel, which alone writes it, runs after this kernel in the stream.
__global__ __launch_bounds__(OX_THREADS) void grad_accum_kernel(const float *__restrict__ g, float *__restrict__ accum, long n,
                                                                float grad_scale, double *__restrict__ partials,
                                                                const long long *__restrict__ acc, int accum_steps) {
    __shared__ double red[OX_THREADS / 64];
    const long long micro = acc[ACC_MICRO];
    const bool first = micro == 0;
    const bool sum = partials != nullptr && micro + 1 >= accum_steps;
    const long n4 = n >> 2;
    const float4 *g4 = reinterpret_cast<const float4 *>(g);
    float4 *a4 = reinterpret_cast<float4 *>(accum);
    double s = 0.0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        float4 v = g4[i];
        if (!first) {
            const float4 o = a4[i];
            v.x = o.x + v.x;
            v.y = o.y + v.y;
            v.z = o.z + v.z;
            v.w = o.w + v.w;
        }
        a4[i] = v;
        if (sum) {
            const double a = (double)(v.x * grad_scale), b = (double)(v.y * grad_scale);
            const double c = (double)(v.z * grad_scale), d = (double)(v.w * grad_scale);
            s += (a * a + b * b) + (c * c + d * d);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long i = n4 * 4 + threadIdx.x;
        float v = g[i];
        if (!first) v = accum[i] + v;
        accum[i] = v;
        if (sum) {
            const double a = (double)(v * grad_scale);
            s += a * a;
        }
    }
    if (!sum) return;                      // (grid-uniform)
    // fixed order: butterfly inside the wave, then the four waves one after the other
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ---------------------------------------------------------------------------------------------- prep
enum { PREP_ADAM = 0, PREP_SGD = 1, PREP_NORM = 2 };

// lr(t) = base * warm(t) * main(e) in double, rounded to float once; t = 1 runs at the base rate (torch's convention when
// scheduler.step() follows optimizer.step()).  base: tb[SCHED_BASE], or a parameter group's own base rate.
__device__ static float sched_lr(const double *__restrict__ tb, unsigned long long step, double base) {
    const double t = (double)step + tb[SCHED_OFFSET];
    const double W = tb[SCHED_WARMUP], s0 = tb[SCHED_START];
    const double e = floor((t - 1.0) / tb[SCHED_EVERY]);
    const double warm = W > 0.0 ? s0 + (1.0 - s0) * fmin(t - 1.0, W) / W : 1.0;
    double main_f = 1.0;
    switch ((int)tb[SCHED_KIND]) {
    case SCHED_STEP: main_f = pow(tb[SCHED_GAMMA], floor(e / tb[SCHED_STEP_SIZE])); break;
    case SCHED_MULTISTEP: {
        int hit = 0;
        const int nm = (int)tb[SCHED_N_MILESTONES];
        for (int i = 0; i < nm && i < 8; ++i) hit += tb[SCHED_MILESTONE0 + i] <= e ? 1 : 0;
        main_f = pow(tb[SCHED_GAMMA], (double)hit);
        break;
    }
    case SCHED_EXPONENTIAL: main_f = pow(tb[SCHED_GAMMA], e); break;
    case SCHED_COSINE: {    // torch's closed form, held at eta_min after T_max
        const double T = tb[SCHED_T_MAX], lo = tb[SCHED_ETA_MIN];
        main_f = (lo + (base - lo) * (1.0 + cos(M_PI * fmin(e, T) / T)) / 2.0) / base;
        break;
    }
    default: break;
    }
    return (float)(base * warm * main_f);
}

// The guard record (the *_guard entry points): four int64 written only by the prep kernel, by one lane.
enum { GUARD_ATTEMPTS = 0, GUARD_SKIPPED = 1, GUARD_LAST = 2, GUARD_RUN = 3, GUARD_WORDS = 4 };

// What one lane of the prep kernel does for a step that is taken: the counter += 1 and everything derived from it.
// sched != nullptr (the *_sched entry points): `lr` is ignored, the step's rate comes from the table and is written with
// AdamW's decay and the EMA's weight to sched_out.
// groups != nullptr (the *_groups entry points, which are scheduled forms): the rate is derived once per group from the group's
// own base (a base of exactly 0 gives 0 without the closed form: cosine divides by the base) and written with what the update
// needs to groups_out; `wd` is ignored, st[0] and sched_out keep group 0's values.
// (Inlined at both of its places in the prep kernel: as a function of its own it costs the kernel a call stack in scratch.)
__device__ __forceinline__ void prep_tick(unsigned long long *__restrict__ step, float *__restrict__ st, int kind, float lr,
                                          float beta1, float beta2, const double *__restrict__ sched,
                                          float *__restrict__ sched_out, float wd, const double *__restrict__ groups,
                                          float *__restrict__ groups_out, int n_groups) {
    const unsigned long long s = *step + 1ull;
    *step = s;
    if (groups != nullptr) {
        const double bc1 = kind == PREP_ADAM ? 1.0 - pow((double)beta1, (double)s) : 1.0;
        for (int k = n_groups - 1; k >= 0; --k) {          // group 0 last: lr and wd leave the loop as group 0's
            const double base = groups[2 * k];
            wd = (float)groups[2 * k + 1];
            lr = base == 0.0 ? 0.f : sched_lr(sched, s, base);
            float *go = groups_out + GROUP_OUT_FLOATS * k;
            go[GOUT_LR] = lr;
            go[GOUT_STEP] = kind == PREP_ADAM ? (float)((double)lr / bc1) : lr;
            go[GOUT_DECAY] = (float)(1.0 - (double)lr * (double)wd);
            go[GOUT_WD] = wd;
        }
        if (kind != PREP_ADAM) wd = 0.f;                   // sched_out's decay is AdamW's: sgd_step passes no wd either
    }
    if (sched != nullptr) {
        if (groups == nullptr) lr = sched_lr(sched, s, sched[SCHED_BASE]);
        const double k = (double)s - 1.0 + sched[SCHED_EMA_OFFSET];       // EMA updates so far
        double keep = sched[SCHED_EMA_DECAY];
        if (sched[SCHED_EMA_WARMUP] != 0.0) keep = fmin(keep, (1.0 + k) / (10.0 + k));
        sched_out[SOUT_LR] = lr;
        sched_out[SOUT_DECAY] = (float)(1.0 - (double)lr * (double)wd);
        sched_out[SOUT_EMA_W] = (float)(1.0 - keep);
        sched_out[SOUT_EMA_FIRST] = k <= 0.0 ? 1.f : 0.f;
    }
    if (kind == PREP_ADAM) {           // {lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)} in double like torch's host arithmetic
        const double bc1 = 1.0 - pow((double)beta1, (double)s);
        const double bc2 = 1.0 - pow((double)beta2, (double)s);
        st[0] = (float)((double)lr / bc1);
        st[1] = (float)(1.0 / sqrt(bc2));
    } else {                           // SGD: the momentum buffer is INITIALISED by the first step (no dampening)
        st[0] = s == 1ull ? 1.f : 0.f;
        st[1] = 0.f;
    }
}

// one workgroup of OX_THREADS.  partials == nullptr: clipping off (st[3] = 1, st[2] untouched).  PREP_NORM: no counter, norm only.
// guard != nullptr (the *_guard entry points; partials is then never null): the partials are reduced FIRST and the step is
// taken only if the fp32 norm is finite.  A skipped step writes st[2] (the offending norm) and the record and nothing else:
// the counter does not tick, so nothing derived from it (bias corrections, the schedule's clock, the EMA's update count and
// first-copy flag, SGD's first-step flag) sees the attempt.  A taken step is the unguarded one, value for value; a negative
// max_norm means clipping off there (st[3] = exactly 1, not max_norm = inf: inf / inf is nan).
// acc != nullptr (the *_accum entry points): the accumulation record is advanced FIRST.  On a hold call -- not the last of its
// cycle -- that is all: no tick, no guard record, no st.  The cycle's last call goes on as above, guard included.
__global__ __launch_bounds__(OX_THREADS) void optim_prep_kernel(unsigned long long *__restrict__ step, float *__restrict__ st,
                                                                int kind, float lr, float beta1, float beta2,
                                                                const double *__restrict__ partials, int nparts,
                                                                float max_norm, const double *__restrict__ sched,
                                                                float *__restrict__ sched_out, float wd,
                                                                const double *__restrict__ groups,
                                                                float *__restrict__ groups_out, int n_groups,
                                                                long long *__restrict__ guard, long long *__restrict__ acc,
                                                                int accum_steps) {
    __shared__ double red[OX_THREADS];
    if (acc != nullptr) {                  // (uniform over the workgroup)
        const long long micro = acc[ACC_MICRO];
        const bool hold = micro + 1 < accum_steps;
        __syncthreads();                   // every lane has read the index before one lane moves it
        if (threadIdx.x == 0) {
            acc[ACC_MICRO] = hold ? micro + 1 : 0;
            acc[ACC_CALLS] = acc[ACC_CALLS] + 1;
            acc[ACC_CYCLES] = acc[ACC_CYCLES] + (hold ? 0 : 1);
            acc[ACC_HOLD] = hold ? 1 : 0;
        }
        if (hold) return;
    }
    if (threadIdx.x == 0 && kind != PREP_NORM && guard == nullptr)
        prep_tick(step, st, kind, lr, beta1, beta2, sched, sched_out, wd, groups, groups_out, n_groups);
    if (partials == nullptr) {             // (uniform over the workgroup)
        if (threadIdx.x == 0) st[3] = 1.f;
        return;
    }
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += OX_THREADS) s += partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int o = OX_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        // torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1; fp32; without the guard a
        // non-finite norm is not special-cased (inf -> 0, nan -> nan)
        const float total = (float)sqrt(red[0]);
        float coef = max_norm / (total + 1e-6f);
        if (guard != nullptr) {
            const bool skip = !isfinite(total);
            guard[GUARD_ATTEMPTS] = guard[GUARD_ATTEMPTS] + 1;
            guard[GUARD_SKIPPED] = guard[GUARD_SKIPPED] + (skip ? 1 : 0);
            guard[GUARD_LAST] = skip ? 1 : 0;
            guard[GUARD_RUN] = skip ? guard[GUARD_RUN] + 1 : 0;
            if (skip) {
                st[2] = total;
                return;
            }
            prep_tick(step, st, kind, lr, beta1, beta2, sched, sched_out, wd, groups, groups_out, n_groups);
            if (max_norm < 0.f) coef = 1.f;
        }
        st[2] = total;
        st[3] = coef > 1.f ? 1.f : coef;
    }
}

// ---------------------------------------------------------------------------------------------- what the update kernels share
// An element's constants travel as one float4 in groups_out's layout {rate, step size, decay, weight decay} (GOUT_*): built
// once per lane from arguments, st and sched_out in FORM_ARG and FORM_SCHED (wave-uniform; no LDS, no barrier), fetched per
// vector or per element from the LDS copy of groups_out in FORM_GROUPS.
enum { FORM_ARG = 0, FORM_SCHED = 1, FORM_GROUPS = 2 };

// The guarded step (guard != nullptr): the prep kernel's verdict on this attempt.  Grid-uniform, and asked before the first
// load, store or barrier of an update kernel: a skipped step's update launch touches nothing.
// The accumulating step (acc != nullptr) asks the same way whether this call is a hold call of its cycle.
__device__ __forceinline__ bool skipped(const long long *__restrict__ guard, const long long *__restrict__ acc) {
    if (acc != nullptr && acc[ACC_HOLD] != 0) return true;
    return guard != nullptr && guard[GUARD_LAST] != 0;
}

// FORM_GROUPS: groups_out goes to LDS once per workgroup (rows past n_groups: rate 0, decay 1); the other forms have no table.
template <int FORM>
__device__ __forceinline__ const float4 *group_table(const float *__restrict__ groups_out, int n_groups) {
    if constexpr (FORM == FORM_GROUPS) {
        __shared__ float4 tab[OX_MAX_GROUPS];
        if (threadIdx.x < OX_MAX_GROUPS)
            tab[threadIdx.x] = (int)threadIdx.x < n_groups ? reinterpret_cast<const float4 *>(groups_out)[threadIdx.x]
                                                           : make_float4(0.f, 0.f, 1.f, 0.f);
        __syncthreads();
        return tab;
    } else {
        return nullptr;
    }
}

// A lane reads the map as one 32-bit word per float4 and, where its four bytes agree (parameters are long runs: almost always),
// fetches one set of constants, else one per element.  Indices are masked: no map value reads outside the table.
__device__ __forceinline__ bool one_group(unsigned w) { return w == (w & 0xffu) * 0x01010101u; }

// the constants of the element whose map byte is the low byte of `byte`: the group's row, or the lane's own set `cu` where
// there are no groups (and no table)
template <int FORM>
__device__ __forceinline__ float4 consts(const float4 *tab, unsigned byte, const float4 &cu) {
    if constexpr (FORM == FORM_GROUPS) return tab[byte & (OX_MAX_GROUPS - 1)];
    else return cu;
}

// The moving average of the parameters, after p is formed: a copy on its first update (the old value is not read), else
// ema += (p - ema) * w as one fused multiply-add.
__device__ __forceinline__ void ema_one(float &a, float p, float w, bool first) {
#pragma clang fp contract(off)
    a = first ? p : __builtin_fmaf(p - a, w, a);
}

// The EMA of vector i and of tail element i: a third read-write stream laid out like p.
__device__ __forceinline__ void ema_four(float4 *__restrict__ e4, long i, const float4 &pv, float w, bool first) {
    float4 ev = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!first) ev = e4[i];
    ema_one(ev.x, pv.x, w, first);
    ema_one(ev.y, pv.y, w, first);
    ema_one(ev.z, pv.z, w, first);
    ema_one(ev.w, pv.w, w, first);
    e4[i] = ev;
}

__device__ __forceinline__ void ema_tail(float *__restrict__ ema, long i, float p, float w, bool first) {
    float ev = first ? 0.f : ema[i];
    ema_one(ev, p, w, first);
    ema[i] = ev;
}

// ---------------------------------------------------------------------------------------------- Adam / AdamW update
// torch.optim.Adam:  m += (g - m)(1 - b1);  v = b2 v + (1 - b2) g^2;  p -= lr/(1 - b1^t) * m / (sqrt(v)/sqrt(1 - b2^t) + eps)
// DECOUPLED = false: weight decay added to the gradient.
// DECOUPLED = true:  torch.optim.AdamW: p *= 1 - lr * wd (`decay`, formed on the host in double) before the moments.
// Exactly three operations are fused (m, the denominator, the parameter); gi and v round after every multiply and add.
template <bool DECOUPLED>
__device__ __forceinline__ void adam_one(float &p, float g, float &m, float &v, float gs, float beta1, float beta2, float eps,
                                         float wd, float decay, float step_size, float inv_sqrt_bc2) {
#pragma clang fp contract(off)
    float gi = g * gs;
    float pi = p;
    if (wd != 0.f) {
        if (DECOUPLED) pi = pi * decay;
        else gi = gi + wd * pi;
    }
    m = __builtin_fmaf(gi - m, 1.f - beta1, m);
    v = v * beta2 + ((1.f - beta2) * gi) * gi;
    p = __builtin_fmaf(-step_size, m / __builtin_fmaf(sqrtf(v), inv_sqrt_bc2, eps), pi);
}

// the four elements of a vector, each with its own constants
template <bool DECOUPLED>
__device__ __forceinline__ void adam_four(float4 &pv, const float4 &gv, float4 &mv, float4 &vv, float gs, float beta1,
                                          float beta2, float eps, float inv_sqrt_bc2, const float4 &c0, const float4 &c1,
                                          const float4 &c2, const float4 &c3) {
    adam_one<DECOUPLED>(pv.x, gv.x, mv.x, vv.x, gs, beta1, beta2, eps, c0.w, c0.z, c0.y, inv_sqrt_bc2);
    adam_one<DECOUPLED>(pv.y, gv.y, mv.y, vv.y, gs, beta1, beta2, eps, c1.w, c1.z, c1.y, inv_sqrt_bc2);
    adam_one<DECOUPLED>(pv.z, gv.z, mv.z, vv.z, gs, beta1, beta2, eps, c2.w, c2.z, c2.y, inv_sqrt_bc2);
    adam_one<DECOUPLED>(pv.w, gv.w, mv.w, vv.w, gs, beta1, beta2, eps, c3.w, c3.z, c3.y, inv_sqrt_bc2);
}

// FORM_ARG: wd and decay are the arguments, the step size is st[0].  FORM_SCHED: decay is so[SOUT_DECAY] (the prep kernel
// formed it from this step's rate); the rate itself is already inside st[0].  FORM_GROUPS: all three from the group's row.
template <bool DECOUPLED, int FORM, bool EMA>
__global__ __launch_bounds__(OX_THREADS) void adam_update_kernel(float *__restrict__ p, const float *__restrict__ g,
                                                                 float *__restrict__ m, float *__restrict__ v, long n,
                                                                 float beta1, float beta2, float eps, float wd, float decay,
                                                                 float grad_scale, const float *__restrict__ st,
                                                                 const float *__restrict__ so, float *__restrict__ ema,
                                                                 const float *__restrict__ groups_out, int n_groups,
                                                                 const unsigned char *__restrict__ map,
                                                                 const long long *__restrict__ guard,
                                                                 const long long *__restrict__ acc) {
    static_assert(FORM != FORM_ARG || !EMA, "the EMA belongs to the scheduled forms");
    if (skipped(guard, acc)) return;
    const float4 *tab = group_table<FORM>(groups_out, n_groups);
    float4 cu = make_float4(0.f, 0.f, 0.f, 0.f);          // the lane's constants; FORM_GROUPS: unused
    if constexpr (FORM == FORM_SCHED) decay = so[SOUT_DECAY];
    if constexpr (FORM != FORM_GROUPS) cu = make_float4(0.f, st[0], decay, wd);
    const float inv_sqrt_bc2 = st[1];
    const float gs = grad_scale * st[3];
    const float ew = EMA ? so[SOUT_EMA_W] : 0.f;
    const bool efirst = EMA && so[SOUT_EMA_FIRST] != 0.f;
    const long n4 = n >> 2;
    float4 *p4 = reinterpret_cast<float4 *>(p), *m4 = reinterpret_cast<float4 *>(m), *v4 = reinterpret_cast<float4 *>(v);
    float4 *e4 = reinterpret_cast<float4 *>(ema);
    const float4 *g4 = reinterpret_cast<const float4 *>(g);
    const unsigned *map4 = reinterpret_cast<const unsigned *>(map);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        unsigned w = 0;                            // without groups: one group, and `w` is not read
        if constexpr (FORM == FORM_GROUPS) w = map4[i];
        float4 pv = p4[i], mv = m4[i], vv = v4[i];
        const float4 gv = g4[i];
        if (one_group(w)) {                        // always, without groups
            const float4 c = consts<FORM>(tab, w, cu);
            adam_four<DECOUPLED>(pv, gv, mv, vv, gs, beta1, beta2, eps, inv_sqrt_bc2, c, c, c, c);
        } else {
            adam_four<DECOUPLED>(pv, gv, mv, vv, gs, beta1, beta2, eps, inv_sqrt_bc2, consts<FORM>(tab, w, cu),
                                 consts<FORM>(tab, w >> 8, cu), consts<FORM>(tab, w >> 16, cu), consts<FORM>(tab, w >> 24, cu));
        }
        p4[i] = pv;
        m4[i] = mv;
        v4[i] = vv;
        if (EMA) ema_four(e4, i, pv, ew, efirst);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long i = n4 * 4 + threadIdx.x;
        unsigned w = 0;
        if constexpr (FORM == FORM_GROUPS) w = map[i];
        const float4 c = consts<FORM>(tab, w, cu);
        adam_one<DECOUPLED>(p[i], g[i], m[i], v[i], gs, beta1, beta2, eps, c.w, c.z, c.y, inv_sqrt_bc2);
        if (EMA) ema_tail(ema, i, p[i], ew, efirst);
    }
}

// ---------------------------------------------------------------------------------------------- SGD update
// torch.optim.SGD, single-tensor path: g' = g * gs + wd * p;  MOM: buf = g' on the first step (st[0] != 0), else
// buf = mu * buf + (1 - dampening) * g';  d = nesterov ? g' + mu * buf : buf;  p += -lr * d.  !MOM: buf is never touched.
// Every multiply-add is fused except mu * buf, which rounds before (1 - dampening) * g' is fused onto it.
template <bool MOM>
__device__ __forceinline__ void sgd_one(float &p, float g, float *buf, float gs, float lr, float wd, float mu, float keep,
                                        bool nesterov, bool first) {
#pragma clang fp contract(off)
    float gi = g * gs;
    const float pi = p;
    if (wd != 0.f) gi = __builtin_fmaf(wd, pi, gi);
    if (MOM) {
        const float bi = first ? gi : __builtin_fmaf(keep, gi, mu * *buf);
        *buf = bi;
        gi = nesterov ? __builtin_fmaf(mu, bi, gi) : bi;
    }
    p = __builtin_fmaf(-lr, gi, pi);
}

// the four elements of a vector, each with its own constants
template <bool MOM>
__device__ __forceinline__ void sgd_four(float4 &pv, const float4 &gv, float4 &bv, float gs, float mu, float keep, bool nest,
                                         bool first, const float4 &c0, const float4 &c1, const float4 &c2, const float4 &c3) {
    sgd_one<MOM>(pv.x, gv.x, &bv.x, gs, c0.x, c0.w, mu, keep, nest, first);
    sgd_one<MOM>(pv.y, gv.y, &bv.y, gs, c1.x, c1.w, mu, keep, nest, first);
    sgd_one<MOM>(pv.z, gv.z, &bv.z, gs, c2.x, c2.w, mu, keep, nest, first);
    sgd_one<MOM>(pv.w, gv.w, &bv.w, gs, c3.x, c3.w, mu, keep, nest, first);
}

// FORM_ARG: lr and wd are the arguments.  FORM_SCHED: lr is so[SOUT_LR].  FORM_GROUPS: both from the group's row.
template <bool MOM, int FORM, bool EMA>
__global__ __launch_bounds__(OX_THREADS) void sgd_update_kernel(float *__restrict__ p, const float *__restrict__ g,
                                                                float *__restrict__ buf, long n, float lr, float wd, float mu,
                                                                float keep, int nesterov, float grad_scale,
                                                                const float *__restrict__ st, const float *__restrict__ so,
                                                                float *__restrict__ ema, const float *__restrict__ groups_out,
                                                                int n_groups, const unsigned char *__restrict__ map,
                                                                const long long *__restrict__ guard,
                                                                const long long *__restrict__ acc) {
    static_assert(FORM != FORM_ARG || !EMA, "the EMA belongs to the scheduled forms");
    if (skipped(guard, acc)) return;
    const float4 *tab = group_table<FORM>(groups_out, n_groups);
    float4 cu = make_float4(0.f, 0.f, 0.f, 0.f);          // the lane's constants; FORM_GROUPS: unused
    if constexpr (FORM == FORM_SCHED) lr = so[SOUT_LR];
    if constexpr (FORM != FORM_GROUPS) cu = make_float4(lr, 0.f, 0.f, wd);
    const bool first = st[0] != 0.f, nest = nesterov != 0;
    const float gs = grad_scale * st[3];
    const float ew = EMA ? so[SOUT_EMA_W] : 0.f;
    const bool efirst = EMA && so[SOUT_EMA_FIRST] != 0.f;
    const long n4 = n >> 2;
    float4 *p4 = reinterpret_cast<float4 *>(p), *b4 = reinterpret_cast<float4 *>(buf);
    float4 *e4 = reinterpret_cast<float4 *>(ema);
    const float4 *g4 = reinterpret_cast<const float4 *>(g);
    const unsigned *map4 = reinterpret_cast<const unsigned *>(map);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        unsigned w = 0;                            // without groups: one group, and `w` is not read
        if constexpr (FORM == FORM_GROUPS) w = map4[i];
        float4 pv = p4[i];
        const float4 gv = g4[i];
        float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (MOM && !first) bv = b4[i];
        if (one_group(w)) {                        // always, without groups
            const float4 c = consts<FORM>(tab, w, cu);
            sgd_four<MOM>(pv, gv, bv, gs, mu, keep, nest, first, c, c, c, c);
        } else {
            sgd_four<MOM>(pv, gv, bv, gs, mu, keep, nest, first, consts<FORM>(tab, w, cu), consts<FORM>(tab, w >> 8, cu),
                          consts<FORM>(tab, w >> 16, cu), consts<FORM>(tab, w >> 24, cu));
        }
        p4[i] = pv;
        if (MOM) b4[i] = bv;
        if (EMA) ema_four(e4, i, pv, ew, efirst);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long i = n4 * 4 + threadIdx.x;
        unsigned w = 0;
        if constexpr (FORM == FORM_GROUPS) w = map[i];
        const float4 c = consts<FORM>(tab, w, cu);
        sgd_one<MOM>(p[i], g[i], MOM ? buf + i : nullptr, gs, c.x, c.w, mu, keep, nest, first);
        if (EMA) ema_tail(ema, i, p[i], ew, efirst);
    }
}

static int launch_sumsq(const float *grad, long n, float grad_scale, double *partials, hipStream_t st) {
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(sumsq_grid(n)), dim3(OX_THREADS), 0, st, grad, n, grad_scale, partials);
    return check_launch("grad_sumsq");
}

static int launch_accum(const float *grad, float *accum, long n, float grad_scale, double *partials, const int64_t *acc,
                        int accum_steps, hipStream_t st) {
    hipLaunchKernelGGL(grad_accum_kernel, dim3(sumsq_grid(n)), dim3(OX_THREADS), 0, st, grad, accum, n, grad_scale, partials,
                       reinterpret_cast<const long long *>(acc), accum_steps);
    return check_launch("grad_accum");
}

static int launch_prep(uint64_t *step_dev, float *st_dev, int kind, float lr, float beta1, float beta2, const double *partials,
                       long n, float max_norm, hipStream_t st, const double *sched = nullptr, float *sched_out = nullptr,
                       float wd = 0.f, const double *groups = nullptr, float *groups_out = nullptr, int n_groups = 0,
                       int64_t *guard = nullptr, int64_t *acc = nullptr, int accum_steps = 1) {
    hipLaunchKernelGGL(optim_prep_kernel, dim3(1), dim3(OX_THREADS), 0, st, reinterpret_cast<unsigned long long *>(step_dev),
                       st_dev, kind, lr, beta1, beta2, partials, partials ? sumsq_grid(n) : 0, max_norm, sched, sched_out, wd,
                       groups, groups_out, n_groups, reinterpret_cast<long long *>(guard), reinterpret_cast<long long *>(acc),
                       accum_steps);
    return check_launch("optim_prep");
}

// What a step's entry point adds to the plain form: all null in FORM_ARG; the table, sched_out and (optionally) the EMA in
// FORM_SCHED and FORM_GROUPS; the groups in FORM_GROUPS.  guard: the record of the *_guard entry points, null elsewhere.
// acc, accum, accum_steps: the record, the accumulator and K of the *_accum entry points, null elsewhere.
struct StepForm {
    int form;
    const double *sched;
    float *sched_out, *ema;
    const double *groups;
    float *groups_out;
    int n_groups;
    const unsigned char *map;
    int64_t *guard;
    int64_t *acc;
    float *accum;
    int accum_steps;
};

// The front of a step: the sum of squares of the gradient (clipping or the guard), or, in the accumulating step, the
// micro-gradient into the accumulator (with the sum on the cycle's last call) -- the step then reads the accumulator under
// grad_scale / accum_steps.
static int step_front(const float *&grad, float &grad_scale, long n, double *partials, const StepForm &f, hipStream_t st) {
    if (f.acc == nullptr) return partials ? launch_sumsq(grad, n, grad_scale, partials, st) : 0;
    grad_scale = (float)((double)grad_scale / f.accum_steps);
    const int rc = launch_accum(grad, f.accum, n, grad_scale, partials, f.acc, f.accum_steps, st);
    grad = f.accum;
    return rc;
}

// a kernel's five instantiations (for one value of its first template parameter) are kept in the order of this index
static int form_index(const StepForm &f) {
    switch (f.form) {
    case FORM_GROUPS: return f.ema ? 4 : 3;
    case FORM_SCHED: return f.ema ? 2 : 1;
    default: return 0;
    }
}

template <bool DECOUPLED>
static auto adam_kernel(const StepForm &f) {
    decltype(&adam_update_kernel<DECOUPLED, FORM_ARG, false>) const five[5] = {
        adam_update_kernel<DECOUPLED, FORM_ARG, false>, adam_update_kernel<DECOUPLED, FORM_SCHED, false>,
        adam_update_kernel<DECOUPLED, FORM_SCHED, true>, adam_update_kernel<DECOUPLED, FORM_GROUPS, false>,
        adam_update_kernel<DECOUPLED, FORM_GROUPS, true>};
    return five[form_index(f)];
}

template <bool MOM>
static auto sgd_kernel(const StepForm &f) {
    decltype(&sgd_update_kernel<MOM, FORM_ARG, false>) const five[5] = {
        sgd_update_kernel<MOM, FORM_ARG, false>, sgd_update_kernel<MOM, FORM_SCHED, false>,
        sgd_update_kernel<MOM, FORM_SCHED, true>, sgd_update_kernel<MOM, FORM_GROUPS, false>,
        sgd_update_kernel<MOM, FORM_GROUPS, true>};
    return five[form_index(f)];
}

// The argument checks of the step entry points; `what` is the entry point's name.  present / aligned: what the rule says
// about its own buffers (parameters, gradient, state, counter, scratch); the form's buffers are checked here.
static int check_step(const char *what, bool present, bool aligned, long n, const StepForm &f) {
    const bool sched = f.form != FORM_ARG;
    ADYOLO_REQUIRE(present && n > 0 && (!sched || (f.sched && f.sched_out)), ADYOLO_EINVAL, "%s: bad arguments", what);
    ADYOLO_REQUIRE(aligned && aligned16(f.ema) && (reinterpret_cast<uintptr_t>(f.sched) & 7) == 0, ADYOLO_EINVAL,
                   "%s: buffers not 16-byte aligned%s", what, sched ? " (or the table not 8-byte aligned)" : "");
    ADYOLO_REQUIRE(f.form != FORM_GROUPS ||
                       (f.groups && f.groups_out && f.map && f.n_groups >= 1 && f.n_groups <= OX_MAX_GROUPS &&
                        (reinterpret_cast<uintptr_t>(f.groups) & 7) == 0 && aligned16(f.groups_out) &&
                        (reinterpret_cast<uintptr_t>(f.map) & 3) == 0),
                   ADYOLO_EINVAL, "%s: 1 to 16 groups, groups_dev 8-byte, groups_out 16-byte and the map 4-byte aligned", what);
    ADYOLO_REQUIRE((reinterpret_cast<uintptr_t>(f.guard) & 7) == 0, ADYOLO_EINVAL, "%s: the guard record not 8-byte aligned", what);
    ADYOLO_REQUIRE((reinterpret_cast<uintptr_t>(f.acc) & 7) == 0 && aligned16(f.accum), ADYOLO_EINVAL,
                   "%s: the accumulator not 16-byte aligned (or the accumulation record not 8-byte aligned)", what);
    return 0;
}

// the Adam / AdamW step behind its entry points: check, sum of squares (clipping only), prep, update.  FORM_ARG: lr is
// the argument (and decay formed from it here); else lr is ignored, and in FORM_GROUPS weight_decay too
static int adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long n, float lr, float beta1,
                     float beta2, float eps, float weight_decay, int decoupled, uint64_t *step_dev, float *st_dev,
                     double *partials, float max_norm, float grad_scale, const StepForm &f, hipStream_t st, const char *what) {
    int rc;
    if ((rc = check_step(what, param && grad && exp_avg && exp_avg_sq && step_dev && st_dev,
                         aligned16(param) && aligned16(grad) && aligned16(exp_avg) && aligned16(exp_avg_sq), n, f)))
        return rc;
    if ((rc = step_front(grad, grad_scale, n, partials, f, st))) return rc;
    if ((rc = launch_prep(step_dev, st_dev, PREP_ADAM, lr, beta1, beta2, partials, n, max_norm, st, f.sched, f.sched_out,
                          weight_decay, f.groups, f.groups_out, f.n_groups, f.guard, f.acc, f.accum_steps)))
        return rc;
    const float decay = (float)(1.0 - (double)lr * (double)weight_decay);
    auto kernel = decoupled ? adam_kernel<true>(f) : adam_kernel<false>(f);
    hipLaunchKernelGGL(kernel, dim3(update_grid(n)), dim3(OX_THREADS), 0, st, param, grad, exp_avg, exp_avg_sq, n, beta1, beta2,
                       eps, weight_decay, decay, grad_scale, (const float *)st_dev, (const float *)f.sched_out, f.ema,
                       (const float *)f.groups_out, f.n_groups, f.map, (const long long *)f.guard,
                       (const long long *)f.acc);
    return check_launch(what);
}

static int sgd_step(float *param, const float *grad, float *momentum_buf, long n, float lr, float weight_decay, float momentum,
                    float dampening, int nesterov, uint64_t *step_dev, float *st_dev, double *partials, float max_norm,
                    float grad_scale, const StepForm &f, hipStream_t st, const char *what) {
    int rc;
    if ((rc = check_step(what, param && grad && step_dev && st_dev && (momentum == 0.f || momentum_buf),
                         aligned16(param) && aligned16(grad) && aligned16(momentum_buf), n, f)))
        return rc;
    if ((rc = step_front(grad, grad_scale, n, partials, f, st))) return rc;
    if ((rc = launch_prep(step_dev, st_dev, PREP_SGD, lr, 0.f, 0.f, partials, n, max_norm, st, f.sched, f.sched_out, 0.f,
                          f.groups, f.groups_out, f.n_groups, f.guard, f.acc, f.accum_steps)))
        return rc;
    const float keep = (float)(1.0 - (double)dampening);
    const bool mom = momentum != 0.f;
    auto kernel = mom ? sgd_kernel<true>(f) : sgd_kernel<false>(f);
    hipLaunchKernelGGL(kernel, dim3(update_grid(n)), dim3(OX_THREADS), 0, st, param, grad, mom ? momentum_buf : (float *)nullptr,
                       n, lr, weight_decay, mom ? momentum : 0.f, keep, nesterov, grad_scale, (const float *)st_dev,
                       (const float *)f.sched_out, f.ema, (const float *)f.groups_out, f.n_groups, f.map,
                       (const long long *)f.guard, (const long long *)f.acc);
    return check_launch(what);
}

}  // namespace adyolo

using namespace adyolo;

extern "C" long adyolo_grad_sumsq_parts(long n) { return n > 0 ? sumsq_grid(n) : 0; }

extern "C" int adyolo_grad_sumsq(const float *grad, long n, float grad_scale, double *partials, void *stream) {
    ADYOLO_REQUIRE(grad && partials && n > 0, ADYOLO_EINVAL, "grad_sumsq: bad arguments");
    ADYOLO_REQUIRE(aligned16(grad) && (reinterpret_cast<uintptr_t>(partials) & 7) == 0, ADYOLO_EINVAL,
                   "grad_sumsq: gradient not 16-byte aligned (or partials not 8-byte aligned)");
    return launch_sumsq(grad, n, grad_scale, partials, as_stream(stream));
}

extern "C" int adyolo_grad_norm_dev(const float *grad, long n, float grad_scale, double *partials, float max_norm, float *st_dev,
                                    void *stream) {
    ADYOLO_REQUIRE(st_dev, ADYOLO_EINVAL, "grad_norm_dev: null scratch");
    int rc = adyolo_grad_sumsq(grad, n, grad_scale, partials, stream);
    if (rc) return rc;
    return launch_prep(nullptr, st_dev, PREP_NORM, 0.f, 0.f, 0.f, partials, n, max_norm, as_stream(stream));
}

extern "C" int adyolo_adam_step_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long n, float lr,
                                    float beta1, float beta2, float eps, float weight_decay, int decoupled, uint64_t *step_dev,
                                    float *st_dev, double *partials, float max_norm, float grad_scale, void *stream) {
    return adam_step(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, decoupled, step_dev, st_dev,
                     partials, max_norm, grad_scale, StepForm{FORM_ARG}, as_stream(stream), "adam_step_dev");
}

extern "C" int adyolo_sgd_step_dev(float *param, const float *grad, float *momentum_buf, long n, float lr, float weight_decay,
                                   float momentum, float dampening, int nesterov, uint64_t *step_dev, float *st_dev,
                                   double *partials, float max_norm, float grad_scale, void *stream) {
    return sgd_step(param, grad, momentum_buf, n, lr, weight_decay, momentum, dampening, nesterov, step_dev, st_dev, partials,
                    max_norm, grad_scale, StepForm{FORM_ARG}, as_stream(stream), "sgd_step_dev");
}

extern "C" int adyolo_sched_table_doubles(void) { return SCHED_TABLE_DOUBLES; }
extern "C" int adyolo_sched_out_floats(void) { return SCHED_OUT_FLOATS; }

extern "C" int adyolo_adam_step_sched_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long n,
                                          float beta1, float beta2, float eps, float weight_decay, int decoupled,
                                          uint64_t *step_dev, float *st_dev, double *partials, float max_norm,
                                          float grad_scale, const double *sched_dev, float *sched_out, float *ema,
                                          void *stream) {
    return adam_step(param, grad, exp_avg, exp_avg_sq, n, 0.f, beta1, beta2, eps, weight_decay, decoupled, step_dev, st_dev,
                     partials, max_norm, grad_scale, StepForm{FORM_SCHED, sched_dev, sched_out, ema}, as_stream(stream),
                     "adam_step_sched_dev");
}

extern "C" int adyolo_sgd_step_sched_dev(float *param, const float *grad, float *momentum_buf, long n, float weight_decay,
                                         float momentum, float dampening, int nesterov, uint64_t *step_dev, float *st_dev,
                                         double *partials, float max_norm, float grad_scale, const double *sched_dev,
                                         float *sched_out, float *ema, void *stream) {
    return sgd_step(param, grad, momentum_buf, n, 0.f, weight_decay, momentum, dampening, nesterov, step_dev, st_dev, partials,
                    max_norm, grad_scale, StepForm{FORM_SCHED, sched_dev, sched_out, ema}, as_stream(stream),
                    "sgd_step_sched_dev");
}

extern "C" int adyolo_optim_max_groups(void) { return OX_MAX_GROUPS; }

extern "C" int adyolo_adam_step_groups_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long n,
                                           float beta1, float beta2, float eps, int decoupled, uint64_t *step_dev,
                                           float *st_dev, double *partials, float max_norm, float grad_scale,
                                           const double *sched_dev, float *sched_out, float *ema, const double *groups_dev,
                                           float *groups_out, int n_groups, const unsigned char *group_map, void *stream) {
    return adam_step(param, grad, exp_avg, exp_avg_sq, n, 0.f, beta1, beta2, eps, 0.f, decoupled, step_dev, st_dev, partials,
                     max_norm, grad_scale,
                     StepForm{FORM_GROUPS, sched_dev, sched_out, ema, groups_dev, groups_out, n_groups, group_map},
                     as_stream(stream), "adam_step_groups_dev");
}

extern "C" int adyolo_sgd_step_groups_dev(float *param, const float *grad, float *momentum_buf, long n, float momentum,
                                          float dampening, int nesterov, uint64_t *step_dev, float *st_dev, double *partials,
                                          float max_norm, float grad_scale, const double *sched_dev, float *sched_out,
                                          float *ema, const double *groups_dev, float *groups_out, int n_groups,
                                          const unsigned char *group_map, void *stream) {
    return sgd_step(param, grad, momentum_buf, n, 0.f, 0.f, momentum, dampening, nesterov, step_dev, st_dev, partials, max_norm,
                    grad_scale, StepForm{FORM_GROUPS, sched_dev, sched_out, ema, groups_dev, groups_out, n_groups, group_map},
                    as_stream(stream), "sgd_step_groups_dev");
}

// The guarded steps: one entry point per rule.  The form is read from the pointers -- groups_dev: grouped (lr and
// weight_decay ignored); else sched_dev: scheduled (lr ignored); else plain (ema must be null) -- and handed to the same
// adam_step / sgd_step.  The sum of squares always runs (partials is required); max_norm < 0: no clipping.
extern "C" int adyolo_optim_guard_words(void) { return GUARD_WORDS; }

static int guard_form(const char *what, const double *sched_dev, float *sched_out, float *ema, const double *groups_dev,
                      float *groups_out, int n_groups, const unsigned char *group_map, int64_t *guard, const double *partials,
                      StepForm *f, bool guard_optional = false) {
    ADYOLO_REQUIRE((guard && partials) || (guard_optional && !guard), ADYOLO_EINVAL,
                   "%s: needs the guard record and the partials", what);
    ADYOLO_REQUIRE(sched_dev || (!groups_dev && !ema), ADYOLO_EINVAL, "%s: groups and the EMA need a schedule table", what);
    const int form = groups_dev ? FORM_GROUPS : (sched_dev ? FORM_SCHED : FORM_ARG);
    *f = StepForm{form, sched_dev, sched_out, ema};
    if (form == FORM_GROUPS) *f = StepForm{form, sched_dev, sched_out, ema, groups_dev, groups_out, n_groups, group_map};
    f->guard = guard;
    return 0;
}

extern "C" int adyolo_adam_step_guard_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long n, float lr,
                                          float beta1, float beta2, float eps, float weight_decay, int decoupled,
                                          uint64_t *step_dev, float *st_dev, double *partials, float max_norm,
                                          float grad_scale, const double *sched_dev, float *sched_out, float *ema,
                                          const double *groups_dev, float *groups_out, int n_groups,
                                          const unsigned char *group_map, int64_t *guard, void *stream) {
    StepForm f;
    int rc = guard_form("adam_step_guard_dev", sched_dev, sched_out, ema, groups_dev, groups_out, n_groups, group_map, guard,
                        partials, &f);
    if (rc) return rc;
    return adam_step(param, grad, exp_avg, exp_avg_sq, n, f.form == FORM_ARG ? lr : 0.f, beta1, beta2, eps,
                     f.form == FORM_GROUPS ? 0.f : weight_decay, decoupled, step_dev, st_dev, partials, max_norm, grad_scale, f,
                     as_stream(stream), "adam_step_guard_dev");
}

extern "C" int adyolo_sgd_step_guard_dev(float *param, const float *grad, float *momentum_buf, long n, float lr,
                                         float weight_decay, float momentum, float dampening, int nesterov, uint64_t *step_dev,
                                         float *st_dev, double *partials, float max_norm, float grad_scale,
                                         const double *sched_dev, float *sched_out, float *ema, const double *groups_dev,
                                         float *groups_out, int n_groups, const unsigned char *group_map, int64_t *guard,
                                         void *stream) {
    StepForm f;
    int rc = guard_form("sgd_step_guard_dev", sched_dev, sched_out, ema, groups_dev, groups_out, n_groups, group_map, guard,
                        partials, &f);
    if (rc) return rc;
    return sgd_step(param, grad, momentum_buf, n, f.form == FORM_ARG ? lr : 0.f, f.form == FORM_GROUPS ? 0.f : weight_decay,
                    momentum, dampening, nesterov, step_dev, st_dev, partials, max_norm, grad_scale, f, as_stream(stream),
                    "sgd_step_guard_dev");
}

// The accumulating steps: one entry point per rule, the guarded entry point's arguments with the guard optional (null:
// unguarded, and partials null: no clipping, as in the unguarded entry points) and then the accumulator, the accumulation
// record and K.  K = 1 makes every call a cycle of its own: the step of the form's own entry point on a copy of the gradient.
extern "C" int adyolo_optim_accum_words(void) { return ACC_WORDS; }

static int accum_form(const char *what, float *accum, int64_t *accum_dev, int accum_steps, StepForm *f) {
    ADYOLO_REQUIRE(accum && accum_dev, ADYOLO_EINVAL, "%s: needs the accumulator and the accumulation record", what);
    ADYOLO_REQUIRE(accum_steps >= 1, ADYOLO_EINVAL, "%s: accum_steps %d, must be at least 1", what, accum_steps);
    f->acc = accum_dev;
    f->accum = accum;
    f->accum_steps = accum_steps;
    return 0;
}

extern "C" int adyolo_adam_step_accum_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long n, float lr,
                                          float beta1, float beta2, float eps, float weight_decay, int decoupled,
                                          uint64_t *step_dev, float *st_dev, double *partials, float max_norm,
                                          float grad_scale, const double *sched_dev, float *sched_out, float *ema,
                                          const double *groups_dev, float *groups_out, int n_groups,
                                          const unsigned char *group_map, int64_t *guard, float *accum, int64_t *accum_dev,
                                          int accum_steps, void *stream) {
    StepForm f;
    int rc = guard_form("adam_step_accum_dev", sched_dev, sched_out, ema, groups_dev, groups_out, n_groups, group_map, guard,
                        partials, &f, true);
    if (rc || (rc = accum_form("adam_step_accum_dev", accum, accum_dev, accum_steps, &f))) return rc;
    return adam_step(param, grad, exp_avg, exp_avg_sq, n, f.form == FORM_ARG ? lr : 0.f, beta1, beta2, eps,
                     f.form == FORM_GROUPS ? 0.f : weight_decay, decoupled, step_dev, st_dev, partials, max_norm, grad_scale, f,
                     as_stream(stream), "adam_step_accum_dev");
}

extern "C" int adyolo_sgd_step_accum_dev(float *param, const float *grad, float *momentum_buf, long n, float lr,
                                         float weight_decay, float momentum, float dampening, int nesterov, uint64_t *step_dev,
                                         float *st_dev, double *partials, float max_norm, float grad_scale,
                                         const double *sched_dev, float *sched_out, float *ema, const double *groups_dev,
                                         float *groups_out, int n_groups, const unsigned char *group_map, int64_t *guard,
                                         float *accum, int64_t *accum_dev, int accum_steps, void *stream) {
    StepForm f;
    int rc = guard_form("sgd_step_accum_dev", sched_dev, sched_out, ema, groups_dev, groups_out, n_groups, group_map, guard,
                        partials, &f, true);
    if (rc || (rc = accum_form("sgd_step_accum_dev", accum, accum_dev, accum_steps, &f))) return rc;
    return sgd_step(param, grad, momentum_buf, n, f.form == FORM_ARG ? lr : 0.f, f.form == FORM_GROUPS ? 0.f : weight_decay,
                    momentum, dampening, nesterov, step_dev, st_dev, partials, max_norm, grad_scale, f, as_stream(stream),
                    "sgd_step_accum_dev");
}
