// launcher interface of the persistent F(4x4,3x3) kernels (wino4p.hpp), shared with the dispatcher in wino4.hip
#pragma once
#include "common.hpp"

namespace adyolo {
namespace w4 {

struct W4Launch {                                         // everything adyolo_wino4_fwd hands to a launcher
    const float *x, *u, *bias, *addend, *addend_mask, *in_scale, *in_shift;
    float *y, *stats;
    const float *stat_aux, *stat_mean, *stat_invstd, *stat_mask;
    int H, W, Cin, Cout, patchesW, patchesH, nsp, ncb, xcd_div, relu, mask_bits, tc, grid, nb;
    hipStream_t st;
};
// EPI: the operand bits of include/adyolo_hip.h (ADYOLO_W4_STATS ... ADYOLO_W4_STAT_MASK).  Compile-time, one translation unit per
// value (wino4p_e<EPI>.hip): the register allocation of a 512-register kernel does not survive run-time operand combinations
// (conditionally loaded operand arrays were merged through scratch memory).
template <int EPI>
void launch_wino4p(const W4Launch &a);

// THE list of operand combinations the persistent kernel is built for: the ones the SE-ResNet block launches (functional.py) -- 0
// plain, 1 forward convolutions, 9 data-gradient of conv2, 2 / 27 / 31 data-gradient of conv1 (projection shortcut after a pooled /
// un-pooled stage boundary, identity shortcut), 15 the same for the first block (statistics against the stem's BatchNorm input: no
// mask).  Every other combination, a bias, and masks given as float tensors take the one-patch kernel.  The dispatcher's membership
// test and its switch are both generated from this list (wino4p_launcher, wino4.hip).  A new entry needs its wino4p_e<EPI>.hip
// (and build.SOURCES); without it the library does not load (undefined symbol launch_wino4p<EPI>).
#define ADYOLO_W4P_BUILT(X) X(0) X(1) X(2) X(9) X(15) X(27) X(31)

#ifndef W4P_BRES
#define W4P_BRES 1        // 1: 32 -> 32 layers take the resident-U form of the kernel (BRES, wino4p.hpp), 0: the B ring as everywhere else
#endif
#ifndef W4P_MKDEDUP
#define W4P_MKDEDUP 1     // 1: the epilogue's ReLU-mask bit loads shared between the pixels of a row segment where Cout allows (32 / 64 / 128)
#endif
#ifndef W4P_FULL
#define W4P_FULL 1        // 1: 32 -> 32 layers with operand sets 15 / 27 / 31 request both halves of the next patch's input lines together
#endif

// THE choice of the persistent kernel's instantiation wino4p_fwd_kernel<TC, AFF, EPI, NB, BRES, FULL, MKM> for a launch:
// launch_wino4p<EPI> (wino4p.hpp) dispatches on what this returns and adyolo_conv_fwd_plan reports it.  Host arithmetic only.
struct W4Variant {
    int tc, aff, nb, bres, full, mkm;
};
inline W4Variant wino4p_variant(int epi, int tc, int nb, int W, int Cin, int Cout, bool affine, int mask_bits) {
    // narrow maps (W <= 8: the middle stages of the ResNet-Conformer): patches one or two tiles wide, plain launches only
    if (epi == 0 && (tc == 1 || tc == 2)) return {tc, 0, 2, 0, 0, 0};
    const bool e3 = epi == 15 || epi == 27 || epi == 31;
    if (e3) {
        // shared ReLU-mask words (MKM): the three shapes the SE-ResNet's data gradients have, bits for every mask that is given
        const int need = ((epi & 4) ? 1 : 0) | ((epi & 16) ? 2 : 0);
        const bool mkshare = W4P_MKDEDUP && (W & 3) == 0 && !affine && (mask_bits & need) == need;
        if (mkshare && nb == 2 && tc == 8 && Cout == 64) return {8, 0, 2, 0, 0, 2};
        // (Cout = 128, two 8-byte words per component and row segment -- MKM 3 -- measured 0.5-2.9 % SLOWER than the dwords and is
        //  not instantiated: profiles/r06_w4p_mkdedup_ab.txt)
        if (mkshare && nb == 1 && tc == 8 && Cout == 32 && Cin == 32 && W4P_FULL) return {8, 0, 1, 0, 1, 1};
    }
    if (nb == 1 && Cin == 32) {
        // 32 -> 32 layers.  Operand sets 15 / 27 / 31: whole input lines at once (resident U does not fit: 20-46 spilled registers
        // and 6-14 % slower, profiles/r06_w4p_bres_ab.txt).  Data gradients carry no producer affine; a launch that does takes
        // the B-ring form, which is the one the affine variants are checked in.
        if (W4P_FULL && e3 && !affine) return {tc, 0, 1, 0, 1, 0};
        // the others: the resident-U form, where the epilogue leaves it the registers
        if (W4P_BRES && (epi == 0 || epi == 1 || epi == 2 || epi == 9)) return {tc, affine ? 1 : 0, 1, 1, 0, 0};
    }
    return {tc, affine ? 1 : 0, nb, 0, 0, 0};
}

// The geometry of an adyolo_wino4_fwd launch (wino4.hip: wino4_fwd_geometry, the one function the launcher and the plan call)
struct W4Geometry {
    int form;                                             // adyolo_wino4_fwd_form: 2 persistent, 1 one-patch, 0 refused
    int narrow, tc, tr, patchesW, patchesH, nsp, nb, ncb, xcd_div, blocks, slots;      // blocks: the grid; slots: persistent only
};

}  // namespace w4
}  // namespace adyolo
