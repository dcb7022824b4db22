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

}  // namespace w4
}  // namespace adyolo
