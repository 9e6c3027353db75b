// conv_ring_kernel (conv_ring_kernel.h) for fp32 operands, on 32-channel K-steps.  Exact fp32 arithmetic
// (v_mfma_f32_16x16x4_f32; es_conv_set_f32_split(0)): the tiles of the bf16 file, no affine epilogue (the
// exact ring declines it and the caller runs the norm pass).  Split-fp32 on pre-split weight planes
// (SPL = 2): 128 / 256 x 64 / 128 tiles (256 x 256 does not fit the LDS), FWD also with the epilogue.
#include "conv_ring_kernel.h"

// every instantiation the planner can ask for (ring_plan in conv_ring_host.hip)
static constexpr ConvRingEntry TABLE[] = {
    ring_entry<MODE_FWD, 128, 64, false, 64, float, 0>(), ring_entry<MODE_FWD, 128, 64, true, 64, float, 0>(),
    ring_entry<MODE_FWD, 128, 128, false, 64, float, 0>(), ring_entry<MODE_FWD, 128, 128, true, 64, float, 0>(),
    ring_entry<MODE_FWD, 256, 64, false, 64, float, 0>(), ring_entry<MODE_FWD, 256, 64, true, 64, float, 0>(),
    ring_entry<MODE_FWD, 256, 128, false, 64, float, 0>(), ring_entry<MODE_FWD, 256, 128, true, 64, float, 0>(),
    ring_entry<MODE_FWD, 256, 256, true, 32, float, 0>(), ring_entry<MODE_DGRAD, 128, 64, false, 64, float, 0>(),
    ring_entry<MODE_DGRAD, 128, 64, true, 64, float, 0>(), ring_entry<MODE_DGRAD, 128, 128, false, 64, float, 0>(),
    ring_entry<MODE_DGRAD, 128, 128, true, 64, float, 0>(), ring_entry<MODE_DGRAD, 256, 64, false, 64, float, 0>(),
    ring_entry<MODE_DGRAD, 256, 64, true, 64, float, 0>(), ring_entry<MODE_DGRAD, 256, 128, false, 64, float, 0>(),
    ring_entry<MODE_DGRAD, 256, 128, true, 64, float, 0>(), ring_entry<MODE_DGRAD, 256, 256, false, 32, float, 0>(),
    ring_entry<MODE_DGRAD, 256, 256, true, 32, float, 0>(),
    ring_entry<MODE_FWD, 128, 64, false, 64, float, 2>(), ring_entry<MODE_FWD, 128, 64, false, 64, float, 2, true>(),
    ring_entry<MODE_FWD, 128, 64, true, 64, float, 2>(), ring_entry<MODE_FWD, 128, 64, true, 64, float, 2, true>(),
    ring_entry<MODE_FWD, 128, 128, false, 64, float, 2>(), ring_entry<MODE_FWD, 128, 128, false, 64, float, 2, true>(),
    ring_entry<MODE_FWD, 128, 128, true, 64, float, 2>(), ring_entry<MODE_FWD, 128, 128, true, 64, float, 2, true>(),
    ring_entry<MODE_FWD, 256, 64, false, 64, float, 2>(), ring_entry<MODE_FWD, 256, 64, false, 64, float, 2, true>(),
    ring_entry<MODE_FWD, 256, 64, true, 64, float, 2>(), ring_entry<MODE_FWD, 256, 64, true, 64, float, 2, true>(),
    ring_entry<MODE_FWD, 256, 128, false, 64, float, 2>(), ring_entry<MODE_FWD, 256, 128, false, 64, float, 2, true>(),
    ring_entry<MODE_FWD, 256, 128, true, 64, float, 2>(), ring_entry<MODE_FWD, 256, 128, true, 64, float, 2, true>(),
    ring_entry<MODE_DGRAD, 128, 64, false, 64, float, 2>(), ring_entry<MODE_DGRAD, 128, 64, true, 64, float, 2>(),
    ring_entry<MODE_DGRAD, 128, 128, false, 64, float, 2>(), ring_entry<MODE_DGRAD, 128, 128, true, 64, float, 2>(),
    ring_entry<MODE_DGRAD, 256, 64, false, 64, float, 2>(), ring_entry<MODE_DGRAD, 256, 64, true, 64, float, 2>(),
    ring_entry<MODE_DGRAD, 256, 128, false, 64, float, 2>(), ring_entry<MODE_DGRAD, 256, 128, true, 64, float, 2>(),
};

bool conv_ring_f32_launch(const RingPlan& p, const ConvArgs& a, hipStream_t st) { return ring_table_launch(TABLE, p, a, st); }
