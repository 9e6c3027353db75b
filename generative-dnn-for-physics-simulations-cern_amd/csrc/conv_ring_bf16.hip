// conv_ring_kernel (conv_ring_kernel.h) for bf16 operands: 128 / 256 x 64 / 128 tiles of 64-channel
// K-steps, the 256 x 256 tiles of 32-channel K-steps (sub-pixel FWD, merged or not, and DGRAD), and the
// FWD instantiations with the affine + activation epilogue.  A plain 256 x 256 FWD is not built: the
// planner takes 256 x 256 tiles for sub-pixel FWD and DGRAD only (it spills registers).
#include "conv_ring_kernel.h"

// every instantiation the planner can ask for (ring_plan in conv_ring_host.hip)
static constexpr ConvRingEntry TABLE[] = {
    ring_entry<MODE_FWD, 128, 64, false, 64, bf16, 0>(), ring_entry<MODE_FWD, 128, 64, false, 64, bf16, 0, true>(),
    ring_entry<MODE_FWD, 128, 64, true, 64, bf16, 0>(), ring_entry<MODE_FWD, 128, 64, true, 64, bf16, 0, true>(),
    ring_entry<MODE_FWD, 128, 128, false, 64, bf16, 0>(), ring_entry<MODE_FWD, 128, 128, false, 64, bf16, 0, true>(),
    ring_entry<MODE_FWD, 128, 128, true, 64, bf16, 0>(), ring_entry<MODE_FWD, 128, 128, true, 64, bf16, 0, true>(),
    ring_entry<MODE_FWD, 256, 64, false, 64, bf16, 0>(), ring_entry<MODE_FWD, 256, 64, false, 64, bf16, 0, true>(),
    ring_entry<MODE_FWD, 256, 64, true, 64, bf16, 0>(), ring_entry<MODE_FWD, 256, 64, true, 64, bf16, 0, true>(),
    ring_entry<MODE_FWD, 256, 128, false, 64, bf16, 0>(), ring_entry<MODE_FWD, 256, 128, false, 64, bf16, 0, true>(),
    ring_entry<MODE_FWD, 256, 128, true, 64, bf16, 0>(), ring_entry<MODE_FWD, 256, 128, true, 64, bf16, 0, true>(),
    ring_entry<MODE_FWD, 256, 256, true, 32, bf16, 0>(), ring_entry<MODE_FWD, 256, 256, true, 32, bf16, 0, true>(),
    ring_entry<MODE_DGRAD, 128, 64, false, 64, bf16, 0>(), ring_entry<MODE_DGRAD, 128, 64, true, 64, bf16, 0>(),
    ring_entry<MODE_DGRAD, 128, 128, false, 64, bf16, 0>(), ring_entry<MODE_DGRAD, 128, 128, true, 64, bf16, 0>(),
    ring_entry<MODE_DGRAD, 256, 64, false, 64, bf16, 0>(), ring_entry<MODE_DGRAD, 256, 64, true, 64, bf16, 0>(),
    ring_entry<MODE_DGRAD, 256, 128, false, 64, bf16, 0>(), ring_entry<MODE_DGRAD, 256, 128, true, 64, bf16, 0>(),
    ring_entry<MODE_DGRAD, 256, 256, false, 32, bf16, 0>(), ring_entry<MODE_DGRAD, 256, 256, true, 32, bf16, 0>(),
};

bool conv_ring_bf16_launch(const RingPlan& p, const ConvArgs& a, hipStream_t st) { return ring_table_launch(TABLE, p, a, st); }
