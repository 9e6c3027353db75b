// conv_igemm_kernel (conv_igemm_kernel.h) for fp32 operands (parity mode, exact fp32 MFMA): 128 x 128 and
// 64 x 64 tiles, the narrow 128 x 32 (FWD / DGRAD) and 32 x 128 (WGRAD) tiles, and the ordered reduce of
// the deterministic split-K partials.
#include <algorithm>

#include "conv_igemm_kernel.h"

namespace {

// every instantiation the planner can ask for (conv_plan in conv_host.hip)
constexpr ConvEntry TABLE[] = {
    ES_IGEMM_TILE(float, MODE_FWD, 128, 128),   ES_IGEMM_TILE(float, MODE_FWD, 64, 64),
    ES_IGEMM_TILE(float, MODE_FWD, 128, 32),    ES_IGEMM_TILE(float, MODE_DGRAD, 128, 128),
    ES_IGEMM_TILE(float, MODE_DGRAD, 64, 64),   ES_IGEMM_TILE(float, MODE_DGRAD, 128, 32),
    ES_IGEMM_TILE(float, MODE_WGRAD, 128, 128), ES_IGEMM_TILE(float, MODE_WGRAD, 64, 64),
    ES_IGEMM_TILE(float, MODE_WGRAD, 32, 128),
};

__global__ void splitk_reduce_kernel(const float* __restrict__ ws, int splits, int64_t n, float* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float v = 0.f;
    for (int z = 0; z < splits; ++z) v += ws[z * n + i];
    out[i] = v;
  }
}

}  // namespace

int conv_igemm_f32_launch(const ConvPlan& p, const ConvArgs& a, hipStream_t st) { return conv_table_launch(TABLE, p, a, st); }

void splitk_reduce_launch(const float* ws, int splits, int64_t n, float* out, hipStream_t st) {
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, st, ws, splits, n, out);
}
