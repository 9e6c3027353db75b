// conv_igemm_kernel (conv_igemm_kernel.h) for bf16 operands: 128 x 128 and 64 x 64 tiles, and the bf16-only
// 4-wave kernels with LDS-DMA staging, conv_glds_kernel (FWD / DGRAD) and conv_wgrad_glds_kernel.
#include "conv_igemm_kernel.h"

namespace {

// ---------------------------------------------------------------------------------------------
// bf16 FWD / DGRAD with LDS-DMA staging (global_load_lds_dwordx4).
//
// Used when every K-step (64 bf16) is ONE filter tap over 64 contiguous channels (C % 64 == 0 for
// FWD, K % 64 == 0 for DGRAD), so each GEMM row of a K-step is one contiguous 128-byte segment of
// an NHWC activation row (or all zero: padding / outside the image / stride-2 holes).
//   * A wave instruction moves 8 rows x 128 B straight into LDS (no register round trip); lanes
//     of padded rows read a 16-byte-aligned zero block instead.
//   * LDS image per operand: [rows][128 B] unpadded; logical 16-byte chunk lc of row r sits at
//     physical chunk lc ^ ((r >> 1) & 7) (the swizzle is applied on the global source address,
//     since the DMA destination is lane-linear), which makes the 16-row ds_read_b128 fragment
//     reads conflict-free.
//   * Two stages; one barrier per K-step: wait(stage t) + barrier, issue stage t+1, MFMAs on t.
//   * Block ids are remapped so that consecutive M tiles run on the same XCD (shared halo rows
//     stay in that XCD's L2).
// ---------------------------------------------------------------------------------------------
__device__ __attribute__((aligned(16))) char g_zero_row[128];   // zero-initialised at load

__device__ __forceinline__ void glds16(const void* src, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

__device__ __forceinline__ int swz(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

template <int RM, int RN>
__device__ __forceinline__ void mma_kstep_swz(const char* As, const char* Bs, int wm0, int wn0,
                                              f32x4 (&acc)[RM][RN]) {
  const int lane = threadIdx.x & 63;
  const int r16 = lane & 15, g = lane >> 4;
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const int seg = kk * 4 + g;
    bf16x8 af[RM], bfr[RN];
#pragma unroll
    for (int i = 0; i < RM; ++i) af[i] = *(const bf16x8*)(As + swz(wm0 + i * 16 + r16, seg));
#pragma unroll
    for (int j = 0; j < RN; ++j) bfr[j] = *(const bf16x8*)(Bs + swz(wn0 + j * 16 + r16, seg));
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int j = 0; j < RN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
  }
}

template <int MODE, int BM, int BN>
__global__ void __launch_bounds__(NTHREADS) conv_glds_kernel(ConvArgs a) {
  constexpr int RM = BM / 32, RN = BN / 32;
  constexpr int AI = BM / 32, BI = BN / 32;            // 8-row DMA pieces per wave (4 waves)
  constexpr int ABYTES = BM * 128, STAGE = (BM + BN) * 128;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const es_conv_desc_t& d = a.d;
  conv_live_gemm(a, MODE);

  // XCD-aware tile order: consecutive tile ids on one XCD (bijective remap).  Dynamic rows: over the
  // live row tiles only (the rest exit), so that they spread over every XCD
  const int mt = (a.M + BM - 1) / BM;
  const int nwg = mt * gridDim.y;
  const int orig = blockIdx.x + blockIdx.y * gridDim.x;
  if (orig >= nwg) return;
  const int q8 = nwg / 8, r8 = nwg % 8, xcd = orig % 8;
  const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + orig / 8;
  const int m0 = (wgid % mt) * BM, n0 = (wgid / mt) * BN;

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm0 = (wid >> 1) * (BM / 2), wn0 = (wid & 1) * (BN / 2);
  const int lrow = lane >> 3, pc = lane & 7;          // row within an 8-row piece, physical chunk

  // per-lane rows of the A pieces: base offset (or -1) and two coordinates
  int64_t aoff[AI];
  int ac0[AI], ac1[AI], alc[AI];
#pragma unroll
  for (int j = 0; j < AI; ++j) {
    const int rr = (wid * AI + j) * 8 + lrow;
    const int row = m0 + rr;
    alc[j] = pc ^ ((rr >> 1) & 7);
    const int rw = row < a.M ? row : 0;
    if constexpr (MODE == MODE_FWD) {
      const int np = fdiv(rw, a.fQ), q = rw - np * d.Q;
      const int n = fdiv(np, a.fP), p = np - n * d.P;
      aoff[j] = row < a.M ? (int64_t)n * a.as[0] + alc[j] * 8 : -1;
      ac0[j] = p * d.stride - d.pad;
      ac1[j] = q * d.stride - d.pad;
    } else if (a.fold) {
      const int nh = fdiv(rw, a.fW), jj = rw - nh * d.W;
      const int n = fdiv(nh, a.fH), ii = nh - n * d.H;
      aoff[j] = row < a.M ? (int64_t)n * a.as[0] + alc[j] * 8 : -1;
      ac0[j] = ii * d.up_h + d.pad;
      ac1[j] = jj * d.up_w + d.pad;
    } else {
      const int nh = fdiv(rw, a.fWu), wu = rw - nh * d.Wu;
      const int n = fdiv(nh, a.fHu), hu = nh - n * d.Hu;
      aoff[j] = row < a.M ? (int64_t)n * a.as[0] + alc[j] * 8 : -1;
      ac0[j] = hu + d.pad;
      ac1[j] = wu + d.pad;
    }
  }
  const int ldb = (MODE == MODE_DGRAD && a.fold) ? d.R * d.S * d.K : a.Kd;
  int64_t boff[BI];
#pragma unroll
  for (int j = 0; j < BI; ++j) {
    const int rr = (wid * BI + j) * 8 + lrow;
    const int row = n0 + rr;
    boff[j] = row < a.Ng ? (int64_t)row * ldb + ((pc ^ ((rr >> 1) & 7)) * 8) : -1;
  }
  const bf16* asrc = (const bf16*)a.a_src;
  const bf16* bsrc = (const bf16*)a.b_src;
  const char* zero = g_zero_row;

  auto issue = [&](int kk, char* stage) {
    // K-step decode (uniform): tap (r, s), channel offset, upsample phase (folded DGRAD)
    int r, s_, ch0, ua = 0, ub = 0, kb = kk;
    if constexpr (MODE == MODE_FWD) {
      const int rs = fdiv(kk, a.fC);
      ch0 = kk - rs * d.C;
      r = fdiv(rs, a.fS); s_ = rs - r * d.S;
    } else {
      int kr = kk;
      if (a.fold) {
        const int ab = fdiv(kk, a.fRSK);
        kr = kk - ab * (d.R * d.S * d.K);
        kb = kr;
        ua = fdiv(ab, a.fUw); ub = ab - ua * d.up_w;
      }
      const int rs = fdiv(kr, a.fK);
      ch0 = kr - rs * d.K;
      r = fdiv(rs, a.fS); s_ = rs - r * d.S;
    }
#pragma unroll
    for (int j = 0; j < AI; ++j) {
      const void* src = zero;
      if (aoff[j] >= 0) {
        if constexpr (MODE == MODE_FWD) {
          const int hu = ac0[j] + r, wu = ac1[j] + s_;
          if (hu >= 0 && hu < d.Hu && wu >= 0 && wu < d.Wu)
            // integer upsample only on this path (no map loads: an ordinary load here would make
            // the compiler drain the in-flight DMA with vmcnt(0))
            src = asrc + aoff[j] + ch0 + (int64_t)(d.up_h > 0 ? fdiv(hu, a.fUh) : hu) * a.as[2] +
                  (int64_t)(d.up_w > 0 ? fdiv(wu, a.fUw) : wu) * a.as[3];
        } else {
          int ph = ac0[j] + ua - r, pw = ac1[j] + ub - s_;
          bool ok = ph >= 0 && pw >= 0;
          if (d.stride == 2) { ok = ok && !(ph & 1) && !(pw & 1); ph >>= 1; pw >>= 1; }
          if (ok && ph < d.P && pw < d.Q)
            src = asrc + aoff[j] + ch0 + (int64_t)ph * a.as[2] + (int64_t)pw * a.as[3];
        }
      }
      glds16(src, stage + (wid * AI + j) * 1024);
    }
#pragma unroll
    for (int j = 0; j < BI; ++j) {
      const void* src = boff[j] >= 0 ? (const void*)(bsrc + boff[j] + kb) : (const void*)zero;
      glds16(src, stage + ABYTES + (wid * BI + j) * 1024);
    }
  };

  f32x4 acc[RM][RN];
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = a.Kd / 64;
  issue(0, smem);
  for (int t = 0; t < nk; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                   // stage t landed; stage t-1 fully read
    char* cur = smem + (t & 1) * STAGE;
    if (t + 1 < nk) issue((t + 1) * 64, smem + ((t + 1) & 1) * STAGE);
    mma_kstep_swz<RM, RN>(cur, cur + ABYTES, wm0, wn0, acc);
  }
  conv_epilogue<bf16, MODE, BM, BN>(a, acc, m0, n0, wm0, wn0);
}

// ---------------------------------------------------------------------------------------------
// bf16 WGRAD with LDS-DMA staging.  GEMM: dW[m = k][ng = (r,s,c)] = sum over pixels of
// dy[pix][k] * x[pix + (r,s)][c]; a K-step is 64 pixels.  Both operands are contiguous along the
// GEMM row (k / c), so each pixel contributes one 256-byte segment per operand per tile
// (K % 128 == 0 and C % 128 == 0: the 128 columns of a tile are one tap).
//   * LDS image [pixel][row] (256-byte k-rows, lane-linear DMA, 4 pixels per wave instruction),
//     read with ds_read_b64_tr_b16.  The 16-byte chunk index of k-row kr is XORed with
//     2*(kr & 3) | 8*((kr >> 3) & 1): the 8 k-rows one 32-lane half reads land on 8 disjoint
//     32-byte bank groups (conflict-free without padding, which a DMA image cannot have).
//   * Split-K over blockIdx.z with fp32 atomics (as the register-staged WGRAD).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int swz_tr(int k) { return ((k & 3) << 1) | (((k >> 3) & 1) << 3); }
// byte offset of element (k-row k, row) in a [64][128] bf16 image with 256-byte k-rows
__device__ __forceinline__ int trs_off(int k, int row) {
  return k * 256 + ((((row >> 3) ^ swz_tr(k)) << 4) | ((row & 7) << 1));
}

__device__ __forceinline__ bf16x8 trs_frag(const char* img, int k0, int r0) {
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int ka = k0 + 8 * g + q;
  const char* p0 = img + trs_off(ka, r0 + 4 * p);
  const char* p1 = img + trs_off(ka + 4, r0 + 4 * p);
  short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4_t*)p0);
  short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4_t*)p1);
  short8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

__global__ void __launch_bounds__(NTHREADS) conv_wgrad_glds_kernel(ConvArgs a) {
  constexpr int BM = 128, BN = 128, RM = 4, RN = 4;
  constexpr int IMG = 64 * 256, STAGE = 2 * IMG;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const es_conv_desc_t& d = a.d;
  conv_live_gemm(a, MODE_WGRAD);

  // XCD-aware order: blocks of one K split (same pixels) are consecutive on one XCD
  const int mt = gridDim.x, ntl = gridDim.y, tiles = mt * ntl;
  const int nwg = tiles * gridDim.z;
  const int orig = blockIdx.x + (blockIdx.y + blockIdx.z * ntl) * mt;
  const int q8 = nwg / 8, r8 = nwg % 8, xcd = orig % 8;
  const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + orig / 8;
  const int tile = wgid % tiles, split = wgid / tiles;
  const int m0 = (tile % mt) * BM, n0 = (tile / mt) * BN;
  const int kbeg = split * a.k_per_split;
  const int kend = min(a.Kd, kbeg + a.k_per_split);

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm0 = (wid >> 1) * (BM / 2), wn0 = (wid & 1) * (BN / 2);
  const int lrow = lane >> 4, pc = lane & 15;          // pixel row within a piece, physical chunk
  // the tile's tap and channel offset (C % 128 == 0: one tap per tile)
  const int rs = fdiv(n0, a.fC), cb = n0 - rs * d.C;
  const int tr = fdiv(rs, a.fS), ts = rs - tr * d.S;
  const bf16* dy = (const bf16*)a.a_src;
  const bf16* x = (const bf16*)a.b_src;
  const char* zero = g_zero_row;

  auto issue = [&](int k0, char* stage) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kr = (wid * 4 + j) * 4 + lrow;          // pixel row of the K-step, 0..63
      const int lc = pc ^ swz_tr(kr);
      const int pix = k0 + kr;
      const void* sa = zero;
      const void* sb = zero;
      if (pix < kend) {
        const int np = fdiv(pix, a.fQ), qq = pix - np * d.Q;
        const int n = fdiv(np, a.fP), pp = np - n * d.P;
        sa = dy + (int64_t)n * a.as[0] + (int64_t)pp * a.as[2] + (int64_t)qq * a.as[3] + m0 + lc * 8;
        const int hu = pp * d.stride - d.pad + tr, wu = qq * d.stride - d.pad + ts;
        if (hu >= 0 && hu < d.Hu && wu >= 0 && wu < d.Wu)
          sb = x + (int64_t)n * a.bs[0] + (int64_t)(d.up_h > 0 ? fdiv(hu, a.fUh) : hu) * a.bs[2] +
               (int64_t)(d.up_w > 0 ? fdiv(wu, a.fUw) : wu) * a.bs[3] + cb + lc * 8;
      }
      glds16(sa, stage + (wid * 4 + j) * 1024);
      glds16(sb, stage + IMG + (wid * 4 + j) * 1024);
    }
  };

  f32x4 acc[RM][RN];
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (kbeg < kend) {
    const int nk = (kend - kbeg + 63) / 64;
    issue(kbeg, smem);
    for (int t = 0; t < nk; ++t) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      const char* cur = smem + (t & 1) * STAGE;
      if (t + 1 < nk) issue(kbeg + (t + 1) * 64, smem + ((t + 1) & 1) * STAGE);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        bf16x8 af[RM], bfr[RN];
#pragma unroll
        for (int i = 0; i < RM; ++i) af[i] = trs_frag(cur, kk * 32, wm0 + i * 16);
#pragma unroll
        for (int j = 0; j < RN; ++j) bfr[j] = trs_frag(cur + IMG, kk * 32, wn0 + j * 16);
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int j = 0; j < RN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
      }
    }
  }
  conv_epilogue<bf16, MODE_WGRAD, BM, BN>(a, acc, m0, n0, wm0, wn0);
}

template <int MODE, int BM, int BN>
void launch_conv_glds(const ConvArgs& a, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((conv_glds_kernel<MODE, BM, BN>), grid, dim3(NTHREADS), 2 * (BM + BN) * 128, st, a);
}
template <int MODE, int BM, int BN>
constexpr ConvEntry glds_entry() { return {glds_key(MODE, BM, BN), &launch_conv_glds<MODE, BM, BN>}; }
void launch_wgrad_glds(const ConvArgs& a, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL(conv_wgrad_glds_kernel, grid, dim3(NTHREADS), 2 * 2 * 64 * 256, st, a);
}

// every instantiation the planner can ask for (conv_plan in conv_host.hip)
constexpr ConvEntry TABLE[] = {
    ES_IGEMM_TILE(bf16, MODE_FWD, 128, 128),   ES_IGEMM_TILE(bf16, MODE_FWD, 64, 64),
    ES_IGEMM_TILE(bf16, MODE_DGRAD, 128, 128), ES_IGEMM_TILE(bf16, MODE_DGRAD, 64, 64),
    ES_IGEMM_TILE(bf16, MODE_WGRAD, 128, 128), ES_IGEMM_TILE(bf16, MODE_WGRAD, 64, 64),
    glds_entry<MODE_FWD, 128, 128>(),          glds_entry<MODE_FWD, 128, 64>(),
    glds_entry<MODE_DGRAD, 128, 128>(),        glds_entry<MODE_DGRAD, 128, 64>(),
    {wgrad_glds_key(), &launch_wgrad_glds},
};

}  // namespace

int conv_igemm_bf16_launch(const ConvPlan& p, const ConvArgs& a, hipStream_t st) { return conv_table_launch(TABLE, p, a, st); }
