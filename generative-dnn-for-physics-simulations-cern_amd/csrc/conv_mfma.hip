// The weight-gradient kernels of the ring family: the bf16 ring WGRAD (atomics into dW) and the
// deterministic fp32 / split-fp32 partial kernels with their ordered reduce.  (This file once held
// the whole family; the conv kernels, the helpers and the dispatcher moved out to conv_ring_kernel.h,
// conv_persist.hip, ring_device.h and conv_ring_host.hip.  The WGRAD kernels stayed, so their history
// stays with them.)
#include <algorithm>

#include "ring_device.h"
#include "ring_plan.h"
#include "split_fp32.h"

namespace {

// ---------------------------------------------------------------------------------------------
// WGRAD: dW[m = k][ng = (r, s, c)] = sum over pixels of dy[pix][k] * xu[pix + (r, s)][c].
// Block tile BM out-channels x BN in-channels of ONE tap (C % BN == 0).  K-step t = (output
// pixel t / G, image group t % G): 64 images at one pixel.  Split over blockIdx.z with fp32
// atomics into the zeroed dw.
// SP: the tile's tap is a (class, d, e) tap of the sub-pixel decomposition; its K runs over the
// class's output pixels, and the epilogue adds the tile into every original tap (r, s) the
// combined tap covers (r in {2d - a, 2d - a + 1} within [0, R), likewise s).
// ---------------------------------------------------------------------------------------------
template <int BM, int BN, bool SP>
__global__ void __launch_bounds__(RT) wgrad_ring_kernel(ConvArgs a) {
  constexpr int WGM = BM >= 64 ? BM / 64 : 1, WGN = 8 / WGM;   // waves along M / N
  constexpr int WM = BM / WGM, WN = BN / WGN;
  constexpr int RM = WM / 16, RN = WN / 16;
  constexpr int AIMG = 64 * BM * 2, SLOT = 64 * (BM + BN) * 2;
  constexpr int APW = BM / 64, BPW = BN / 64;   // 1 KiB pieces per wave per slot
  constexpr int PW = APW + BPW;
  constexpr int ALPR = BM / 8, BLPR = BN / 8;   // lanes (16-byte chunks) per k-row
  __shared__ __attribute__((aligned(16))) char smem[NSLOT * SLOT];
  const es_conv_desc_t& d = a.d;
  const int NL = conv_live(a);   // live images (dynamic rows)
  const SubPixel& sp = a.sp;
  const int G = (NL + 63) >> 6;

  // blocks of one K split (same pixels) are consecutive on one XCD
  const int mt = gridDim.x, ntl = gridDim.y, tiles = mt * ntl;
  const int orig = blockIdx.x + (blockIdx.y + blockIdx.z * ntl) * mt;
  const int wg = xcd_remap(orig, tiles * gridDim.z);
  const int tile = wg % tiles, split = wg / tiles;
  const int m0 = (tile % mt) * BM, n0 = (tile / mt) * BN;
  const int rs = n0 / d.C, cb = n0 - rs * d.C;   // tap of the tile, channel base
  // the tile's tap and the pixel grid its K runs over
  int cls = 0, tr, ts, gq, npix;
  if constexpr (SP) {
    cls = (rs >= sp.tap0[1]) + (rs >= sp.tap0[2]) + (rs >= sp.tap0[3]);
    const int de = rs - sp.tap0[cls];
    tr = de / sp.dw[cls];
    ts = de - tr * sp.dw[cls];
    gq = sp.pw[cls];
    npix = sp.ph[cls] * gq;
  } else {
    tr = rs / d.S;
    ts = rs - tr * d.S;
    gq = d.Q;
    npix = d.P * d.Q;
  }
  const int kps = NL == a.d.N ? a.k_per_split : (npix * G + gridDim.z - 1) / gridDim.z;   // live K-steps
  const int tbeg = split * kps;                  // in K-steps
  const int tend = min(npix * G, tbeg + kps);
  if (tbeg >= tend) return;

  const int lane = threadIdx.x & 63, wid = uni(threadIdx.x >> 6);
  const int wm0 = (wid / WGN) * WM, wn0 = (wid % WGN) * WN;
  const __amdgpu_buffer_rsrc_t ares = mkres(a.a_src, (uint32_t)(NL * a.as[0] * 2));
  const __amdgpu_buffer_rsrc_t bres = mkres(a.b_src, (uint32_t)(NL * a.bs[0] * 2));
  const int as0b = (int)a.as[0] * 2, as2b = (int)a.as[2] * 2, as3b = (int)a.as[3] * 2;
  const int bs0b = (int)a.bs[0] * 2, bs2b = (int)a.bs[2] * 2, bs3b = (int)a.bs[3] * 2;

  uint32_t alane[APW], blane[BPW];
#pragma unroll
  for (int j = 0; j < APW; ++j) {
    const int kr = (wid * APW + j) * (64 / ALPR) + lane / ALPR;   // image of the K-step
    alane[j] = (uint32_t)(kr * as0b + (m0 + ((lane % ALPR) ^ swz_tr<BM>(kr)) * 8) * 2);
  }
#pragma unroll
  for (int j = 0; j < BPW; ++j) {
    const int kr = (wid * BPW + j) * (64 / BLPR) + lane / BLPR;
    const int chg = (lane % BLPR) ^ swz_tr<BN>(kr);
    blane[j] = (uint32_t)(kr * bs0b + (cb + chg * 8) * 2);
  }

  // K-step cursor (uniform): pixel (p, q) of the grid and image group gi of step t = (p*gq + q)*G + gi
  int cp, cq, cg, cstep = tbeg;
  {
    const int pix = tbeg / G;
    cg = tbeg - pix * G;
    cp = pix / gq;
    cq = pix - cp * gq;
  }
  // the tile's class values as register copies (no kernel-argument reloads inside the loop)
  const int cp0 = SP ? uni(sp.p0[cls]) : 0, cq0 = SP ? uni(sp.q0[cls]) : 0;
  const int coh = SP ? uni(sp.oh[cls]) : 0, cow = SP ? uni(sp.ow[cls]) : 0;
  auto issue = [&](char* slot) {
    const bool live = cstep < tend;
    uint32_t ua, ub;
    if constexpr (SP) {   // dy at output pixel (p0 + 2p, q0 + 2q), x at source (p + oh + d, q + ow + e)
      ua = live ? (uint32_t)(cg * 64 * as0b + (cp0 + 2 * cp) * as2b + (cq0 + 2 * cq) * as3b) : OOB;
      const int hs = cp + coh + tr, ws = cq + cow + ts;
      const bool ok = live && (unsigned)hs < (unsigned)d.H && (unsigned)ws < (unsigned)d.W;
      ub = ok ? (uint32_t)(cg * 64 * bs0b + hs * bs2b + ws * bs3b) : OOB;
    } else {
      ua = live ? (uint32_t)(cg * 64 * as0b + cp * as2b + cq * as3b) : OOB;
      const int hu = cp * d.stride - d.pad + tr, wu = cq * d.stride - d.pad + ts;
      const bool ok = live && (unsigned)hu < (unsigned)d.Hu && (unsigned)wu < (unsigned)d.Wu;
      ub = ok ? (uint32_t)(cg * 64 * bs0b + fdiv(hu, a.fUh) * bs2b + fdiv(wu, a.fUw) * bs3b) : OOB;
    }
#pragma unroll
    for (int j = 0; j < APW; ++j) bdma16(ares, alane[j] + ua, slot + (wid * APW + j) * 1024);
#pragma unroll
    for (int j = 0; j < BPW; ++j) bdma16(bres, blane[j] + ub, slot + AIMG + (wid * BPW + j) * 1024);
    ++cstep;
    ++cg;
    const bool w1 = cg == G;
    cg = w1 ? 0 : cg;
    cq += w1;
    const bool w2 = cq == gq;
    cq = w2 ? 0 : cq;
    cp += w2;
  };

  f32x4 acc[RM][RN];
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  struct Frag {
    bf16x8 a[RM], b[RN];
  };
  auto load = [&](Frag& f, const char* slot, int kk) {
    const uint32_t base = lds_u32(slot);
#pragma unroll
    for (int i = 0; i < RM; ++i) f.a[i] = tr_frag_asm<BM>(base, kk * 32, wm0 + i * 16);
#pragma unroll
    for (int j = 0; j < RN; ++j) f.b[j] = tr_frag_asm<BN>(base + AIMG, kk * 32, wn0 + j * 16);
  };
  auto fence = [&](Frag& f) {
#pragma unroll
    for (int i = 0; i < RM; ++i) fence_frag(f.a[i]);
#pragma unroll
    for (int j = 0; j < RN; ++j) fence_frag(f.b[j]);
  };
  auto mma = [&](const Frag& f) {
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int j = 0; j < RN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.a[i], f.b[j], acc[i][j], 0, 0, 0);
  };
  ring_loop<PW, 2 * (RM + RN)>(tend - tbeg, smem, SLOT, issue, load, mma, fence);

  const int col16 = lane & 15, rq = (lane >> 4) * 4;
  float* out = (float*)a.out;
  // original taps this tile's tap feeds: one (no SP) or up to 2 x 2 (SP)
  int r0 = tr, r1 = tr, s0 = ts, s1 = ts;
  if constexpr (SP) {
    const int ca = cls >> 1, cbb = cls & 1;
    r0 = max(0, 2 * tr - ca);
    r1 = min(d.R - 1, 2 * tr - ca + 1);
    s0 = max(0, 2 * ts - cbb);
    s1 = min(d.S - 1, 2 * ts - cbb + 1);
  }
  const int ldo = d.R * d.S * d.C;
  for (int r = r0; r <= r1; ++r)
    for (int s_ = s0; s_ <= s1; ++s_) {
      float* o = out + (r * d.S + s_) * d.C + cb + wn0 + col16;
#pragma unroll
      for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int m = m0 + wm0 + i * 16 + rq + jj;
#pragma unroll
          for (int j = 0; j < RN; ++j) atomicAdd(o + (int64_t)m * ldo + j * 16, acc[i][j][jj]);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// fp32 WGRAD (parity mode, v_mfma_f32_16x16x4_f32): the same product and image-minor K order as
// wgrad_ring_kernel, with K-steps of KI = 32 images at one pixel (so a slot has the bf16 kernel's
// byte geometry: 1 KiB DMA pieces, 3-slot ring).  An fp32 operand needs no transposing read: lane l
// of a 16x16x4 MFMA takes A[m = l & 15][k = l >> 4], one float of k-row k, so the LDS image is the
// DMA's natural [image][channel] layout read with ds_read_b32.  Odd k-rows have their 64-byte
// halves swapped (16-byte chunk c stored at c ^ 4): the two k-rows one 32-lane group reads then
// hit disjoint banks.
// DETERMINISTIC: every (tile, K split) stores its raw fp32 tile into its own slot of the partial
// buffer ws[split][M][taps * C] (no atomics); wgrad_reduce_kernel sums the splits (and, for SP, the
// four classes' combined taps over each original tap) in a fixed order.  The reference's same-seed
// reruns are bit-identical; with this, so are the parity mode's.
// ---------------------------------------------------------------------------------------------
// SPL: split-fp32 arithmetic (see split8).  A lane's 8 k-values of a 16x16x32 fragment are the
// images 4 j + (lane >> 4), j = 0..7, of the step (MFMA k = 8 (lane >> 4) + j; the same permutation
// for A and B), so each of the 8 ds_read_b32 instructions reads four consecutive k-rows, the access
// pattern the k-row swizzle was laid out for.
template <int BM, int BN, bool SP, bool SPL = false>
__global__ void __launch_bounds__(RT) wgrad_f32_kernel(ConvArgs a, float* __restrict__ ws, int ngt) {
  constexpr int KI = 32;                                       // images per K-step
  // waves along M / N: every wave tile at least 16 x 16 (64 x 64 tiles: 2 x 4 waves of 32 x 16)
  constexpr int WGM = BM >= 128 ? BM / 64 : (BN >= 128 ? 1 : 2), WGN = 8 / WGM;
  static_assert(BM / WGM >= 16 && BN / WGN >= 16, "wave tile below one 16 x 16 MFMA block");
  constexpr int WM = BM / WGM, WN = BN / WGN;
  constexpr int RM = WM / 16, RN = WN / 16;
  constexpr int AIMG = KI * BM * 4, SLOT = KI * (BM + BN) * 4;
  constexpr int NSW = 3 * SLOT > 150 * 1024 ? 2 : NSLOT;        // (64 x 512 split tiles: 72 KiB slots)
  constexpr bool MT = BN == 512 && !SP;                         // a tile spans several taps (C < 512)
  constexpr int APW = BM / 64, BPW = BN / 64;                  // 1 KiB pieces per wave per slot
  constexpr int PW = APW + BPW;
  constexpr int ALPR = BM / 4, BLPR = BN / 4;                  // lanes (16-byte chunks) per k-row
  static_assert(ALPR >= 8 && BLPR >= 8, "the k-row swizzle flips 64-byte halves");
  __shared__ __attribute__((aligned(16))) char smem[NSW * SLOT];
  const es_conv_desc_t& d = a.d;
  const int NL = conv_live(a);   // live images (dynamic rows)
  const SubPixel& sp = a.sp;
  const int G = (NL + KI - 1) / KI;

  const int mt = gridDim.x, ntl = gridDim.y, tiles = mt * ntl;
  const int orig = blockIdx.x + (blockIdx.y + blockIdx.z * ntl) * mt;
  const int wg = xcd_remap(orig, tiles * gridDim.z);
  const int tile = wg % tiles, split = wg / tiles;
  const int m0 = (tile % mt) * BM, n0 = (tile / mt) * BN;
  const int rs = n0 / d.C, cb = n0 - rs * d.C;
  int cls = 0, tr, ts, gq, npix;
  if constexpr (SP) {
    cls = (rs >= sp.tap0[1]) + (rs >= sp.tap0[2]) + (rs >= sp.tap0[3]);
    const int de = rs - sp.tap0[cls];
    tr = de / sp.dw[cls];
    ts = de - tr * sp.dw[cls];
    gq = sp.pw[cls];
    npix = sp.ph[cls] * gq;
  } else {
    tr = rs / d.S;
    ts = rs - tr * d.S;
    gq = d.Q;
    npix = d.P * d.Q;
  }
  const int kps = NL == a.d.N ? a.k_per_split : (npix * G + gridDim.z - 1) / gridDim.z;   // live K-steps
  const int tbeg = min(split * kps, npix * G);
  const int tend = min(npix * G, tbeg + kps);

  const int lane = threadIdx.x & 63, wid = uni(threadIdx.x >> 6);
  const int wm0 = (wid / WGN) * WM, wn0 = (wid % WGN) * WN;
  const int col16 = lane & 15, rq = (lane >> 4) * 4;
  f32x4 acc[RM][RN];
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (tbeg < tend) {
    const __amdgpu_buffer_rsrc_t ares = mkres(a.a_src, (uint32_t)(NL * a.as[0] * 4));
    const __amdgpu_buffer_rsrc_t bres = mkres(a.b_src, (uint32_t)(NL * a.bs[0] * 4));
    const int as0b = (int)a.as[0] * 4, as2b = (int)a.as[2] * 4, as3b = (int)a.as[3] * 4;
    const int bs0b = (int)a.bs[0] * 4, bs2b = (int)a.bs[2] * 4, bs3b = (int)a.bs[3] * 4;
    uint32_t alane[APW], blane[BPW];
    int btr[MT ? BPW : 1], bts[MT ? BPW : 1];
#pragma unroll
    for (int j = 0; j < APW; ++j) {
      const int kr = (wid * APW + j) * (64 / ALPR) + lane / ALPR;   // image of the K-step
      alane[j] = (uint32_t)(kr * as0b + (m0 + ((lane % ALPR) ^ ((kr & 1) << 2)) * 4) * 4);
    }
#pragma unroll
    for (int j = 0; j < BPW; ++j) {
      // (a k-row of a 512-column tile spans two pieces)
      const int pc = wid * BPW + j;
      const int kr = BLPR > 64 ? pc / (BLPR / 64) : pc * (64 / BLPR) + lane / BLPR;
      const int ch = BLPR > 64 ? (pc % (BLPR / 64)) * 64 + lane : lane % BLPR;
      if constexpr (MT) {   // the lane's own tap and channel (the swizzle stays inside a tap: C % 32 == 0)
        const int ng = n0 + (ch ^ ((kr & 1) << 2)) * 4, rl = ng / d.C;
        btr[j] = rl / d.S;
        bts[j] = rl - btr[j] * d.S;
        blane[j] = (uint32_t)(kr * bs0b + (ng - rl * d.C) * 4);
      } else {
        blane[j] = (uint32_t)(kr * bs0b + (cb + (ch ^ ((kr & 1) << 2)) * 4) * 4);
      }
    }
    int cp, cq, cg, cstep = tbeg;
    if constexpr (MT) {   // pixel-minor K order: a step's right-hand taps are the next step's left ones (L2)
      cg = tbeg / npix;
      const int pix = tbeg - cg * npix;
      cp = pix / gq;
      cq = pix - cp * gq;
    } else {
      const int pix = tbeg / G;
      cg = tbeg - pix * G;
      cp = pix / gq;
      cq = pix - cp * gq;
    }
    const int cp0 = SP ? uni(sp.p0[cls]) : 0, cq0 = SP ? uni(sp.q0[cls]) : 0;
    const int coh = SP ? uni(sp.oh[cls]) : 0, cow = SP ? uni(sp.ow[cls]) : 0;
    auto issue = [&](char* slot) {
      const bool live = cstep < tend;
      uint32_t ua, ub;
      if constexpr (SP) {   // dy at output pixel (p0 + 2p, q0 + 2q), x at source (p + oh + d, q + ow + e)
        ua = live ? (uint32_t)(cg * KI * as0b + (cp0 + 2 * cp) * as2b + (cq0 + 2 * cq) * as3b) : OOB;
        const int hs = cp + coh + tr, wsx = cq + cow + ts;
        const bool ok = live && (unsigned)hs < (unsigned)d.H && (unsigned)wsx < (unsigned)d.W;
        ub = ok ? (uint32_t)(cg * KI * bs0b + hs * bs2b + wsx * bs3b) : OOB;
      } else if constexpr (MT) {   // one pixel per lane group: the B pieces' own taps
        ua = live ? (uint32_t)(cg * KI * as0b + cp * as2b + cq * as3b) : OOB;
        const int hb = cp * d.stride - d.pad, wb = cq * d.stride - d.pad;
#pragma unroll
        for (int j = 0; j < BPW; ++j) {
          const int hu = hb + btr[j], wu = wb + bts[j];
          const bool ok = live && (unsigned)hu < (unsigned)d.Hu && (unsigned)wu < (unsigned)d.Wu;
          const uint32_t u = ok ? (uint32_t)(cg * KI * bs0b + fdiv(hu, a.fUh) * bs2b + fdiv(wu, a.fUw) * bs3b) : OOB;
          bdma16(bres, blane[j] + u, slot + AIMG + (wid * BPW + j) * 1024);
        }
        ub = 0;
      } else {
        ua = live ? (uint32_t)(cg * KI * as0b + cp * as2b + cq * as3b) : OOB;
        const int hu = cp * d.stride - d.pad + tr, wu = cq * d.stride - d.pad + ts;
        const bool ok = live && (unsigned)hu < (unsigned)d.Hu && (unsigned)wu < (unsigned)d.Wu;
        ub = ok ? (uint32_t)(cg * KI * bs0b + fdiv(hu, a.fUh) * bs2b + fdiv(wu, a.fUw) * bs3b) : OOB;
      }
#pragma unroll
      for (int j = 0; j < APW; ++j) bdma16(ares, alane[j] + ua, slot + (wid * APW + j) * 1024);
      if constexpr (!MT) {
#pragma unroll
        for (int j = 0; j < BPW; ++j) bdma16(bres, blane[j] + ub, slot + AIMG + (wid * BPW + j) * 1024);
      }
      ++cstep;
      if constexpr (MT) {
        ++cq;
        const bool w1 = cq == gq;
        cq = w1 ? 0 : cq;
        cp += w1;
        const bool w2 = cp == d.P;
        cp = w2 ? 0 : cp;
        cg += w2;
      } else {
        ++cg;
        const bool w1 = cg == G;
        cg = w1 ? 0 : cg;
        cq += w1;
        const bool w2 = cq == gq;
        cq = w2 ? 0 : cq;
        cp += w2;
      }
    };
    // fragment set kk: images 16 kk .. 16 kk + 15 of the step, as 4 MFMA k-groups of 4 images
    struct Frag {
      float a[4][RM], b[4][RN];
    };
    const int kl = lane >> 4;
    auto rd = [&](const char* img, int rowb, int k, int row) {   // float (k-row k, row) of an image
      return *(const float*)(img + k * rowb + ((((row >> 2) ^ ((k & 1) << 2)) << 4) | ((row & 3) << 2)));
    };
    auto load = [&](Frag& f, const char* slot, int kk) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int k = kk * 16 + 4 * t + kl;
#pragma unroll
        for (int i = 0; i < RM; ++i) f.a[t][i] = rd(slot, BM * 4, k, wm0 + i * 16 + col16);
#pragma unroll
        for (int j = 0; j < RN; ++j) f.b[t][j] = rd(slot + AIMG, BN * 4, k, wn0 + j * 16 + col16);
      }
    };
    auto mma = [&](const Frag& f) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int j = 0; j < RN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a[t][i], f.b[t][j], acc[i][j], 0, 0, 0);
    };
    if constexpr (SPL) {
      struct FragS {
        float a[8][RM], b[8][RN];
      };
      // the lane's byte offsets of float (k-row 4 j + kl, row base + 16 i + col16) for i even / odd
      // (the odd-k-row swizzle flips bit 0 of base / 16 + i); the rest is an immediate 4 j rowb + 64 i
      const int sw = (kl & 1) * 64;
      const int sa0 = (wm0 >> 4) & 1 ? -sw : sw, sb0 = (wn0 >> 4) & 1 ? -sw : sw;
      const int oa0 = kl * BM * 4 + (wm0 + col16) * 4 + sa0, oa1 = oa0 - 2 * sa0;
      const int ob0 = AIMG + kl * BN * 4 + (wn0 + col16) * 4 + sb0, ob1 = ob0 - 2 * sb0;
      auto load_s = [&](FragS& f, const char* slot, int) {
        const char* pa[2] = {slot + oa0, slot + oa1};
        const char* pb[2] = {slot + ob0, slot + ob1};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
#pragma unroll
          for (int i = 0; i < RM; ++i) f.a[j][i] = *(const float*)(pa[i & 1] + j * 4 * BM * 4 + 64 * i);
#pragma unroll
          for (int jn = 0; jn < RN; ++jn) f.b[j][jn] = *(const float*)(pb[jn & 1] + j * 4 * BN * 4 + 64 * jn);
        }
      };
      auto mma_s = [&](const FragS& f) {
        bf16x8 bp[RN][3], ap[3];
        auto sa = [&](int i) {
          split8(f32x4{f.a[0][i], f.a[1][i], f.a[2][i], f.a[3][i]}, f32x4{f.a[4][i], f.a[5][i], f.a[6][i], f.a[7][i]},
                 ap);
        };
        sa(0);
#pragma unroll
        for (int jn = 0; jn < RN; ++jn) {   // B tiles split just before their first MFMAs
          split8(f32x4{f.b[0][jn], f.b[1][jn], f.b[2][jn], f.b[3][jn]},
                 f32x4{f.b[4][jn], f.b[5][jn], f.b[6][jn], f.b[7][jn]}, bp[jn]);
          acc[0][jn] = mfma_split6(ap, bp[jn], acc[0][jn]);
        }
#pragma unroll
        for (int i = 1; i < RM; ++i) {
          sa(i);
#pragma unroll
          for (int jn = 0; jn < RN; ++jn) acc[i][jn] = mfma_split6(ap, bp[jn], acc[i][jn]);
        }
      };
      if (a.prio && wid >= 4) __builtin_amdgcn_s_setprio(1);
      ring_loop_lean<PW, NSW>(tend - tbeg, smem, SLOT, issue, load_s, mma_s);
    } else {
      auto nofence = [](Frag&) {};
      ring_loop<PW, 0>(tend - tbeg, smem, SLOT, issue, load, mma, nofence);
    }
  }
  // the raw tile of this split (zeros for an empty split): plain stores into its own slot
  float* o = ws + ((int64_t)split * a.M + m0 + wm0) * ngt + n0 + wn0 + col16;
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int j = 0; j < RN; ++j) o[(int64_t)(i * 16 + rq + jj) * ngt + j * 16] = acc[i][j][jj];
}

// Ring loop that keeps the previous step's slot: compute of step t reads slots t and t-1, so the DMA
// issued at step t (step t + NS - 2) goes into step t-2's slot; NS - 2 steps in flight.
template <int PW, int NS, typename Issue, typename Load, typename Mma>
__device__ __forceinline__ void ring_loop_keep(int nk, char* smem, int slot_bytes, Issue& issue, Load& load,
                                               Mma& mma) {
  using Frag = typename std::remove_reference<typename lambda_arg<Load>::type>::type;
  static_assert(NS >= 3, "two live slots plus one in flight");
#pragma unroll
  for (int i = 0; i < NS - 2; ++i) issue(smem + i * slot_bytes);
  int cur = 0, prv = NS - 1, nxt = NS - 2;
  for (int t = 0; t < nk; ++t) {
    wait_vmcnt<(NS - 3) * PW>();                         // step t landed (this wave's pieces)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's reads of step t-1 are done
    ring_barrier();
    issue(smem + nxt * slot_bytes);                      // step t + NS - 2 into step t-2's slot
    Frag f;
    load(f, smem + cur * slot_bytes, smem + prv * slot_bytes);
    mma(f);
    prv = cur;
    cur = cur == NS - 1 ? 0 : cur + 1;
    nxt = nxt == NS - 1 ? 0 : nxt + 1;
  }
  wait_vmcnt<0>();   // drain the zero-fill steps before the workgroup may exit
}

// Split-fp32 WGRAD of a 2 x 2, stride-1 convolution with 128 input and 64 output channels (neutron
// G conv_layers.9: 128 -> 64 on 46 x 46): one 64 x 512 tile (the four taps x 128 channels) whose
// K-steps walk the output columns of one row: column-step j of (image group g, row p) DMAs the input
// column x[g][p - pad + {0, 1}][j - pad][:] (2 rows x 128 channels) and dy[g][p][j - 1][:] (64
// channels), and multiplies dy(p, j - 1) with its four taps: the right-hand taps from this step's
// slot, the left-hand ones from the previous step's, so every input pixel is DMA'd into LDS once per
// row instead of once per tap (40 KiB per step instead of 72 KiB: the multi-tap tiles of
// wgrad_f32_kernel<64, 512> are LDS-fill bound).  A row is Q + 1 column-steps (the first loads only);
// a split starting inside a row first reloads the column before it (no MFMAs on such steps).
// Same deterministic partial slots and ordered reduce as wgrad_f32_kernel.
// (wgrad_f32_col2_kernel; a first version that split dy in every wave was slower.)  dy is split once per workgroup: the 8 waves share the tile's 64 dy rows,
// so instead of every wave splitting all of them (32 of a lane's 64 split values per step), dy is
// buffer-loaded into registers one step ahead (4 values per lane), split by the loading lane and
// written to LDS as bf16 planes in the fragment layout (as wgrad_coop_kernel), double-buffered; the
// x columns keep the DMA ring (32 KiB slots, two steps ahead, the previous slot kept).
__global__ void __launch_bounds__(RT) wgrad_f32_col2_kernel(ConvArgs a, float* __restrict__ ws, int ngt) {
  constexpr int KI = 32, CC = 128;
  constexpr int RM = 4, RN = 4;
  constexpr int SLOT = KI * 2 * CC * 4;                        // x: 32 images x 2 rows x 128 channels
  constexpr int NS = 4, BPW = 4;
  constexpr int APL = 4 * 1024, ABUF = 3 * APL;                // dy planes [plane][block][lane][8 k]
  __shared__ __attribute__((aligned(16))) char smem[NS * SLOT + 2 * ABUF];
  char* const abase = smem + NS * SLOT;
  const es_conv_desc_t& d = a.d;
  const int NL = conv_live(a);   // live images (dynamic rows)
  const int G = (NL + KI - 1) / KI, Q1 = d.Q + 1;
  const int split = xcd_remap(blockIdx.z, gridDim.z);
  const int nst = G * d.P * Q1;
  const int kps = NL == a.d.N ? a.k_per_split : (nst + gridDim.z - 1) / gridDim.z;   // live K-steps
  const int tbeg = min(split * kps, nst), tend = min(nst, tbeg + kps);

  const int lane = threadIdx.x & 63, wid = uni(threadIdx.x >> 6);
  const int tap = wid >> 1, wtr = tap >> 1, wts = tap & 1, wc0 = (wid & 1) * 64;
  const int col16 = lane & 15, rq = (lane >> 4) * 4, kl = lane >> 4;
  f32x4 acc[RM][RN];
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (tbeg < tend) {
    const __amdgpu_buffer_rsrc_t ares = mkres(a.a_src, (uint32_t)(NL * a.as[0] * 4));
    const __amdgpu_buffer_rsrc_t bres = mkres(a.b_src, (uint32_t)(NL * a.bs[0] * 4));
    const int as0b = (int)a.as[0] * 4, as2b = (int)a.as[2] * 4, as3b = (int)a.as[3] * 4;
    const int bs0b = (int)a.bs[0] * 4, bs2b = (int)a.bs[2] * 4, bs3b = (int)a.bs[3] * 4;
    // dy half-block of this wave: rows 16 (wid >> 1) + col16, images 4 (4 (wid & 1) + jj) + kl
    const uint32_t alo = (uint32_t)((16 * (wid & 1) + kl) * as0b + (16 * (wid >> 1) + col16) * 4);
    const int awo = (wid >> 1) * 1024 + lane * 16 + (wid & 1) * 8;
    uint32_t blane[BPW];
    const int ltr = lane >> 5;
#pragma unroll
    for (int j = 0; j < BPW; ++j) {
      const int kr = wid * BPW + j;
      blane[j] = (uint32_t)(kr * bs0b + (((lane ^ ((kr & 1) << 2)) & 31) * 4) * 4);
    }
    int cg, cp, cj;
    {
      cg = tbeg / (d.P * Q1);
      const int r = tbeg - cg * d.P * Q1;
      cp = r / Q1;
      cj = r - cp * Q1;
    }
    const int s0 = tbeg - (cj > 0);
    cj -= cj > 0;
    int bstep = s0, bg = cg, bpr = cp, bj = cj;                 // DMA side (two steps ahead)
    int astep = s0, ag = cg, apr = cp, aj = cj;                 // dy side (one step ahead)
    {
      float4* z = (float4*)(smem + (NS - 1) * SLOT);
      for (int i = threadIdx.x; i < SLOT / 16; i += RT) z[i] = float4{0.f, 0.f, 0.f, 0.f};
    }
    auto adv = [&](int& st, int& g, int& pr, int& j) {
      ++st;
      ++j;
      const bool w1 = j == Q1;
      j = w1 ? 0 : j;
      pr += w1;
      const bool w2 = pr == d.P;
      pr = w2 ? 0 : pr;
      g += w2;
    };
    auto issue_b = [&](char* slot) {
      const int hu = bpr - d.pad + ltr, wu = bj - d.pad;
      const bool ok = bstep < tend && (unsigned)hu < (unsigned)d.H && (unsigned)wu < (unsigned)d.W;
      const uint32_t ub = ok ? (uint32_t)(bg * KI * bs0b + hu * bs2b + wu * bs3b) : OOB;
#pragma unroll
      for (int j = 0; j < BPW; ++j) bdma16(bres, blane[j] + ub, slot + (wid * BPW + j) * 1024);
      adv(bstep, bg, bpr, bj);
    };
    auto load_a = [&](float (&v)[4]) {   // zero on a row's first column and on a reloaded column
      const uint32_t ua = astep < tend && aj > 0 && astep >= tbeg
                              ? (uint32_t)(ag * KI * as0b + apr * as2b + (aj - 1) * as3b) : OOB;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
        v[jj] = __builtin_bit_cast(float,
                                   __builtin_amdgcn_raw_buffer_load_b32(ares, (int)(ua + alo + jj * 4 * as0b), 0, 0));
      adv(astep, ag, apr, aj);
    };
    auto store_a = [&](const float (&v)[4], char* pb) {
      uint32_t h0, m0_, l0, h1, m1, l1;
      split_pair(v[0], v[1], h0, m0_, l0);
      split_pair(v[2], v[3], h1, m1, l1);
      *(uint2*)(pb + awo) = uint2{h0, h1};
      *(uint2*)(pb + APL + awo) = uint2{m0_, m1};
      *(uint2*)(pb + 2 * APL + awo) = uint2{l0, l1};
    };
    const int sw = (kl & 1) * 64;
    const int ob0 = kl * 2 * CC * 4 + (wtr * CC + wc0 + col16) * 4 + sw, ob1 = ob0 - 2 * sw;
    auto compute = [&](const char* slot, const char* prev, const char* pa) {
      const char* bimg = wts ? slot : prev;
      const char* pb[2] = {bimg + ob0, bimg + ob1};
      float fb[8][RN];
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int jn = 0; jn < RN; ++jn) fb[j][jn] = *(const float*)(pb[jn & 1] + j * 4 * 2 * CC * 4 + 64 * jn);
      bf16x8 bp[RN][3], ap[3];
      const char* q = pa + lane * 16;
#pragma unroll
      for (int p = 0; p < 3; ++p) ap[p] = *(const bf16x8*)(q + p * APL);
#pragma unroll
      for (int jn = 0; jn < RN; ++jn) {
        split8(f32x4{fb[0][jn], fb[1][jn], fb[2][jn], fb[3][jn]}, f32x4{fb[4][jn], fb[5][jn], fb[6][jn], fb[7][jn]},
               bp[jn]);
        acc[0][jn] = mfma_split6(ap, bp[jn], acc[0][jn]);
      }
#pragma unroll
      for (int i = 1; i < RM; ++i) {
#pragma unroll
        for (int p = 0; p < 3; ++p) ap[p] = *(const bf16x8*)(q + p * APL + i * 1024);
#pragma unroll
        for (int jn = 0; jn < RN; ++jn) acc[i][jn] = mfma_split6(ap, bp[jn], acc[i][jn]);
      }
    };
    float av[4];
    load_a(av);                       // dy of the first step
    asm volatile("" ::: "memory");
    issue_b(smem);                    // x of the first two steps
    issue_b(smem + SLOT);
    store_a(av, abase);
    int cur = 0, prv = NS - 1, nxt = 2;
    const int nk = tend - s0;
    // (the x DMA of step t + 2 is issued after the dy planes are written: hipcc makes an LDS store
    // wait for every LDS-DMA in flight, vmcnt(0), which would otherwise drain it one step early)
    for (int t = 0; t < nk; ++t) {
      wait_vmcnt<BPW>();                                   // x of step t landed
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // dy planes of step t written, step t-1 read
      ring_barrier();
      load_a(av);                                          // dy of step t + 1
      asm volatile("" ::: "memory");
      compute(smem + cur * SLOT, smem + prv * SLOT, abase + (t & 1) * ABUF);
      store_a(av, abase + ((t & 1) ^ 1) * ABUF);           // (last read in step t - 1)
      asm volatile("" ::: "memory");
      issue_b(smem + nxt * SLOT);                          // x of step t + 2 (step t-2's slot)
      prv = cur;
      cur = cur == NS - 1 ? 0 : cur + 1;
      nxt = nxt == NS - 1 ? 0 : nxt + 1;
    }
    wait_vmcnt<0>();
  }
  float* o = ws + (int64_t)split * a.M * ngt + tap * CC + wc0 + col16;
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int j = 0; j < RN; ++j) o[(int64_t)(i * 16 + rq + jj) * ngt + j * 16] = acc[i][j][jj];
}

// Split-fp32 WGRAD with a cooperative split (BM = 128: 2 x 4 waves of 64 x BN / 4).  In the
// DMA-ring kernels every wave splits its own A rows and B columns, so each value is split by the
// BN / WN (A) or BM / WM (B) waves that share it: 64 values per lane per K-step of 128 x 256,
// ~5.5 VALU instructions each, more vector issue than the step's 96 MFMAs leave free.  Here each
// value is split once: a K-step's A and B values are loaded straight into registers (one step
// ahead, plain buffer loads, zero outside the tensor), split by the lane that loaded them and
// written to LDS as three bf16 planes in the MFMA fragment layout ([plane][16-row block][lane]
// [8 k-values]: a wave's fragment is one conflict-free ds_read_b128), double-buffered behind one
// barrier per step.  (BM + BN) / 64 half-blocks of 4 values per lane: 24 values per lane per
// step of 128 x 256.  Same K order, arithmetic and partial slots as wgrad_f32_kernel<SPL>.
template <int BM, int BN, bool SP>
__global__ void __launch_bounds__(RT) wgrad_coop_kernel(ConvArgs a, float* __restrict__ ws, int ngt) {
  constexpr int KI = 32;
  constexpr int WGM = BM / 64, WGN = 8 / WGM;
  constexpr int WM = BM / WGM, WN = BN / WGN, RM = WM / 16, RN = WN / 16;
  static_assert(BM == 128 && WN >= 16, "128-row tiles, wave tiles of >= 16 columns");
  constexpr int NBA = BM / 16, NB = (BM + BN) / 16;            // 16-row blocks: A's, A's and B's
  constexpr int NH = NB * 2 / 8, NHA = NBA * 2 / 8;             // half-blocks per wave (A's first)
  static_assert(NB * 2 % 8 == 0 && NBA * 2 % 8 == 0, "half-blocks split evenly over 8 waves");
  constexpr int PLANE = NB * 1024, PBUF = 3 * PLANE;
  __shared__ __attribute__((aligned(16))) char smem[2 * PBUF];
  const es_conv_desc_t& d = a.d;
  const int NL = conv_live(a);   // live images (dynamic rows)
  const SubPixel& sp = a.sp;
  const int G = (NL + KI - 1) / KI;

  const int mt = gridDim.x, ntl = gridDim.y, tiles = mt * ntl;
  const int orig = blockIdx.x + (blockIdx.y + blockIdx.z * ntl) * mt;
  const int wg = xcd_remap(orig, tiles * gridDim.z);
  const int tile = wg % tiles, split = wg / tiles;
  const int m0 = (tile % mt) * BM, n0 = (tile / mt) * BN;
  const int rs = n0 / d.C, cb = n0 - rs * d.C;
  int cls = 0, tr, ts, gq, npix;
  if constexpr (SP) {
    cls = (rs >= sp.tap0[1]) + (rs >= sp.tap0[2]) + (rs >= sp.tap0[3]);
    const int de = rs - sp.tap0[cls];
    tr = de / sp.dw[cls];
    ts = de - tr * sp.dw[cls];
    gq = sp.pw[cls];
    npix = sp.ph[cls] * gq;
  } else {
    tr = rs / d.S;
    ts = rs - tr * d.S;
    gq = d.Q;
    npix = d.P * d.Q;
  }
  const int kps = NL == a.d.N ? a.k_per_split : (npix * G + gridDim.z - 1) / gridDim.z;   // live K-steps
  const int tbeg = min(split * kps, npix * G);
  const int tend = min(npix * G, tbeg + kps);

  const int lane = threadIdx.x & 63, wid = uni(threadIdx.x >> 6);
  const int wm0 = (wid / WGN) * WM, wn0 = (wid % WGN) * WN;
  const int col16 = lane & 15, rq = (lane >> 4) * 4, kl = lane >> 4;
  f32x4 acc[RM][RN];
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (tbeg < tend) {
    const __amdgpu_buffer_rsrc_t ares = mkres(a.a_src, (uint32_t)(NL * a.as[0] * 4));
    const __amdgpu_buffer_rsrc_t bres = mkres(a.b_src, (uint32_t)(NL * a.bs[0] * 4));
    const int as0b = (int)a.as[0] * 4, as2b = (int)a.as[2] * 4, as3b = (int)a.as[3] * 4;
    const int bs0b = (int)a.bs[0] * 4, bs2b = (int)a.bs[2] * 4, bs3b = (int)a.bs[3] * 4;
    // half-block h of this wave: block b = (8 h + wid) / 2, k-half hh = wid & 1 (images
    // 4 (4 hh + jj) + kl, jj = 0..3, of the step), row / column 16 b + col16 of the tile
    uint32_t lofs[NH];
    int wofs[NH];   // LDS byte offset of the lane's 8 bytes in plane 0
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int hb = 8 * h + wid, b = hb >> 1, hh = hb & 1;
      if (h < NHA) lofs[h] = (uint32_t)((16 * hh + kl) * as0b + (m0 + 16 * b + col16) * 4);
      else lofs[h] = (uint32_t)((16 * hh + kl) * bs0b + (cb + 16 * (b - NBA) + col16) * 4);
      wofs[h] = b * 1024 + lane * 16 + hh * 8;
    }
    int cp, cq, cg;
    {
      const int pix = tbeg / G;
      cg = tbeg - pix * G;
      cp = pix / gq;
      cq = pix - cp * gq;
    }
    int cstep = tbeg;
    const int cp0 = SP ? uni(sp.p0[cls]) : 0, cq0 = SP ? uni(sp.q0[cls]) : 0;
    const int coh = SP ? uni(sp.oh[cls]) : 0, cow = SP ? uni(sp.ow[cls]) : 0;
    typedef float Stage[NH][4];
    auto load = [&](Stage& v) {   // the next K-step's values (zero past tend or outside the tensor)
      const bool live = cstep < tend;
      uint32_t ua, ub;
      if constexpr (SP) {
        ua = live ? (uint32_t)(cg * KI * as0b + (cp0 + 2 * cp) * as2b + (cq0 + 2 * cq) * as3b) : OOB;
        const int hs = cp + coh + tr, wsx = cq + cow + ts;
        const bool ok = live && (unsigned)hs < (unsigned)d.H && (unsigned)wsx < (unsigned)d.W;
        ub = ok ? (uint32_t)(cg * KI * bs0b + hs * bs2b + wsx * bs3b) : OOB;
      } else {
        ua = live ? (uint32_t)(cg * KI * as0b + cp * as2b + cq * as3b) : OOB;
        const int hu = cp * d.stride - d.pad + tr, wu = cq * d.stride - d.pad + ts;
        const bool ok = live && (unsigned)hu < (unsigned)d.Hu && (unsigned)wu < (unsigned)d.Wu;
        ub = ok ? (uint32_t)(cg * KI * bs0b + fdiv(hu, a.fUh) * bs2b + fdiv(wu, a.fUw) * bs3b) : OOB;
      }
#pragma unroll
      for (int h = 0; h < NH; ++h)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const uint32_t o = h < NHA ? ua + lofs[h] + jj * 4 * as0b : ub + lofs[h] + jj * 4 * bs0b;
          v[h][jj] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(h < NHA ? ares : bres,
                                                                                   (int)o, 0, 0));
        }
      ++cstep;
      ++cg;
      const bool w1 = cg == G;
      cg = w1 ? 0 : cg;
      cq += w1;
      const bool w2 = cq == gq;
      cq = w2 ? 0 : cq;
      cp += w2;
    };
    auto store = [&](const Stage& v, char* pb) {   // split and write the three planes
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        uint32_t h0, m0_, l0, h1, m1, l1;
        split_pair(v[h][0], v[h][1], h0, m0_, l0);
        split_pair(v[h][2], v[h][3], h1, m1, l1);
        *(uint2*)(pb + wofs[h]) = uint2{h0, h1};
        *(uint2*)(pb + PLANE + wofs[h]) = uint2{m0_, m1};
        *(uint2*)(pb + 2 * PLANE + wofs[h]) = uint2{l0, l1};
      }
    };
    auto load_b = [&](const char* pb, bf16x8 (&bp)[RN][3]) {
      const char* q = pb + lane * 16;
#pragma unroll
      for (int jn = 0; jn < RN; ++jn)
#pragma unroll
        for (int p = 0; p < 3; ++p) bp[jn][p] = *(const bf16x8*)(q + p * PLANE + (NBA + wn0 / 16 + jn) * 1024);
    };
    auto rows = [&](const char* pb, const bf16x8 (&bp)[RN][3]) {
      const char* q = pb + lane * 16;
      bf16x8 ap[3];
#pragma unroll
      for (int i = 0; i < RM; ++i) {
#pragma unroll
        for (int p = 0; p < 3; ++p) ap[p] = *(const bf16x8*)(q + p * PLANE + (wm0 / 16 + i) * 1024);
#pragma unroll
        for (int jn = 0; jn < RN; ++jn) acc[i][jn] = mfma_split6(ap, bp[jn], acc[i][jn]);
      }
    };
    auto compute = [&](const char* pb) {
      bf16x8 bp[RN][3];
      load_b(pb, bp);
      rows(pb, bp);
    };
    auto sync = [] {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      ring_barrier();
    };
    Stage s0;
    const int nk = tend - tbeg;
    load(s0);
    store(s0, smem);
    sync();
    // one stage of registers: step t + 1's loads are issued before step t's MFMAs and split after
    // them (two stages, 24 more registers, spill at 128 x 256; measured slower, round 4)
    for (int t = 0; t < nk; ++t) {
      char* cur = smem + (t & 1) * PBUF;
      char* nxt = smem + ((t & 1) ^ 1) * PBUF;
      load(s0);                 // step t + 1
      asm volatile("" ::: "memory");
      compute(cur);             // step t
      store(s0, nxt);           // step t + 1 (its buffer was last read in step t - 1)
      sync();
    }
    wait_vmcnt<0>();
    wait_vmcnt<0>();
  }
  float* o = ws + ((int64_t)split * a.M + m0 + wm0) * ngt + n0 + wn0 + col16;
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int j = 0; j < RN; ++j) o[(int64_t)(i * 16 + rq + jj) * ngt + j * 16] = acc[i][j][jj];
}

// dW (torch layout [K][C][R][S], fp32) = beta * dW + sum over the splits of the partials
// ws[split][K][taps * C]; SP: original tap (r, s) sums the four classes' combined taps
// (d, e) = ((r + a) >> 1, (s + b) >> 1) of class (a, b).  A workgroup takes 32 consecutive outputs
// (c fastest: coalesced partial reads) x 8 split lanes; lane q sums splits q, q + 8, ... (classes
// innermost) and lane 0 adds the 8 lane sums in order: a fixed summation order, so reruns are bitwise
// equal.  (One thread per output looping over all splits was latency bound: 166 us for
// conv_layers.9's 512 splits.)
constexpr int WR_LANES = 8;
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float* __restrict__ ws, int splits, int K, int C,
                                                           int R, int S, int ngt, SubPixel sp, float* __restrict__ dw,
                                                           float beta) {
  __shared__ float part[WR_LANES][32];
  const int64_t n = (int64_t)K * R * S * C;
  const int64_t zst = (int64_t)K * ngt;
  const int o = threadIdx.x & 31, q = threadIdx.x >> 5;
  for (int64_t i0 = blockIdx.x * (int64_t)32; i0 < n; i0 += (int64_t)gridDim.x * 32) {
    const int64_t i = i0 + o;
    float v = 0.f;
    int k = 0, r = 0, s = 0, c = 0;
    if (i < n) {
      c = (int)(i % C);
      int64_t t = i / C;
      s = (int)(t % S);
      t /= S;
      r = (int)(t % R);
      k = (int)(t / R);
      const float* p = ws + (int64_t)k * ngt + c + q * zst;
      if (sp.on) {
        int off[4];
#pragma unroll
        for (int cl = 0; cl < 4; ++cl)
          off[cl] = (sp.tap0[cl] + ((r + (cl >> 1)) >> 1) * sp.dw[cl] + ((s + (cl & 1)) >> 1)) * C;
        for (int z = q; z < splits; z += WR_LANES, p += WR_LANES * zst) {
#pragma unroll
          for (int cl = 0; cl < 4; ++cl) v += p[off[cl]];
        }
      } else {
        const int off = (r * S + s) * C;
#pragma unroll 4
        for (int z = q; z < splits; z += WR_LANES, p += WR_LANES * zst) v += p[off];
      }
    }
    part[q][o] = v;
    __syncthreads();
    if (q == 0 && i < n) {
      float u = part[0][o];
#pragma unroll
      for (int l = 1; l < WR_LANES; ++l) u += part[l][o];
      float* g = dw + (((int64_t)k * C + c) * R + r) * S + s;
      *g = (beta != 0.f ? beta * *g : 0.f) + u;
    }
    __syncthreads();
  }
}

// The same reduce with 4 consecutive channels per thread (C % 4 == 0): 16-byte partial loads, 128
// outputs per workgroup row; per output the summation order is the one above, so the results are
// bitwise those of wgrad_reduce_kernel (measured: that kernel moved its partials at ~1.4 TB/s, 23 us
// for conv_layers.5's 33.5 MB).
__global__ void __launch_bounds__(256) wgrad_reduce4_kernel(const float* __restrict__ ws, int splits, int K, int C,
                                                            int R, int S, int ngt, SubPixel sp, float* __restrict__ dw,
                                                            float beta) {
  __shared__ float4 part[WR_LANES][32];
  const int64_t n4 = (int64_t)K * R * S * (C >> 2);
  const int64_t zst = (int64_t)K * ngt;
  const int o = threadIdx.x & 31, q = threadIdx.x >> 5, C4 = C >> 2;
  for (int64_t i0 = blockIdx.x * (int64_t)32; i0 < n4; i0 += (int64_t)gridDim.x * 32) {
    const int64_t i = i0 + o;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    int k = 0, r = 0, s = 0, c = 0;
    if (i < n4) {
      c = (int)(i % C4) * 4;
      int64_t t = i / C4;
      s = (int)(t % S);
      t /= S;
      r = (int)(t % R);
      k = (int)(t / R);
      const float* p = ws + (int64_t)k * ngt + c + q * zst;
      if (sp.on) {
        int off[4];
#pragma unroll
        for (int cl = 0; cl < 4; ++cl)
          off[cl] = (sp.tap0[cl] + ((r + (cl >> 1)) >> 1) * sp.dw[cl] + ((s + (cl & 1)) >> 1)) * C;
#pragma unroll 2
        for (int z = q; z < splits; z += WR_LANES, p += WR_LANES * zst) {
#pragma unroll
          for (int cl = 0; cl < 4; ++cl) {
            const float4 w = *(const float4*)(p + off[cl]);
            v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
          }
        }
      } else {
        const int off = (r * S + s) * C;
#pragma unroll 4
        for (int z = q; z < splits; z += WR_LANES, p += WR_LANES * zst) {
          const float4 w = *(const float4*)(p + off);
          v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
        }
      }
    }
    part[q][o] = v;
    __syncthreads();
    if (q == 0 && i < n4) {
      float4 u = part[0][o];
#pragma unroll
      for (int l = 1; l < WR_LANES; ++l) {
        const float4 w = part[l][o];
        u.x += w.x; u.y += w.y; u.z += w.z; u.w += w.w;
      }
      const float uu[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float* g = dw + (((int64_t)k * C + c + j) * R + r) * S + s;
        *g = (beta != 0.f ? beta * *g : 0.f) + uu[j];
      }
    }
    __syncthreads();
  }
}

// Every instantiation the planners can ask for (ring_plan, wgrad_f32_plan in conv_ring_host.hip).  The
// split arithmetic of wgrad_f32_kernel is built for its 64 x 512 tile only: split-fp32 128-row tiles take
// the cooperative (or wave-specialised) kernel, and on the other 64-row tiles the in-kernel split was
// VALU-bound, so they stay exact.
template <int BM, int BN, bool SP>
void launch_wgrad_ring(const ConvArgs& a, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((wgrad_ring_kernel<BM, BN, SP>), grid, dim3(RT), 0, st, a);
}
template <int BM, int BN, bool SP, bool SPL>
void launch_wgrad_f32(const ConvArgs& a, dim3 grid, float* wsc, int ngt, hipStream_t st) {
  hipLaunchKernelGGL((wgrad_f32_kernel<BM, BN, SP, SPL>), grid, dim3(RT), 0, st, a, wsc, ngt);
}
template <int BM, int BN, bool SP>
void launch_wgrad_coop(const ConvArgs& a, dim3 grid, float* wsc, int ngt, hipStream_t st) {
  hipLaunchKernelGGL((wgrad_coop_kernel<BM, BN, SP>), grid, dim3(RT), 0, st, a, wsc, ngt);
}
void launch_wgrad_col2(const ConvArgs& a, dim3 grid, float* wsc, int ngt, hipStream_t st) {
  hipLaunchKernelGGL(wgrad_f32_col2_kernel, grid, dim3(RT), 0, st, a, wsc, ngt);
}
const RingEntry<void (*)(const ConvArgs&, dim3, hipStream_t)> RING_TABLE[] = {
    {wgrad_ring_key(256, 128, false), &launch_wgrad_ring<256, 128, false>}, {wgrad_ring_key(256, 128, true), &launch_wgrad_ring<256, 128, true>},
    {wgrad_ring_key(128, 256, false), &launch_wgrad_ring<128, 256, false>}, {wgrad_ring_key(128, 256, true), &launch_wgrad_ring<128, 256, true>},
    {wgrad_ring_key(128, 128, false), &launch_wgrad_ring<128, 128, false>}, {wgrad_ring_key(128, 128, true), &launch_wgrad_ring<128, 128, true>},
    {wgrad_ring_key(64, 128, false), &launch_wgrad_ring<64, 128, false>}, {wgrad_ring_key(64, 128, true), &launch_wgrad_ring<64, 128, true>},
};
const RingEntry<void (*)(const ConvArgs&, dim3, float*, int, hipStream_t)> F32_TABLE[] = {
    {wgrad_f32_key(128, 256, false, false), &launch_wgrad_f32<128, 256, false, false>}, {wgrad_f32_key(128, 256, true, false), &launch_wgrad_f32<128, 256, true, false>},
    {wgrad_f32_key(128, 128, false, false), &launch_wgrad_f32<128, 128, false, false>}, {wgrad_f32_key(128, 128, true, false), &launch_wgrad_f32<128, 128, true, false>},
    {wgrad_f32_key(128, 64, false, false), &launch_wgrad_f32<128, 64, false, false>}, {wgrad_f32_key(128, 64, true, false), &launch_wgrad_f32<128, 64, true, false>},
    {wgrad_f32_key(64, 128, false, false), &launch_wgrad_f32<64, 128, false, false>}, {wgrad_f32_key(64, 128, true, false), &launch_wgrad_f32<64, 128, true, false>},
    {wgrad_f32_key(64, 64, false, false), &launch_wgrad_f32<64, 64, false, false>}, {wgrad_f32_key(64, 64, true, false), &launch_wgrad_f32<64, 64, true, false>},
    {wgrad_f32_key(64, 512, false, true), &launch_wgrad_f32<64, 512, false, true>}, {wgrad_col2_key(), &launch_wgrad_col2},
    {wgrad_coop_key(128, 256, false), &launch_wgrad_coop<128, 256, false>}, {wgrad_coop_key(128, 256, true), &launch_wgrad_coop<128, 256, true>},
    {wgrad_coop_key(128, 128, false), &launch_wgrad_coop<128, 128, false>}, {wgrad_coop_key(128, 128, true), &launch_wgrad_coop<128, 128, true>},
    {wgrad_coop_key(128, 64, false), &launch_wgrad_coop<128, 64, false>}, {wgrad_coop_key(128, 64, true), &launch_wgrad_coop<128, 64, true>},
};

}  // namespace

bool wgrad_ring_launch(const RingPlan& p, const ConvArgs& a, hipStream_t st) {
  const auto* e = ring_find(RING_TABLE, p.key);
  if (e) e->launch(a, dim3(p.grid[0], p.grid[1], p.grid[2]), st);
  return e != nullptr;
}

bool wgrad_f32_launch(const RingKey& key, const int grid[3], const ConvArgs& a, float* wsc, int ngt, hipStream_t st) {
  const auto* e = ring_find(F32_TABLE, key);
  if (e) e->launch(a, dim3(grid[0], grid[1], grid[2]), wsc, ngt, st);
  return e != nullptr;
}

// one deterministic reduce launch (the vector kernel when the channels allow it)
void wgrad_reduce_launch(const float* ws, int splits, int K, int C, int R, int S, int ngt, const SubPixel& sp, float* dw,
                         float beta, hipStream_t st) {
  if (C % 4 == 0 && ngt % 4 == 0) {
    const int64_t n4 = (int64_t)K * C / 4 * R * S;
    const int blocks = (int)std::min<int64_t>((n4 + 31) / 32, 16384);
    hipLaunchKernelGGL(wgrad_reduce4_kernel, dim3(blocks), dim3(256), 0, st, ws, splits, K, C, R, S, ngt, sp, dw, beta);
    return;
  }
  const int64_t n = (int64_t)K * C * R * S;
  const int blocks = (int)std::min<int64_t>((n + 31) / 32, 16384);
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(blocks), dim3(256), 0, st, ws, splits, K, C, R, S, ngt, sp, dw, beta);
}
