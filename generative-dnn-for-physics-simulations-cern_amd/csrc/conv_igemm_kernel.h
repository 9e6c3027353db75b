// Implicit-GEMM convolution (and linear) forward / dgrad / wgrad on gfx950 MFMA.
//
// Replaces aten::convolution, aten::convolution_backward and aten::addmm/mm for every nn.Conv2d
// and nn.Linear on the expertsim hot path (see include/expertsim_hip.h for the call sites).
//
// GEMM views (one kernel template, three operand gathers):
//   FWD   : M = N*P*Q (output pixels), Ng = K (out channels), Kd = R*S*C  (c fastest)
//           A[m][kk] = xu[n, c, p*st-pad+r, q*st-pad+s]    B[ng][kk] = Wk[k][r][s][c]
//   DGRAD : M = N*Hu*Wu (upsampled input pixels), Ng = C, Kd = R*S*K (k fastest)
//           A[m][kk] = dy[n, k, (hu+pad-r)/st, (wu+pad-s)/st] (0 unless divisible / in range)
//           B[ng][kk] = Wd[c][r][s][k]
//   WGRAD : M = K, Ng = R*S*C, Kd = N*P*Q (split over blockIdx.z, fp32 atomics)
//           A[m][kk] = dy[pix][k]                        B[ng][kk] = xu[pix shifted by (r,s)][c]
// The nearest upsample of the generators (neutron/generator.py:23,29; proton/generator.py:26,32)
// is folded into the x gather through hmap/wmap (up row -> source row).
//
// Tiling: 256 threads = 4 waves in a 2x2 grid, block tile BM x BN, K-step = 128 bytes of operand
// per row (bf16: 64, fp32: 32).  LDS holds both operands K-contiguous ([row][k], 144-byte padded
// rows -> conflict-free 16-byte fragment reads), double buffered; global->register->LDS staging
// with the next tile's loads issued before the current tile's MFMAs.
//   bf16 : v_mfma_f32_16x16x32_bf16, lane l reads A[l&15][8*(l>>4)+0..7] as one 16-byte read
//   fp32 : v_mfma_f32_16x16x4_f32 x4, lane l reads A[l&15][4*(l>>4)+0..3] once and feeds the
//          four MFMAs with k = 4*(l>>4)+t (A and B use the same permutation of k, so the sum over
//          k is unchanged; each MFMA is an exact fp32 FMA chain).
//
// This header holds the register-staged kernel template; conv_igemm_bf16.hip and conv_igemm_f32.hip
// instantiate it, each behind one key -> kernel table and one launch function (conv_plan.h).
#pragma once
#include "conv_plan.h"

namespace {


constexpr int KSTEP_BYTES = 128;               // operand bytes per row per K-step
constexpr int ROW_BYTES = KSTEP_BYTES + 16;    // padded LDS row
constexpr int NTHREADS = 256;

// LDS image of one operand for one K-step.
//  default : [rows][k] K-contiguous, 144-byte rows (fragments read with 16-byte ds_read)
//  TR      : bf16 WGRAD operands, whose global data is contiguous along the GEMM row (m / n):
//            [k][rows] row-contiguous image written with 16-byte stores (no transpose in
//            registers) and read with ds_read_b64_tr_b16 (gfx950 transposing LDS read).
//            Row stride = rows*2 + 32 bytes, and k-rows with bit 3 set XOR their byte column by
//            rows bytes, so the two 16-lane groups of a half-wave (k rows 8 apart) hit disjoint
//            banks.
template <typename T, int MODE, int BROWS>
struct LdsImg {
  static constexpr bool TR = (MODE == 2) && sizeof(T) == 2;
  static constexpr int BK = KSTEP_BYTES / sizeof(T);
  static constexpr int ROWB = TR ? BROWS * 2 + 32 : ROW_BYTES;
  static constexpr int BYTES = TR ? BK * ROWB : BROWS * ROW_BYTES;
  __device__ static __forceinline__ int tr_off(int k, int row) {   // byte offset of (k, row)
    return k * ROWB + ((row * 2) ^ (((k >> 3) & 1) * BROWS));
  }
};

__device__ __forceinline__ int src_row(const int32_t* map, int u) { return map ? map[u] : u; }
// nearest-upsample source index of upsampled row / column u
__device__ __forceinline__ int src_h(const ConvArgs& a, int u) {
  return a.d.up_h > 0 ? fdiv(u, a.fUh) : src_row(a.d.hmap, u);
}
__device__ __forceinline__ int src_w(const ConvArgs& a, int u) {
  return a.d.up_w > 0 ? fdiv(u, a.fUw) : src_row(a.d.wmap, u);
}

template <typename T> struct Vec16;
template <> struct Vec16<float> { typedef float4 type; static constexpr int N = 4; };
template <> struct Vec16<bf16> { typedef uint4 type; static constexpr int N = 8; };



// ---------------------------------------------------------------------------------------------
// Element gathers (scalar); used by the generic path and by the vector path for the base address
// ---------------------------------------------------------------------------------------------
// a Linear as a 1x1 conv of 1x1 images: rows m = sample, kk = feature (the generic decomposition
// below costs 8 integer divisions per element, ~30 us per launch for the small linears)
__device__ __forceinline__ bool is_linear(const ConvArgs& a) {
  const es_conv_desc_t& d = a.d;
  return d.R == 1 && d.S == 1 && d.P == 1 && d.Q == 1 && d.Hu == 1 && d.Wu == 1 && d.stride == 1 && d.pad == 0 &&
         !a.fold && d.hmap == nullptr;
}

template <typename T, int MODE>
__device__ __forceinline__ float gather_a(const ConvArgs& a, int m, int kk) {
  const es_conv_desc_t& d = a.d;
  const T* src = (const T*)a.a_src;
  if (is_linear(a)) {   // branch-free: clamped index + select (the loads of a chunk issue together)
    const bool ok = m < a.M && kk < a.Kd;
    int64_t i;
    if constexpr (MODE == MODE_WGRAD) i = (int64_t)kk * a.as[0] + (int64_t)m * a.as[1];
    else i = (int64_t)m * a.as[0] + (int64_t)kk * a.as[1];
    const float v = to_f(src[ok ? i : 0]);
    return ok ? v : 0.f;
  }
  if (m >= a.M || kk >= a.Kd) return 0.f;
  if constexpr (MODE == MODE_FWD) {
    const int c = kk % d.C; const int rs = kk / d.C; const int s = rs % d.S; const int r = rs / d.S;
    const int q = m % d.Q; const int np = m / d.Q; const int p = np % d.P; const int n = np / d.P;
    const int hu = p * d.stride - d.pad + r, wu = q * d.stride - d.pad + s;
    if (hu < 0 || hu >= d.Hu || wu < 0 || wu >= d.Wu) return 0.f;
    return to_f(src[off4(a.as, n, c, src_h(a, hu), src_w(a, wu))]);
  } else if constexpr (MODE == MODE_DGRAD) {
    int kr = kk, hu, wu, n;
    if (a.fold) {   // rows on the source grid, kk = (a, b, r, s, k)
      const int ab = kk / (d.R * d.S * d.K);
      kr = kk - ab * (d.R * d.S * d.K);
      const int ua = ab / d.up_w, ub = ab - ua * d.up_w;
      const int j = m % d.W; const int nh = m / d.W; const int i = nh % d.H; n = nh / d.H;
      hu = i * d.up_h + ua; wu = j * d.up_w + ub;
    } else {
      wu = m % d.Wu; const int nh = m / d.Wu; hu = nh % d.Hu; n = nh / d.Hu;
    }
    const int k = kr % d.K; const int rs = kr / d.K; const int s = rs % d.S; const int r = rs / d.S;
    const int ph = hu + d.pad - r, pw = wu + d.pad - s;
    if (ph < 0 || pw < 0 || ph % d.stride || pw % d.stride) return 0.f;
    const int p = ph / d.stride, q = pw / d.stride;
    if (p >= d.P || q >= d.Q) return 0.f;
    return to_f(src[off4(a.as, n, k, p, q)]);
  } else {  // WGRAD: A[m=k][kk=pix]
    const int q = kk % d.Q; const int np = kk / d.Q; const int p = np % d.P; const int n = np / d.P;
    return to_f(src[off4(a.as, n, m, p, q)]);
  }
}

template <typename T, int MODE>
__device__ __forceinline__ float gather_b(const ConvArgs& a, int ng, int kk) {
  const es_conv_desc_t& d = a.d;
  const T* src = (const T*)a.b_src;
  if (is_linear(a)) {
    const bool ok = ng < a.Ng && kk < a.Kd;
    int64_t i;
    if constexpr (MODE == MODE_WGRAD) i = (int64_t)kk * a.bs[0] + (int64_t)ng * a.bs[1];
    else i = (int64_t)ng * a.Kd + kk;   // packed weights (no upsample fold for a linear)
    const float v = to_f(src[ok ? i : 0]);
    return ok ? v : 0.f;
  }
  if (ng >= a.Ng || kk >= a.Kd) return 0.f;
  if constexpr (MODE == MODE_FWD) {
    return to_f(src[(int64_t)ng * a.Kd + kk]);
  } else if constexpr (MODE == MODE_DGRAD) {
    const int rsk = d.R * d.S * d.K;
    return to_f(src[(int64_t)ng * rsk + (a.fold ? kk % rsk : kk)]);
  } else {  // WGRAD: B[ng=(r,s,c)][kk=pix] = xu
    const int c = ng % d.C; const int rs = ng / d.C; const int s = rs % d.S; const int r = rs / d.S;
    const int q = kk % d.Q; const int np = kk / d.Q; const int p = np % d.P; const int n = np / d.P;
    const int hu = p * d.stride - d.pad + r, wu = q * d.stride - d.pad + s;
    if (hu < 0 || hu >= d.Hu || wu < 0 || wu >= d.Wu) return 0.f;
    return to_f(src[off4(a.bs, n, c, src_h(a, hu), src_w(a, wu))]);
  }
}

// ---------------------------------------------------------------------------------------------
// Tile staging.  A "chunk" is 16 bytes of one LDS row (VEC elements along k).
//   K-contiguous operands (FWD/DGRAD A, FWD/DGRAD B): a chunk = VEC consecutive kk of one row.
//   WGRAD operands: global data is contiguous along m / ng, so a chunk holds VEC consecutive rows
//   of one kk and is scattered into LDS element by element (transposing store).
// ---------------------------------------------------------------------------------------------
template <typename T, int MODE, int BROWS, bool IS_A, bool VEC>
struct Stager {
  typedef typename Vec16<T>::type V;
  static constexpr int VN = Vec16<T>::N;
  static constexpr int BK = KSTEP_BYTES / sizeof(T);
  static constexpr int CPR = KSTEP_BYTES / 16;          // chunks per LDS row (K-contiguous image)
  static constexpr int CHUNKS = BROWS * CPR;
  static constexpr int PER_THREAD = CHUNKS / NTHREADS;
  static constexpr bool TRANS = (MODE == MODE_WGRAD);
  V reg[PER_THREAD];
  // per-chunk state precomputed once per block (vector path): a base offset and two coordinates
  int64_t boff[PER_THREAD];
  int c0_[PER_THREAD], c1_[PER_THREAD];

  // --------------------------------------------------------------- precomputation (vector path)
  __device__ __forceinline__ void init(const ConvArgs& a, int row0) {
    if constexpr (!VEC) return;
    const es_conv_desc_t& d = a.d;
#pragma unroll
    for (int i = 0; i < PER_THREAD; ++i) {
      const int idx = threadIdx.x + i * NTHREADS;
      if constexpr (!TRANS) {
        const int row = row0 + idx / CPR;
        if constexpr (IS_A) {
          const int rr = row < a.M ? row : 0;
          if constexpr (MODE == MODE_FWD) {       // row = (n, p, q)
            const int np = fdiv(rr, a.fQ), q = rr - np * d.Q;
            const int n = fdiv(np, a.fP), p = np - n * d.P;
            boff[i] = row < a.M ? (int64_t)n * a.as[0] : -1;
            c0_[i] = p * d.stride - d.pad;
            c1_[i] = q * d.stride - d.pad;
          } else if (a.fold) {                      // DGRAD, folded upsample: row = (n, i, j) source grid
            const int nh = fdiv(rr, a.fW), j = rr - nh * d.W;
            const int n = fdiv(nh, a.fH), ii = nh - n * d.H;
            boff[i] = row < a.M ? (int64_t)n * a.as[0] : -1;
            c0_[i] = ii * d.up_h + d.pad;
            c1_[i] = j * d.up_w + d.pad;
          } else {                                  // DGRAD: row = (n, hu, wu)
            const int nh = fdiv(rr, a.fWu), wu = rr - nh * d.Wu;
            const int n = fdiv(nh, a.fHu), hu = nh - n * d.Hu;
            boff[i] = row < a.M ? (int64_t)n * a.as[0] : -1;
            c0_[i] = hu + d.pad;
            c1_[i] = wu + d.pad;
          }
        } else {
          const int ldb = (MODE == MODE_DGRAD && a.fold) ? d.R * d.S * d.K : a.Kd;
          boff[i] = row < a.Ng ? (int64_t)row * ldb : -1;
          c0_[i] = c1_[i] = 0;
        }
      } else {
        const int row = row0 + (idx % (BROWS / VN)) * VN;
        if constexpr (IS_A) {                       // WGRAD A: m = out channel
          boff[i] = row < a.M ? (int64_t)row * a.as[1] : -1;
          c0_[i] = c1_[i] = 0;
        } else {                                    // WGRAD B: ng = (r, s, c)
          const int rr = row < a.Ng ? row : 0;
          const int rs = fdiv(rr, a.fC), c = rr - rs * d.C;
          const int r = fdiv(rs, a.fS), s_ = rs - r * d.S;
          boff[i] = row < a.Ng ? (int64_t)c * a.bs[1] : -1;
          c0_[i] = r - d.pad;
          c1_[i] = s_ - d.pad;
        }
      }
    }
  }

  __device__ __forceinline__ void load(const ConvArgs& a, int row0, int k0) {
    if constexpr (VEC) {
      load_vec(a, k0);
    } else {
#pragma unroll
      for (int i = 0; i < PER_THREAD; ++i) {
        const int idx = threadIdx.x + i * NTHREADS;
        int row, kk;
        if constexpr (!TRANS) {
          row = row0 + idx / CPR;
          kk = k0 + (idx % CPR) * VN;
        } else {
          row = row0 + (idx % (BROWS / VN)) * VN;
          kk = k0 + idx / (BROWS / VN);
        }
        reg[i] = fetch_scalar(a, row, kk);
      }
    }
  }

  __device__ __forceinline__ V fetch_scalar(const ConvArgs& a, int row, int kk) {
    T e[VN];
#pragma unroll
    for (int j = 0; j < VN; ++j) {
      float f;
      if constexpr (!TRANS) f = IS_A ? gather_a<T, MODE>(a, row, kk + j) : gather_b<T, MODE>(a, row, kk + j);
      else f = IS_A ? gather_a<T, MODE>(a, row + j, kk) : gather_b<T, MODE>(a, row + j, kk);
      e[j] = from_f<T>(f);
    }
    V v; memcpy(&v, e, sizeof(v)); return v;
  }

  // vector path: the vector dimension is contiguous and VN-divisible (checked on the host)
  __device__ __forceinline__ void load_vec(const ConvArgs& a, int k0) {
    const es_conv_desc_t& d = a.d;
    const T* src = IS_A ? (const T*)a.a_src : (const T*)a.b_src;
    if constexpr (!TRANS) {
      const int kk = k0 + (int)(threadIdx.x % CPR) * VN;   // same column for all chunks
      const bool kin = kk < a.Kd;
      if constexpr (IS_A) {
        // kk -> (r, s, ch): ch = input channel (FWD) / output channel (DGRAD), fastest
        const FastDiv fch = MODE == MODE_FWD ? a.fC : a.fK;
        const int nch = MODE == MODE_FWD ? d.C : d.K;
        int kr = kk, ua = 0, ub = 0;
        if (MODE == MODE_DGRAD && a.fold) {        // kk = (phase a, phase b, r, s, k)
          const int ab = fdiv(kk, a.fRSK);
          kr = kk - ab * (d.R * d.S * d.K);
          ua = fdiv(ab, a.fUw); ub = ab - ua * d.up_w;
        }
        const int rs = fdiv(kr, fch), ch = kr - rs * nch;
        const int r = fdiv(rs, a.fS), s_ = rs - r * d.S;
#pragma unroll
        for (int i = 0; i < PER_THREAD; ++i) {
          const T* p = nullptr;
          if (kin && boff[i] >= 0) {
            if constexpr (MODE == MODE_FWD) {
              const int hu = c0_[i] + r, wu = c1_[i] + s_;
              if (hu >= 0 && hu < d.Hu && wu >= 0 && wu < d.Wu)
                p = src + boff[i] + (int64_t)ch * a.as[1] + (int64_t)src_h(a, hu) * a.as[2] +
                    (int64_t)src_w(a, wu) * a.as[3];
            } else {
              int ph = c0_[i] + ua - r, pw = c1_[i] + ub - s_;
              bool ok = ph >= 0 && pw >= 0;
              if (d.stride == 2) { ok = ok && !(ph & 1) && !(pw & 1); ph >>= 1; pw >>= 1; }
              if (ok && ph < d.P && pw < d.Q)
                p = src + boff[i] + (int64_t)ch * a.as[1] + (int64_t)ph * a.as[2] + (int64_t)pw * a.as[3];
            }
          }
          reg[i] = p ? *(const V*)p : V{};
        }
      } else {
        int kb = kk;
        if (MODE == MODE_DGRAD && a.fold) kb = kk - fdiv(kk, a.fRSK) * (d.R * d.S * d.K);
#pragma unroll
        for (int i = 0; i < PER_THREAD; ++i)
          reg[i] = (kin && boff[i] >= 0) ? *(const V*)(src + boff[i] + kb) : V{};
      }
    } else {
#pragma unroll
      for (int i = 0; i < PER_THREAD; ++i) {
        const int idx = threadIdx.x + i * NTHREADS;
        const int kk = k0 + idx / (BROWS / VN);                 // pixel (n, p, q)
        const T* p = nullptr;
        if (kk < a.Kd && boff[i] >= 0) {
          const int np = fdiv(kk, a.fQ), q = kk - np * d.Q;
          const int n = fdiv(np, a.fP), pp = np - n * d.P;
          if constexpr (IS_A) {
            p = src + boff[i] + (int64_t)n * a.as[0] + (int64_t)pp * a.as[2] + (int64_t)q * a.as[3];
          } else {
            const int hu = pp * d.stride + c0_[i], wu = q * d.stride + c1_[i];
            if (hu >= 0 && hu < d.Hu && wu >= 0 && wu < d.Wu)
              p = src + boff[i] + (int64_t)n * a.bs[0] + (int64_t)src_h(a, hu) * a.bs[2] +
                  (int64_t)src_w(a, wu) * a.bs[3];
          }
        }
        reg[i] = p ? *(const V*)p : V{};
      }
    }
  }

  __device__ __forceinline__ void store(char* lds) {
#pragma unroll
    for (int i = 0; i < PER_THREAD; ++i) {
      const int idx = threadIdx.x + i * NTHREADS;
      if constexpr (!TRANS) {
        const int row = idx / (KSTEP_BYTES / 16), ch = idx % (KSTEP_BYTES / 16);
        *(V*)(lds + row * ROW_BYTES + ch * 16) = reg[i];
      } else if constexpr (LdsImg<T, MODE, BROWS>::TR) {
        const int row = (idx % (BROWS / VN)) * VN, kk = idx / (BROWS / VN);
        *(V*)(lds + LdsImg<T, MODE, BROWS>::tr_off(kk, row)) = reg[i];
      } else {
        const int row = (idx % (BROWS / VN)) * VN, kk = idx / (BROWS / VN);
        T e[VN];
        memcpy(e, &reg[i], sizeof(e));
#pragma unroll
        for (int j = 0; j < VN; ++j) *(T*)(lds + (row + j) * ROW_BYTES + kk * sizeof(T)) = e[j];
      }
    }
  }
};

// ---------------------------------------------------------------------------------------------
// MFMA micro-kernel on one K-step held in LDS
// ---------------------------------------------------------------------------------------------
template <typename T, int RM, int RN>
__device__ __forceinline__ void mma_kstep(const char* As, const char* Bs, int wm0, int wn0,
                                          f32x4 (&acc)[RM][RN]) {
  const int lane = threadIdx.x & 63;
  const int r16 = lane & 15, g = lane >> 4;
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const int seg = kk * 4 + g;
    if constexpr (sizeof(T) == 2) {
      bf16x8 af[RM], bfr[RN];
#pragma unroll
      for (int i = 0; i < RM; ++i) af[i] = *(const bf16x8*)(As + (wm0 + i * 16 + r16) * ROW_BYTES + seg * 16);
#pragma unroll
      for (int j = 0; j < RN; ++j) bfr[j] = *(const bf16x8*)(Bs + (wn0 + j * 16 + r16) * ROW_BYTES + seg * 16);
#pragma unroll
      for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    } else {
      float4 af[RM], bfr[RN];
#pragma unroll
      for (int i = 0; i < RM; ++i) af[i] = *(const float4*)(As + (wm0 + i * 16 + r16) * ROW_BYTES + seg * 16);
#pragma unroll
      for (int j = 0; j < RN; ++j) bfr[j] = *(const float4*)(Bs + (wn0 + j * 16 + r16) * ROW_BYTES + seg * 16);
#pragma unroll
      for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].x, bfr[j].x, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].y, bfr[j].y, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].z, bfr[j].z, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].w, bfr[j].w, acc[i][j], 0, 0, 0);
        }
    }
  }
}

typedef short short4_t __attribute__((ext_vector_type(4)));
typedef short short8_t __attribute__((ext_vector_type(8)));

template <int BROWS>
__device__ __forceinline__ bf16x8 tr_frag(const char* img, int k0, int r0) {
  // A/B fragment of v_mfma_f32_16x16x32_bf16 from a [k][rows] image: lane l gets rows r0+(l&15),
  // k = k0 + 8*(l>>4) + 0..7, as two ds_read_b64_tr_b16 (4 k each).
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  typedef LdsImg<bf16, 2, BROWS> L;
  const int ka = k0 + 8 * g + q;
  const char* p0 = img + L::tr_off(ka, r0 + 4 * p);
  const char* p1 = img + L::tr_off(ka + 4, r0 + 4 * p);
  short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4_t*)p0);
  short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4_t*)p1);
  short8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

template <int RM, int RN, int BM, int BN>
__device__ __forceinline__ void mma_kstep_tr(const char* As, const char* Bs, int wm0, int wn0,
                                             f32x4 (&acc)[RM][RN]) {
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    bf16x8 af[RM], bfr[RN];
#pragma unroll
    for (int i = 0; i < RM; ++i) af[i] = tr_frag<BM>(As, kk * 32, wm0 + i * 16);
#pragma unroll
    for (int j = 0; j < RN; ++j) bfr[j] = tr_frag<BN>(Bs, kk * 32, wn0 + j * 16);
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int j = 0; j < RN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
  }
}

// Epilogue shared by the GEMM kernels: row -> output offset, bias (FWD, split 0), beta, dtype,
// fp32 atomics for WGRAD and split-K.
template <typename T, int MODE, int BM, int BN>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& a, const f32x4 (&acc)[BM / 32][BN / 32], int m0,
                                              int n0, int wm0, int wn0) {
  constexpr int RM = BM / 32, RN = BN / 32;
  const int lane = threadIdx.x & 63;
  const int col16 = lane & 15, rq = (lane >> 4) * 4;
  const es_conv_desc_t& d = a.d;
#pragma unroll
  for (int i = 0; i < RM; ++i) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int m = m0 + wm0 + i * 16 + rq + jj;
      if (m >= a.M) continue;
      int64_t rowoff = 0;
      if constexpr (MODE == MODE_FWD) {
        const int np = fdiv(m, a.fQ), q = m - np * d.Q;
        const int n = fdiv(np, a.fP), p = np - n * d.P;
        rowoff = n * a.os[0] + p * a.os[2] + q * a.os[3];
      } else if constexpr (MODE == MODE_DGRAD) {
        if (a.fold) {
          const int nh = fdiv(m, a.fW), j = m - nh * d.W;
          const int n = fdiv(nh, a.fH), ii = nh - n * d.H;
          rowoff = n * a.os[0] + ii * a.os[2] + j * a.os[3];
        } else {
          const int nh = fdiv(m, a.fWu), wu = m - nh * d.Wu;
          const int n = fdiv(nh, a.fHu), hu = nh - n * d.Hu;
          rowoff = n * a.os[0] + hu * a.os[2] + wu * a.os[3];
        }
      }
#pragma unroll
      for (int j = 0; j < RN; ++j) {
        const int ng = n0 + wn0 + j * 16 + col16;
        if (ng >= a.Ng) continue;
        float v = acc[i][j][jj];
        if constexpr (MODE == MODE_WGRAD) {
          if (a.det) ((float*)a.out)[((int64_t)blockIdx.z * a.mslot + m) * a.Ng + ng] = v;   // own partial slot
          else atomicAdd((float*)a.out + (int64_t)m * a.Ng + ng, v);
        } else {
          if constexpr (MODE == MODE_FWD) {
            if (a.bias && blockIdx.z == 0) v += a.bias[ng];
          }
          const int64_t o = rowoff + (int64_t)ng * a.os[1];
          if (a.splitk) {
            if (a.det) ((float*)a.det_ws)[(int64_t)blockIdx.z * a.mslot * a.Ng + o] = v;   // own partial slot
            else atomicAdd((float*)a.out + o, v);
          } else if (a.out_bf16) {
            bf16* y = (bf16*)a.out + o;
            if (a.beta != 0.f) v += a.beta * (float)(*y);
            *y = (bf16)v;
          } else {
            float* y = (float*)a.out + o;
            if (a.beta != 0.f) v += a.beta * (*y);
            *y = v;
          }
        }
      }
    }
  }
}

template <typename T, int MODE, int BM, int BN, bool AVEC, bool BVEC>
__global__ void __launch_bounds__(NTHREADS) conv_igemm_kernel(ConvArgs a) {
  constexpr int BK = KSTEP_BYTES / sizeof(T);
  constexpr int RM = BM / 32, RN = BN / 32;   // 16x16 tiles per wave (2x2 wave grid)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef LdsImg<T, MODE, BM> LA;
  typedef LdsImg<T, MODE, BN> LB;
  constexpr int BUF = LA::BYTES + LB::BYTES;   // one stage: A image then B image

  conv_live_gemm(a, MODE);
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int kbeg = blockIdx.z * a.k_per_split;
  const int kend = min(a.Kd, kbeg + a.k_per_split);
  if ((kbeg >= kend || m0 >= a.M) && !a.det) return;   // (a partial slot is written even when empty)
  const int wid = threadIdx.x >> 6;
  const int wm0 = (wid >> 1) * (BM / 2), wn0 = (wid & 1) * (BN / 2);

  f32x4 acc[RM][RN];
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  Stager<T, MODE, BM, true, AVEC> sa;
  Stager<T, MODE, BN, false, BVEC> sb;
  sa.init(a, m0);
  sb.init(a, n0);
  sa.load(a, m0, kbeg);
  sb.load(a, n0, kbeg);
  sa.store(smem);
  sb.store(smem + LA::BYTES);
  __syncthreads();
  int cur = 0;
  for (int k0 = kbeg; k0 < kend; k0 += BK) {
    const bool more = k0 + BK < kend;
    if (more) {
      sa.load(a, m0, k0 + BK);
      sb.load(a, n0, k0 + BK);
    }
    if constexpr (LA::TR)
      mma_kstep_tr<RM, RN, BM, BN>(smem + cur * BUF, smem + cur * BUF + LA::BYTES, wm0, wn0, acc);
    else
      mma_kstep<T, RM, RN>(smem + cur * BUF, smem + cur * BUF + LA::BYTES, wm0, wn0, acc);
    if (more) {
      sa.store(smem + (cur ^ 1) * BUF);
      sb.store(smem + (cur ^ 1) * BUF + LA::BYTES);
    }
    __syncthreads();
    cur ^= 1;
  }
  (void)BK;

  conv_epilogue<T, MODE, BM, BN>(a, acc, m0, n0, wm0, wn0);
}

// ---------------------------------------------------------------- table rows and the launch
template <typename T, int MODE, int BM, int BN, bool AV, bool BV>
void launch_conv_igemm(const ConvArgs& a, dim3 grid, hipStream_t st) {
  const size_t lds = 2 * (LdsImg<T, MODE, BM>::BYTES + LdsImg<T, MODE, BN>::BYTES);
  hipLaunchKernelGGL((conv_igemm_kernel<T, MODE, BM, BN, AV, BV>), grid, dim3(NTHREADS), lds, st, a);
}
template <typename T, int MODE, int BM, int BN, bool AV, bool BV>
constexpr ConvEntry igemm_entry() {
  return {igemm_key(sizeof(T), MODE, BM, BN, AV, BV), &launch_conv_igemm<T, MODE, BM, BN, AV, BV>};
}
// the four vector combinations of one tile
#define ES_IGEMM_TILE(T, MODE, BM, BN)                                                           \
  igemm_entry<T, MODE, BM, BN, true, true>(), igemm_entry<T, MODE, BM, BN, true, false>(),       \
      igemm_entry<T, MODE, BM, BN, false, true>(), igemm_entry<T, MODE, BM, BN, false, false>()

// looks the plan's key up and launches it, behind the zero fill of a split-K output (fp32 atomics)
template <int N>
int conv_table_launch(const ConvEntry (&table)[N], const ConvPlan& p, const ConvArgs& a, hipStream_t st) {
  const ConvEntry* e = conv_find(table, p.key);
  if (!e) return 0;
  if (p.zero_out && hipMemsetAsync(a.out, 0, (size_t)a.M * a.Ng * sizeof(float), st) != hipSuccess) {
    es_set_error("conv: split-K memset failed");
    return -1;
  }
  e->launch(a, dim3(p.grid[0], p.grid[1], p.grid[2]), st);
  return 1;
}

}  // namespace
