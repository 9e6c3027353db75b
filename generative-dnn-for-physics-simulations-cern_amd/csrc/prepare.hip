// Dataset preparation on the device (the reference's data-prep notebooks): the SDI-GAN
// diversity weight of every condition group, and the photon sum and peak position of every image.
//
// es_group_diversity.  Group g = rows perm[offs[g] .. offs[g+1]) of x [n,1,h,w] (fp32 or fp64 pixels, any
// strides).  A lane owns two neighbouring pixels and walks the group's members in perm order, so a member
// row is one contiguous read across the wave (one 8-byte load per lane for fp32, 16-byte for fp64, where
// the strides and the alignment allow; two scalar loads otherwise -- the arithmetic is the same); a
// 128-pixel tile of a group is the unit of work and T = ceil(h*w / 128) tiles cover an image.  Per pixel,
// fp64, contraction off (include/expertsim_hip.h has the definition):
//   S = sum x, m = S / n, Q = sum (x - m)^2 (product rounded, then added), var = Q / n, sd = sqrt(var).
//   n <= 8    one wave per (group, tile); the members are loaded once into registers (all loads in flight)
//             and both sums run over the registers: HBM is read once.
//   n <= 256  one wave per (group, tile); two sequential passes, 8 member loads in flight, the members' rows
//             fetched 64 at a time by one coalesced load and read with readlane; the second pass
//             re-reads the n x 128 pixels the wave has just read (n x 512 B fp32, n x 1 KiB fp64: L2 or
//             Infinity Cache).
//   n  > 256  the group is appended to a list (an integer atomic; the slot changes which workgroup takes
//             the group, never a result) and a second launch gives each (group, tile) a 16-wave workgroup:
//             wave c takes the members [c L, min(n, (c+1) L)), L = ceil(n / 16), sequentially from +0.0
//             (16 member loads in flight for fp32, 8 for fp64: 8 KiB per wave with pair loads),
//             and the 16 chunk sums are added in chunk order from +0.0 (S, then Q likewise) through LDS.
// A lane adds its two sd values (0 for a pixel past h*w), the 64 lane values are added by the xor butterfly
// of wave_sum_d (strides 32, 16, .., 1) into partial[g][tile]; a last launch adds a group's T partials in
// tile order from +0.0.  No float atomics; a group's result depends on its members, their order and h*w
// alone.
//
// LDS (large groups only): double2 [16][64], 16 KiB, written and read with a lane stride of 16 bytes
// (ds_read_b128: the 16 lanes of each of its lane groups hold 64 different dwords mod 64; ds_write_b128: the
// 8 contiguous lanes of a group cover 32 consecutive dwords), so there is no bank conflict (computed from
// the bank rule, not measured).
//
// es_image_sum_peak.  One wave per image, four images per workgroup: lane l adds the pixels l, l + 64, ..
// in that order from +0.0 (fp64) and keeps its first maximum (compared in the input's precision); the wave
// combines with the same butterfly, the smaller index winning a tie.  HBM-bound: h*w*elem bytes read and
// 16 bytes written per image.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "segment.h"

namespace {

constexpr int PREP_TILE = 128;                      // pixels of one tile: two per lane
constexpr int PREP_REG_MAX = 8;                     // members held in registers
constexpr int PREP_SPLIT_MIN = ES_PREP_SPLIT_MIN;   // above: the group's members are split over 16 waves
constexpr int PREP_CHUNKS = ES_PREP_CHUNKS;
constexpr int PREP_MAX_HW = 4096;

// rows perm[b .. b + n) of group g, clamped to the n_rows entries of perm: a segment without a cap
__device__ __forceinline__ SegSpan prep_range(const int32_t* offs, int g, int n_rows) {
  return seg_span(offs[g], offs[g + 1], n_rows);
}

template <typename T> struct PrepPair;
template <> struct PrepPair<float> { typedef float2 type; };
template <> struct PrepPair<double> { typedef double2 type; };

// A lane's two pixels 2l and 2l + 1 of the tile: element offsets inside an image and whether they exist.
// VEC (decided on the host from the strides and the alignment): the two are adjacent in memory, the
// pair is aligned to its size and both exist, so one 8-byte (fp32) or 16-byte (fp64) load fetches them.
template <typename T, bool VEC>
struct PrepLane {
  const T* x0;
  const T* x1;
  bool l0, l1;
  __device__ __forceinline__ void load(int64_t row_off, T& a, T& b) const {
    if (VEC) {
      if (l0) {
        const typename PrepPair<T>::type v = *reinterpret_cast<const typename PrepPair<T>::type*>(x0 + row_off);
        a = v.x;
        b = v.y;
      } else {
        a = (T)0;
        b = (T)0;
      }
    } else {
      a = l0 ? x0[row_off] : (T)0;
      b = l1 ? x1[row_off] : (T)0;
    }
  }
};

// The clamped row of member k0 + lane (0 past e): one coalesced load of 64 members' rows, which the
// chains then read lane by lane with readlane -- no scalar load sits between two batches of pixel loads.
__device__ __forceinline__ int prep_rows(const int32_t* perm, int k0, int e, int lane, int n_rows) {
  const int k = k0 + lane;
  return k < e ? seg_row(perm, k, n_rows) : 0;
}

// The sums over the members perm[b .. e), in that order from +0.0, of x (SQ = false) or of (x - m)^2
// (SQ = true) at this lane's two pixels; F member loads in flight and the next 64 rows fetched while the
// current 64 members are summed.  Called by whole waves.  The large groups' waves keep 8 KiB in flight with
// pair loads (PrepFlight); the one-wave groups keep 8 members in flight, which leaves them 8 waves per SIMD.
template <typename T> struct PrepFlight { static constexpr int N = 16; };
template <> struct PrepFlight<double> { static constexpr int N = 8; };
constexpr int PREP_SMALL_FLIGHT = 8;
template <typename T, bool VEC, bool SQ, int F>
__device__ __forceinline__ void prep_chain(const PrepLane<T, VEC>& ln, int64_t sn, int n_rows, const int32_t* perm,
                                           int b, int e, int lane, double m0, double m1, double& r0, double& r1) {
#pragma clang fp contract(off)
  double a0 = 0.0, a1 = 0.0;
  int next = prep_rows(perm, b, e, lane, n_rows);
  for (int k0 = b; k0 < e; k0 += 64) {
    const int rows = next;
    if (k0 + 64 < e) next = prep_rows(perm, k0 + 64, e, lane, n_rows);
    const int cnt = e - k0 < 64 ? e - k0 : 64;
    int jj = 0;
    for (; jj + F <= cnt; jj += F) {
      T v0[F], v1[F];
#pragma unroll
      for (int j = 0; j < F; ++j) ln.load((int64_t)__builtin_amdgcn_readlane(rows, jj + j) * sn, v0[j], v1[j]);
#pragma unroll
      for (int j = 0; j < F; ++j) {
        if (SQ) {
          const double d0 = (double)v0[j] - m0, d1 = (double)v1[j] - m1;
          const double q0 = d0 * d0, q1 = d1 * d1;
          a0 += q0;
          a1 += q1;
        } else {
          a0 += (double)v0[j];
          a1 += (double)v1[j];
        }
      }
    }
    for (; jj < cnt; ++jj) {
      T v0, v1;
      ln.load((int64_t)__builtin_amdgcn_readlane(rows, jj) * sn, v0, v1);
      if (SQ) {
        const double d0 = (double)v0 - m0, d1 = (double)v1 - m1;
        const double q0 = d0 * d0, q1 = d1 * d1;
        a0 += q0;
        a1 += q1;
      } else {
        a0 += (double)v0;
        a1 += (double)v1;
      }
    }
  }
  r0 = a0;
  r1 = a1;
}

struct PrepArgs {
  int n, hw, w, G, tiles;
  int64_t sn, sh, sw;
  const int32_t* perm;
  const int32_t* offs;
  double* partial;    // [G][tiles]
  double* pix_var;    // [G][hw] or NULL
  int32_t* list;      // [G] groups above PREP_SPLIT_MIN
  int32_t* count;     // [1] entries of list
};

template <typename T, bool VEC>
__device__ __forceinline__ PrepLane<T, VEC> prep_lane(const T* x, const PrepArgs& a, int t, int lane) {
  const int p = t * PREP_TILE + 2 * lane;
  PrepLane<T, VEC> ln;
  ln.l0 = p < a.hw;
  ln.l1 = p + 1 < a.hw;
  ln.x0 = x + (ln.l0 ? (int64_t)(p / a.w) * a.sh + (int64_t)(p % a.w) * a.sw : 0);
  ln.x1 = x + (ln.l1 ? (int64_t)((p + 1) / a.w) * a.sh + (int64_t)((p + 1) % a.w) * a.sw : 0);
  return ln;
}

// the variances of the lane's two pixels: store them, add the tile's sd values and store the partial
__device__ __forceinline__ void prep_finish(const PrepArgs& a, int g, int t, int lane, bool l0, bool l1, double var0,
                                            double var1) {
#pragma clang fp contract(off)
  const double sd0 = l0 ? sqrt(var0) : 0.0, sd1 = l1 ? sqrt(var1) : 0.0;
  if (a.pix_var) {
    double* pv = a.pix_var + (int64_t)g * a.hw + t * PREP_TILE + 2 * lane;
    if (l0) pv[0] = var0;
    if (l1) pv[1] = var1;
  }
  const double tot = wave_sum_d(sd0 + sd1);
  if (lane == 0) a.partial[(int64_t)g * a.tiles + t] = tot;
}

// one wave per (group, tile): groups of up to PREP_SPLIT_MIN members; larger groups go to the list
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) diversity_small_kernel(const T* __restrict__ x, PrepArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int unit = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (unit >= a.G * a.tiles) return;                  // wave-uniform; the kernel has no barrier
  const int g = unit / a.tiles, t = unit - g * a.tiles;
  const SegSpan r = prep_range(a.offs, g, a.n);
  if (r.n > PREP_SPLIT_MIN) {
    if (t == 0 && lane == 0) a.list[atomicAdd(a.count, 1)] = g;   // at most one entry per group: < G
    return;
  }
  const PrepLane<T, VEC> ln = prep_lane<T, VEC>(x, a, t, lane);
  double var0 = 0.0, var1 = 0.0;                      // an empty group
  if (r.n > 0) {
    const double dn = (double)r.n;
    double S0 = 0.0, S1 = 0.0, Q0 = 0.0, Q1 = 0.0;
    if (r.n <= PREP_REG_MAX) {
      T v0[PREP_REG_MAX], v1[PREP_REG_MAX];
      const int rows = prep_rows(a.perm, r.b, r.b + r.n, lane, a.n);
#pragma unroll
      for (int j = 0; j < PREP_REG_MAX; ++j) {
        v0[j] = (T)0;
        v1[j] = (T)0;
        if (j < r.n) ln.load((int64_t)__builtin_amdgcn_readlane(rows, j) * a.sn, v0[j], v1[j]);
      }
#pragma unroll
      for (int j = 0; j < PREP_REG_MAX; ++j) {
        S0 = j < r.n ? S0 + (double)v0[j] : S0;
        S1 = j < r.n ? S1 + (double)v1[j] : S1;
      }
      const double m0 = S0 / dn, m1 = S1 / dn;
#pragma unroll
      for (int j = 0; j < PREP_REG_MAX; ++j) {
        const double d0 = (double)v0[j] - m0, d1 = (double)v1[j] - m1;
        const double q0 = d0 * d0, q1 = d1 * d1;
        Q0 = j < r.n ? Q0 + q0 : Q0;
        Q1 = j < r.n ? Q1 + q1 : Q1;
      }
    } else {
      prep_chain<T, VEC, false, PREP_SMALL_FLIGHT>(ln, a.sn, a.n, a.perm, r.b, r.b + r.n, lane, 0.0, 0.0, S0, S1);
      const double m0 = S0 / dn, m1 = S1 / dn;
      prep_chain<T, VEC, true, PREP_SMALL_FLIGHT>(ln, a.sn, a.n, a.perm, r.b, r.b + r.n, lane, m0, m1, Q0, Q1);
    }
    var0 = Q0 / dn;
    var1 = Q1 / dn;
  }
  prep_finish(a, g, t, lane, ln.l0, ln.l1, var0, var1);
}

// one 16-wave workgroup per (listed group, tile); cap = listed groups the grid covers in one sweep
template <typename T, bool VEC>
__global__ void __launch_bounds__(PREP_CHUNKS * 64) diversity_large_kernel(const T* __restrict__ x, PrepArgs a,
                                                                           int cap) {
#pragma clang fp contract(off)
  __shared__ double2 part[PREP_CHUNKS][64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int listed = a.count[0];
  listed = listed < 0 ? 0 : (listed > a.G ? a.G : listed);
  const int t = blockIdx.x % a.tiles;
  const PrepLane<T, VEC> ln = prep_lane<T, VEC>(x, a, t, lane);
  for (int j = blockIdx.x / a.tiles; j < listed; j += cap) {      // block-uniform trip count
    int g = a.list[j];
    g = g < 0 ? 0 : (g >= a.G ? a.G - 1 : g);
    const SegSpan r = prep_range(a.offs, g, a.n);
    const int L = (r.n + PREP_CHUNKS - 1) / PREP_CHUNKS;
    const int lo = wid * L < r.n ? wid * L : r.n, hi = (wid + 1) * L < r.n ? (wid + 1) * L : r.n;
    const double dn = (double)r.n;
    double c0, c1;
    prep_chain<T, VEC, false, PrepFlight<T>::N>(ln, a.sn, a.n, a.perm, r.b + lo, r.b + hi, lane, 0.0, 0.0, c0, c1);
    part[wid][lane] = make_double2(c0, c1);
    __syncthreads();
    double S0 = 0.0, S1 = 0.0;
#pragma unroll
    for (int c = 0; c < PREP_CHUNKS; ++c) {
      const double2 v = part[c][lane];
      S0 += v.x;
      S1 += v.y;
    }
    __syncthreads();
    const double m0 = S0 / dn, m1 = S1 / dn;
    prep_chain<T, VEC, true, PrepFlight<T>::N>(ln, a.sn, a.n, a.perm, r.b + lo, r.b + hi, lane, m0, m1, c0, c1);
    part[wid][lane] = make_double2(c0, c1);
    __syncthreads();
    if (wid == 0) {
      double Q0 = 0.0, Q1 = 0.0;
#pragma unroll
      for (int c = 0; c < PREP_CHUNKS; ++c) {
        const double2 v = part[c][lane];
        Q0 += v.x;
        Q1 += v.y;
      }
      prep_finish(a, g, t, lane, ln.l0, ln.l1, r.n > 0 ? Q0 / dn : 0.0, r.n > 0 ? Q1 / dn : 0.0);
    }
    __syncthreads();
  }
}

// group_sum[g] = the tile partials of group g in tile order, from +0.0
__global__ void __launch_bounds__(256) diversity_close_kernel(const double* __restrict__ partial, int G, int tiles,
                                                              double* __restrict__ group_sum) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  double s = 0.0;
  for (int t = 0; t < tiles; ++t) s += partial[(int64_t)g * tiles + t];
  group_sum[g] = s;
}

template <typename T>
__global__ void __launch_bounds__(256) image_sum_peak_kernel(const T* __restrict__ x, int n, int hw, int w,
                                                             int64_t sn, int64_t sh, int64_t sw,
                                                             double* __restrict__ sum, int32_t* __restrict__ peak) {
  const int lane = threadIdx.x & 63;
  const int img = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (img >= n) return;                               // wave-uniform; the kernel has no barrier
  const T* p = x + (int64_t)img * sn;
  // pixel index i = lane + 64k, tracked as (row, col) without a division per pixel
  int r = lane / w, c = lane - (lane / w) * w;
  const int dr = 64 / w, dc = 64 - (64 / w) * w;
  double acc = 0.0;
  T best_v = (T)(-INFINITY);
  int best_i = INT_MAX;                               // INT_MAX: this lane has seen no pixel
#pragma unroll 4
  for (int i = lane; i < hw; i += 64) {
    const T v = p[r * sh + c * sw];
    acc += (double)v;
    if (best_i == INT_MAX || v > best_v) { best_v = v; best_i = i; }   // i ascends: the first maximum stays
    r += dr;
    c += dc;
    if (c >= w) { c -= w; ++r; }
  }
  if (sum) {
    acc = wave_sum_d(acc);
    if (lane == 0) sum[img] = acc;
  }
  if (peak) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const T ov = __shfl_xor(best_v, o, 64);
      const int oi = __shfl_xor(best_i, o, 64);
      if (ov > best_v || (ov == best_v && oi < best_i)) { best_v = ov; best_i = oi; }
    }
    if (lane == 0) {
      peak[(int64_t)img * 2] = best_i / w;
      peak[(int64_t)img * 2 + 1] = best_i - (best_i / w) * w;
    }
  }
}

int prep_tiles(int hw) { return (hw + PREP_TILE - 1) / PREP_TILE; }
size_t prep_partial_bytes(int n_groups, int hw) { return (size_t)n_groups * (size_t)prep_tiles(hw) * sizeof(double); }

bool prep_shape_ok(const es_view_t* x) {
  return x->c == 1 && x->h >= 1 && x->w >= 1 && (int64_t)x->h * x->w <= PREP_MAX_HW;
}

}  // namespace

extern "C" size_t es_group_diversity_workspace(int n_groups, int h, int w) {
  if (n_groups <= 0 || h < 1 || w < 1 || (int64_t)h * w > PREP_MAX_HW) return 0;
  // tile partials [G][T] fp64, the list of large groups [G] int32, its length (padded to 8 bytes)
  return prep_partial_bytes(n_groups, h * w) + (size_t)n_groups * sizeof(int32_t) + 8;
}

extern "C" int es_group_diversity(const es_view_t* x, int x_f64, const void* xp, const int32_t* perm,
                                  const int32_t* offs, int n_groups, double* group_sum, double* pix_var, void* work,
                                  size_t work_bytes, es_stream_t stream) {
  ES_CHECK_ARG(x && xp && perm && offs && group_sum, "group_diversity: null argument");
  ES_CHECK_ARG(x_f64 == 0 || x_f64 == 1, "group_diversity: x_f64 = %d, not 0 or 1", x_f64);
  ES_CHECK_ARG(x->c == 1, "group_diversity: images must have one channel (got %d)", x->c);
  ES_CHECK_ARG(prep_shape_ok(x), "group_diversity: image %dx%d outside 1 <= h*w <= %d", x->h, x->w, PREP_MAX_HW);
  ES_CHECK_ARG(x->n >= 0 && n_groups >= 0, "group_diversity: n=%d n_groups=%d", x->n, n_groups);
  if (x->n == 0 || n_groups == 0) return ES_OK;
  const int hw = x->h * x->w, tiles = prep_tiles(hw);
  ES_CHECK_ARG((int64_t)n_groups * tiles <= INT_MAX - 8, "group_diversity: %d groups x %d tiles above 2^31", n_groups,
               tiles);
  const size_t need = es_group_diversity_workspace(n_groups, x->h, x->w);
  ES_CHECK_ARG(work && work_bytes >= need, "group_diversity: workspace of %zu bytes, %zu needed", work_bytes, need);
  double* partial = (double*)work;
  int32_t* list = (int32_t*)((char*)work + prep_partial_bytes(n_groups, hw));
  int32_t* count = list + n_groups;
  const PrepArgs a = {x->n, hw, x->w, n_groups, tiles, x->s[0], x->s[2], x->s[3], perm, offs,
                      partial, pix_var, list, count};
  const hipStream_t st = (hipStream_t)stream;
  (void)hipMemsetAsync(count, 0, sizeof(int32_t), st);   // a failure shows in ES_CHECK_LAUNCH below
  const unsigned units = (unsigned)n_groups * (unsigned)tiles;
  const int large_max = x->n / (PREP_SPLIT_MIN + 1);            // disjoint groups above PREP_SPLIT_MIN members
  const int cap = large_max < n_groups ? large_max : n_groups;
  // pairs of pixels in one load: unit pixel stride, the pair inside one row (w even) or the rows dense
  // (sh == w, so the offset is the pixel index) with an even pixel count, even row and image strides
  // where they enter the offset, and a base aligned to the pair
  const size_t elem = x_f64 ? sizeof(double) : sizeof(float);
  const bool rows_even = x->w % 2 == 0 && x->s[2] % 2 == 0, dense = x->s[2] == x->w && hw % 2 == 0;
  const bool vec = x->s[3] == 1 && (rows_even || dense) && x->s[0] % 2 == 0 && (uintptr_t)xp % (2 * elem) == 0;
  const dim3 gs((units + 3) / 4), gl((unsigned)cap * tiles), bs(256), bl(PREP_CHUNKS * 64);
#define PREP_LAUNCH(T, VEC)                                                                                  \
  do {                                                                                                       \
    hipLaunchKernelGGL((diversity_small_kernel<T, VEC>), gs, bs, 0, st, (const T*)xp, a);                    \
    if (cap > 0) hipLaunchKernelGGL((diversity_large_kernel<T, VEC>), gl, bl, 0, st, (const T*)xp, a, cap);  \
  } while (0)
  if (x_f64 && vec) PREP_LAUNCH(double, true);
  else if (x_f64) PREP_LAUNCH(double, false);
  else if (vec) PREP_LAUNCH(float, true);
  else PREP_LAUNCH(float, false);
#undef PREP_LAUNCH
  hipLaunchKernelGGL(diversity_close_kernel, dim3((n_groups + 255) / 256), dim3(256), 0, st, partial, n_groups, tiles,
                     group_sum);
  ES_CHECK_LAUNCH();
  return ES_OK;
}

extern "C" int es_image_sum_peak(const es_view_t* x, int x_f64, const void* xp, double* sum, int32_t* peak,
                                 es_stream_t stream) {
  ES_CHECK_ARG(x && xp, "image_sum_peak: null argument");
  ES_CHECK_ARG(sum || peak, "image_sum_peak: both outputs are NULL");
  ES_CHECK_ARG(x_f64 == 0 || x_f64 == 1, "image_sum_peak: x_f64 = %d, not 0 or 1", x_f64);
  ES_CHECK_ARG(x->c == 1, "image_sum_peak: images must have one channel (got %d)", x->c);
  ES_CHECK_ARG(prep_shape_ok(x), "image_sum_peak: image %dx%d outside 1 <= h*w <= %d", x->h, x->w, PREP_MAX_HW);
  ES_CHECK_ARG(x->n >= 0, "image_sum_peak: negative count");
  if (x->n == 0) return ES_OK;
  const dim3 grid((x->n + 3) / 4), block(256);
  const int hw = x->h * x->w;
  if (x_f64)
    hipLaunchKernelGGL(image_sum_peak_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)xp, x->n, hw,
                       x->w, x->s[0], x->s[2], x->s[3], sum, peak);
  else
    hipLaunchKernelGGL(image_sum_peak_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)xp, x->n, hw,
                       x->w, x->s[0], x->s[2], x->s[3], sum, peak);
  ES_CHECK_LAUNCH();
  return ES_OK;
}
