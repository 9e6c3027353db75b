// Host side of the 8-wave LDS-DMA ring kernels: the library switches, the plan a dispatcher
// (conv_ring_host.hip) makes for one launch, and the launch functions of the kernel files.
//
// Plan, then launch: ring_plan() is a pure function of the call.  It answers "not eligible" (0),
// "error" (< 0) or fills a RingPlan: which kernel, on which grid, and every ConvArgs field and ConvCall
// result the launch sets.  The caller applies the plan (ring_apply) only when it launches, so a
// declined call leaves its arguments as they were.  Each kernel file exports one function that looks
// the plan's key up in its table of instantiations; a key that is not there is an error, never a
// silent fall-back.
#pragma once
#include "conv_common.h"

// es_conv_set_*: test hooks (the kernel tests compare the paths bitwise) and the fp32 arithmetic mode
struct RingSwitches {
  bool ring = true;       // es_conv_set_ring(0) routes the bf16 shapes to the 4-wave kernels of conv_igemm_bf16.hip
  bool glds = true;       // es_conv_set_glds(0) forces the register-staged kernels (tests compare the paths)
  bool subpixel = true;   // es_conv_set_subpixel
  bool ring256 = true;    // es_conv_set_ring256: 256 x 256 tiles
  bool persist = true;    // es_conv_set_persist: the persistent short-K DGRAD
  bool p256 = true;       // es_conv_set_p256: the persistent 256 x 256 merged sub-pixel FWD
  // split-fp32 WGRAD with 128-row tiles: the wave-specialised kernel (1) or wgrad_coop_kernel (0);
  // bitwise the same partials (es_conv_set_wgrad_ws, tests / A-B)
  int wgrad_ws = 1;
  int f32_chunk = 0;      // es_conv_set_f32_chunk: at most this many images per ring launch (0: no limit)
  // fp32 MFMA arithmetic of the ring kernels (es_conv_set_f32_split): 0 = exact fp32
  // (v_mfma_f32_16x16x4_f32), 2 = split-fp32 (three bf16 planes, 6 products on
  // v_mfma_f32_16x16x32_bf16) with the packed weights' planes precomputed (es_pack_weight_planes)
  int f32_split = 0;
};
// the library's switches (conv_ring_host.hip holds them and their setters)
__attribute__((visibility("hidden"))) const RingSwitches& es_conv_switches();

enum { RK_RING, RK_PERSIST, RK_P256, RK_WGRAD_RING, RK_WGRAD_F32, RK_WGRAD_COL2, RK_WGRAD_COOP };

// One instantiation.  Fields a family does not have are 0.
//   RK_RING        conv_ring_kernel<mode, bm, bn, sp, bk, T (eb bytes), spl, flag = AFF>
//   RK_PERSIST     conv_persist_kernel<bn, flag = BNR>
//   RK_P256        conv_p256_kernel<bn / 256, flag = AFF>
//   RK_WGRAD_RING  wgrad_ring_kernel<bm, bn, sp>
//   RK_WGRAD_F32   wgrad_f32_kernel<bm, bn, sp, spl != 0>
//   RK_WGRAD_COL2  wgrad_f32_col2_kernel
//   RK_WGRAD_COOP  wgrad_coop_kernel<bm, bn, sp>
struct RingKey { int family, mode, bm, bn, sp, bk, eb, spl, flag; };
constexpr bool operator==(const RingKey& x, const RingKey& y) {
  return x.family == y.family && x.mode == y.mode && x.bm == y.bm && x.bn == y.bn && x.sp == y.sp && x.bk == y.bk &&
         x.eb == y.eb && x.spl == y.spl && x.flag == y.flag;
}
constexpr RingKey ring_key(int mode, int bm, int bn, bool sp, int bk, int eb, int spl, bool aff) {
  return RingKey{RK_RING, mode, bm, bn, sp, bk, eb, spl, aff};
}
constexpr RingKey persist_key(int bn, bool bnr) { return RingKey{RK_PERSIST, MODE_DGRAD, 128, bn, 0, 64, 2, 0, bnr}; }
constexpr RingKey p256_key(int nt, bool aff) { return RingKey{RK_P256, MODE_FWD, 256, nt * 256, 1, 32, 2, 0, aff}; }
constexpr RingKey wgrad_ring_key(int bm, int bn, bool sp) { return RingKey{RK_WGRAD_RING, MODE_WGRAD, bm, bn, sp, 64, 2, 0, 0}; }
constexpr RingKey wgrad_f32_key(int bm, int bn, bool sp, bool spl) {
  return RingKey{RK_WGRAD_F32, MODE_WGRAD, bm, bn, sp, 0, 4, spl ? 2 : 0, 0};
}
// (2 x 2 taps x 128 channels -> 64: one 64 x 512 tile spans the whole weight gradient)
constexpr RingKey wgrad_col2_key() { return RingKey{RK_WGRAD_COL2, MODE_WGRAD, 64, 512, 0, 0, 4, 2, 0}; }
constexpr RingKey wgrad_coop_key(int bm, int bn, bool sp) { return RingKey{RK_WGRAD_COOP, MODE_WGRAD, bm, bn, sp, 0, 4, 2, 0}; }

struct RingPlan {
  RingKey key;
  int grid[3];
  int karg;   // the kernel's scalar behind ConvArgs: tiles (RK_PERSIST), row tiles (RK_P256)
  ConvArgs a;   // the launch's arguments: the caller's with the fields the plan decides (ng, vec_out, sp, sp_tpc,
                // sp_merge, k_per_split, stats_part, epi_*, bnr_*, b_src behind the split-fp32 weight planes)
  int stats_chunks, bnr_chunks;   // ConvCall results, with the two below
  int aff_fused;   // 1: the kernel applies the affine epilogue
  int path;        // PATH_* bits of the launch
};

// FWD / DGRAD (eb = 2: bf16, 4: fp32 with split level spl) and the bf16 WGRAD.  1: p is the plan.
int ring_plan(const ConvArgs& a, int mode, const ConvCall& call, int eb, int spl, const RingSwitches& sw, RingPlan& p);
void ring_apply(const RingPlan& p, ConvArgs& a, ConvCall& call);

// Deterministic fp32 WGRAD: tile, image chunks, K splits per chunk.  The partial kernel of a chunk is
// key (with ws: the wave-specialised kernel of conv_wgrad_ws.hip first, key when that declines).
struct WgF32Plan {
  RingKey key;
  int ws, sp, nc, nchunks, sc, ngt;
  int npix;   // K pixels of a chunk's image (the largest sub-pixel class; RK_WGRAD_COL2: P * (Q + 1) column steps)
  SubPixel spg;
};
bool wgrad_f32_plan(const es_conv_desc_t& d, const int64_t ys[4], const int64_t xs[4], const RingSwitches& sw,
                    WgF32Plan& p);

// images per launch of a batch of N whose gathered operand takes img_bytes per image
int ring_chunk_images(int64_t img_bytes, int N, const RingSwitches& sw);

// One row of a kernel file's table (key -> launch of that instantiation) and the lookup
template <typename F>
struct RingEntry {
  RingKey key;
  F launch;
};
template <typename F, int N>
const RingEntry<F>* ring_find(const RingEntry<F> (&table)[N], const RingKey& key) {
  for (const RingEntry<F>& e : table)
    if (e.key == key) return &e;
  return nullptr;
}

// The kernel files' launch functions: false when the key is not one of the file's instantiations.
bool conv_ring_bf16_launch(const RingPlan& p, const ConvArgs& a, hipStream_t st);    // conv_ring_bf16.hip
bool conv_ring_f32_launch(const RingPlan& p, const ConvArgs& a, hipStream_t st);     // conv_ring_f32.hip
bool conv_persist_launch(const RingPlan& p, const ConvArgs& a, hipStream_t st);      // conv_persist.hip
bool wgrad_ring_launch(const RingPlan& p, const ConvArgs& a, hipStream_t st);        // conv_mfma.hip
bool wgrad_f32_launch(const RingKey& key, const int grid[3], const ConvArgs& a, float* wsc, int ngt, hipStream_t st);
void wgrad_reduce_launch(const float* ws, int splits, int K, int C, int R, int S, int ngt, const SubPixel& sp, float* dw,
                         float beta, hipStream_t st);
