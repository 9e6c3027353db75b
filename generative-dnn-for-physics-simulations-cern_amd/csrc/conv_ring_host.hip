// Host dispatcher of the 8-wave LDS-DMA ring kernels (ring_plan.h): the library switches and their
// setters, the sub-pixel geometry, the plans (which kernel a call takes, on which grid, with which
// arguments) and the launches over image chunks.  Host code only: the kernels are in
// conv_ring_bf16.hip / conv_ring_f32.hip (conv_ring_kernel.h), conv_persist.hip and conv_mfma.hip, each
// behind one launch function.
#include <algorithm>

#include "conv_common.h"
#include "ring_plan.h"

namespace {

RingSwitches g_sw;

// split-fp32 kernels: static s_setprio 1 for waves 4-7 (measured against 0: equal within noise, kept)
constexpr int SPL_PRIO = 1;

// minimum K-steps per WGRAD K-split (each split flushes its whole fp32 tile with atomics; 8 / 32 / 64
// / 128 measured within noise at B = 1024 and E = 4 B = 512, 128 slower)
constexpr int WGRAD_MINK = 8;

// Tuning constants, each chosen by alternating A/B on whole train steps:
//   * short-K FWD (<= 8 K-steps, e.g. conv_layers.9): 128 x 64 tiles, two workgroups per CU (201 -> 177 us);
//   * image-group size 64 of the row order (64 > 16 > 8 on the whole step; 8 for an isolated FWD),
//     16 under dynamic rows;
//   * sub-pixel FWD: class-interleaved tile order (14.45 -> 14.33 ms per step), one 256 x 256 GEMM over
//     (class, channel) columns when the 4 classes share their geometry;
//   * 256 x 256 tiles with 32-deep K-steps for FWD / DGRAD with >= 256 output columns;
//   * persistent short-K DGRAD (conv_persist_kernel: conv_layers.9 387 -> 259 us; as FWD it was slower
//     with fused statistics, 376 vs 364 us, and was removed) and the persistent 256 x 256 merged
//     sub-pixel FWD.
constexpr int RING_NG = 64;
// Dynamic rows (multi-expert steps: capacity-B launches, a device count of live images): groups of
// 16 images, so the last, partly live group of an expert's rows carries at most 15 dead images
// through the MFMAs instead of up to 63 (E = 4, B = 512: 28.1 -> 26.8 ms/step fp32, 13.07 -> 12.69
// bf16, alternating against 64 and 32 on one box; profiles/r05_ngdyn_ab.log).  16 is also the
// smallest group the 32-deep K-step kernels' 16-row DMA pieces allow.
constexpr int RING_NG_DYN = 16;

// a dense NHWC image stack (n outermost, rows of c contiguous values); dense_small: below 1 GiB of eb-byte values
bool dense(const int64_t s[4], int c, int h, int w) {
  return s[1] == 1 && s[3] == c && s[2] == (int64_t)w * c && s[0] == (int64_t)h * w * c;
}
bool dense_small(const int64_t s[4], int n, int c, int h, int w, int eb) {
  return dense(s, c, h, w) && (int64_t)n * s[0] * eb < (1ll << 30);
}

// host-side count of the MFMA conv kernels issued (ring / persistent / p256 / fp32 wgrad), read by
// bench.py's probe to state how many launches one probed op is (fp32 image chunks)
int64_t g_conv_launches = 0;

}  // namespace

extern "C" int64_t es_conv_launch_count() { return g_conv_launches; }

// Class geometry of the sub-pixel decomposition (see SubPixel): output row p belongs to class
// a = (p - pad) mod 2, p = p0 + 2u, source row of combined tap d = u + oh + d, dh = taps.
// tile0: prefix over the classes of ceil(class pixels / row_tile) (row_tile = pixels per FWD tile).
void es_make_subpixel(const es_conv_desc_t& d, int row_tile, SubPixel& sp) {
  int dhv[2], dwv[2], p0v[2], q0v[2], phv[2], pwv[2], ohv[2], owv[2];
  for (int a = 0; a < 2; ++a) {
    dhv[a] = ((a + d.R - 1) >> 1) + 1;
    dwv[a] = ((a + d.S - 1) >> 1) + 1;
    p0v[a] = (a + d.pad) & 1;
    q0v[a] = (a + d.pad) & 1;
    phv[a] = d.P > p0v[a] ? (d.P - p0v[a] + 1) / 2 : 0;
    pwv[a] = d.Q > q0v[a] ? (d.Q - q0v[a] + 1) / 2 : 0;
    ohv[a] = (p0v[a] - d.pad - a) / 2;
    owv[a] = (q0v[a] - d.pad - a) / 2;
  }
  sp.on = 1;
  sp.tap0[0] = 0;
  sp.tile0[0] = 0;
  for (int c = 0; c < 4; ++c) {
    const int a = c >> 1, b = c & 1;
    sp.ph[c] = phv[a];
    sp.pw[c] = pwv[b];
    sp.p0[c] = p0v[a];
    sp.q0[c] = q0v[b];
    sp.oh[c] = ohv[a];
    sp.ow[c] = owv[b];
    sp.dh[c] = dhv[a];
    sp.dw[c] = dwv[b];
    sp.tap0[c + 1] = sp.tap0[c] + dhv[a] * dwv[b];
    const int pix = phv[a] * pwv[b];
    sp.tile0[c + 1] = sp.tile0[c] + (row_tile > 0 ? (pix + row_tile - 1) / row_tile : 0);
  }
}

// the setters return the previous value
template <typename T>
static int set_switch(T& sw, T v) {
  const int old = sw;
  sw = v;
  return old;
}
extern "C" int es_conv_set_ring(int on) { return set_switch(g_sw.ring, on != 0); }
extern "C" int es_conv_set_glds(int on) { return set_switch(g_sw.glds, on != 0); }
// (bit 0: the persistent short-K DGRAD kernel on / off; the other bits are ignored)
extern "C" int es_conv_set_persist(int on) { return set_switch(g_sw.persist, (on & 1) != 0); }
extern "C" int es_conv_set_p256(int on) { return set_switch(g_sw.p256, on != 0); }
extern "C" int es_conv_set_ring256(int on) { return set_switch(g_sw.ring256, on != 0); }
extern "C" int es_conv_set_subpixel(int on) { return set_switch(g_sw.subpixel, on != 0); }
extern "C" int es_conv_set_f32_chunk(int images) { return set_switch(g_sw.f32_chunk, images > 0 ? images : 0); }
extern "C" int es_conv_set_wgrad_ws(int on) { return set_switch(g_sw.wgrad_ws, on ? 1 : 0); }
// 0: exact fp32; any other value: split-fp32 on pre-split weight planes (level 2, the only split level)
extern "C" int es_conv_set_f32_split(int on) { return set_switch(g_sw.f32_split, on ? 2 : 0); }
int es_f32_split_level() { return g_sw.f32_split; }
const RingSwitches& es_conv_switches() { return g_sw; }

extern "C" int es_subpixel_taps(int R, int S) {
  return (((R - 1) >> 1) + 1 + (R >> 1) + 1) * (((S - 1) >> 1) + 1 + (S >> 1) + 1);
}

// Whether es_conv2d_fwd / es_conv2d_dgrad take the sub-pixel path for this conv (then the weights
// must be packed with es_pack_conv_weight mode 2 / 3 and d->subpixel set): bf16, x2 integer
// upsample, stride 1, channels % 64 == 0, below the ring's size limits.  The activations must be
// dense NHWC at call time.
extern "C" int es_conv_subpixel_ok(const es_conv_desc_t* d, es_dtype_t dt) {
  if (!g_sw.ring || !g_sw.subpixel || !d || (dt != ES_BF16 && dt != ES_F32)) return 0;
  if (d->up_h != 2 || d->up_w != 2 || d->hmap || d->stride != 1) return 0;
  if (d->C % 64 || d->K % 64) return 0;
  const int eb = dt == ES_F32 ? 4 : 2;
  const int64_t wbytes = (int64_t)d->K * d->C * es_subpixel_taps(d->R, d->S) * eb;
  // (operands of >= 1 GiB run as image chunks, es_conv_ring_launch / es_conv_ring_launch_f32; the
  // merged 256 x 256 kernel's 32-bit output offsets are checked where it is chosen)
  return wbytes < (1ll << 30) && (int64_t)d->H * d->W * d->C * eb < (1ll << 24) &&
         (int64_t)d->P * d->Q * d->K * eb < (1ll << 24);
}

// ---------------------------------------------------------------------------------------------
// Image chunks.  The ring's buffer offsets are 32-bit with an out-of-range marker at 2^31, so every
// gathered operand must stay below 1 GiB; larger batches (conv_layers.5's fp32 output gradient at
// B = 1024 is 1.1 GB, a capacity-2048 expert's in bf16 too) run as launches over image chunks on
// offset base pointers (chunks of whole 64-image groups).
// ---------------------------------------------------------------------------------------------
// images per launch: equal chunks (whole 64-image groups where the limit allows) below the limit
int ring_chunk_images(int64_t img_bytes, int N, const RingSwitches& sw) {
  int64_t lim = ((1ll << 30) - 1) / std::max<int64_t>(img_bytes, 1);
  if (sw.f32_chunk > 0) lim = std::min<int64_t>(lim, sw.f32_chunk);
  if (lim >= N) return N;
  lim = std::max<int64_t>(lim, 1);
  const int64_t nchunks = (N + lim - 1) / lim;
  int64_t nc = (N + nchunks - 1) / nchunks;
  if (nc % 64 && (nc + 63) / 64 * 64 <= lim) nc = (nc + 63) / 64 * 64;
  return (int)nc;
}

namespace {   // the plans

// bf16 WGRAD (atomics into dW): 256 x 128 / 128 x 256 / 128 x 128 / 64 x 128 tiles, K split over z
int plan_wgrad(const ConvArgs& a, const RingSwitches& sw, RingPlan& p) {
  const es_conv_desc_t& d = a.d;
  if (!dense_small(a.as, d.N, d.K, d.P, d.Q, 2) || !dense_small(a.bs, d.N, d.C, d.H, d.W, 2)) return 0;
  const bool sp = sw.subpixel && d.up_h == 2 && d.up_w == 2 && d.stride == 1;
  int BM, BN;
  if (d.K % 256 == 0 && d.C % 128 == 0) BM = 256, BN = 128;
  else if (d.K % 128 == 0 && d.C % 256 == 0) BM = 128, BN = 256;
  else if (d.K % 128 == 0 && d.C % 128 == 0) BM = 128, BN = 128;
  else if (d.K == 64 && d.C % 128 == 0) BM = 64, BN = 128;   // neutron G conv_layers.9 (128 -> 64)
  else return 0;
  if (sp) es_make_subpixel(d, 0, p.a.sp);
  const int taps = sp ? p.a.sp.tap0[4] : d.R * d.S;
  const int tiles = (a.M / BM) * (taps * d.C / BN);
  int npix = d.P * d.Q;
  if (sp)
    for (int c = 0; c < 4; ++c) npix = c == 0 ? p.a.sp.ph[0] * p.a.sp.pw[0] : std::max(npix, p.a.sp.ph[c] * p.a.sp.pw[c]);
  const int ks = npix * ((d.N + 63) / 64);   // K-steps (the largest class)
  // one workgroup per CU: aim at two full rounds of the 256 CUs, >= WGRAD_MINK K-steps per split
  const int want = std::max(1, std::min(ks / WGRAD_MINK, 512 / tiles));
  const int per = (ks + want - 1) / want;
  p.a.k_per_split = per;
  p.key = wgrad_ring_key(BM, BN, sp);
  p.grid[0] = a.M / BM; p.grid[1] = taps * d.C / BN; p.grid[2] = (ks + per - 1) / per;
  p.path = PATH_RING | (sp ? PATH_SUBPIXEL : 0);
  return 1;
}

// FWD / DGRAD for bf16 or fp32 operands (fp32: the parity mode's exact fp32 MFMA, or with spl the
// split-fp32 bf16-plane MFMA on 32-channel K-steps; the persistent kernels are bf16-only)
int plan_fd(const ConvArgs& a, int mode, const ConvCall& call, int EB, int spl, const RingSwitches& sw, RingPlan& p) {
  const es_conv_desc_t& d = a.d;
  const bool sp_weights = d.subpixel != 0;
  if (spl) {   // the pre-split B planes follow the fp32 packing (es_pack_weight_planes)
    const int64_t nel = (int64_t)d.K * d.C * (sp_weights ? es_subpixel_taps(d.R, d.S) : d.R * d.S);
    p.a.b_src = (const char*)a.b_src + es_weight_planes_offset(nel);
  }
  // affine + activation epilogue requested (es_conv2d_fwd_affine): bf16 and split-fp32 FWD kernels
  // carry it; the exact-fp32 ring does not (the caller then runs the norm pass)
  const bool aff = mode == MODE_FWD && call.aff != nullptr && (EB == 2 || spl > 0);
  if (aff) {
    p.a.epi_scale = call.aff->scale;
    p.a.epi_shift = call.aff->shift;
    p.a.epi_act = call.aff->act;
    p.a.epi_slope = call.aff->slope;
  }
  // fused BatchNorm statistics (es_conv2d_fwd_stats): n [3][Ng] partials, when the caller's buffer holds them
  auto offer_stats = [&](int n) {
    const bool ok = mode == MODE_FWD && call.stats_part && n > 0 && (int64_t)n * 3 * a.Ng <= call.stats_floats;
    p.a.stats_part = ok ? call.stats_part : nullptr;
    p.stats_chunks = ok ? n : 0;
  };
  // caller checked: channels % (128 / EB) == 0, K % (128 / EB) == 0 per step
  int PQ;
  if (mode == MODE_FWD) {
    if (!dense_small(a.as, d.N, d.C, d.H, d.W, EB)) return sp_weights ? -1 : 0;
    PQ = d.P * d.Q;
  } else {
    if (!dense_small(a.as, d.N, d.K, d.P, d.Q, EB)) return sp_weights ? -1 : 0;
    PQ = a.fold ? d.H * d.W : d.Hu * d.Wu;
  }
  if ((int64_t)a.Ng * a.Kd * EB * (sp_weights ? 2 : 1) >= (1ll << 30)) return sp_weights ? -1 : 0;
  p.path = PATH_RING | (EB == 4 && spl ? PATH_SPLIT : 0) | (sp_weights ? PATH_SUBPIXEL : 0);
  // image group size of the row order (see conv_ring_kernel).  Measured on the whole train step
  // (tools/gpu_ab.sh, one box): 64 > 16 > 8 for both FWD and DGRAD, although an isolated FWD
  // prefers 8 (less MALL traffic).  Dynamic rows take 16 (RING_NG_DYN).
  p.a.ng = d.rows ? RING_NG_DYN : RING_NG;
  while (p.a.ng > 8 && p.a.ng / 2 >= d.N) p.a.ng /= 2;   // small batches (per-expert shards): no empty rows
  const int NGI = (d.N + p.a.ng - 1) / p.a.ng;
  const int nt128 = (a.Ng + 127) / 128;
  // short-K FWD (<= 8 K-steps, e.g. conv_layers.9: 2x2 taps x 128 channels): 128 x 64 tiles (72 KiB
  // of LDS, two workgroups per CU) so one tile's fill and epilogue overlap another's MFMAs
  // (measured 201 -> 177 us; the same rule on the DGRAD of that conv was slower)
  // (bf16 only: the fp32 kernels' K-steps are 32 channels, so the same conv has 16 of them and takes
  // the 256-row tiles: conv_layers.9 FWD 1109 -> 1064 us per op at B = 1024, round 5)
  const bool shortk = mode == MODE_FWD && !sp_weights && a.Kd / 64 <= 8 && EB == 2;
  // persistent short-K DGRAD (conv_persist_kernel): stride 1, no upsample / sub-pixel, <= 8 K-steps,
  // the whole weight panel (nk x Ng x 128 B) within 64 KiB, dense 16-byte output rows
  if (EB == 2 && sw.persist && mode == MODE_DGRAD) {
    const int nkk = a.Kd / 64;
    const bool rows16 = a.os[1] == 1 && a.beta == 0.f && a.out_bf16 && a.os[0] % 8 == 0 && a.os[2] % 8 == 0 &&
                        a.os[3] % 8 == 0 && ((uintptr_t)a.out & 15) == 0 &&
                        (int64_t)d.N * a.os[0] * 2 < (1ll << 31);
    const bool geo = d.stride == 1 && !sp_weights && !a.fold && d.hmap == nullptr && d.up_h <= 0 &&
                     d.Hu == d.H && d.Wu == d.W && d.K % 64 == 0 && a.Kd % 64 == 0;
    const int NS = a.Ng <= 64 ? 4 : 3;
    if (geo && rows16 && (a.Ng == 64 || a.Ng == 128) && nkk >= NS - 1 && nkk <= 8 && nkk * a.Ng <= 512 &&
        p.a.ng >= 16) {
      const int NB = 128 / p.a.ng, TT = (PQ + NB - 1) / NB;
      const int ntiles = NGI * TT;
      const int nwg = std::min(ntiles, 256);
      // fused BatchNorm-backward reduction over the stored dy (es_conv2d_dgrad_bnred)
      const es_norm_t* nm = call.bnr_nm;
      const es_chain_t* ch = call.bnr_ch;
      bool bnr = false;
      if (call.bnr_part && (int64_t)nwg * 3 * a.Ng <= call.bnr_floats && nm && ch && call.bnr_x &&
          ((uintptr_t)call.bnr_x & 15) == 0 && (ch->act == ES_ACT_LRELU || ch->act == ES_ACT_RELU) &&
          (!ch->drop.enabled || ch->keep) && a.os[3] == a.Ng && a.os[2] == (int64_t)d.W * a.Ng &&
          a.os[0] == (int64_t)d.H * d.W * a.Ng) {
        p.a.bnr_x = call.bnr_x;
        p.a.bnr_keep = ch->keep;
        p.a.bnr_mean = nm->mean; p.a.bnr_invstd = nm->invstd; p.a.bnr_gamma = nm->gamma; p.a.bnr_beta = nm->beta;
        p.a.bnr_drop = ch->drop.enabled != 0;
        p.a.bnr_scale = p.a.bnr_drop ? ch->drop.scale : 1.f;
        p.a.bnr_dfirst = ch->dropout_first;
        p.a.bnr_slope = ch->act == ES_ACT_LRELU ? ch->slope : 0.f;
        p.a.bnr_part = call.bnr_part;
        p.bnr_chunks = nwg;
        bnr = true;
      }
      p.key = persist_key(a.Ng, bnr);
      p.grid[0] = nwg; p.grid[1] = p.grid[2] = 1;
      p.karg = ntiles;
      return 1;
    }
  }
  // >= 3 rounds of 256-row tiles
  const bool big = !shortk && (int64_t)NGI * p.a.ng * PQ / 256 * nt128 >= 768;
  const int BM = big ? 256 : 128, NB = BM / p.a.ng;
  int row_tiles = NGI * ((PQ + NB - 1) / NB);
  if (sp_weights) {
    es_make_subpixel(d, NB, p.a.sp);   // FWD: tile0 = per-class tile prefix of one image group
    if (mode == MODE_FWD) row_tiles = NGI * p.a.sp.tile0[4];
  }
  // staged 16-byte row stores: channel-contiguous rows, 16-byte aligned, no beta
  const int vel = a.out_bf16 ? 8 : 4;
  p.a.vec_out = a.os[1] == 1 && a.beta == 0.f && a.os[0] % vel == 0 && a.os[2] % vel == 0 && a.os[3] % vel == 0 &&
              a.Ng % vel == 0 && ((uintptr_t)a.out & 15) == 0;
  p.a.sp_tpc = 0;
  p.a.sp_merge = 0;
  if (sp_weights && mode == MODE_FWD && sw.ring256 && big && p.a.vec_out && p.a.ng >= 16 && a.Ng % 64 == 0) {
    bool same = true;
    for (int c = 1; c < 4; ++c)
      same = same && p.a.sp.dh[c] == p.a.sp.dh[0] && p.a.sp.dw[c] == p.a.sp.dw[0] && p.a.sp.ph[c] == p.a.sp.ph[0] &&
             p.a.sp.pw[c] == p.a.sp.pw[0] && p.a.sp.oh[c] == p.a.sp.oh[0] && p.a.sp.ow[c] == p.a.sp.ow[0];
    if (same) {
      p.a.sp_merge = 1;
      row_tiles = NGI * p.a.sp.tile0[1];
    }
  }
  if (sp_weights && mode == MODE_FWD && !p.a.sp_merge) {
    for (int c = 0; c < 4; ++c) p.a.sp_tpc = std::max(p.a.sp_tpc, p.a.sp.tile0[c + 1] - p.a.sp.tile0[c]);
    row_tiles = NGI * 4 * p.a.sp_tpc;
  }
  // one partial per row tile (and class of a merged tile), written by the staged epilogue
  offer_stats(p.a.vec_out ? (p.a.sp_merge ? 4 * row_tiles : row_tiles) : 0);
  // the ring kernel of a tile, with the affine epilogue when the arguments carry one (FWD with bf16
  // or split-fp32 operands)
  auto ring = [&](int bm, int bn, int bk, int cols) {
    const bool affk = mode == MODE_FWD && (EB == 2 || spl > 0) && p.a.epi_scale != nullptr;
    p.key = ring_key(mode, bm, bn, sp_weights, bk, EB, spl, affk);
    p.aff_fused = affk;
    p.grid[0] = row_tiles; p.grid[1] = (cols + bn - 1) / bn; p.grid[2] = 1;
    return 1;
  };
  if (p.a.sp_merge) {   // (vec_out: the merged epilogue is the staged one)
    const int NT = 4 * a.Ng / 256;
    if (EB == 2 && sw.p256 && (4 * a.Ng) % 256 == 0 && (NT == 1 || NT == 2 || NT == 4) && row_tiles >= 64 &&
        a.out_bf16 && (int64_t)d.N * a.os[0] * 2 < (1ll << 31)) {
      offer_stats(256 * 4);
      p.key = p256_key(NT, aff);
      p.aff_fused = aff;
      p.grid[0] = 256; p.grid[1] = p.grid[2] = 1;
      p.karg = row_tiles;
      return 1;
    }
    // split-fp32: 256 x 128 tiles (a wave's 128 columns within one class) or 256 x 64; else 256 x 256
    // tiles of 32-channel steps
    if (spl) return ring(256, a.Ng % 128 == 0 ? 128 : 64, 64, 4 * a.Ng);
    return ring(256, 256, 32, 4 * a.Ng);
  }
  const bool wide = sw.ring256 && big && !shortk && a.Ng >= 256 && p.a.ng >= 16 && p.a.vec_out &&
                    (sp_weights || mode == MODE_DGRAD);   // (plain FWD: register spills at 256 x 256)
  if (wide) {   // split-fp32 (pre-split B): 256 x 128 tiles (256 x 256 does not fit the LDS)
    if (spl) return ring(256, 128, 64, a.Ng);
    return ring(256, 256, 32, a.Ng);
  }
  return ring(big ? 256 : 128, a.Ng <= 64 || shortk ? 64 : 128, 64, a.Ng);
}

}  // namespace

int ring_plan(const ConvArgs& a, int mode, const ConvCall& call, int eb, int spl, const RingSwitches& sw, RingPlan& p) {
  p = RingPlan{};
  p.a = a;
  p.stats_chunks = call.stats_chunks;
  p.bnr_chunks = call.bnr_chunks;
  if (mode == MODE_WGRAD) return eb == 2 ? plan_wgrad(a, sw, p) : 0;
  return plan_fd(a, mode, call, eb, eb == 4 ? spl : 0, sw, p);
}

void ring_apply(const RingPlan& p, ConvArgs& a, ConvCall& call) {
  a = p.a;
  call.stats_chunks = p.stats_chunks;
  call.bnr_chunks = p.bnr_chunks;
  if (p.aff_fused) call.aff_fused = 1;
  call.path |= p.path;
}

namespace {

// plan, and when there is one, apply and launch it: 1 launched, 0 not eligible (a and call untouched),
// < 0 error
int ring_run(ConvArgs& a, int mode, ConvCall& call, int eb, hipStream_t st) {
  RingPlan p;
  const int rc = ring_plan(a, mode, call, eb, g_sw.f32_split, g_sw, p);
  if (rc <= 0) return rc;
  ring_apply(p, a, call);
  ++g_conv_launches;
  const bool ok = p.key.family == RK_RING ? (eb == 2 ? conv_ring_bf16_launch(p, a, st) : conv_ring_f32_launch(p, a, st))
                  : p.key.family == RK_WGRAD_RING ? wgrad_ring_launch(p, a, st) : conv_persist_launch(p, a, st);
  if (!ok) {
    es_set_error("conv ring: no kernel for family %d mode %d tile %d x %d sp %d bk %d eb %d spl %d flag %d", p.key.family,
                 p.key.mode, p.key.bm, p.key.bn, p.key.sp, p.key.bk, p.key.eb, p.key.spl, p.key.flag);
    return -1;
  }
  return 1;
}

// Ring launches over chunks of nc images (operands of eb bytes per value): each chunk on offset base
// pointers with its first image as the dynamic-rows base, under a call context of its own.  FWD
// statistics partials are appended chunk after chunk and the call reports their sum (0 when a chunk
// wrote none); the fused BatchNorm-backward reduction of the persistent DGRAD is not offered to chunks
// (the caller runs the reduction pass).  bf16 WGRAD: the chunks' atomic accumulations into dW.  The
// first chunk's "not eligible" is the call's; a later chunk's is an error.  (One loop for any number
// of chunks, a single one included.)
int ring_launch_chunks(ConvArgs& a, int mode, int nc, int eb, ConvCall& call, hipStream_t st) {
  const es_conv_desc_t& d = a.d;
  const int esz = a.out_bf16 ? 2 : 4;
  int used = 0;
  bool stats_ok = call.stats_part != nullptr;
  for (int n0 = 0; n0 < d.N; n0 += nc) {
    ConvArgs c = a;
    c.d.N = std::min(nc, d.N - n0);
    c.nbase = a.nbase + n0;
    c.a_src = (const char*)a.a_src + (int64_t)n0 * a.as[0] * eb;
    if (mode == MODE_WGRAD) {
      c.b_src = (const char*)a.b_src + (int64_t)n0 * a.bs[0] * eb;
      c.Kd = c.d.N * d.P * d.Q;
    } else {
      c.out = (char*)a.out + (int64_t)n0 * a.os[0] * esz;
      c.M = mode == MODE_FWD ? c.d.N * d.P * d.Q : (int)dgrad_rows(d, c.d.N);
    }
    ConvCall cc;
    cc.aff = call.aff;
    if (call.stats_part) {
      cc.stats_part = call.stats_part + (int64_t)used * 3 * a.Ng;
      cc.stats_floats = call.stats_floats - (int64_t)used * 3 * a.Ng;
    }
    if (eb == 4) c.prio = SPL_PRIO;
    const int rc = ring_run(c, mode, cc, eb, st);
    if (rc <= 0) {
      if (n0 == 0) return rc;
      es_set_error(eb == 2 ? "conv bf16 ring: image chunk at %d not eligible" : "conv f32 ring: chunk %d not eligible",
                   n0);
      return -1;
    }
    stats_ok = stats_ok && cc.stats_chunks > 0;
    used += cc.stats_chunks;
    call.aff_fused |= cc.aff_fused;
    call.path |= cc.path;
  }
  call.stats_chunks = stats_ok ? used : 0;
  return 1;
}

}  // namespace

// bf16 operands: FWD / DGRAD / WGRAD.  1 launched, 0 not eligible (nothing launched), < 0 error
int es_conv_ring_launch(ConvArgs& a, int mode, ConvCall& call, hipStream_t st) {
  const es_conv_desc_t& d = a.d;
  const bool sp_weights = d.subpixel != 0;   // FWD / DGRAD operands packed for the sub-pixel path
  if (!g_sw.ring && !sp_weights) return 0;
  if (d.hmap != nullptr || d.stride > 2 || a.splitk) return sp_weights ? -1 : 0;
  // gathered operands of >= 1 GiB (a capacity-2048 expert's conv_layers.5 output gradient is 1.1 GB
  // in bf16): launches over image chunks below the limit, as the fp32 ring does
  const int64_t img = (mode == MODE_WGRAD ? std::max<int64_t>(a.as[0], a.bs[0]) : a.as[0]) * 2;
  const int nc = ring_chunk_images(img, d.N, g_sw);
  if (nc < d.N) return ring_launch_chunks(a, mode, nc, 2, call, st);
  return ring_run(a, mode, call, 2, st);
}

// fp32 operands, FWD / DGRAD: same return convention
int es_conv_ring_launch_f32(ConvArgs& a, int mode, ConvCall& call, hipStream_t st) {
  const es_conv_desc_t& d = a.d;
  if (mode == MODE_WGRAD || d.hmap != nullptr || d.stride > 2 || a.splitk) return d.subpixel ? -1 : 0;
  return ring_launch_chunks(a, mode, ring_chunk_images(a.as[0] * 4, d.N, g_sw), 4, call, st);
}

// ---------------------------------------------------------------- deterministic fp32 WGRAD
bool wgrad_f32_plan(const es_conv_desc_t& d, const int64_t ys[4], const int64_t xs[4], const RingSwitches& sw,
                    WgF32Plan& p) {
  if (!sw.ring || d.hmap != nullptr || d.stride > 2) return false;
  if (!dense(ys, d.K, d.P, d.Q) || !dense(xs, d.C, d.H, d.W)) return false;
  if (d.K % 64 || d.C % 64) return false;
  const int split = sw.f32_split;
  int bm = d.K % 128 == 0 ? 128 : 64;
  int bn = d.C % 256 == 0 && bm == 128 ? 256 : (d.C % 128 == 0 ? 128 : 64);
  // split-fp32 with 64 output channels: 64 x 512 tiles (8 waves of 64 x 64, the per-wave shape of the
  // 128 x 256 tiles; 64 x 128 tiles make the in-kernel split VALU-bound: 1.59 ms vs 1.41 exact for
  // conv_layers.9 at B = 1024, so the other 64-row tiles stay exact)
  p.sp = sw.subpixel && d.up_h == 2 && d.up_w == 2 && d.stride == 1;
  if (split && bm == 64 && !p.sp && (d.R * d.S * d.C) % 512 == 0) bn = 512;
  const bool col = split && !p.sp && d.R == 2 && d.S == 2 && d.stride == 1 && d.Hu == d.H && d.Wu == d.W &&
                   d.C == 128 && d.K == 64;
  p.spg = SubPixel{};
  int taps = d.R * d.S;
  p.npix = d.P * d.Q;
  if (p.sp) {
    es_make_subpixel(d, 0, p.spg);
    taps = p.spg.tap0[4];
    p.npix = 0;
    for (int c = 0; c < 4; ++c) p.npix = std::max(p.npix, p.spg.ph[c] * p.spg.pw[c]);
  }
  p.ngt = taps * d.C;
  p.nc = ring_chunk_images(std::max(ys[0], xs[0]) * 4, d.N, sw);
  p.nchunks = (d.N + p.nc - 1) / p.nc;
  const int tiles = (d.K / bm) * (p.ngt / bn);
  const int ks = p.npix * ((p.nc + 31) / 32);   // K-steps of a full chunk (the largest class)
  // one round of 256 one-workgroup-per-CU tiles, >= 16 K-steps per split
  p.sc = std::max(1, std::min(256 / std::max(tiles, 1), ks / 16));
  // the partial kernel: the 2 x 2 column kernel, the wave-specialised / cooperative split kernels of
  // the 128-row tiles, else wgrad_f32_kernel (split arithmetic on its 64 x 512 tile only)
  p.ws = 0;
  if (col) {
    p.key = wgrad_col2_key();
    p.npix = d.P * (d.Q + 1);
  } else if (split && bm == 128) {
    p.key = wgrad_coop_key(bm, bn, p.sp);
    p.ws = sw.wgrad_ws;
  } else {
    p.key = wgrad_f32_key(bm, bn, p.sp, split && bn == 512);
  }
  return true;
}

int64_t es_wgrad_f32_ring_floats(const es_conv_desc_t& d, const int64_t ys[4], const int64_t xs[4]) {
  WgF32Plan p;
  if (!wgrad_f32_plan(d, ys, xs, g_sw, p)) return -1;
  return (int64_t)p.nchunks * p.sc * d.K * p.ngt;
}

// launches the partial kernels (into call.det_ws) and the reduce into dw (torch layout); 1 done, 0 not
// eligible
int es_wgrad_f32_ring(const es_conv_desc_t& d, const void* dy, const int64_t ys[4], const void* x,
                      const int64_t xs[4], float* dw, float beta, ConvCall& call, hipStream_t st) {
  WgF32Plan p;
  if (!wgrad_f32_plan(d, ys, xs, g_sw, p)) return 0;
  float* ws = call.det_ws;
  const int64_t need = (int64_t)p.nchunks * p.sc * d.K * p.ngt;
  if (ws == nullptr || call.det_floats < need) {
    es_set_error("conv wgrad det: workspace of %lld floats, %lld needed", (long long)call.det_floats, (long long)need);
    return -1;
  }
  for (int ch = 0; ch < p.nchunks; ++ch) {
    const int n0 = ch * p.nc;
    ConvArgs a{};
    a.d = d;
    a.prio = SPL_PRIO;
    a.d.N = std::min(p.nc, d.N - n0);
    a.nbase = n0;
    a.a_src = (const char*)dy + (int64_t)n0 * ys[0] * 4;
    a.b_src = (const char*)x + (int64_t)n0 * xs[0] * 4;
    for (int i = 0; i < 4; ++i) { a.as[i] = ys[i]; a.bs[i] = xs[i]; }
    a.fUh = mkdiv(d.up_h > 0 ? d.up_h : 1); a.fUw = mkdiv(d.up_w > 0 ? d.up_w : 1);
    a.M = d.K;
    a.sp = p.spg;
    const int ks = p.npix * ((a.d.N + 31) / 32);
    a.k_per_split = (ks + p.sc - 1) / p.sc;
    float* wsc = ws + (int64_t)ch * p.sc * d.K * p.ngt;
    const int grid[3] = {d.K / p.key.bm, p.ngt / p.key.bn, p.sc};
    ++g_conv_launches;
    if (p.ws && es_wgrad_ws_launch(p.key.bn, p.sp, dim3(grid[0], grid[1], grid[2]), a, wsc, p.ngt, st) == 1) continue;
    if (!wgrad_f32_launch(p.key, grid, a, wsc, p.ngt, st)) {
      es_set_error("conv wgrad det: no kernel for family %d tile %d x %d sp %d spl %d", p.key.family, p.key.bm, p.key.bn,
                   p.key.sp, p.key.spl);
      return -1;
    }
  }
  wgrad_reduce_launch(ws, p.nchunks * p.sc, d.K, d.C, d.R, d.S, p.ngt, p.spg, dw, beta, st);
  call.path |= PATH_RING | (g_sw.f32_split ? PATH_SPLIT : 0) | (p.sp ? PATH_SUBPIXEL : 0);
  return 1;
}

// reduce of generic per-split partials ws[split][K][R*S*C] (conv_igemm / thin WGRAD, deterministic
// mode) into dW (torch layout)
void es_wgrad_reduce_plain(const float* ws, int splits, int K, int C, int R, int S, float* dw, float beta,
                           hipStream_t st) {
  SubPixel none{};
  wgrad_reduce_launch(ws, splits, K, C, R, S, R * S * C, none, dw, beta, st);
}
