// 8-wave LDS-DMA ring kernels for the bf16 implicit-GEMM convolutions (the generator convs of
// neutron/generator.py:24,29,33 and proton/generator.py:27,33,38 and the aux-regressor convs:
// everything whose K-step is one filter tap over 64 contiguous channels).
//
// Same products as conv_igemm_kernel.h (FWD: y = conv(x, W); DGRAD: dx with the integer upsample
// folded; WGRAD: dW), re-tiled for gfx950:
//   * 512 threads = 8 waves, one workgroup per CU (the 3-slot ring takes up to 144 KiB of the
//     160 KiB LDS), two waves per SIMD, each wave a 64x64 (64x32 / 32x64) tile of
//     v_mfma_f32_16x16x32_bf16;
//   * block tiles 256x128 (FWD/DGRAD) and 128x256 / 256x128 (WGRAD): 48 KiB of operands per
//     64-deep K-step for 4.2 MFLOP;
//   * operands go global -> LDS by DMA (buffer_load_dwordx4 ... lds, 1 KiB per wave instruction,
//     no register round trip) into a 3-slot ring: at step t a wave waits only for ITS pieces of
//     slot t (s_waitcnt vmcnt(pieces per slot): slot t+1 stays in flight), one s_barrier, then it
//     issues slot t+2 into the slot everyone finished reading at t-1 and runs the MFMAs of t;
//   * IMAGE-MINOR ROW ORDER.  GEMM rows (FWD/DGRAD) and GEMM K (WGRAD) enumerate pixels as
//     (image group g of 64 images, pixel, image within the group): m = (g*PQ + pix)*64 + nl.
//     Each 8-row DMA piece (and each 64-deep WGRAD K-step) is then 8 (64) images at ONE pixel,
//     so the im2col gather address of a piece is a per-lane constant (image nl) plus a
//     WAVE-UNIFORM pixel/tap offset computed on the scalar unit: one VALU add per piece per
//     K-step instead of a per-lane coordinate decode (which made the first version VALU-issue
//     bound at ~4x the MFMA time).  Padding / out-of-image taps are uniform per piece and use an
//     out-of-range buffer offset, which the buffer unit returns as zeros; images beyond N fall
//     outside the buffer's num_records the same way;
//   * workgroup ids are remapped so that consecutive tiles (same 64 images, neighbouring pixels)
//     run on one XCD and share its L2.
//
// LDS images (per slot):
//   FWD/DGRAD  [rows][128 B] per operand, 16-byte chunk c of row r stored at chunk
//              c ^ ((r >> 1) & 7): the 16-row ds_read_b128 fragment reads are conflict-free.
//   WGRAD      [64 images][rows] per operand (rows contiguous in global memory: channels), read
//              with ds_read_b64_tr_b16; chunk c of k-row k stored at c ^ (2(k&3) | 8((k>>3)&1)).
#pragma once
#include "ring_device.h"
#include "ring_plan.h"
#include "split_fp32.h"

namespace {

// split-fp32 SPB loop (8-wave FWD / DGRAD): column tiles of B planes read ahead of their MFMAs
constexpr int SPB_PFD = 2;
// SPB loop: column tile at which waves 4-7 issue their step's DMA (capped at RN - 1; waves 0-3 issue
// after column tile 0).  The two waves of a SIMD (w, w + 4) otherwise stall on their 7 LDS-DMA issues
// at the same point, leaving the SIMD's matrix pipe idle.  Measured (alternating A/B, B = 1024,
// ms/step): base 44.8-45.3; tile 2 45.34, 4 44.54, 5 44.60, 6 44.19 / 44.12, 7 44.05 / 44.50
// (conv_layers.5 FWD / DGRAD 3.15 / 3.05 -> 2.95 / 2.85 ms at 6).  Other placements (waves 0-3 later,
// the A(t+1) split of waves 4-7 moved, one fresh accumulator per two K-steps, the 4-wave SPB4 / SPA
// kernels, pre-split activation planes) measured slower or drifted and were removed in round 5
// (DESIGN.md §4 keeps the numbers).
constexpr int SPB_DMA_HI = 6;

// split-fp32 helpers (split_pair / split8 / mfma_split6): split_fp32.h

// ---------------------------------------------------------------------------------------------
// FWD / DGRAD.  Rows m = (g*PQ + pix)*64 + nl (image n = 64 g + nl, pixel pix on the row grid),
// columns = channels of the packed weight, K-step = one tap x 64 channels.
//
// SP (sub-pixel decomposition of a conv over a x2 nearest-upsampled input, SubPixel in
// conv_common.h): FWD row tiles belong to one parity class of output pixels and run the class's
// dh x dw conv on the SOURCE grid with combined weights (packed by es_pack_conv_weight mode 2);
// DGRAD rows are source pixels and the K-steps run over (class, d, e, channels) against the
// mode-3 packing.  3x3 taps on the upsampled grid become 4 taps on the source grid: 2.25x fewer
// MACs and gathered bytes for the same result (up to the rounding of the combined weights).
// ---------------------------------------------------------------------------------------------
//
// BK = 64: K-steps of 64 channels (128-byte slot rows), 3 slots, 4 x 2 waves.
// BK = 32 (256 x 256 tiles): K-steps of 32 channels (64-byte rows), 4 slots (three steps in flight),
// 2 x 4 waves of 128 x 64; per step 32 KiB of operands for 4.2 MFLOP (the 256 x 128 BK = 64 tile
// moves 48 KiB for the same work), and an A row tile is gathered once for 256 output channels.
//
// SPL == 2 (SPB; T = float, BK = 64: 32 fp32 channels per K-step): split-fp32 arithmetic.  A lane reads
// the 16-byte chunks g16 and g16 + 4 of its fragment row (channels 4 g16 .. +3 and 16 + 4 g16 .. +3),
// splits the 8 values into bf16 planes and issues the 6 plane products as v_mfma_f32_16x16x32_bf16.
// The B operand (packed weights) arrives pre-split: es_pack_weight_planes stores each 32-element K
// block of the fp32 packing as three 64-byte bf16 planes (192 bytes, k in the same permutation as
// the A fragments), so only A is split in the kernel.  (SPL is 0 or 2: level 1, both operands split
// in the kernel, was never selected and is gone.)  The slot holds B plane-major,
// [3][BN rows][64 B] (swizzled as the BK = 32 images), and the 8 waves are stacked along M (wave
// tile BM/8 x BN): every A element is split by one wave only.
//
// AFF (FWD only, es_conv2d_fwd_affine): the epilogue applies the per-output-channel affine and the
// activation of ConvArgs.epi_* to acc + bias before the rounding to the output dtype (an eval-mode
// BatchNorm -> LeakyReLU chain, neutron/generator.py:13-36, folded by es_bn_fold).  A template
// parameter: the instantiations without it are the code they were before it existed.
template <int MODE, int BM, int BN, bool SP, int BK = 64, typename T = bf16, int SPL = 0, bool AFF = false>
__global__ void __launch_bounds__(RT) conv_ring_kernel(ConvArgs a) {
  static_assert(SPL == 0 || (SPL == 2 && sizeof(T) == 4 && BK == 64), "split-fp32: fp32 operands, 128-byte slot rows");
  static_assert(!AFF || MODE == MODE_FWD, "affine epilogue: FWD only");
  constexpr bool SPB = SPL == 2;
  constexpr int NW = 8, NT = 64 * NW;                    // waves / threads per workgroup
  constexpr int WGM = SPB ? NW : (BK == 32 ? 2 : 4), WGN = NW / WGM;   // waves along M / N
  constexpr int WM = BM / WGM, WN = BN / WGN;
  constexpr int RM = WM / 16, RN = WN / 16;
  constexpr int ROWB = BK * 2, PROWS = 1024 / ROWB;      // slot row bytes, rows per 1 KiB piece
  constexpr int EB = sizeof(T), BKC = ROWB / EB;         // operand bytes, channels per K-step (fp32: BK / 2)
  constexpr int EA = EB;                                 // bytes per value of the gathered (A) image
  constexpr int CPR = ROWB / 16;                         // 16-byte chunks per row
  constexpr int EBB = SPB ? 6 : EB;                      // bytes per B element in global memory
  constexpr int BPL = BN / 16;                           // SPB: 1 KiB pieces per B plane
  constexpr int BPIECES = SPB ? 3 * BPL : BN / PROWS;    // (SPB, BN = 64: 12 pieces + 4 zero-fill dummies)
  constexpr int APW = BM / PROWS / NW, BPW = (BPIECES + NW - 1) / NW;   // pieces per wave per slot
  constexpr int PW = APW + BPW;
  constexpr int ABYTES = BM * ROWB, BBYTES = SPB ? 3 * BN * 64 : BN * ROWB;
  constexpr int SLOT = ABYTES + BBYTES;
  // SPB ring depths: three full slots when they fit (NS = 3); else A gets three slots and B (the
  // weights, L2-resident) two: A stays two steps ahead, B one (SPLITD)
  constexpr bool SPLITD = SPB && 3 * SLOT > 144 * 1024;
  // (SPB 128 x 64: two slots, so that two workgroups share a CU and one's fill / epilogue overlaps
  // the other's MFMAs, as the short-K bf16 tiles do)
  constexpr int NS = SPB ? (BM == 128 && BN == 64 ? 2 : 3) : (BK == 32 ? 4 : NSLOT);
  constexpr int KH = BK == 64 ? 2 : 1;                   // MFMA K-halves per step
  constexpr int RMF = RM / (3 - KH);                     // A tiles per fragment set
  constexpr int SROWS = WM < 64 ? WM : 64;               // epilogue staging rows per pass
  constexpr int STAGE0 = NW * SROWS * (WN * 4 + 16);
  constexpr int TPITCH = BN * 2 + 16;                    // BK = 32 bf16 epilogue: whole-tile image
  constexpr int STAGE = BK == 32 && BM * TPITCH > STAGE0 ? BM * TPITCH : STAGE0;
  constexpr int RINGB = SPLITD ? 3 * ABYTES + 2 * BBYTES : NS * SLOT;
  constexpr int RING = RINGB > STAGE ? RINGB : STAGE;
  constexpr int JUNK = BPW * NW > BPIECES ? 1024 : 0;    // landing area of the dummy pieces
  // ONE __shared__ object (a second one beside the DMA ring makes hipcc wait vmcnt(0) before
  // every ds_read of the loop): the ring slots (also the epilogue staging), then the fused-stats
  // scratch [3][WGM][BN] floats, which no DMA targets
  __shared__ __attribute__((aligned(16))) char smem[RING + 3 * WGM * BN * 4 + JUNK];
  const es_conv_desc_t& d = a.d;
  const int NL = conv_live(a);   // live images (dynamic rows)
  const SubPixel& sp = a.sp;

  // Row order: image groups g of NG = a.ng images (8..64); inside a group, per class (SP FWD: 4
  // parity classes, else one) the class's pixels in tiles of NB = BM/NG pixels (each class
  // segment padded to whole tiles); a tile is NG images x NB pixels, a DMA piece (8 rows) is 8
  // images at one pixel.  Consecutive tiles (one XCD) stay on the same images, so their sources
  // share the L2; the host picks NG per operand (small groups keep a forward gather's source
  // footprint inside one XCD's L2).
  const int NG = a.ng, PPG = NG / PROWS;                 // pieces per pixel
  const int NB = BM / NG;
  int TT;                                                // row tiles per image group
  if constexpr (MODE == MODE_FWD && SP) TT = a.sp_merge ? sp.tile0[1] : (a.sp_tpc > 0 ? 4 * a.sp_tpc : sp.tile0[4]);
  else if constexpr (MODE == MODE_FWD) TT = (d.P * d.Q + NB - 1) / NB;
  else TT = ((a.fold ? d.H * d.W : d.Hu * d.Wu) + NB - 1) / NB;
  // tile order: the column tiles of one row tile are consecutive (they share the gathered rows).
  // Dynamic rows: the tiles of the live image groups (a prefix) are the ones remapped over the
  // XCDs, so that they spread over the whole chip; the others exit below.
  const int nt = gridDim.y, ntot = gridDim.x * nt, lin = blockIdx.x + blockIdx.y * gridDim.x;
  const int nlive = NL == d.N ? ntot : min(ntot, (NL + NG - 1) / NG * TT * nt);
  const int wg = lin < nlive ? xcd_remap(lin, nlive) : lin;
  const int tl = wg / nt, n0 = (wg % nt) * BN;
  int cls = 0, gh, gw, jt;
  if constexpr (MODE == MODE_FWD && SP) {
    if (a.sp_merge) {
      // merged classes: the rows are the (shared) source pixels of class 0's geometry, the
      // columns (class, channel); the class is resolved per wave in the epilogue
      jt = tl % TT;
    } else if (a.sp_tpc > 0) {
      // class-interleaved: tile r = 4 jt + class, so the 4 class tiles of the same source
      // pixels run back to back (one XCD, shared L2); classes with fewer tiles skip the tail
      const int r = tl % TT;
      cls = r & 3;
      jt = r >> 2;
      if (jt >= sp.tile0[cls + 1] - sp.tile0[cls]) {
        if (a.stats_part) {   // empty partial (count 0) for this tile
          float* pp = a.stats_part + (int64_t)tl * 3 * a.Ng;
          for (int c = threadIdx.x; c < BN; c += NT)
            if (n0 + c < a.Ng) pp[n0 + c] = 0.f;
        }
        return;
      }
    } else {
      const int r = tl % TT;
      cls = (r >= sp.tile0[1]) + (r >= sp.tile0[2]) + (r >= sp.tile0[3]);
      jt = r - sp.tile0[cls];
    }
    gh = sp.ph[cls];
    gw = sp.pw[cls];
  } else {
    if constexpr (MODE == MODE_FWD) {
      gh = d.P;
      gw = d.Q;
    } else {
      gh = a.fold ? d.H : d.Hu;
      gw = a.fold ? d.W : d.Wu;
    }
    jt = tl % TT;
  }
  const int PQ = gh * gw;
  const int gi = tl / TT;                                // image group: images NG gi ..
  const int pix0 = jt * NB;                              // first pixel of the tile
  if (gi * NG >= NL) {   // past the live images (dynamic rows): an empty partial, no work
    if (MODE == MODE_FWD && a.stats_part) {
      for (int c = threadIdx.x; c < BN; c += NT) {
        const int gc = n0 + c, cc = a.sp_merge ? gc / a.Ng : 0, ch = gc - cc * a.Ng;
        if (cc < 4 && ch < a.Ng) {
          float* pp = a.stats_part + (int64_t)(a.sp_merge ? tl * 4 + cc : tl) * 3 * a.Ng;
          pp[ch] = 0.f;
          pp[a.Ng + ch] = 0.f;
          pp[2 * a.Ng + ch] = 0.f;
        }
      }
    }
    return;
  }

  const int lane = threadIdx.x & 63, wid = uni(threadIdx.x >> 6);
  const int wm0 = (wid / WGN) * WM, wn0 = (wid % WGN) * WN;
  const int lrow = lane / CPR, pc = lane % CPR;

  const __amdgpu_buffer_rsrc_t ares = mkres(a.a_src, (uint32_t)(NL * a.as[0] * EA));
  // packed weights: row stride ldb (elements) and the class's block offset
  int ldb, bbase = 0, bbytes;
  if constexpr (SP && MODE == MODE_FWD) {
    ldb = sp.dh[cls] * sp.dw[cls] * d.C;
    bbase = sp.tap0[cls] * a.Ng * d.C;
    bbytes = sp.tap0[4] * a.Ng * d.C * EBB;
  } else if constexpr (SP) {
    ldb = sp.tap0[4] * d.K;
    bbytes = a.Ng * ldb * EBB;
  } else {
    ldb = (MODE == MODE_DGRAD && a.fold) ? d.R * d.S * d.K : a.Kd;
    bbytes = a.Ng * ldb * EBB;
  }
  const __amdgpu_buffer_rsrc_t bres = mkres(a.b_src, (uint32_t)bbytes);
  const int as2b = (int)a.as[2] * EA, as3b = (int)a.as[3] * EA;

  // A pieces: per-lane constant (image, 16-byte chunk) + per-piece uniform pixel coordinates.
  constexpr int APC = APW, ALN = APW;
  uint32_t alane[ALN];
  int pc0[APC], pc1[APC];
  bool pval[APC];
#pragma unroll
  for (int j = 0; j < ALN; ++j) {
    const int pi = wid * APW + j;                 // piece of the tile: pixel pix0 + pi / PPG
    const int rr = pi * PROWS + lrow;             // row within the tile (swizzle)
    const int lc = pc ^ swz_x<BK>(rr);
    const int ppix = pi / PPG;
    const int pix = pix0 + ppix;
    pval[j] = pix < PQ;
    const int pp = pval[j] ? pix : 0;
    const int y = pp / gw, x = pp - y * gw;
    const int img = gi * NG + (pi - ppix * PPG) * PROWS + lrow;
    alane[j] = (uint32_t)(img * (int)a.as[0] * EB + lc * 16);   // images >= N: past num_records
    if constexpr (MODE == MODE_FWD && SP) {       // source row = u + oh + d
      pc0[j] = y + sp.oh[cls];
      pc1[j] = x + sp.ow[cls];
    } else if constexpr (MODE == MODE_FWD) {
      pc0[j] = y * d.stride - d.pad;
      pc1[j] = x * d.stride - d.pad;
    } else if constexpr (SP) {                    // source pixel (i, j)
      pc0[j] = y;
      pc1[j] = x;
    } else if (a.fold) {
      pc0[j] = y * d.up_h + d.pad;
      pc1[j] = x * d.up_w + d.pad;
    } else {
      pc0[j] = y + d.pad;
      pc1[j] = x + d.pad;
    }
  }
  constexpr int BLN = BPW;
  uint32_t blane[BLN];
#pragma unroll
  for (int j = 0; j < BLN; ++j) {
    if constexpr (SPB) {   // piece q: plane q / BPL, rows 16 (q % BPL) + lane / 4, 16-byte chunk lane % 4
      const int q = wid * BPW + j;
      const int rr = (q % BPL) * 16 + (lane >> 2);
      blane[j] = q < BPIECES ? (uint32_t)((bbase + (n0 + rr) * ldb) * EBB + (q / BPL) * 64 +
                                          (((lane & 3) ^ swz_x<32>(rr)) * 16))
                             : OOB;
    } else {
      const int rr = (wid * BPW + j) * PROWS + lrow;
      // rows past Ng read garbage columns that the epilogue drops (or zeros past num_records)
      blane[j] = (uint32_t)((bbase + (n0 + rr) * ldb) * EB + ((pc ^ swz_x<BK>(rr)) * 16));
    }
  }

  // K-step cursor (uniform, advanced once per issued slot).
  //   FWD      kk = ((r*S + s)*C + ch)                      (SP: taps d < dh, e < dw of the class)
  //   DGRAD    kk = (((ua*up_w + ub)*R + r)*S + s)*K + ch  with weight column kb = kk mod R*S*K
  //   DGRAD SP kk = ((class, d, e), ch)                    with column (tap0[class] + d*dw + e)*K + ch
  int cr = 0, cs = 0, cch = 0, cua = 0, cub = 0, ckb = 0, ccls = 0, cstep = 0;
  const int nch = MODE == MODE_FWD ? d.C : d.K;
  const int upw = d.up_w > 0 ? d.up_w : 1;
  int nk;
  if constexpr (SP && MODE == MODE_FWD) nk = ldb / BKC;
  else if constexpr (SP) nk = ldb / BKC;
  else nk = a.Kd / BKC;
  ClsReg Roh, Row, Rph, Rpw, Rp0, Rq0, Rtap0, Rdh, Rdw;
  if constexpr (SP && MODE == MODE_DGRAD) {
    Roh.init(sp.oh); Row.init(sp.ow); Rph.init(sp.ph); Rpw.init(sp.pw); Rp0.init(sp.p0); Rq0.init(sp.q0);
    Rtap0.init(sp.tap0); Rdh.init(sp.dh); Rdw.init(sp.dw);
  }
  int kh = SP ? uni(sp.dh[cls]) : d.R, kw = SP ? uni(sp.dw[cls]) : d.S;   // taps of the cursor's class
  // Per-tap cache: the pieces' offsets only change when the cursor enters a new tap (every
  // nch / BK steps); inside a tap a step adds BK channels.  Recomputing them every step cost
  // ~100 scalar instructions per K-step, which made the loop issue-bound (the CU's scalar unit
  // is shared by its 8 waves).
  uint32_t ua_t[APC], ub_t = 0;
#pragma unroll
  for (int j = 0; j < APC; ++j) ua_t[j] = OOB;
  auto issue = [&](char* slot) {
    if (cch == 0) {   // first step of a tap (wave-uniform branch, scalar work only)
      const bool live = cstep < nk;
#pragma unroll
      for (int j = 0; j < APC; ++j) {
        uint32_t u;
        if constexpr (MODE == MODE_FWD && SP) {
          const int hs = pc0[j] + cr, ws = pc1[j] + cs;
          const bool ok = live && pval[j] && (unsigned)hs < (unsigned)d.H && (unsigned)ws < (unsigned)d.W;
          u = ok ? (uint32_t)(hs * as2b + ws * as3b) : OOB;
        } else if constexpr (MODE == MODE_FWD) {
          const int hu = pc0[j] + cr, wu = pc1[j] + cs;
          const bool ok = live && pval[j] && (unsigned)hu < (unsigned)d.Hu && (unsigned)wu < (unsigned)d.Wu;
          // integer nearest upsample folded into the gather (factor 1 without upsample)
          const int sh = fdiv(hu, a.fUh), sw = fdiv(wu, a.fUw);
          u = ok ? (uint32_t)(sh * as2b + sw * as3b) : OOB;
        } else if constexpr (SP) {
          // output pixel (p0 + 2u, q0 + 2v) of class ccls feeds source pixel u + oh + d
          const int uu = pc0[j] - cr - Roh(ccls), vv = pc1[j] - cs - Row(ccls);
          const bool ok = live && pval[j] && (unsigned)uu < (unsigned)Rph(ccls) &&
                          (unsigned)vv < (unsigned)Rpw(ccls);
          u = ok ? (uint32_t)((Rp0(ccls) + 2 * uu) * as2b + (Rq0(ccls) + 2 * vv) * as3b) : OOB;
        } else {
          const int ph = pc0[j] + cua - cr, pw = pc1[j] + cub - cs;
          const int sh = d.stride == 2 ? 1 : 0;
          const bool ok = live && pval[j] && ph >= 0 && pw >= 0 && !(((ph | pw) & sh)) &&
                          (ph >> sh) < d.P && (pw >> sh) < d.Q;
          u = ok ? (uint32_t)((ph >> sh) * as2b + (pw >> sh) * as3b) : OOB;
        }
        ua_t[j] = u;
      }
      int kb;
      if constexpr (MODE == MODE_FWD) kb = (cr * kw + cs) * d.C;
      else if constexpr (SP) kb = (Rtap0(ccls) + cr * kw + cs) * d.K;
      else kb = ckb;
      ub_t = live ? (uint32_t)(kb * EBB) : OOB;
    }
    // (OOB + a channel offset stays past every num_records: offsets are < 1 GiB)
    const uint32_t co = (uint32_t)(cch * EA), cob = (uint32_t)(cch * EBB);
#pragma unroll
    for (int j = 0; j < APW; ++j) bdma16(ares, alane[j] + (ua_t[j] + co), slot + (wid * APW + j) * 1024);
    if constexpr (!SPB) {   // (SPB: B has its own ring and issue_b)
#pragma unroll
      for (int j = 0; j < BPW; ++j) {
        const int q = wid * BPW + j;
        char* dst = (!JUNK || q < BPIECES) ? slot + ABYTES + q * 1024 : smem + RING + 3 * WGM * BN * 4;
        bdma16(bres, blane[j] + (ub_t + cob), dst);
      }
    }
    ++cstep;
    cch += BKC;
    if (cch == nch) {   // tap done: advance the tap cursor (wave-uniform branch)
      cch = 0;
      ckb += nch;
      ++cs;
      const bool w2 = cs == kw;
      cs = w2 ? 0 : cs;
      cr += w2;
      const bool w3 = cr == kh;
      cr = w3 ? 0 : cr;
      ckb = w3 ? 0 : ckb;
      cub += w3;
      const bool w4 = cub == upw;
      cub = w4 ? 0 : cub;
      cua += w4;
      if constexpr (SP && MODE == MODE_DGRAD) {
        ccls += w3;
        const int cn = ccls < 4 ? ccls : 3;
        kh = Rdh(cn);
        kw = Rdw(cn);
      }
    }
  };

  f32x4 acc[RM][RN];
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment set kk: BK = 64 -> K half kk (all RM x RN tiles); BK = 32 -> the step's 32 channels
  // for A tiles kk*RM/2 .. (the wave's row half kk) and all RN B tiles
  const int r16 = lane & 15, g16 = lane >> 4;
  // (fp32: a lane's 16-byte chunk is 4 channels, fed to 4 v_mfma_f32_16x16x4_f32 with k = 4 g16 + t:
  // A and B use the same permutation of k, so each MFMA stays an exact fp32 FMA chain)
  typedef typename std::conditional<EB == 2, bf16x8, f32x4>::type FragT;
  struct Frag {
    FragT a[RMF], b[RN];
    int h;
  };
  auto load = [&](Frag& f, const char* slot, int kk) {
    const int seg = KH == 2 ? kk * 4 + g16 : g16;
    const int i0 = KH == 2 ? 0 : kk * RMF;
    f.h = kk;
#pragma unroll
    for (int i = 0; i < RMF; ++i) f.a[i] = *(const FragT*)(slot + swz<BK>(wm0 + (i0 + i) * 16 + r16, seg));
#pragma unroll
    for (int j = 0; j < RN; ++j) f.b[j] = *(const FragT*)(slot + ABYTES + swz<BK>(wn0 + j * 16 + r16, seg));
  };
  auto mma = [&](const Frag& f) {
    const int i0 = KH == 2 ? 0 : f.h * RMF;
#pragma unroll
    for (int i = 0; i < RMF; ++i)
#pragma unroll
      for (int j = 0; j < RN; ++j) {
        if constexpr (EB == 2) {
          acc[i0 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.a[i], f.b[j], acc[i0 + i][j], 0, 0, 0);
        } else {
#pragma unroll
          for (int t = 0; t < 4; ++t)
            acc[i0 + i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a[i][t], f.b[j][t], acc[i0 + i][j], 0, 0, 0);
        }
      }
  };
  if constexpr (SPB) {
    // Software-pipelined split-fp32 loop.  A (activations, fp32) and B (pre-split weight planes) have
    // their own rings: A in NSA slots, B in NSB.  Step t's MFMAs use A planes split during step t-1
    // (registers) and B(t) read from LDS per column tile; under them the wave reads A(t+1) and splits
    // it, and issues the DMA of B(t+NSB-1) / A(t+NSA).  Slot reuse: A(s) is read during step s-1 and
    // B(s) during step s, so behind the barrier of step t the slots of A(t) and B(t-1) are free.
    // Issue order A(0), B(0), A(1), [B(1), A(2)] ..., then per step B(t+NSB-1), A(t+NSA): at the top
    // of step t everything but the last (NSA-2) A and (NSB-2) B groups has landed, i.e. B(t), A(t+1).
    constexpr int NSA = SPLITD ? 3 : NS, NSB = SPLITD ? 2 : NS;
    constexpr int PROWAIT = (NSA - 1) * APW + (NSB - 1) * BPW, LOOPWAIT = (NSA - 2) * APW + (NSB - 2) * BPW;
    char* const aring = smem;
    char* const bring = smem + NSA * ABYTES;
    // B step s: the packed weight columns are K-linear, so its offset is (s mod period) * BKC elements
    // (DGRAD with a folded upsample repeats the R*S*K columns per upsample phase)
    const int bper = (MODE == MODE_DGRAD && !SP) ? (d.R * d.S * d.K) / BKC : nk;
    int bs = 0, bsm = 0;
    auto issue_b = [&](char* bslot) {
      const uint32_t ub = bs < nk ? (uint32_t)(bsm * BKC * EBB) : OOB;
#pragma unroll
      for (int j = 0; j < BPW; ++j) {
        const int q = wid * BPW + j;
        char* dst = (!JUNK || q < BPIECES) ? bslot + q * 1024 : smem + RING + 3 * WGM * BN * 4;
        bdma16(bres, blane[j] + ub, dst);
      }
      ++bs;
      bsm = bsm + 1 == bper ? 0 : bsm + 1;
    };
    auto rd_a = [&](f32x4 (&r)[RM][2], const char* aslot) {
#pragma unroll
      for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int h = 0; h < 2; ++h) r[i][h] = *(const f32x4*)(aslot + swz<BK>(wm0 + i * 16 + r16, g16 + 4 * h));
    };
    auto rd_b = [&](bf16x8 (&bp)[3], const char* bimg, int j) {
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
        bp[pl] = *(const bf16x8*)(bimg + pl * (BN * 64) + swz<32>(wn0 + j * 16 + r16, g16));
    };
    if (a.prio && wid >= 4) __builtin_amdgcn_s_setprio(1);
    issue(aring);
#pragma unroll
    for (int st = 0; st < NSB - 1; ++st) {
      issue_b(bring + st * BBYTES);
      issue(aring + (st + 1) * ABYTES);
    }
#pragma unroll
    for (int st = NSB - 1; st < NSA - 1; ++st) issue(aring + (st + 1) * ABYTES);
    wait_vmcnt<PROWAIT>();
    ring_barrier();
    bf16x8 apc[RM][3];
    {
      f32x4 r[RM][2];
      rd_a(r, aring);
#pragma unroll
      for (int i = 0; i < RM; ++i) split8(r[i][0], r[i][1], apc[i]);
    }
    int sa1 = 1 % NSA, sb = 0, ia = 0, ib = NSB - 1;   // slots: A(t+1), B(t), A(t+NSA), B(t+NSB-1)
    constexpr int JS = RN > 2 ? RN / 2 : RN - 1;       // column tile after which A(t+1) is split
    constexpr int JDMA = SPB_DMA_HI < RN ? SPB_DMA_HI : RN - 1;
    for (int t = 0; t < nk; ++t) {
      wait_vmcnt<LOOPWAIT>();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's reads of the last step are done
      ring_barrier();
      const char* bimg = bring + sb * BBYTES;
      // B planes PFD column tiles ahead (LDS latency under load exceeds one tile's 12 MFMAs)
      constexpr int PFD = SPB_PFD;
      bf16x8 bq[PFD + 1][3];
#pragma unroll
      for (int j = 0; j < PFD && j < RN; ++j) rd_b(bq[j], bimg, j);
      f32x4 ra[RM][2];
      rd_a(ra, aring + sa1 * ABYTES);
      bf16x8 apn[RM][3];
#pragma unroll
      for (int j = 0; j < RN; ++j) {
        if (j + PFD < RN) rd_b(bq[(j + PFD) % (PFD + 1)], bimg, j + PFD);
#pragma unroll
        for (int i = 0; i < RM; ++i) acc[i][j] = mfma_split6(apc[i], bq[j % (PFD + 1)], acc[i][j]);
        // the step's DMA, once its first MFMAs are queued (STAGGER: the two waves of a SIMD, w and
        // w + 4, at different column tiles, so one issues MFMAs while the other stalls on the issue)
        if (j == (wid >= 4 ? JDMA : 0)) {
          issue_b(bring + ib * BBYTES);
          issue(aring + ia * ABYTES);
        }
        if (j == JS) {
#pragma unroll
          for (int i = 0; i < RM; ++i) split8(ra[i][0], ra[i][1], apn[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) apc[i][pl] = apn[i][pl];
      sa1 = sa1 + 1 == NSA ? 0 : sa1 + 1;
      ia = ia + 1 == NSA ? 0 : ia + 1;
      sb = sb + 1 == NSB ? 0 : sb + 1;
      ib = ib + 1 == NSB ? 0 : ib + 1;
    }
    wait_vmcnt<0>();   // drain the zero-fill steps before the workgroup may exit
  } else {
    auto nofence = [](Frag&) {};
    ring_loop<PW, 0, NS>(nk, smem, SLOT, issue, load, mma, nofence);
  }

  // epilogue.  Wave row r (0..WM-1) = tile row t = wm0 + r: pixel pix0 + t / NG, image
  // NG gi + t % NG.
  const int col16 = lane & 15, rq = (lane >> 4) * 4;
  // (no integer divisions per row: NG is a power of two and gw is divided by magic numbers; the
  // generic divides cost ~100 VALU per stored row, a third of the whole epilogue)
  const int lgNG = uni(31 - __builtin_clz(NG));
  FastDiv fgw;
  {
    uint32_t l = 0;
    while ((1u << l) < (uint32_t)gw) ++l;
    fgw.l = uni((int)l);
    fgw.m = (uint32_t)uni((int)(uint32_t)(((1ull << 32) * ((1ull << l) - (uint32_t)gw)) / (uint32_t)gw + 1));
  }
  auto row_pix = [&](int r) { return pix0 + ((wm0 + r) >> lgNG); };
  auto row_img = [&](int r) { return gi * NG + ((wm0 + r) & (NG - 1)); };
  // the wave's output columns: class ecls (merged sub-pixel FWD: column block / Ng), first
  // output channel kc0 (a wave's WN columns never straddle a class: Ng % 64 == 0)
  int ecls = cls, kc0 = n0 + wn0;
  if constexpr (SP && MODE == MODE_FWD) {
    if (a.sp_merge) {
      ecls = kc0 / a.Ng;
      kc0 -= ecls * a.Ng;
    }
  }
  auto row_off = [&](int r) -> int64_t {   // element offset of the wave row's output pixel
    const int pix = row_pix(r);
    int y = fdiv(pix, fgw), x = pix - y * gw;
    if constexpr (SP && MODE == MODE_FWD) {
      y = sp.p0[ecls] + 2 * y;
      x = sp.q0[ecls] + 2 * x;
    }
    return (int64_t)row_img(r) * a.os[0] + (int64_t)y * a.os[2] + (int64_t)x * a.os[3];
  };
  const int NLP = conv_live_px(a);   // pixel rows (rows_px > 0): image i pixel p live when i*PQ + p < NLP
  auto row_ok = [&](int r) { return row_pix(r) < PQ && row_img(r) < NL && row_img(r) * PQ + row_pix(r) < NLP; };
  // final values (bias added, rounded to the output dtype) back into acc
#pragma unroll
  for (int j = 0; j < RN; ++j) {
    const int ng = kc0 + j * 16 + col16;
    float bv = 0.f;
    if constexpr (MODE == MODE_FWD) bv = (a.bias && ng < a.Ng) ? a.bias[ng] : 0.f;
    if constexpr (AFF) {
      // scale * (acc + bias) + shift as one fma per value: shift' = scale * bias + shift
      const float sc = ng < a.Ng ? a.epi_scale[ng] : 0.f;
      const float sh = fmaf(bv, sc, ng < a.Ng ? a.epi_shift[ng] : 0.f);
      const float neg = a.epi_act == ES_ACT_LRELU ? a.epi_slope : (a.epi_act == ES_ACT_RELU ? 0.f : 1.f);
#pragma unroll
      for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          float v = fmaf(acc[i][j][jj], sc, sh);
          v = v > 0.f ? v : v * neg;
          acc[i][j][jj] = a.out_bf16 ? (float)(bf16)v : v;
        }
    } else {
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const float v = acc[i][j][jj] + bv;
        acc[i][j][jj] = a.out_bf16 ? (float)(bf16)v : v;
      }
    }
  }
  if (BK == 32 || a.vec_out) {   // (the host runs BK = 32 only with vec_out)
    // BatchNorm statistics of the stored values (conv -> BatchNorm fusion): per column, count /
    // mean / M2 over the wave's valid rows (lanes own 16 rows, Chan-merged across the 4 row
    // groups by shuffles), then across the 4 row waves in LDS -> one [3][Ng] partial per row tile
    float* part = MODE == MODE_FWD ? a.stats_part : nullptr;   // (FWD only: compiled out of DGRAD)
    float (*st_n)[BN] = (float (*)[BN])(smem + RING);
    float (*st_m)[BN] = st_n + WGM;
    float (*st_q)[BN] = st_n + 2 * WGM;
    if (part) {
      const int wmi = wid / WGN;
      bool okr[RM][4];
#pragma unroll
      for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) okr[i][jj] = row_ok(i * 16 + rq + jj);
      bool allok = true;
#pragma unroll
      for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) allok = allok && okr[i][jj];
      const bool full = __all(allok);   // wave-uniform: no row of the wave is padding
#pragma unroll
      for (int j = 0; j < RN; ++j) {
        float n_, m_, q;
        if (BK == 32 && full) {
          // 256 x 256 tiles: per column sum and sum of squares of the lane's 32 values (2 VALU per
          // value; the two-pass Chan form cost ~85 us of conv_layers.5's B = 1024 FWD epilogue),
          // summed over the 4 row groups, then (count, mean, M2) of the wave's 128 rows
          float s = 0.f, s2 = 0.f;
#pragma unroll
          for (int i = 0; i < RM; ++i)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
              const float v = acc[i][j][jj];
              s += v;
              s2 = fmaf(v, v, s2);
            }
#pragma unroll
          for (int o = 16; o <= 32; o <<= 1) {
            s += __shfl_xor(s, o, 64);
            s2 += __shfl_xor(s2, o, 64);
          }
          n_ = (float)(RM * 16);
          m_ = s * (1.f / (RM * 16));
          q = fmaxf(s2 - s * m_, 0.f);
        } else {
        float cnt = 0.f, s = 0.f;
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj)
            if (okr[i][jj]) { cnt += 1.f; s += acc[i][j][jj]; }
        const float mu = cnt > 0.f ? s / cnt : 0.f;
        q = 0.f;
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj)
            if (okr[i][jj]) { const float e = acc[i][j][jj] - mu; q += e * e; }
        n_ = cnt; m_ = mu;
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
          const float nb = __shfl_xor(n_, o, 64), mb = __shfl_xor(m_, o, 64), qb = __shfl_xor(q, o, 64);
          const float nt = n_ + nb;
          if (nt > 0.f) {
            const float dl = mb - m_, f = nb / nt;
            m_ += dl * f;
            q += qb + dl * dl * n_ * f;
          }
          n_ = nt;
        }
        }
        if (lane < 16) {
          st_n[wmi][wn0 + j * 16 + col16] = n_;
          st_m[wmi][wn0 + j * 16 + col16] = m_;
          st_q[wmi][wn0 + j * 16 + col16] = q;
        }
      }
    }
    if (BK == 32 && BN == 256 && a.out_bf16) {
      // The whole 256 x 256 tile is staged in LDS ([row][256 columns], pitch TPITCH), then every
      // store instruction writes two full 512-byte rows: tile rows t0 = (2 pp) NG + n and
      // t0 + NG, i.e. one image at two consecutive pixels.  Consecutive tile rows are different
      // images (image-minor order), so the per-wave staging below wrote 128-byte pieces of 8
      // images per instruction; with 1-KiB runs (merged sub-pixel FWD: pixels 2u..2u+3 of one
      // output row) the conv_layers.0 / .5 FWD epilogues drop from ~170 / ~245 us (B = 1024).
      __syncthreads();   // every wave is done with the ring slots
#pragma unroll
      for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
          for (int j = 0; j < RN; ++j)
            *(bf16*)(smem + (wm0 + i * 16 + rq + jj) * TPITCH + (wn0 + j * 16 + col16) * 2) = (bf16)acc[i][j][jj];
      __syncthreads();
      const int half = lane >> 5, kq = lane & 31;
      int scls = cls, sch = n0 + kq * 8;          // class / output channel of this lane's chunk
      if constexpr (SP && MODE == MODE_FWD) {
        if (a.sp_merge) {
          scls = sch / a.Ng;
          sch -= scls * a.Ng;
        }
      }
      const bool colok = sch < a.Ng && scls < 4;
      int py0 = 0, px0 = 0;
      if constexpr (SP && MODE == MODE_FWD) {
        py0 = (scls >> 1) ? sp.p0[2] : sp.p0[0];
        px0 = (scls & 1) ? sp.q0[1] : sp.q0[0];
      }
      for (int q = wid; q < BM / 2; q += 8) {
        const int t = ((2 * (q >> lgNG) + half) << lgNG) + (q & (NG - 1));
        const int pix = pix0 + (t >> lgNG), img = gi * NG + (t & (NG - 1));
        if (colok && pix < PQ && img < NL) {
          int y = fdiv(pix, fgw), x = pix - y * gw;
          if constexpr (SP && MODE == MODE_FWD) {
            y = py0 + 2 * y;
            x = px0 + 2 * x;
          }
          const int64_t o = (int64_t)img * a.os[0] + (int64_t)y * a.os[2] + (int64_t)x * a.os[3] + sch;
          *(uint4*)((bf16*)a.out + o) = *(const uint4*)(smem + t * TPITCH + kq * 16);
        }
      }
    } else {
    // stage the wave's tile in LDS (rows of WN values; passes of SROWS rows), then 16-byte
    // row-contiguous stores
    constexpr int PITCH = WN * 4 + 16;
    const int esz = a.out_bf16 ? 2 : 4;
    const int pitch = WN * esz + 16;
    char* stg = smem + wid * (SROWS * PITCH);
    const int cpr = WN * esz / 16;          // 16-byte chunks per row
    const int rpi = 64 / cpr;               // rows per wave instruction
    const int lr = lane / cpr, lch = lane % cpr;
#pragma unroll
    for (int ps = 0; ps < WM / SROWS; ++ps) {
      __syncthreads();   // every wave is done with the ring slots / the previous pass
#pragma unroll
      for (int i = 0; i < SROWS / 16; ++i)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
          for (int j = 0; j < RN; ++j) {
            char* p = stg + (i * 16 + rq + jj) * pitch + (j * 16 + col16) * esz;
            const float v = acc[ps * (SROWS / 16) + i][j][jj];
            if (a.out_bf16) *(bf16*)p = (bf16)v;
            else *(float*)p = v;
          }
      __syncthreads();
      if (kc0 + lch * 16 / esz < a.Ng) {
        char* obase = (char*)a.out + (int64_t)kc0 * esz + lch * 16;
        for (int r = lr; r < SROWS; r += rpi)
          if (row_ok(ps * SROWS + r)) {
            const int64_t ro = row_off(ps * SROWS + r);
            const f32x4 vv = *(const f32x4*)(stg + r * pitch + lch * 16);
            *(uint4*)(obase + ro * esz) = __builtin_bit_cast(uint4, vv);
          }
      }
    }
    }
    if (part && wid < WGN) {   // the waves of row block 0 merge the WGM row waves of their columns
      for (int c = lane; c < WN; c += 64) {
        const int col = wn0 + c;
        float n_ = st_n[0][col], m_ = st_m[0][col], q = st_q[0][col];
        for (int w = 1; w < WGM; ++w) {
          const float nb = st_n[w][col];
          if (nb > 0.f) {
            const float mb = st_m[w][col], nt = n_ + nb, dl = mb - m_, f = nb / nt;
            m_ += dl * f;
            q += st_q[w][col] + dl * dl * n_ * f;
            n_ = nt;
          }
        }
        const int kc = kc0 + c;
        if (kc < a.Ng) {
          // one partial per row tile (merged sub-pixel FWD: per row tile and class)
          float* pp = part + (int64_t)(a.sp_merge ? tl * 4 + ecls : tl) * 3 * a.Ng;
          pp[kc] = n_;
          pp[a.Ng + kc] = m_;
          pp[2 * a.Ng + kc] = q;
        }
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < RM; ++i) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int r = i * 16 + rq + jj;
      if (!row_ok(r)) continue;
      const int64_t rowoff = row_off(r);
#pragma unroll
      for (int j = 0; j < RN; ++j) {
        const int ng = n0 + wn0 + j * 16 + col16;
        if (ng >= a.Ng) continue;
        float v = acc[i][j][jj];
        const int64_t o = rowoff + (int64_t)ng * a.os[1];
        if (a.out_bf16) {
          bf16* yp = (bf16*)a.out + o;
          if (a.beta != 0.f) v += a.beta * (float)(*yp);
          *yp = (bf16)v;
        } else {
          float* yp = (float*)a.out + o;
          if (a.beta != 0.f) v += a.beta * (*yp);
          *yp = v;
        }
      }
    }
  }
}

// One table row per instantiation: the kernel files list the rows they build (conv_ring_bf16.hip,
// conv_ring_f32.hip).
typedef RingEntry<void (*)(const ConvArgs&, dim3, hipStream_t)> ConvRingEntry;
template <int MODE, int BM, int BN, bool SP, int BK, typename T, int SPL, bool AFF>
void launch_conv_ring(const ConvArgs& a, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((conv_ring_kernel<MODE, BM, BN, SP, BK, T, SPL, AFF>), grid, dim3(RT), 0, st, a);
}
template <int MODE, int BM, int BN, bool SP, int BK, typename T, int SPL, bool AFF = false>
constexpr ConvRingEntry ring_entry() {
  return {ring_key(MODE, BM, BN, SP, BK, sizeof(T), SPL, AFF), &launch_conv_ring<MODE, BM, BN, SP, BK, T, SPL, AFF>};
}
template <int N>
bool ring_table_launch(const ConvRingEntry (&table)[N], const RingPlan& p, const ConvArgs& a, hipStream_t st) {
  const ConvRingEntry* e = ring_find(table, p.key);
  if (e) e->launch(a, dim3(p.grid[0], p.grid[1], p.grid[2]), st);
  return e != nullptr;
}

}  // namespace
