// The persistent ring kernels: workgroups that loop over their tiles with the DMA ring running across
// tile boundaries (the short-K DGRAD of conv_layers.9 and the merged 256 x 256 sub-pixel FWD).
#include "ring_device.h"
#include "ring_plan.h"

namespace {

// ---------------------------------------------------------------------------------------------
// PERSISTENT short-K DGRAD: the input gradient of the generator's conv_layers.9
// (neutron/generator.py:33, 2x2 taps x 128 channels -> 64: 4 K-steps, 128 output columns); stride 1,
// no upsample, no sub-pixel packing.  (The FWD of that conv ran here too; with fused statistics it
// was slower than the ring kernel, 376 vs 364 us, was never selected and is gone.)  With so few K-steps the ring
// kernel's per-tile pipeline fill and epilogue dominate: one 128 x 64 tile's 8 steps took ~11 us
// for ~1 us of MFMA work (0.30 of the HBM roofline at B = 1024).  Here
//   * one workgroup per CU loops over its tiles; the whole packed weight panel (nk K-steps x BN
//     rows x 128 B <= 64 KiB) is DMA'd into LDS once;
//   * the A ring runs over the workgroup's (tile, K-step) sequence without draining between tiles:
//     the next tile's first steps are in flight while the current tile's epilogue stores;
//   * the epilogue stages each wave's sub-tile in a private LDS region through inline-asm LDS
//     accesses (invisible to hipcc's wait insertion, ordered by explicit lgkmcnt waits) and stores
//     16-byte rows with buffer stores (invalid rows: out-of-range offsets, dropped), so every wave
//     issues a FIXED number of vector-memory ops per tile and the counted vmcnt waits stay exact
//     (vmcnt retires in issue order across loads, stores and LDS-DMA);
// Tile rows in the ring kernel's image-minor order (NG images x NB = BM / NG pixels per tile).  The
// tiles are split into 8 contiguous ranges, one per XCD, so the concurrently running tiles of one
// XCD are neighbouring pixels of the same images (shared input rows in its L2).
// BNR (DGRAD only): the epilogue also runs the reduction pass of the BatchNorm backward that reads
// this dgrad's output dy (norm_fast.hip bn_reduce_fast, MODE 1): per channel sum of dnorm and
// dnorm * xhat, dnorm = d(chain)/dz * dy at z = gamma * xhat + beta, xhat = (h - mean) * invstd,
// with the stored bf16 dy values and the forward's dropout keep bits.  Each tile's epilogue issues
// LDS-DMA of the h rows (and keep bytes) its lanes just stored dy for into the wave's staging
// region; the NEXT tile's epilogue consumes them (by then the DMA has long landed, so the ring never
// drains for it) before it stages its own accumulators there.  The dgrad output is unchanged.
template <int BN, bool BNR = false>
__global__ void __launch_bounds__(RT) conv_persist_kernel(ConvArgs a, int ntiles) {
  constexpr int BM = 128, BK = 64, WGM = 4, WGN = 2;
  constexpr int WM = BM / WGM, WN = BN / WGN;              // 32 x 32 (BN 64) / 32 x 64 (BN 128)
  constexpr int RM = WM / 16, RN = WN / 16;
  constexpr int ROWB = 2 * BK, PROWS = 1024 / ROWB, CPR = ROWB / 16;
  constexpr int APW = BM / PROWS / 8;                      // A pieces per wave per K-step
  constexpr int ABYTES = BM * ROWB;
  constexpr int NS = BN <= 64 ? 4 : 3;                     // ring slots (NS - 1 steps in flight)
  constexpr int PANEL = 65536;
  constexpr int SPITCH = WN * 2 + 16, STAGE = WM * SPITCH; // per-wave bf16 staging
  constexpr int OCPR = WN * 2 / 16, ORPI = 64 / OCPR, NST = WM / ORPI;   // 16-byte stores per tile
  constexpr int STB = 3 * WGM * BN * 4;
  // BNR: per wave NST x 1 KiB of h rows (lane-linear: piece p, lane l = the row / chunk the lane
  // stored in pass p) + 256 B of keep bytes ([32 rows][WN / 8]) in the staging region
  constexpr int KOFF = NST * 1024, KB = WN / 8, DPR = KB / 4;
  constexpr int NH = BNR ? NST + 1 : 0;                    // epilogue DMA ops (h pieces + keep)
  static_assert(!BNR || (KOFF + 256 <= STAGE && KB % 4 == 0), "BNR staging");
  __shared__ __attribute__((aligned(16))) char smem[PANEL + NS * ABYTES + 8 * STAGE + STB];
  char* const panel = smem;
  char* const ring = smem + PANEL;
  const es_conv_desc_t& d = a.d;
  const int NL = conv_live(a);   // live images (dynamic rows)
  const int nch = d.K;
  const int cpt = nch / BK, nk = a.Kd / BK;
  const int lane = threadIdx.x & 63, wid = uni(threadIdx.x >> 6);
  const int wm0 = (wid / WGN) * WM, wn0 = (wid % WGN) * WN;
  const int lrow = lane / CPR, pc = lane % CPR;
  const uint32_t stg = lds_u32(ring + NS * ABYTES + wid * STAGE);
  float* const stb = (float*)(ring + NS * ABYTES + 8 * STAGE);
  const int NG = a.ng, PPG = NG / PROWS, NB = BM / NG;
  const int gh = d.H, gw = d.W;
  const int PQ = gh * gw, TT = (PQ + NB - 1) / NB;
  ntiles = min(ntiles, (NL + NG - 1) / NG * TT);          // the live image groups' tiles
  const int lgNG = uni(31 - __builtin_clz(NG));
  FastDiv fgw;
  {
    uint32_t l2 = 0;
    while ((1u << l2) < (uint32_t)gw) ++l2;
    fgw.l = uni((int)l2);
    fgw.m = (uint32_t)uni((int)(uint32_t)(((1ull << 32) * ((1ull << l2) - (uint32_t)gw)) / (uint32_t)gw + 1));
  }
  // this workgroup's tiles: XCD x = blockIdx % 8 owns tiles [x * T / 8, (x + 1) * T / 8); its
  // workgroups (blockIdx / 8 = l of L) take every L-th tile of that range
  const int xcd = blockIdx.x & 7, L = (gridDim.x - xcd + 7) >> 3, lw = blockIdx.x >> 3;
  const int t_lo = (int)(((int64_t)ntiles * xcd) >> 3), t_hi = (int)(((int64_t)ntiles * (xcd + 1)) >> 3);
  const int my = t_hi - t_lo > lw ? (t_hi - t_lo - lw + L - 1) / L : 0;
  const int nsteps = my * nk;

  const __amdgpu_buffer_rsrc_t ares = mkres(a.a_src, (uint32_t)(NL * a.as[0] * 2));
  const __amdgpu_buffer_rsrc_t bres = mkres(a.b_src, (uint32_t)(a.Ng * a.Kd * 2));
  const __amdgpu_buffer_rsrc_t ores = mkres(a.out, (uint32_t)(NL * a.os[0] * 2));
  // the weight panel: K-step k occupies [BN rows][128 B] at panel + k * BN * 128 (ring B layout)
  for (int pi = wid; pi < nk * (BN / PROWS); pi += 8) {
    const int k = pi / (BN / PROWS), rb = pi - k * (BN / PROWS);
    const int rr = rb * PROWS + lrow;
    bdma16(bres, (uint32_t)((rr * a.Kd + k * BK) * 2 + ((pc ^ swz_x<BK>(rr)) * 16)), panel + k * BN * ROWB + rb * 1024);
  }
  wait_vmcnt<0>();

  // issue cursor (tile iteration ii, K-step ik) and the issued tile's A pieces
  const int as0b = (int)a.as[0] * 2, as2b = (int)a.as[2] * 2, as3b = (int)a.as[3] * 2;
  uint32_t alane[APW];
  int pc0[APW], pc1[APW];
  bool pval[APW];
  int ii = 0, ik = 0;
  int icb = 0, ics = 0, icr = 0;   // issue K-step as (channel block, tap column, tap row): no divisions
  auto issue = [&](char* slot) {
    const bool live = ii < my;
    if (ik == 0 && live) {
      const int t = t_lo + lw + ii * L;
      const int gi = t / TT, pix0 = (t - gi * TT) * NB;
#pragma unroll
      for (int j = 0; j < APW; ++j) {
        const int pi = wid * APW + j, rr = pi * PROWS + lrow;
        const int ppix = pi / PPG, pix = pix0 + ppix;
        pval[j] = pix < PQ;
        const int pp = pval[j] ? pix : 0;
        const int y = fdiv(pp, fgw), x = pp - y * gw;
        const int img = gi * NG + (pi - ppix * PPG) * PROWS + lrow;
        alane[j] = (uint32_t)(img * as0b + ((pc ^ swz_x<BK>(rr)) * 16));   // images >= N: past num_records
        pc0[j] = y + d.pad;
        pc1[j] = x + d.pad;
      }
    }
    const int cb = icb, cr = icr, cs = ics;
#pragma unroll
    for (int j = 0; j < APW; ++j) {
      int hh, ww;
      bool ok;
      hh = pc0[j] - cr; ww = pc1[j] - cs;
      ok = (unsigned)hh < (unsigned)d.P && (unsigned)ww < (unsigned)d.Q;
      ok = ok && live && pval[j];
      const uint32_t u = ok ? (uint32_t)(hh * as2b + ww * as3b + cb * ROWB) : OOB;
      bdma16(ares, alane[j] + u, slot + (wid * APW + j) * 1024);
    }
    if (++icb == cpt) {
      icb = 0;
      if (++ics == d.S) {
        ics = 0;
        ++icr;
      }
    }
    if (++ik == nk) { ik = 0; ++ii; icb = ics = icr = 0; }
  };

  f32x4 acc[RM][RN];
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // A DGRAD has no bias.  The epilogue still adds a per-column zero where the FWD side of this kernel
  // added its bias: -0 accumulators keep storing +0, and the compiler emits the instruction stream
  // it always did (a literal 0.f reorders its register allocation).
  float zcol[RN];
#pragma unroll
  for (int j = 0; j < RN; ++j) zcol[j] = 0.f;
  const int r16 = lane & 15, g16 = lane >> 4, col16 = lane & 15, rq = (lane >> 4) * 4;
  const int elr = lane / OCPR, elch = lane % OCPR;        // epilogue: row pass / 8-channel chunk
  // BNR: the lane's 8 channels are fixed (wn0 + 8 elch ..), so are their statistics (loaded before
  // the ring starts: a VGPR load inside the loop makes hipcc drain every DMA in flight with vmcnt(0)
  // at its first use)
  float bmu[8], bis[8], bsc[8], bsh[8], bs1[8], bs2[8];
  int4v pdy[NST];                                         // the previous tile's stored dy
  const __amdgpu_buffer_rsrc_t hres = mkres(a.bnr_x, BNR ? (uint32_t)(NL * a.os[0] * 2) : 0u);
  const __amdgpu_buffer_rsrc_t kres = mkres(a.bnr_keep, BNR ? (uint32_t)((int64_t)NL * PQ * (a.Ng / 8)) : 0u);
  if constexpr (BNR) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = wn0 + elch * 8 + k;
      bmu[k] = a.bnr_mean[c];
      bis[k] = a.bnr_invstd[c];
      const float s = (a.bnr_gamma ? a.bnr_gamma[c] : 1.f) * bis[k];
      bsc[k] = s;
      bsh[k] = (a.bnr_beta ? a.bnr_beta[c] : 0.f) - bmu[k] * s;
      bs1[k] = bs2[k] = 0.f;
    }
#pragma unroll
    for (int p = 0; p < NST; ++p) pdy[p] = int4v{0, 0, 0, 0};
  }
  char* const stgp = ring + NS * ABYTES + wid * STAGE;
  // BNR: fold the previous tile's dy (pdy) with its h / keep bytes (landed in this wave's staging
  // region) into the per-lane sums; same expressions as bn_reduce_fast (norm_fast.hip)
  auto bnr_consume = [&]() {
    int4v hv[NST];
    uint32_t kb[NST];
#pragma unroll
    for (int p = 0; p < NST; ++p) {
      const int r = p * ORPI + elr;
      hv[p] = ds_read_b128_asm(stg + r * (WN * 2) + elch * 16);
      kb[p] = ds_read_u8_asm(stg + KOFF + r * KB + elch);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int p = 0; p < NST; ++p) {
      asm volatile("" : "+v"(hv[p]), "+v"(kb[p]));
      const bf16x8 h8 = __builtin_bit_cast(bf16x8, hv[p]), d8 = __builtin_bit_cast(bf16x8, pdy[p]);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float v = (float)h8[k], dy = (float)d8[k];
        const bool keep = !a.bnr_drop || ((kb[p] >> k) & 1u);
        const float z = v * bsc[k] + bsh[k];
        const float zs = a.bnr_drop && a.bnr_dfirst ? z * a.bnr_scale : z;
        const float dsc = a.bnr_drop ? a.bnr_scale : 1.f;
        const float dn = keep ? dy * (zs > 0.f ? 1.f : a.bnr_slope) * dsc : 0.f;
        const float xh = (v - bmu[k]) * bis[k];
        bs1[k] += dn;
        bs2[k] += dn * xh;
      }
    }
  };
  struct Frag {
    bf16x8 a[RM], b[RN];
  };
  auto load = [&](Frag& f, const char* slot, const char* bk, int kk) {
    const int seg = kk * 4 + g16;
#pragma unroll
    for (int i = 0; i < RM; ++i) f.a[i] = *(const bf16x8*)(slot + swz<BK>(wm0 + i * 16 + r16, seg));
#pragma unroll
    for (int j = 0; j < RN; ++j) f.b[j] = *(const bf16x8*)(bk + swz<BK>(wn0 + j * 16 + r16, seg));
  };
  auto mma = [&](const Frag& f) {
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int j = 0; j < RN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.a[i], f.b[j], acc[i][j], 0, 0, 0);
  };

  // epilogue of tile iteration ci: bias, rounding, fused statistics, staged 16-byte stores
  auto epilogue = [&](int ci) {
    const int t = t_lo + lw + ci * L;
    const int gi = t / TT, pix0 = (t - gi * TT) * NB;
    auto row_pix = [&](int r) { return pix0 + ((wm0 + r) >> lgNG); };
    auto row_img = [&](int r) { return gi * NG + ((wm0 + r) & (NG - 1)); };
    auto row_ok = [&](int r) { return row_pix(r) < PQ && row_img(r) < NL; };
    if constexpr (BNR) {
      if (ci > 0) {
        // the previous tile's h / keep DMA: older than the NS - 1 steps issued since (nk >= NS - 1)
        wait_vmcnt<(NS - 1) * APW>();
        bnr_consume();
      }
    }
#pragma unroll
    for (int j = 0; j < RN; ++j) {
#pragma unroll
      for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc[i][j][jj] = (float)(bf16)(acc[i][j][jj] + zcol[j]);
    }
    // stage the wave's 32 x WN bf16 sub-tile (row pitch SPITCH), then 16-byte row stores
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int j = 0; j < RN; ++j) {
          const bf16 v = (bf16)acc[i][j][jj];
          ds_write_u16(stg + (i * 16 + rq + jj) * SPITCH + (j * 16 + col16) * 2, (uint32_t)__builtin_bit_cast(uint16_t, v));
        }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const int lr = elr, lch = elch;
    int4v vals[NST];
#pragma unroll
    for (int p = 0; p < NST; ++p) vals[p] = ds_read_b128_asm(stg + (p * ORPI + lr) * SPITCH + lch * 16);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int p = 0; p < NST; ++p) asm volatile("" : "+v"(vals[p]));   // no use above the wait
    uint32_t voffs[NST];
#pragma unroll
    for (int p = 0; p < NST; ++p) {
      const int r = p * ORPI + lr;
      uint32_t voff = OOB;
      if (row_ok(r)) {
        const int pix = row_pix(r);
        const int y = fdiv(pix, fgw), x = pix - y * gw;
        const int64_t off = (int64_t)row_img(r) * a.os[0] + (int64_t)y * a.os[2] + (int64_t)x * a.os[3] + wn0 + lch * 8;
        voff = (uint32_t)(off * 2);
      }
      voffs[p] = voff;
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u32_t, vals[p]), ores, voff, 0, 0);
    }
    if constexpr (BNR) {
      // this tile's h rows (the stored dy's positions: h has the output's layout) and keep bytes
      // -> the wave's staging region, consumed by the next epilogue (or after the loop)
#pragma unroll
      for (int p = 0; p < NST; ++p) {
        pdy[p] = vals[p];
        bdma16(hres, voffs[p], stgp + p * 1024);
      }
      const int kr = lane / DPR;
      uint32_t koff = OOB;
      if (kr < WM && row_ok(kr))
        koff = (uint32_t)(((int64_t)row_img(kr) * PQ + row_pix(kr)) * (a.Ng / 8) + (wn0 / 8) + (lane % DPR) * 4);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(kres, (lds_void*)(stgp + KOFF), 4, (int)koff, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int j = 0; j < RN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  };

#pragma unroll
  for (int i = 0; i < NS - 1; ++i) issue(ring + i * ABYTES);
  int cur = 0, prv = NS - 1, ck = 0, ci = 0, last_epi = -1000;
  for (int s = 0; s < nsteps; ++s) {
    // step s landed: younger than its DMA are the NS - 2 later steps' pieces and, when an epilogue
    // ran within the last NS - 1 iterations (after step s was issued), its NST stores (+ BNR: its
    // NH h / keep DMA ops)
    if (s - last_epi <= NS - 1) wait_vmcnt<(NS - 2) * APW + NST + NH>();
    else wait_vmcnt<(NS - 2) * APW>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's reads of step s - 1 are done
    ring_barrier();
    issue(ring + prv * ABYTES);                          // step s + NS - 1 into step s - 1's slot
    const char* slot = ring + cur * ABYTES;
    const char* bk = panel + ck * BN * ROWB;
    Frag f;
    load(f, slot, bk, 0);
    mma(f);
    load(f, slot, bk, 1);
    mma(f);
    if (++ck == nk) {
      epilogue(ci);
      ck = 0;
      ++ci;
      last_epi = s;
    }
    prv = cur;
    cur = cur == NS - 1 ? 0 : cur + 1;
  }
  wait_vmcnt<0>();
  if constexpr (BNR) {
    if (my > 0) bnr_consume();   // the last tile's rows
    // the workgroup's sums: the 64 / OCPR lanes of one channel chunk, then the WGM row waves
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
      for (int o = OCPR; o < 64; o <<= 1) {
        bs1[k] += __shfl_xor(bs1[k], o, 64);
        bs2[k] += __shfl_xor(bs2[k], o, 64);
      }
    float (*s1w)[BN] = (float (*)[BN])stb;
    float (*s2w)[BN] = s1w + WGM;
    const int wmi = wid / WGN;
    __syncthreads();
    if (lane < OCPR) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        s1w[wmi][wn0 + lane * 8 + k] = bs1[k];
        s2w[wmi][wn0 + lane * 8 + k] = bs2[k];
      }
    }
    __syncthreads();
    if (wid < WGN) {
      for (int c = lane; c < WN; c += 64) {
        const int col = wn0 + c;
        float t1 = 0.f, t2 = 0.f;
        for (int w = 0; w < WGM; ++w) {
          t1 += s1w[w][col];
          t2 += s2w[w][col];
        }
        float* pp = a.bnr_part + (int64_t)blockIdx.x * 3 * a.Ng;
        pp[col] = 0.f;
        pp[a.Ng + col] = t1;
        pp[2 * a.Ng + col] = t2;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// PERSISTENT 256 x 256 merged sub-pixel FWD: the generator's conv_layers.0 / conv_layers.5
// (neutron/generator.py:25,30; 3x3 over the x2 upsample, run as one GEMM over (class, channel)
// columns, see conv_ring_kernel).  Measured on the ring kernel at B = 1024 (tools/ring_exp.py with
// the ES_RING_EXP builds): conv_layers.5 FWD 766 us with its epilogue, 521 us without; the
// epilogue (bias, statistics, 128 KiB of stores per tile) ran with the CU's MFMAs idle, since a
// 128 KiB ring leaves one workgroup per CU.  Here
//   * 256 workgroups (one per CU) loop over row tiles with a FIXED column tile each: the NT column
//     tiles of a row tile run side by side on one XCD (workgroups lw = NT l + ct), and each XCD
//     walks a contiguous range of row tiles (neighbouring pixels of the same images share its L2);
//   * the 4-slot ring (A and B pieces, 32-deep K-steps) continues across tiles: the next tile's
//     first steps are in flight while the epilogue runs, and its stores drain under the next
//     tile's MFMAs (fixed-count buffer stores, invalid rows at out-of-range offsets, so the
//     counted vmcnt waits stay exact: vmcnt retires in issue order across loads, stores, DMA);
//   * the epilogue stages 16-row passes of each wave's 128 x 64 sub-tile in a private 2.3 KiB LDS
//     region (inline-asm LDS accesses with explicit lgkmcnt waits) for 16-byte row stores;
//   * BatchNorm partials: per lane running sums / sums of squares of its 4 columns over all its
//     tiles (fixed columns), merged across lanes and row waves once at the end: one [3][Ng]
//     partial per (workgroup, class), chunks = 4 x 256.
// AFF: the affine + activation epilogue of es_conv2d_fwd_affine (see conv_ring_kernel); the scale
// table takes the first [BN] floats of the statistics area, which such a launch never uses.
template <int NT, bool AFF = false>
__global__ void __launch_bounds__(RT) conv_p256_kernel(ConvArgs a, int R) {
  constexpr int BM = 256, BN = 256, BK = 32, WGN = 4;
  constexpr int WM = 128, WN = 64, RM = WM / 16, RN = WN / 16, RMF = RM / 2;
  constexpr int ROWB = 2 * BK, PROWS = 1024 / ROWB, CPR = ROWB / 16;
  constexpr int APW = BM / PROWS / 8, BPW = BN / PROWS / 8, PW = APW + BPW;
  constexpr int NS = 4, ABYTES = BM * ROWB, SLOT = (BM + BN) * ROWB;
  constexpr int SPITCH = WN * 2 + 16, STAGE = 16 * SPITCH;   // per-wave staging: 16 rows
  constexpr int NST = WM / 8;                                 // 16-byte stores per tile per wave
  constexpr int LR = 32 / NT;                                 // workgroups per column tile per XCD
  __shared__ __attribute__((aligned(16))) char smem[NS * SLOT + 8 * STAGE + BN * 4 + 2 * 3 * BN * 4];
  const es_conv_desc_t& d = a.d;
  const int NL = conv_live(a);   // live images (dynamic rows)
  const SubPixel& sp = a.sp;
  const int lane = threadIdx.x & 63, wid = uni(threadIdx.x >> 6);
  const uint32_t sbias = lds_u32(smem + NS * SLOT + 8 * STAGE);   // [BN] floats
  const uint32_t sst = sbias + BN * 4;                              // [2][3][BN] floats
  const int wm0 = (wid / WGN) * WM, wn0 = (wid % WGN) * WN;
  const int lrow = lane / CPR, pc = lane % CPR;
  const int r16 = lane & 15, g16 = lane >> 4;
  const uint32_t stg = lds_u32(smem + NS * SLOT + wid * STAGE);

  // work of this workgroup: XCD x (blockIdx % 8) owns row tiles [R x / 8, R (x + 1) / 8); its
  // workgroup lw = NT l + ct takes column tile ct and every LR-th row tile from l
  const int xcd = blockIdx.x & 7, lw = blockIdx.x >> 3;
  const int ct = lw % NT, lr = lw / NT;
  const int n0 = ct * BN;
  const int NG = a.ng, PPG = NG / PROWS, NB = BM / NG;
  const int lgNG = uni(31 - __builtin_clz(NG));
  const int TT = sp.tile0[1], gh = sp.ph[0], gw = sp.pw[0], PQ = gh * gw;
  R = min(R, (NL + NG - 1) / NG * TT);                   // the live image groups' row tiles
  const int r_lo = (int)(((int64_t)R * xcd) >> 3), r_hi = (int)(((int64_t)R * (xcd + 1)) >> 3);
  const int my = r_hi - r_lo > lr ? (r_hi - r_lo - lr + LR - 1) / LR : 0;
  const int oh0 = sp.oh[0], ow0 = sp.ow[0], kw = sp.dw[0];
  const int ldb = sp.dh[0] * sp.dw[0] * d.C, nk = ldb / BK;
  FastDiv fgw;
  {
    uint32_t l = 0;
    while ((1u << l) < (uint32_t)gw) ++l;
    fgw.l = uni((int)l);
    fgw.m = (uint32_t)uni((int)(uint32_t)(((1ull << 32) * ((1ull << l) - (uint32_t)gw)) / (uint32_t)gw + 1));
  }
  // the wave's output class and first channel (a wave's 64 columns never straddle a class)
  const int ecls = (n0 + wn0) / a.Ng, kc0 = n0 + wn0 - ecls * a.Ng;
  const int py0 = sp.p0[0] + ((ecls >> 1) ? sp.p0[2] - sp.p0[0] : 0);
  const int px0 = sp.q0[0] + ((ecls & 1) ? sp.q0[1] - sp.q0[0] : 0);

  const __amdgpu_buffer_rsrc_t ares = mkres(a.a_src, (uint32_t)(NL * a.as[0] * 2));
  const __amdgpu_buffer_rsrc_t bres = mkres(a.b_src, (uint32_t)(sp.tap0[4] * a.Ng * d.C * 2));
  const __amdgpu_buffer_rsrc_t ores = mkres(a.out, (uint32_t)(NL * a.os[0] * 2));
  const int as0b = (int)a.as[0] * 2, as2b = (int)a.as[2] * 2, as3b = (int)a.as[3] * 2;
  const int os0 = (int)a.os[0], os2 = (int)a.os[2], os3 = (int)a.os[3];   // (N * os0 * 2 < 2^31: host)
  uint32_t blane[BPW];
#pragma unroll
  for (int j = 0; j < BPW; ++j) {
    const int rr = (wid * BPW + j) * PROWS + lrow;
    blane[j] = (uint32_t)((n0 + rr) * ldb * 2 + ((pc ^ swz_x<BK>(rr)) * 16));
  }

  // issue cursor: tile iteration ii, K-step ik = (tap cr, cs; channel cch); per-tap offset cache
  uint32_t alane[APW], ua_t[APW], ub_t = OOB;
  int pc0[APW], pc1[APW];
  bool pval[APW];
#pragma unroll
  for (int j = 0; j < APW; ++j) { alane[j] = 0; ua_t[j] = OOB; pc0[j] = pc1[j] = 0; pval[j] = false; }
  int ii = 0, ik = 0, cr = 0, cs = 0, cch = 0;
  auto issue = [&](char* slot) {
    const bool live = ii < my;
    if (ik == 0 && live) {   // a new tile: its A pieces (wave-uniform branch)
      const int tl = r_lo + lr + ii * LR;
      const int gi = tl / TT, pix0 = (tl - gi * TT) * NB;
#pragma unroll
      for (int j = 0; j < APW; ++j) {
        const int pi = wid * APW + j;
        const int rr = pi * PROWS + lrow;
        const int ppix = pi / PPG, pix = pix0 + ppix;
        pval[j] = pix < PQ;
        const int pp = pval[j] ? pix : 0;
        const int y = fdiv(pp, fgw), x = pp - y * gw;
        const int img = gi * NG + (pi - ppix * PPG) * PROWS + lrow;
        alane[j] = (uint32_t)(img * as0b + ((pc ^ swz_x<BK>(rr)) * 16));   // images >= N: past num_records
        pc0[j] = y + oh0;
        pc1[j] = x + ow0;
      }
    }
    if (cch == 0) {   // first step of a tap
#pragma unroll
      for (int j = 0; j < APW; ++j) {
        const int hs = pc0[j] + cr, ws = pc1[j] + cs;
        const bool ok = live && pval[j] && (unsigned)hs < (unsigned)d.H && (unsigned)ws < (unsigned)d.W;
        ua_t[j] = ok ? (uint32_t)(hs * as2b + ws * as3b) : OOB;
      }
      ub_t = live ? (uint32_t)((cr * kw + cs) * d.C * 2) : OOB;
    }
    const uint32_t co = (uint32_t)(cch * 2);
#pragma unroll
    for (int j = 0; j < APW; ++j) bdma16(ares, alane[j] + (ua_t[j] + co), slot + (wid * APW + j) * 1024);
#pragma unroll
    for (int j = 0; j < BPW; ++j) bdma16(bres, blane[j] + (ub_t + co), slot + ABYTES + (wid * BPW + j) * 1024);
    cch += BK;
    if (cch == d.C) {
      cch = 0;
      if (++cs == kw) { cs = 0; ++cr; }
    }
    if (++ik == nk) { ik = 0; ++ii; cr = cs = cch = 0; }
  };

  f32x4 acc[RM][RN];
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // bias of the lane's columns and the running statistics (sum, sum of squares, count)
  // the column tile's bias and the workgroup's statistics accumulators [2 row waves][3][BN] in LDS
  // (nothing of the epilogue stays in registers across the main loop), written through inline asm
  // like every epilogue LDS access (invisible to hipcc's DMA wait insertion)
  if constexpr (AFF) {
    // sbias holds shift' = scale * bias + shift, sst[0 .. BN) the scale (no statistics: stats_part NULL)
    if (threadIdx.x < BN) {
      const int gcol = n0 + threadIdx.x, ch = gcol - (gcol / a.Ng) * a.Ng;
      const float sc = a.epi_scale[ch];
      ds_write_f32_asm(sbias + threadIdx.x * 4, fmaf(a.bias ? a.bias[ch] : 0.f, sc, a.epi_shift[ch]));
      ds_write_f32_asm(sst + threadIdx.x * 4, sc);
    }
  } else {
  if (threadIdx.x < BN) {
    const int gcol = n0 + threadIdx.x;
    ds_write_f32_asm(sbias + threadIdx.x * 4, a.bias ? a.bias[gcol - (gcol / a.Ng) * a.Ng] : 0.f);
  }
  for (int i = threadIdx.x; i < 2 * 3 * BN; i += RT) ds_write_f32_asm(sst + i * 4, 0.f);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  const bool want_stats = !AFF && a.stats_part != nullptr;
  const float eneg = a.epi_act == ES_ACT_LRELU ? a.epi_slope : (a.epi_act == ES_ACT_RELU ? 0.f : 1.f);

  struct Frag {
    bf16x8 a[RMF], b[RN];
  };
  auto load = [&](Frag& f, const char* slot, int kk) {
#pragma unroll
    for (int i = 0; i < RMF; ++i) f.a[i] = *(const bf16x8*)(slot + swz<BK>(wm0 + (kk * RMF + i) * 16 + r16, g16));
#pragma unroll
    for (int j = 0; j < RN; ++j) f.b[j] = *(const bf16x8*)(slot + ABYTES + swz<BK>(wn0 + j * 16 + r16, g16));
  };
  auto mma = [&](const Frag& f, int kk) {
#pragma unroll
    for (int i = 0; i < RMF; ++i)
#pragma unroll
      for (int j = 0; j < RN; ++j)
        acc[kk * RMF + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.a[i], f.b[j], acc[kk * RMF + i][j], 0, 0, 0);
  };

  auto epilogue = [&](int ci) {
    const int tl = r_lo + lr + ci * LR;
    const int gi = tl / TT, pix0 = (tl - gi * TT) * NB;
    // per-lane values laundered through an empty asm: otherwise hipcc hoists the epilogue's
    // lane-constant addresses out of the main loop and spills them across it
    int le = lane;
    uint32_t stg_e = stg;
    asm volatile("" : "+v"(le), "+v"(stg_e));
    const int col16 = le & 15, rq = (le >> 4) * 4;
    float bcol[RN];
#pragma unroll
    for (int j = 0; j < RN; ++j) bcol[j] = ds_read_f32_asm(sbias + (wn0 + j * 16 + col16) * 4);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // (every value an asm LDS read returned is passed through an empty asm after the wait, so no
    // use of it can be scheduled above the wait)
#pragma unroll
    for (int j = 0; j < RN; ++j) asm volatile("" : "+v"(bcol[j]));
    float scol[AFF ? RN : 1];
    if constexpr (AFF) {
#pragma unroll
      for (int j = 0; j < RN; ++j) scol[j] = ds_read_f32_asm(sst + (wn0 + j * 16 + col16) * 4);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int j = 0; j < RN; ++j) asm volatile("" : "+v"(scol[j]));
    }
    // store lanes: row lr8 (+ 8) of a pass, 16-byte chunk lch of the wave's 64 columns
    const int lr8 = le & 7, lch = le >> 3;
    float ts[8], ts2[8], npad = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) ts[k] = ts2[k] = 0.f;
    // 8 passes of 16 rows: bias + rounding, stage (row pitch SPITCH), then two 16-byte stores of
    // 8 rows each; the statistics accumulate from the stored rows (channels lch*8 .. of the lane)
#pragma unroll
    for (int i = 0; i < RM; ++i) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int j = 0; j < RN; ++j) {
          float vf;
          if constexpr (AFF) {
            vf = fmaf(acc[i][j][jj], scol[j], bcol[j]);
            vf = vf > 0.f ? vf : vf * eneg;
          } else {
            vf = acc[i][j][jj] + bcol[j];
          }
          const bf16 vb = (bf16)vf;
          ds_write_u16(stg_e + (rq + jj) * SPITCH + (j * 16 + col16) * 2, (uint32_t)__builtin_bit_cast(uint16_t, vb));
        }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      int4v v0 = ds_read_b128_asm(stg_e + lr8 * SPITCH + lch * 16);
      int4v v1 = ds_read_b128_asm(stg_e + (lr8 + 8) * SPITCH + lch * 16);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      asm volatile("" : "+v"(v0), "+v"(v1));
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        // branch-free: the address is computed for every row, padding rows store out of range
        const int t = wm0 + i * 16 + p * 8 + lr8;
        const int pix = pix0 + (t >> lgNG), img = gi * NG + (t & (NG - 1));
        const bool ok = pix < PQ && img < NL;
        const int yy = fdiv(pix, fgw), xx = pix - yy * gw;
        const uint32_t voff = ok ? (uint32_t)(img * os0 + (py0 + 2 * yy) * os2 + (px0 + 2 * xx) * os3 + kc0 + lch * 8) * 2u : OOB;
        const int4v vv = p ? v1 : v0;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u32_t, vv), ores, voff, 0, 0);
        // a padding row gathered only zeros (out-of-range DMA), so its value is exactly
        // bf16(bias): summed with the rest, counted, and subtracted at the end of the tile
        npad += ok ? 0.f : 1.f;
        if (want_stats) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float lo = __uint_as_float((uint32_t)vv[k] << 16), hi = __uint_as_float((uint32_t)vv[k] & 0xFFFF0000u);
            ts[2 * k] += lo;
            ts2[2 * k] = fmaf(lo, lo, ts2[2 * k]);
            ts[2 * k + 1] += hi;
            ts2[2 * k + 1] = fmaf(hi, hi, ts2[2 * k + 1]);
          }
        }
      }
    }
    if (want_stats) {
      // the 8 row lanes of a chunk (lane bits 0..2), then lane lr8 == 0 adds the wave's totals of
      // its 8 channels into the row wave's LDS accumulators (one owner per address: deterministic)
#pragma unroll
      for (int o = 1; o <= 4; o <<= 1) {
        npad += __shfl_xor(npad, o, 64);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          ts[k] += __shfl_xor(ts[k], o, 64);
          ts2[k] += __shfl_xor(ts2[k], o, 64);
        }
      }
      if (lr8 == 0) {
        const int wmi = wid / WGN;
        const uint32_t base = sst + (wmi * 3 * BN + wn0 + lch * 8) * 4;
        float o0[8], o1[8], o2[8], bb[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          o0[k] = ds_read_f32_asm(base + k * 4);
          o1[k] = ds_read_f32_asm(base + (BN + k) * 4);
          o2[k] = ds_read_f32_asm(base + (2 * BN + k) * 4);
          bb[k] = ds_read_f32_asm(sbias + (wn0 + lch * 8 + k) * 4);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int k = 0; k < 8; ++k) asm volatile("" : "+v"(o0[k]), "+v"(o1[k]), "+v"(o2[k]), "+v"(bb[k]));
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float vb = (float)(bf16)bb[k];
          ds_write_f32_asm(base + k * 4, o0[k] + ((float)WM - npad));
          ds_write_f32_asm(base + (BN + k) * 4, o1[k] + (ts[k] - npad * vb));
          ds_write_f32_asm(base + (2 * BN + k) * 4, o2[k] + (ts2[k] - npad * vb * vb));
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
    }
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int j = 0; j < RN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  };

  // the ring (ring_loop_lean's single fragment set: register room for the epilogue), continued
  // across the workgroup's tiles
  const int nsteps = my * nk;
#pragma unroll
  for (int i = 0; i < NS - 1; ++i) issue(smem + i * SLOT);
  int cur = 0, prv = NS - 1, ck = 0, ci = 0, last_epi = -1000;
  for (int s = 0; s < nsteps; ++s) {
    // step s landed: younger than its DMA are the NS - 2 later steps' pieces and, when an
    // epilogue ran within the last NS - 1 iterations (after step s was issued), its NST stores
    if (s - last_epi <= NS - 1) wait_vmcnt<(NS - 2) * PW + NST>();
    else wait_vmcnt<(NS - 2) * PW>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's reads of step s - 1 are done
    ring_barrier();
    issue(smem + prv * SLOT);                            // step s + NS - 1 into step s - 1's slot
    Frag f;
    load(f, smem + cur * SLOT, 0);
    mma(f, 0);
    load(f, smem + cur * SLOT, 1);
    mma(f, 1);
    if (++ck == nk) {
      epilogue(ci);
      ck = 0;
      ++ci;
      last_epi = s;
    }
    prv = cur;
    cur = cur == NS - 1 ? 0 : cur + 1;
  }
  wait_vmcnt<0>();   // every DMA (zero-fill steps included) and store retired
  if (want_stats) {
    // merge the 2 row waves' accumulators -> (count, mean, M2) per (workgroup, class)
    __syncthreads();
    for (int col = threadIdx.x; col < BN; col += RT) {
      float v[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) v[q] = ds_read_f32_asm(sst + (q * BN + col) * 4);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int q = 0; q < 6; ++q) asm volatile("" : "+v"(v[q]));
      const float n_ = v[0] + v[3], s_ = v[1] + v[4], q_ = v[2] + v[5];
      const float mu = n_ > 0.f ? s_ / n_ : 0.f;
      const int gcol = n0 + col, cc = gcol / a.Ng, ch = gcol - cc * a.Ng;
      float* pp = a.stats_part + ((int64_t)blockIdx.x * 4 + cc) * 3 * a.Ng;
      pp[ch] = n_;
      pp[a.Ng + ch] = mu;
      pp[2 * a.Ng + ch] = fmaxf(q_ - s_ * mu, 0.f);
    }
    // the classes outside this column tile: empty partials
    const int c_lo = n0 / a.Ng, c_hi = (n0 + BN - 1) / a.Ng;
    for (int idx = threadIdx.x; idx < 4 * a.Ng; idx += RT) {
      const int cc = idx / a.Ng, ch = idx - cc * a.Ng;
      if (cc < c_lo || cc > c_hi) {
        float* pp = a.stats_part + ((int64_t)blockIdx.x * 4 + cc) * 3 * a.Ng;
        pp[ch] = 0.f;
        pp[a.Ng + ch] = 0.f;
        pp[2 * a.Ng + ch] = 0.f;
      }
    }
  }
}

// every instantiation the planner can ask for (ring_plan in conv_ring_host.hip); the kernels take the
// plan's scalar (tiles / row tiles) behind ConvArgs
template <int BN, bool BNR>
void launch_persist(const ConvArgs& a, dim3 grid, int ntiles, hipStream_t st) {
  hipLaunchKernelGGL((conv_persist_kernel<BN, BNR>), grid, dim3(RT), 0, st, a, ntiles);
}
template <int NT, bool AFF>
void launch_p256(const ConvArgs& a, dim3 grid, int row_tiles, hipStream_t st) {
  hipLaunchKernelGGL((conv_p256_kernel<NT, AFF>), grid, dim3(RT), 0, st, a, row_tiles);
}
const RingEntry<void (*)(const ConvArgs&, dim3, int, hipStream_t)> TABLE[] = {
    {persist_key(64, false), &launch_persist<64, false>},   {persist_key(64, true), &launch_persist<64, true>},
    {persist_key(128, false), &launch_persist<128, false>}, {persist_key(128, true), &launch_persist<128, true>},
    {p256_key(1, false), &launch_p256<1, false>},           {p256_key(1, true), &launch_p256<1, true>},
    {p256_key(2, false), &launch_p256<2, false>},           {p256_key(2, true), &launch_p256<2, true>},
    {p256_key(4, false), &launch_p256<4, false>},           {p256_key(4, true), &launch_p256<4, true>},
};

}  // namespace

bool conv_persist_launch(const RingPlan& p, const ConvArgs& a, hipStream_t st) {
  const auto* e = ring_find(TABLE, p.key);
  if (e) e->launch(a, dim3(p.grid[0], p.grid[1], p.grid[2]), p.karg, st);
  return e != nullptr;
}
