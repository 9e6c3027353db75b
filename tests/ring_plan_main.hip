// Stand-alone host program of tests/test_ring_plan_cpu.py: runs the ring dispatcher
// (csrc/conv_ring_host.hip, compiled host-only) over a fixed list of calls and prints, per call, every
// launch it would make (kernel, grid, the ConvArgs fields the plan sets) and the call's answer.  The
// kernel files are replaced by the recording launch functions at the end of this file, so no kernel
// is compiled and nothing touches a device.  The output is compared with tests/golden/ring_plan.json.gz,
// which was recorded once from the single-file dispatcher this one replaced.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "conv_common.h"
#include "ring_plan.h"

extern "C" {
int es_conv_set_ring(int), es_conv_set_ring256(int), es_conv_set_persist(int), es_conv_set_p256(int);
int es_conv_set_subpixel(int), es_conv_set_wgrad_ws(int), es_conv_set_f32_chunk(int), es_conv_set_f32_split(int);
int es_conv_subpixel_ok(const es_conv_desc_t*, es_dtype_t);
}

// ---------------------------------------------------------------- what the library provides elsewhere
bool g_es_det = false;
void es_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  printf("E ");
  vprintf(fmt, ap);
  printf("\n");
  va_end(ap);
}
extern "C" int64_t es_weight_planes_offset(int64_t n) { return (n * 4 + 255) / 256 * 256; }

// ---------------------------------------------------------------- fake operands (never dereferenced)
static char* const A_BASE = (char*)0x100000000000ull;
static char* const B_BASE = (char*)0x200000000000ull;
static char* const O_BASE = (char*)0x300000000000ull;
static float* const STATS = (float*)0x400000000000ull;
static float* const BNRP = (float*)0x500000000000ull;
static float* const WS = (float*)0x600000000000ull;
static float* const DW = (float*)0x700000000000ull;
static const float* const FAKE = (const float*)0x800000000000ull;
static const int32_t* const ROWS = (const int32_t*)0x900000000000ull;

static uint32_t fnv(const void* p, size_t n) {
  uint32_t h = 2166136261u;
  for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 16777619u;
  return h;
}

// one launch: the kernel's name as the compiler prints its instantiation, the grid, the kernel's
// scalar arguments behind ConvArgs, and the ConvArgs fields a ring plan or the chunk loop sets (those
// of them that differ from what the caller passed, g_in, or from zero)
static ConvArgs g_in;
void rec_launch(const char* kernel, dim3 g, const ConvArgs& a, long karg, const float* wsc) {
  printf("L %s g=%u,%u,%u", kernel, g.x, g.y, g.z);
  if (karg) printf(" k=%ld", karg);
  if (wsc) printf(" ws=%lld", (long long)(wsc - WS));
  if (a.d.N != g_in.d.N) printf(" N=%d", a.d.N);
  if (a.nbase) printf(" nb=%d", a.nbase);
  if (a.M != g_in.M) printf(" M=%d", a.M);
  if (a.Kd != g_in.Kd) printf(" Kd=%d", a.Kd);
  if (a.a_src != g_in.a_src) printf(" ao=%lld", (long long)((const char*)a.a_src - (const char*)g_in.a_src));
  if (a.b_src != g_in.b_src) printf(" bo=%lld", (long long)((const char*)a.b_src - (const char*)g_in.b_src));
  if (a.out != g_in.out) printf(" oo=%lld", (long long)((const char*)a.out - (const char*)g_in.out));
  printf(" ng=%d vo=%d", a.ng, a.vec_out);
  if (a.sp.on) printf(" sp=%08x", fnv(&a.sp, sizeof(a.sp)));
  if (a.sp_tpc) printf(" tpc=%d", a.sp_tpc);
  if (a.sp_merge) printf(" mg=%d", a.sp_merge);
  if (a.k_per_split != g_in.k_per_split) printf(" kps=%d", a.k_per_split);
  if (a.stats_part) printf(" st=%lld", (long long)(a.stats_part - STATS));
  if (a.epi_scale) printf(" epi=%d,%g", a.epi_act, a.epi_slope);
  if (a.bnr_part) printf(" bnr=%d,%d,%g,%g", a.bnr_drop, a.bnr_dfirst, a.bnr_scale, a.bnr_slope);
  if (a.prio != g_in.prio) printf(" pr=%d", a.prio);
  printf("\n");
}
// the ordered reduce of the fp32 WGRAD partials (its two kernels differ in vector width only)
void rec_reduce(const float* ws, int splits, int K, int C, int R, int S, int ngt, const SubPixel& sp, float beta) {
  printf("L wgrad_reduce ws=%lld splits=%d K=%d C=%d R=%d S=%d ngt=%d sp=%08x beta=%g\n", (long long)(ws - WS), splits, K,
         C, R, S, ngt, sp.on ? fnv(&sp, sizeof(sp)) : 0u, beta);
}
// (the wave-specialised WGRAD kernel has a file and a dispatcher of its own, conv_wgrad_ws.hip)
int es_wgrad_ws_launch(int bn, bool sp, dim3 grid, const ConvArgs& a, float* wsc, int ngt, hipStream_t) {
  char name[64];
  snprintf(name, sizeof name, "wgrad_ws<%d, %s>", bn, sp ? "true" : "false");
  rec_launch(name, grid, a, ngt, wsc);
  return 1;
}

// ---------------------------------------------------------------- the calls
struct Shape {
  const char* name;
  int C, H, W, K, k, stride, pad, up;
};
// tests/test_f32_ring_gpu.py::CASES; its first three are the bench shapes c0, c5 and c9 of neutron
static const Shape SHAPES[] = {
    {"c0", 128, 13, 13, 256, 3, 1, 0, 2},  {"c5", 256, 24, 24, 128, 3, 1, 0, 2}, {"c9", 128, 46, 46, 64, 2, 1, 0, 0},
    {"p1", 512, 18, 10, 256, 4, 1, 1, 2},  {"p8", 128, 56, 30, 64, 3, 1, 1, 0},  {"n56", 256, 16, 16, 128, 3, 1, 0, 2},
    {"pa", 64, 7, 4, 64, 5, 1, 2, 0},      {"na", 64, 14, 8, 128, 3, 1, 1, 0},
};
static const int BATCHES[] = {8, 12, 67, 200, 512, 1024, 2048};
enum { REQ_STATS = 1, REQ_AFF = 2, REQ_BNRED = 4 };

static es_conv_desc_t make_desc(const Shape& s, int N, es_dtype_t dt, bool dyn) {
  es_conv_desc_t d{};
  d.N = N; d.C = s.C; d.H = s.H; d.W = s.W;
  d.Hu = s.up ? s.H * s.up : s.H; d.Wu = s.up ? s.W * s.up : s.W;
  d.K = s.K; d.R = d.S = s.k; d.stride = s.stride; d.pad = s.pad;
  d.P = (d.Hu + 2 * d.pad - d.R) / d.stride + 1;
  d.Q = (d.Wu + 2 * d.pad - d.S) / d.stride + 1;
  d.up_h = d.up_w = s.up;
  d.rows = dyn ? ROWS : nullptr;
  d.subpixel = es_conv_subpixel_ok(&d, dt);   // (as the callers pack: sub-pixel weights whenever the path takes them)
  return d;
}
static void nhwc(int64_t s[4], int c, int h, int w) {
  s[0] = (int64_t)h * w * c; s[1] = 1; s[2] = (int64_t)w * c; s[3] = c;
}

// mode: 0 FWD, 1 DGRAD, 2 WGRAD; op: 'b' bf16, 'x' exact fp32, 's' split fp32
static void run_case(const std::string& id, const Shape& s, int N, int mode, char op, bool dyn, int req) {
  const es_dtype_t dt = op == 'b' ? ES_BF16 : ES_F32;
  const int eb = op == 'b' ? 2 : 4;
  es_conv_set_f32_split(op == 's' ? 2 : 0);
  const es_conv_desc_t d = make_desc(s, N, dt, dyn);
  static es_affine_t aff;
  static es_norm_t nm;
  static es_chain_t ch;
  aff.scale = FAKE; aff.shift = FAKE; aff.act = ES_ACT_LRELU; aff.slope = 0.1f;
  nm.mean = nm.invstd = nm.gamma = nm.beta = FAKE;
  ch.act = ES_ACT_LRELU; ch.slope = 0.1f; ch.dropout_first = 1; ch.drop.enabled = 1; ch.drop.scale = 1.25f;
  ch.keep = (uint8_t*)FAKE;
  ConvCall call;
  if (req & REQ_STATS) { call.stats_part = STATS; call.stats_floats = 1ll << 40; }
  if (req & REQ_AFF) call.aff = &aff;
  if (req & REQ_BNRED) {
    call.bnr_x = FAKE; call.bnr_nm = &nm; call.bnr_ch = &ch; call.bnr_part = BNRP; call.bnr_floats = 1ll << 40;
  }
  int64_t xs[4], ys[4], dxs[4];
  nhwc(xs, d.C, d.H, d.W);
  nhwc(ys, d.K, d.P, d.Q);
  printf("C %s\n", id.c_str());
  int rc;
  bool same = true;
  if (mode == MODE_WGRAD && dt == ES_F32) {
    call.det_ws = WS; call.det_floats = 1ll << 40;
    memset(&g_in, 0, sizeof g_in);
    g_in.d = d; g_in.a_src = A_BASE; g_in.b_src = B_BASE; g_in.M = d.K;
    const ConvCall before = call;
    rc = es_wgrad_f32_ring(d, A_BASE, ys, B_BASE, xs, DW, 0.f, call, nullptr);
    same = memcmp(&before, &call, sizeof call) == 0;
  } else {
    ConvArgs a;
    memset(&a, 0, sizeof a);
    a.d = d; a.a_src = A_BASE; a.b_src = B_BASE; a.out = O_BASE;
    a.out_bf16 = dt == ES_BF16;
    if (mode == MODE_FWD) {
      for (int i = 0; i < 4; ++i) { a.as[i] = xs[i]; a.os[i] = ys[i]; }
      a.bias = FAKE;
      a.M = d.N * d.P * d.Q; a.Ng = d.K; a.Kd = d.R * d.S * d.C;
    } else if (mode == MODE_DGRAD) {
      a.fold = d.up_h > 0;
      nhwc(dxs, d.C, a.fold ? d.H : d.Hu, a.fold ? d.W : d.Wu);
      for (int i = 0; i < 4; ++i) { a.as[i] = ys[i]; a.os[i] = dxs[i]; }
      a.M = (int)dgrad_rows(d, d.N); a.Ng = d.C;
      a.Kd = (a.fold ? d.up_h * d.up_w : 1) * d.R * d.S * d.K;
    } else {
      for (int i = 0; i < 4; ++i) { a.as[i] = ys[i]; a.bs[i] = xs[i]; }
      a.out = DW;
      a.M = d.K; a.Ng = d.R * d.S * d.C; a.Kd = d.N * d.P * d.Q;
    }
    a.fUh = mkdiv(d.up_h > 0 ? d.up_h : 1); a.fUw = mkdiv(d.up_w > 0 ? d.up_w : 1);
    a.k_per_split = a.Kd;
    memcpy(&g_in, &a, sizeof a);
    const ConvCall before = call;
    rc = eb == 4 ? es_conv_ring_launch_f32(a, mode, call, nullptr) : es_conv_ring_launch(a, mode, call, nullptr);
    same = memcmp(&g_in, &a, sizeof a) == 0 && memcmp(&before, &call, sizeof call) == 0;
  }
  printf("R %d sc=%d bc=%d af=%d path=%d\n", rc, call.stats_chunks, call.bnr_chunks, call.aff_fused, call.path);
  if (rc <= 0) printf("U %d\n", same ? 1 : 0);   // a declined call leaves its arguments as they were
}

int main() {
  static const char* MODES = "FDW";
  static const char* OPS = "bxs";
  char id[96];
  // every shape, batch, mode and operand type, with and without dynamic rows; each request alone (static rows)
  for (const Shape& s : SHAPES)
    for (int N : BATCHES)
      for (int mode = 0; mode < 3; ++mode)
        for (int o = 0; o < 3; ++o)
          for (int dyn = 0; dyn < 2; ++dyn)
            for (int req : {0, (int)REQ_STATS, (int)REQ_AFF, (int)REQ_BNRED}) {
              if (req && dyn) continue;
              if ((req == REQ_STATS || req == REQ_AFF) && mode != MODE_FWD) continue;
              if (req == REQ_BNRED && mode != MODE_DGRAD) continue;
              snprintf(id, sizeof id, "%s/%d/%c/%c/d%d/r%d", s.name, N, MODES[mode], OPS[o], dyn, req);
              run_case(id, s, N, mode, OPS[o], dyn != 0, req);
            }
  // each switch off once (every shape, mode and operand type at B = 1024, all requests made),
  // and forced 64-image chunks (B = 200: chunks of 64, 64, 64 and 8 images)
  typedef int (*Setter)(int);
  static const struct { const char* name; Setter set; int n; } SW[] = {
      {"ring", es_conv_set_ring, 1024},       {"ring256", es_conv_set_ring256, 1024},
      {"persist", es_conv_set_persist, 1024}, {"p256", es_conv_set_p256, 1024},
      {"subpixel", es_conv_set_subpixel, 1024}, {"wgrad_ws", es_conv_set_wgrad_ws, 1024},
      {"chunk64", es_conv_set_f32_chunk, 200},
  };
  for (const auto& sw : SW) {
    const bool chunk = sw.set == es_conv_set_f32_chunk;
    const int old = sw.set(chunk ? 64 : 0);
    for (const Shape& s : SHAPES)
      for (int mode = 0; mode < 3; ++mode)
        for (int o = 0; o < 3; ++o) {
          const int req = mode == MODE_FWD ? REQ_STATS | REQ_AFF : (mode == MODE_DGRAD ? REQ_BNRED : 0);
          snprintf(id, sizeof id, "%s/%d/%c/%c/d0/r%d/%s", s.name, sw.n, MODES[mode], OPS[o], req, sw.name);
          run_case(id, s, sw.n, mode, OPS[o], false, req);
        }
    sw.set(old);
  }
  return 0;
}

// ---------------------------------------------------------------- the kernel files' launch functions
static const char* key_name(const RingKey& k, char* buf, size_t n) {
  const char* b[2] = {"false", "true"};
  const char* t = k.eb == 2 ? "__bf16" : "float";
  switch (k.family) {
    case RK_RING:
      snprintf(buf, n, "conv_ring_kernel<%d, %d, %d, %s, %d, %s, %d, %s>", k.mode, k.bm, k.bn, b[k.sp], k.bk, t, k.spl, b[k.flag]);
      break;
    case RK_PERSIST: snprintf(buf, n, "conv_persist_kernel<%d, %s>", k.bn, b[k.flag]); break;
    case RK_P256: snprintf(buf, n, "conv_p256_kernel<%d, %s>", k.bn / 256, b[k.flag]); break;
    case RK_WGRAD_RING: snprintf(buf, n, "wgrad_ring_kernel<%d, %d, %s>", k.bm, k.bn, b[k.sp]); break;
    case RK_WGRAD_F32: snprintf(buf, n, "wgrad_f32_kernel<%d, %d, %s, %s>", k.bm, k.bn, b[k.sp], b[k.spl != 0]); break;
    case RK_WGRAD_COL2: snprintf(buf, n, "wgrad_f32_col2_kernel"); break;
    case RK_WGRAD_COOP: snprintf(buf, n, "wgrad_coop_kernel<%d, %d, %s>", k.bm, k.bn, b[k.sp]); break;
    default: snprintf(buf, n, "?"); break;
  }
  return buf;
}
static bool rec_plan(const RingKey& k, const int grid[3], const ConvArgs& a, long karg, const float* wsc) {
  char buf[128];
  rec_launch(key_name(k, buf, sizeof buf), dim3(grid[0], grid[1], grid[2]), a, karg, wsc);
  return true;
}
bool conv_ring_bf16_launch(const RingPlan& p, const ConvArgs& a, hipStream_t) { return rec_plan(p.key, p.grid, a, 0, nullptr); }
bool conv_ring_f32_launch(const RingPlan& p, const ConvArgs& a, hipStream_t) { return rec_plan(p.key, p.grid, a, 0, nullptr); }
bool conv_persist_launch(const RingPlan& p, const ConvArgs& a, hipStream_t) { return rec_plan(p.key, p.grid, a, p.karg, nullptr); }
bool wgrad_ring_launch(const RingPlan& p, const ConvArgs& a, hipStream_t) { return rec_plan(p.key, p.grid, a, 0, nullptr); }
bool wgrad_f32_launch(const RingKey& k, const int grid[3], const ConvArgs& a, float* wsc, int ngt, hipStream_t) {
  return rec_plan(k, grid, a, ngt, wsc);
}
void wgrad_reduce_launch(const float* ws, int splits, int K, int C, int R, int S, int ngt, const SubPixel& sp, float*,
                         float beta, hipStream_t) {
  rec_reduce(ws, splits, K, C, R, S, ngt, sp, beta);
}
