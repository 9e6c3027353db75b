// Stand-alone host program of tests/test_conv_plan_cpu.py: runs the conv dispatcher (csrc/conv_host.hip,
// with csrc/conv_ring_host.hip below it, both compiled host-only) over a fixed list of calls and prints,
// per call, every launch it would make (kernel, grid, the ConvArgs fields the plan sets, a "Z" when the
// launch first zeroes the output) and the call's answer.  The kernel files are replaced by the recording
// launch functions at the end of this file, so no kernel is compiled and nothing touches a device.  The
// output is compared with tests/golden/conv_plan.json.gz, which was recorded once from the single-file
// dispatcher this one replaced.  With the argument "fail" the bf16 ring kernel files answer "no such
// key" instead (the calls of that mode are not in the recording).
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "conv_plan.h"

// ---------------------------------------------------------------- what the library provides elsewhere
void es_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  printf("E ");
  vprintf(fmt, ap);
  printf("\n");
  va_end(ap);
}
// (conv_thin.hip and its own dispatch are not part of this test: no call is a thin conv here)
int es_thin_conv_fwd(const es_conv_desc_t*, es_dtype_t, const void*, const int64_t[4], const void*, const float*, void*,
                     es_dtype_t, const int64_t[4], ConvCall&, hipStream_t) { return 0; }
int es_thin_conv_dgrad(const es_conv_desc_t*, es_dtype_t, const void*, const int64_t[4], const void*, void*, es_dtype_t,
                       const int64_t[4], float, ConvCall&, hipStream_t) { return 0; }
int es_thin_conv_wgrad(const es_conv_desc_t*, es_dtype_t, const void*, const int64_t[4], const void*, const int64_t[4],
                       float*, ConvCall&, hipStream_t) { return 0; }

// ---------------------------------------------------------------- fake operands (never dereferenced)
static char* const A_BASE = (char*)0x100000000000ull;
static char* const B_BASE = (char*)0x200000000000ull;
static char* const O_BASE = (char*)0x300000000000ull;
static float* const WS = (float*)0x600000000000ull;
static float* const DW = (float*)0x700000000000ull;
static const float* const FAKE = (const float*)0x800000000000ull;
static const int32_t* const MAPS = (const int32_t*)0x900000000000ull;

static bool g_fail = false;   // "fail": the bf16 ring kernel files have no kernel for any key

// one launch: the kernel's name as the compiler prints its instantiation, the grid, the ConvArgs fields a
// plan (of this layer or of the ring) or the ring's chunk loop sets, and Z for a zeroed output
static void rec_launch(const char* kernel, dim3 g, const ConvArgs& a, bool zeroed) {
  printf("L %s g=%u,%u,%u kps=%d sk=%d det=%d", kernel, g.x, g.y, g.z, a.k_per_split, a.splitk, a.det);
  if (a.det_ws) printf(" dws=%lld", (long long)(a.det_ws - WS));
  if (a.nbase) printf(" nb=%d", a.nbase);
  printf(" o=%c%s\n", a.out == (void*)WS ? 'W' : (a.out == (void*)DW ? 'D' : (a.out == (void*)O_BASE ? 'O' : '+')),
         zeroed ? " Z" : "");
}
static void rec_igemm(int eb, int mode, int bm, int bn, bool av, bool bv, dim3 g, const ConvArgs& a, bool zeroed) {
  char name[96];
  snprintf(name, sizeof name, "conv_igemm_kernel<%s, %d, %d, %d, %s, %s>", eb == 2 ? "__bf16" : "float", mode, bm, bn,
           av ? "true" : "false", bv ? "true" : "false");
  rec_launch(name, g, a, zeroed);
}
static void rec_glds(int mode, int bm, int bn, dim3 g, const ConvArgs& a) {
  char name[64];
  snprintf(name, sizeof name, "conv_glds_kernel<%d, %d, %d>", mode, bm, bn);
  rec_launch(name, g, a, false);
}

// ---------------------------------------------------------------- the calls
struct Shape {
  const char* name;
  int C, H, W, K, k, stride, pad, up;
  int Hu, Wu;   // > 0: resized through hmap / wmap
  int nchw;     // the activations' channel stride is not 1
};
// tests/test_f32_ring_gpu.py::CASES (the ring hand-off)
static const Shape RING[] = {
    {"c0", 128, 13, 13, 256, 3, 1, 0, 2},  {"c5", 256, 24, 24, 128, 3, 1, 0, 2}, {"c9", 128, 46, 46, 64, 2, 1, 0, 0},
    {"p1", 512, 18, 10, 256, 4, 1, 1, 2},  {"p8", 128, 56, 30, 64, 3, 1, 1, 0},  {"n56", 256, 16, 16, 128, 3, 1, 0, 2},
    {"pa", 64, 7, 4, 64, 5, 1, 2, 0},      {"na", 64, 14, 8, 128, 3, 1, 1, 0},
};
// expertsim/models: the linears (1 x 1 convs on 1 x 1 images) and the small and irregular convs
static const Shape SMALL[] = {
    {"g_fc1", 19, 1, 1, 256, 1, 1, 0, 0},          // generator fc1: C % 4 != 0, no vector gather
    {"g_fc2n", 256, 1, 1, 21632, 1, 1, 0, 0},      // neutron generator fc2 (128 x 13 x 13)
    {"g_fc2p", 256, 1, 1, 92160, 1, 1, 0, 0},      // proton generator fc2 (512 x 18 x 10)
    {"d_fc1", 1305, 1, 1, 128, 1, 1, 0, 0},        // discriminator fc1 (16 x 9 x 9 + 9 conditions)
    {"d_fc2", 128, 1, 1, 64, 1, 1, 0, 0},
    {"d_fc3", 64, 1, 1, 1, 1, 1, 0, 0},
    {"a_dense", 64, 1, 1, 2, 1, 1, 0, 0},          // neutron aux regressor's dense
    {"r_fc1", 9, 1, 1, 128, 1, 1, 0, 0},           // router fc_layers.0 and .2
    {"r_fc2", 128, 1, 1, 64, 1, 1, 0, 0},
    {"d_c4", 32, 21, 21, 16, 3, 1, 0, 0},          // discriminator conv_layers.4 (narrow tiles)
    {"an_c2", 32, 21, 21, 64, 3, 1, 0, 0},         // neutron aux regressor conv2 .. conv4, reduce
    {"an_c3", 64, 9, 19, 128, 3, 1, 0, 0},
    {"an_c4", 128, 3, 17, 256, 3, 1, 0, 0},
    {"an_red", 256, 1, 15, 64, 1, 1, 0, 0},
    {"ap_c1", 32, 27, 14, 32, 5, 2, 2, 0},         // proton aux regressor res1.conv1 and its downsample
    {"ap_ds", 32, 27, 14, 32, 1, 2, 0, 0},
    {"ap_c2", 32, 14, 7, 64, 5, 2, 2, 0},          // res2.conv1
    {"p_c5", 256, 35, 19, 128, 4, 1, 1, 0, 56, 30},   // proton generator conv_layers.5: resized to 56 x 30 by maps
    {"nchw", 64, 14, 8, 128, 3, 1, 1, 0, 0, 0, 1},    // an NCHW-strided input
    {"s3", 32, 21, 21, 32, 3, 3, 0, 0},               // synthetic: stride 3 (no vector gather)
    {"w128", 128, 12, 12, 128, 3, 1, 1, 0},           // synthetic: the bf16 WGRAD LDS-DMA tiles with the ring off
    {"n96", 25, 10, 10, 96, 3, 1, 1, 0},              // synthetic: 128 x 128 tiles without vector gathers
    {"nchw16", 32, 21, 21, 16, 3, 1, 0, 0, 0, 0, 1},  // synthetic: 128 x 32 tiles, vector gather of the weights only
    {"w_tf", 3, 21, 21, 16, 3, 1, 0, 0},              // synthetic: 32 x 128 WGRAD tiles, vector gather of dy only
    {"wl", 4098, 1, 1, 4096, 1, 1, 0, 0},             // synthetic: 128 x 128 WGRAD tiles, vector gather of dy only
};

static es_conv_desc_t make_desc(const Shape& s, int N, es_dtype_t dt) {
  es_conv_desc_t d{};
  d.N = N; d.C = s.C; d.H = s.H; d.W = s.W;
  d.Hu = s.Hu ? s.Hu : (s.up ? s.H * s.up : s.H);
  d.Wu = s.Wu ? s.Wu : (s.up ? s.W * s.up : s.W);
  d.K = s.K; d.R = d.S = s.k; d.stride = s.stride; d.pad = s.pad;
  d.P = (d.Hu + 2 * d.pad - d.R) / d.stride + 1;
  d.Q = (d.Wu + 2 * d.pad - d.S) / d.stride + 1;
  d.up_h = d.up_w = s.up;
  if (s.Hu) d.hmap = d.wmap = MAPS;
  d.subpixel = es_conv_subpixel_ok(&d, dt);   // (as the callers pack: sub-pixel weights whenever the path takes them)
  return d;
}
static void strides(int64_t s[4], int c, int h, int w, bool nchw) {
  if (nchw) { s[0] = (int64_t)c * h * w; s[1] = (int64_t)h * w; s[2] = w; s[3] = 1; }
  else { s[0] = (int64_t)h * w * c; s[1] = 1; s[2] = (int64_t)w * c; s[3] = c; }
}

// mode: 0 FWD, 1 DGRAD, 2 WGRAD; op: 'b' bf16, 'x' exact fp32, 's' split fp32; det: deterministic mode;
// ws: the workspace of the es_conv2d_*_det entries: 0 absent (the plain entries), 1 as es_conv2d_splitk_ws_bytes /
// es_conv2d_wgrad_det_ws_bytes size it, 2 one partial slot; aff: an affine epilogue is requested (FWD)
static int run_case(const std::string& id, const Shape& s, int N, int mode, char op, int det, int ws, bool aff) {
  const es_dtype_t dt = op == 'b' ? ES_BF16 : ES_F32;
  es_conv_set_f32_split(op == 's' ? 2 : 0);
  es_set_deterministic(det);
  const es_conv_desc_t d = make_desc(s, N, dt);
  static es_affine_t epi;
  epi.scale = FAKE; epi.shift = FAKE; epi.act = ES_ACT_LRELU; epi.slope = 0.1f;
  int64_t xs[4], ys[4], dxs[4];
  strides(xs, d.C, d.H, d.W, s.nchw != 0);
  strides(ys, d.K, d.P, d.Q, s.nchw != 0);
  const bool fold = d.up_h > 0;
  strides(dxs, d.C, fold ? d.H : d.Hu, fold ? d.W : d.Wu, s.nchw != 0);
  ConvCall call;
  if (aff) call.aff = &epi;
  if (ws) {
    const int64_t slot = mode == MODE_WGRAD ? (int64_t)d.K * d.R * d.S * d.C
                         : (mode == MODE_FWD ? (int64_t)d.N * d.P * d.Q * d.K : dgrad_rows(d, d.N) * d.C);
    const int64_t full = mode == MODE_WGRAD ? es_conv2d_wgrad_det_ws_bytes(&d, dt, ys, xs) : es_conv2d_splitk_ws_bytes(&d, mode);
    call.det_ws = WS;
    call.det_floats = ws == 1 ? full / 4 : slot;
  }
  printf("C %s\n", id.c_str());
  const ConvCall before = call;
  int rc;
  if (mode == MODE_FWD) rc = conv_fwd(&d, dt, A_BASE, xs, B_BASE, FAKE, O_BASE, dt, ys, call, nullptr);
  else if (mode == MODE_DGRAD) rc = conv_dgrad(&d, dt, A_BASE, ys, B_BASE, O_BASE, dt, dxs, 0.f, call, nullptr);
  else rc = conv_wgrad(&d, dt, A_BASE, ys, B_BASE, xs, DW, call, nullptr);
  printf("R %d ds=%d af=%d path=%d\n", rc, call.det_splits, call.aff_fused, call.path);
  if (rc != ES_OK) printf("U %d\n", memcmp(&before, &call, sizeof call) == 0 ? 1 : 0);   // a failed call leaves its context
  return rc;
}

static const char* MODES = "FDW";
// bf16; exact and split fp32 without and with deterministic mode, and in it the three workspaces
static const struct { char op; int det, ws; } VARIANTS[] = {
    {'b', 0, 0}, {'x', 0, 0}, {'x', 1, 0}, {'x', 1, 1}, {'x', 1, 2}, {'s', 0, 0}, {'s', 1, 0}, {'s', 1, 1}, {'s', 1, 2},
};

template <int NS, int NB>
static void sweep(const Shape (&shapes)[NS], const int (&batches)[NB], bool with_aff) {
  char id[96];
  for (const Shape& s : shapes)
    for (int N : batches)
      for (int mode = 0; mode < 3; ++mode)
        for (const auto& v : VARIANTS)
          for (int aff = 0; aff < (with_aff && mode == MODE_FWD && v.ws == 0 ? 2 : 1); ++aff) {
            snprintf(id, sizeof id, "%s/%d/%c/%c/d%d/w%d/a%d", s.name, N, MODES[mode], v.op, v.det, v.ws, aff);
            run_case(id, s, N, mode, v.op, v.det, v.ws, aff != 0);
          }
}

int main(int argc, char** argv) {
  char id[96];
  if (argc > 1 && !strcmp(argv[1], "fail")) {
    // the three places that ask the bf16 ring: FWD / DGRAD, WGRAD, and the sub-pixel hand-off
    g_fail = true;
    run_case("fail/fwd", RING[2], 1024, MODE_FWD, 'b', 0, 0, false);
    run_case("fail/dgrad", RING[4], 1024, MODE_DGRAD, 'b', 0, 0, false);
    run_case("fail/wgrad", RING[2], 1024, MODE_WGRAD, 'b', 0, 0, false);
    run_case("fail/subpixel", RING[0], 1024, MODE_FWD, 'b', 0, 0, false);
    return 0;
  }
  static const int RING_BATCHES[] = {8, 200, 1024}, SMALL_BATCHES[] = {8, 200, 512, 1024};
  sweep(RING, RING_BATCHES, true);
  sweep(SMALL, SMALL_BATCHES, false);
  // es_conv_set_glds(0) and es_conv_set_ring(0), each once over all shapes at batch 1024
  typedef int (*Setter)(int);
  static const struct { const char* name; Setter set; } SW[] = {{"glds", es_conv_set_glds}, {"ring", es_conv_set_ring}};
  for (const auto& sw : SW) {
    const int old = sw.set(0);
    for (int k = 0; k < 2; ++k)
      for (const Shape* s = k ? SMALL : RING; s != (k ? SMALL + sizeof SMALL / sizeof *SMALL : RING + sizeof RING / sizeof *RING); ++s)
        for (int mode = 0; mode < 3; ++mode)
          for (char op : {'b', 'x', 's'}) {
            snprintf(id, sizeof id, "%s/1024/%c/%c/d0/w0/a0/%s", s->name, MODES[mode], op, sw.name);
            run_case(id, *s, 1024, mode, op, 0, 0, false);
          }
    sw.set(old);
  }
  return 0;
}

// ---------------------------------------------------------------- the kernel files' launch functions
// the weight packing's plane offset (conv_pack.hip)
extern "C" int64_t es_weight_planes_offset(int64_t n) { return (n * 4 + 255) / 256 * 256; }

static int rec_conv(const ConvPlan& p, const ConvArgs& a) {
  const ConvKey& k = p.key;
  const dim3 g(p.grid[0], p.grid[1], p.grid[2]);
  if (k.family == ROUTE_IGEMM) rec_igemm(k.eb, k.mode, k.bm, k.bn, k.avec, k.bvec, g, a, p.zero_out);
  else if (k.family == ROUTE_GLDS) rec_glds(k.mode, k.bm, k.bn, g, a);
  else rec_launch("conv_wgrad_glds_kernel", g, a, false);
  return 1;
}
int conv_igemm_bf16_launch(const ConvPlan& p, const ConvArgs& a, hipStream_t) { return p.key.eb == 2 ? rec_conv(p, a) : 0; }
int conv_igemm_f32_launch(const ConvPlan& p, const ConvArgs& a, hipStream_t) { return p.key.eb == 4 ? rec_conv(p, a) : 0; }
void splitk_reduce_launch(const float*, int, int64_t, float*, hipStream_t) {}

// the ring kernel files (tests/test_ring_plan_cpu.py pins what the ring plans): family, tile and grid
static bool rec_ring(const RingKey& k, const int grid[3], const ConvArgs& a) {
  char name[96];
  snprintf(name, sizeof name, "ring%d<%d, %d, %d, %d, %d, %d, %d, %d>", k.family, k.mode, k.bm, k.bn, k.sp, k.bk, k.eb, k.spl, k.flag);
  rec_launch(name, dim3(grid[0], grid[1], grid[2]), a, false);
  return true;
}
bool conv_ring_bf16_launch(const RingPlan& p, const ConvArgs& a, hipStream_t) { return !g_fail && rec_ring(p.key, p.grid, a); }
bool conv_ring_f32_launch(const RingPlan& p, const ConvArgs& a, hipStream_t) { return rec_ring(p.key, p.grid, a); }
bool conv_persist_launch(const RingPlan& p, const ConvArgs& a, hipStream_t) { return !g_fail && rec_ring(p.key, p.grid, a); }
bool wgrad_ring_launch(const RingPlan& p, const ConvArgs& a, hipStream_t) { return !g_fail && rec_ring(p.key, p.grid, a); }
bool wgrad_f32_launch(const RingKey& k, const int grid[3], const ConvArgs& a, float*, int, hipStream_t) { return rec_ring(k, grid, a); }
void wgrad_reduce_launch(const float*, int, int, int, int, int, int, const SubPixel&, float*, float, hipStream_t) {}
int es_wgrad_ws_launch(int, bool, dim3, const ConvArgs&, float*, int, hipStream_t) { return 0; }
