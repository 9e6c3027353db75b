// Host side of the convolution entries (conv_host.hip): the plan the top-level dispatcher makes for one
// call, and the launch functions of the kernel files below it (conv_igemm_bf16.hip, conv_igemm_f32.hip).
//
// Plan, then launch, as one layer down (ring_plan.h): conv_plan() is a pure function of the call.  It
// answers an error or fills a ConvPlan: whether a ring dispatcher is asked first, which 4-wave kernel
// runs when none is asked or the ring declines, on which grid, and every ConvArgs field and ConvCall
// result that launch sets.  conv_dispatch() applies a plan to its own copy of the arguments only when
// it launches, so a declined or failed call leaves the caller's ConvArgs and ConvCall as they were.
// Each kernel file exports one function that looks the plan's key up in its table of instantiations; a
// key that is not there is an error, never a silent fall-back.
#pragma once
#include "conv_common.h"
#include "ring_plan.h"

// ROUTE_RING_*: hand the call to es_conv_ring_launch / es_conv_ring_launch_f32 (their own planner
// decides; a declined call goes to ConvPlan::fallback)
enum { ROUTE_NONE, ROUTE_RING_BF16, ROUTE_RING_F32, ROUTE_GLDS, ROUTE_WGRAD_GLDS, ROUTE_IGEMM };

// One instantiation of the 4-wave kernels.  Fields a family does not have are 0.
//   ROUTE_IGEMM       conv_igemm_kernel<T (eb bytes), mode, bm, bn, avec, bvec>
//   ROUTE_GLDS        conv_glds_kernel<mode, bm, bn>
//   ROUTE_WGRAD_GLDS  conv_wgrad_glds_kernel
struct ConvKey { int family, eb, mode, bm, bn, avec, bvec; };
constexpr bool operator==(const ConvKey& x, const ConvKey& y) {
  return x.family == y.family && x.eb == y.eb && x.mode == y.mode && x.bm == y.bm && x.bn == y.bn && x.avec == y.avec &&
         x.bvec == y.bvec;
}
constexpr ConvKey igemm_key(int eb, int mode, int bm, int bn, bool avec, bool bvec) {
  return ConvKey{ROUTE_IGEMM, eb, mode, bm, bn, avec, bvec};
}
constexpr ConvKey glds_key(int mode, int bm, int bn) { return ConvKey{ROUTE_GLDS, 2, mode, bm, bn, 1, 1}; }
constexpr ConvKey wgrad_glds_key() { return ConvKey{ROUTE_WGRAD_GLDS, 2, MODE_WGRAD, 128, 128, 1, 1}; }

struct ConvPlan {
  int route;      // ROUTE_*: where the call goes first
  int fallback;   // route is a ring: the 4-wave route when the ring declines (ROUTE_NONE: an error, only the
                  // ring reads sub-pixel operands)
  // the launch of the 4-wave route (route, or fallback behind a ring)
  ConvKey key;
  int grid[3];
  int k_per_split, splitk, det;   // ConvArgs fields of that launch
  float* det_ws;
  int det_splits;   // ConvCall result
  bool zero_out;    // split-K with atomics: the launch first zeroes the dense fp32 output
};

// (library-internal: these functions are not part of the exported symbol set)
#pragma GCC visibility push(hidden)

// Everything the dispatcher decides itself.  avec / bvec: 16-byte vector gathers of the A / B operand are
// possible (vec16); det_mode: es_set_deterministic.  ES_OK: p is the plan.
int conv_plan(const ConvArgs& a, int mode, es_dtype_t dt, bool avec, bool bvec, const ConvCall& call,
              const RingSwitches& sw, bool det_mode, ConvPlan& p);
void conv_apply(const ConvPlan& p, ConvArgs& a, ConvCall& call);
// plans the call with the library's switches and launches it
int conv_dispatch(const ConvArgs& a, int mode, es_dtype_t dt, bool avec, bool bvec, ConvCall& call, hipStream_t st);

// The three convolutions under the C-ABI entries, per call context.  They read no launch status: each
// entry does that once, after they return.
int conv_fwd(const es_conv_desc_t* d, es_dtype_t dt, const void* x, const int64_t xs[4], const void* wk,
             const float* bias, void* y, es_dtype_t ydt, const int64_t ys[4], ConvCall& call, hipStream_t st);
int conv_dgrad(const es_conv_desc_t* d, es_dtype_t dt, const void* dy, const int64_t ys[4], const void* wd,
               void* dxu, es_dtype_t dxdt, const int64_t dxs[4], float beta, ConvCall& call, hipStream_t st);
int conv_wgrad(const es_conv_desc_t* d, es_dtype_t dt, const void* dy, const int64_t ys[4], const void* x,
               const int64_t xs[4], float* dw, ConvCall& call, hipStream_t st);

// One row of a kernel file's table (key -> launch of that instantiation) and the lookup
struct ConvEntry {
  ConvKey key;
  void (*launch)(const ConvArgs&, dim3, hipStream_t);
};
template <int N>
const ConvEntry* conv_find(const ConvEntry (&table)[N], const ConvKey& key) {
  for (const ConvEntry& e : table)
    if (e.key == key) return &e;
  return nullptr;
}

// The kernel files' launch functions: 1 launched, 0 when the key is not one of the file's instantiations,
// < 0 when zeroing the output failed (ES_ERR_HIP, message set).
int conv_igemm_bf16_launch(const ConvPlan& p, const ConvArgs& a, hipStream_t st);   // conv_igemm_bf16.hip
int conv_igemm_f32_launch(const ConvPlan& p, const ConvArgs& a, hipStream_t st);    // conv_igemm_f32.hip
// out[i] = sum over z of ws[z * n + i], in order (deterministic split-K FWD / DGRAD; conv_igemm_f32.hip)
void splitk_reduce_launch(const float* ws, int splits, int64_t n, float* out, hipStream_t st);

#pragma GCC visibility pop
