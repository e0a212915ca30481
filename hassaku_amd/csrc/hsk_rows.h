// hsk_rows.h -- embedding-row register tiles, dimension dispatch and small device helpers shared by the
// training kernels.  One wavefront owns one row: lane l holds elements (c*64 + l)*V .. +V of chunk c.
#pragma once
#include "hsk_common.h"
#include <hip/hip_ext.h>
#include <type_traits>

#define HSK_OWNER_NONE 0x7fffffff

// Device-resident step descriptor.  A replayed HIP graph has its kernel arguments frozen at capture time, so what
// changes from one replay to the next -- where the run of batches starts, how many steps were applied before it (RNG
// stream id, Adam bias corrections), the epoch permutation -- is read from here; a kernel of step `rel` of the run
// adds its own (frozen) offset.  desc == NULL: the immediate arguments apply (eager launches).
struct hsk_step_desc {
  long long start0;        // position of the run's first batch in `order`
  const int64_t* order;    // epoch permutation (NULL: identity)
  int step0;               // optimiser steps applied before the run
  int pad;
};

// ---------------------------------------------------------------------------------------------
// dimension dispatch: V floats per lane per chunk, NCH chunks per row, FULL = no tail predicate
// ---------------------------------------------------------------------------------------------
template <typename F>
static int hsk_dispatch_dim(int64_t D, F&& f) {
  int V = (D % 4 == 0) ? 4 : (D % 2 == 0) ? 2 : 1;
  int64_t chunks = hsk_ceil_div(D, (int64_t)64 * V);
  int nch = chunks <= 1 ? 1 : chunks <= 2 ? 2 : chunks <= 4 ? 4 : chunks <= 8 ? 8 : 0;
  if (nch == 0) {
    hsk_set_error("embedding_dim %lld not supported (max %d for this alignment)", (long long)D, 64 * V * 8);
    return HSK_ERR_UNSUPPORTED;
  }
  bool full = (D == (int64_t)64 * V * nch);
#define HSK_CASE(v, n)                                                                          \
  if (V == v && nch == n) {                                                                     \
    if (v == 4 && full)                                                                         \
      return f(std::integral_constant<int, v>{}, std::integral_constant<int, n>{}, std::true_type{}); \
    return f(std::integral_constant<int, v>{}, std::integral_constant<int, n>{}, std::false_type{});  \
  }
  HSK_CASE(4, 1) HSK_CASE(4, 2) HSK_CASE(4, 4) HSK_CASE(4, 8)
  HSK_CASE(2, 1) HSK_CASE(2, 2) HSK_CASE(2, 4) HSK_CASE(2, 8)
  HSK_CASE(1, 1) HSK_CASE(1, 2) HSK_CASE(1, 4) HSK_CASE(1, 8)
#undef HSK_CASE
  hsk_set_error("internal: no kernel for dim %lld", (long long)D);
  return HSK_ERR_UNSUPPORTED;
}

// runtime booleans -> template flags: f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...), the first flag first.
// f is instantiated for EVERY combination, so a combination without a kernel needs an `if constexpr` inside f.
template <typename F>
static int hsk_dispatch_flags(F&& f) { return f(); }
template <typename F, typename... Bs>
static int hsk_dispatch_flags(F&& f, bool b0, Bs... bs) {
  auto bound = [&](auto c0) { return hsk_dispatch_flags([&](auto... cs) { return f(c0, cs...); }, bs...); };
  return b0 ? bound(std::true_type{}) : bound(std::false_type{});
}

// loss kind -> f(std::integral_constant<int, HSK_LOSS_*>{}).  WITH_SSM = false: for kernels that carry the bpr and bce
// epilogues only (every other kind takes the bpr one, the callers keep sampled softmax away from them)
template <bool WITH_SSM, typename F>
static int hsk_dispatch_loss(int kind, F&& f) {
  if (kind == HSK_LOSS_BCE) return f(std::integral_constant<int, HSK_LOSS_BCE>{});
  if constexpr (WITH_SSM)
    if (kind == HSK_LOSS_SSM) return f(std::integral_constant<int, HSK_LOSS_SSM>{});
  return f(std::integral_constant<int, HSK_LOSS_BPR>{});
}

// One launch that may carry events: hipExtLaunchKernelGGL with `beg` / `end` (NULL: none) as the dispatch's own start /
// stop timestamps, or, capturing, an ordinary launch.  Every kernel argument is written out, defaults included.
template <typename... KArgs, typename... Args>
static void hsk_launch_ev(void (*kernel)(KArgs...), dim3 grid, dim3 block, unsigned lds_bytes, hipStream_t stream,
                          bool capturing, hipEvent_t beg, hipEvent_t end, const Args&... args) {
  static_assert(sizeof...(KArgs) == sizeof...(Args), "hsk_launch_ev: pass every kernel argument, defaults included");
  if (capturing)
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, static_cast<KArgs>(args)...);
  else
    hipExtLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, beg, end, 0, static_cast<KArgs>(args)...);
}

// ---------------------------------------------------------------------------------------------
// row helpers
// ---------------------------------------------------------------------------------------------
template <int V, int NCH>
struct hsk_row {
  hsk_vec<V> c[NCH];
};

template <int V, int NCH, bool FULL>
__device__ __forceinline__ void hsk_row_load(hsk_row<V, NCH>& r, const float* __restrict__ base, int lane, int D) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int off = (c * 64 + lane) * V;
    if (FULL || off < D)
      r.c[c] = hsk_ldg<V>(base + off);
    else
      r.c[c] = hsk_zero<V>();
  }
}

template <int V, int NCH, bool FULL>
__device__ __forceinline__ void hsk_row_store(const hsk_row<V, NCH>& r, float* __restrict__ base, int lane, int D) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int off = (c * 64 + lane) * V;
    if (FULL || off < D) hsk_stg<V>(base + off, r.c[c]);
  }
}

// the same under a store policy (hsk_common.h); `base` is wave-uniform, as everywhere a wave owns a row
template <int POL, int V, int NCH, bool FULL>
__device__ __forceinline__ void hsk_row_store_as(const hsk_row<V, NCH>& r, float* __restrict__ base, int lane, int D) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int off = (c * 64 + lane) * V;
    if (FULL || off < D) hsk_stg_as<POL, V>(base, off, D, r.c[c]);
  }
}
template <int V, int NCH, bool FULL>
__device__ __forceinline__ void hsk_row_store_wt(const hsk_row<V, NCH>& r, float* __restrict__ base, int lane, int D) {
  hsk_row_store_as<HSK_ST_WT, V, NCH, FULL>(r, base, lane, D);
}

template <int V, int NCH>
__device__ __forceinline__ void hsk_row_zero(hsk_row<V, NCH>& r) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) r.c[c] = hsk_zero<V>();
}

template <int V, int NCH>
__device__ __forceinline__ float hsk_row_dot_partial(const hsk_row<V, NCH>& a, const hsk_row<V, NCH>& b) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int i = 0; i < V; ++i) s = fmaf(a.c[c].v[i], b.c[c].v[i], s);
  return s;
}

template <int V, int NCH>
__device__ __forceinline__ void hsk_row_axpy(hsk_row<V, NCH>& acc, float a, const hsk_row<V, NCH>& x) {
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int i = 0; i < V; ++i) acc.c[c].v[i] = fmaf(a, x.c[c].v[i], acc.c[c].v[i]);
}

template <int V, int NCH>
__device__ __forceinline__ void hsk_row_add(hsk_row<V, NCH>& acc, const hsk_row<V, NCH>& x) {
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int i = 0; i < V; ++i) acc.c[c].v[i] += x.c[c].v[i];
}

__device__ __forceinline__ float hsk_softplus(float z) {
  // BCEWithLogits(x, 1) = softplus(-x) = max(-x,0) + log1p(exp(-|x|)); here z = -x
  return fmaxf(z, 0.f) + log1pf(expf(-fabsf(z)));
}

// inv * sigma(-x) = inv / (1 + exp(x)): the weight of a BPR / BCE entry.  Past x = 88.72 expf(x) is +inf and the quotient
// 0, while inv * exp(-x) is still an fp32 subnormal (up to inv * 2^-128: hundreds of steps of 2^-149 at a small batch).
// TINY: there the weight is taken from expf(-x) instead; wherever expf(x) is finite the bits are those of the quotient.
// The empty asm keeps the second exponential behind a branch that no lane takes on ordinary scores (left to itself the
// compiler evaluates both on every call: 17 vector instructions per buffer of rows).  (tests/test_loss_range.py, `wide`)
// TINY = false is the plain quotient, kept in k_fwd_part alone, whose gather loop has no register to spare
// (hsk_fwd_part.h) and whose instruction stream this leaves as it was.  It is launched from B >= 2048 and N >= 16 only
// (hsk_part_rule), so inv <= 2^-15 and an entry past x = 88.72 loses at most inv * 2^-128 <= 2^-143: 0.1 * 2^21 / (B N)
// steps of 2^-149 of exp_avg -- up to 6.4 steps PER ENTRY at B N = 32 768, under one step from B N = 2.1e5 on.  The
// 8 + (n - 1) steps tests/test_loss_range.py grants an element of n entries therefore hold for k_fwd_part only where
// n = 1 or B N >= 2.1e5 (the tested shape, B N = 278 528: 0.75 steps per entry); below that, and for x > 88.72 only,
// k_fwd_part and the other forwards differ by those few steps of 2^-149.
template <bool TINY = true>
__device__ __forceinline__ float hsk_sigmoid_neg_scaled(float inv, float x) {
  const float e = expf(x);
  float g = inv / (1.f + e);
  if (TINY && e == INFINITY) {
    float nx = -x;
    asm volatile("" : "+v"(nx));
    g = inv * expf(nx);
  }
  return g;
}

// Weigh the rows of one buffer (BPR and BCE): buf[0..R) hold entries j .. j+R-1 of a chunk of nr <= 64 entries, lane l
// of `mybias` holds entry l's item bias.  The score of entry j+r is written into lane j+r of one vector, so x and
// g = d loss / d s are evaluated ONCE per buffer, lane-parallel, instead of once per row in all 64 lanes (expf, the
// IEEE division and the lane selects were 32 of the 56 vector instructions a row cost).  expf and '/' are pure per-lane
// functions and the reduction tree, the operands of the bias add, the order of gsum and of the axpys are what the
// row-by-row loop had: identical bits.  Lanes outside [j, j+R) n [0, nr) carry garbage through expf and the division;
// they reach neither gv / xv (the chunk's per-lane g and x, merged here) nor gsum nor acc.
// FULL_BUF: the caller vouches for j + R <= nr -- no test per row, no clamp of `mine`: one straight-line block, which the
// overlapped gather loop (hsk_fwd_part.h) needs around its loads; the same operations on the same operands otherwise.
template <int LOSS, bool TINY = true, bool FULL_BUF = false, int V, int NCH, int R>
__device__ __forceinline__ void hsk_weigh_rows(const hsk_row<V, NCH>& ur, const hsk_row<V, NCH> (&buf)[R], int j, int nr,
                                               int lane, float mybias, float s0, float inv_norm, hsk_row<V, NCH>& acc,
                                               float& gsum, float& gv, float& xv) {
  static_assert(LOSS == HSK_LOSS_BPR || LOSS == HSK_LOSS_BCE, "the sampled softmax keeps a running max: row by row");
  if (!FULL_BUF && j >= nr) return;
  float sv = 0.f;
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (FULL_BUF || j + r < nr) sv = hsk_writelane_f(hsk_wave_sum(hsk_row_dot_partial(ur, buf[r])), j + r, sv);
  const float s = sv + mybias;
  float x, g;
  if (LOSS == HSK_LOSS_BPR) {
    x = s0 - s;
    g = hsk_sigmoid_neg_scaled<TINY>(inv_norm, x);    // sigma(-x)/(B*N) = d loss / d s_neg
  } else {
    x = s;
    g = hsk_sigmoid_neg_scaled<TINY>(inv_norm, -s);   // sigma(s)/(B*K), label 0
  }
  const bool mine = lane >= j && lane < (FULL_BUF ? j + R : min(j + R, nr));
  gv = mine ? g : gv;
  xv = mine ? x : xv;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (FULL_BUF || j + r < nr) {
      const float gr = hsk_readlane_f(g, j + r);
      if (LOSS == HSK_LOSS_BPR) gsum += gr;   // row order
      hsk_row_axpy(acc, gr, buf[r]);
    }
  }
}

__device__ __forceinline__ int hsk_clamp_index(long long idx, long long n, int32_t* status) {
  if (idx < 0 || idx >= n) {
    if (status) atomicOr(status, HSK_STATUS_BAD_INDEX);
    return 0;
  }
  return (int)idx;
}
