// hsk_rows.h -- embedding-row register tiles, dimension dispatch and small device helpers shared by the
// training kernels.  One wavefront owns one row: lane l holds elements (c*64 + l)*V .. +V of chunk c.
#pragma once
#include "hsk_common.h"
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

// Weigh the rows of one buffer (BPR and BCE): buf[0..R) hold entries j .. j+R-1 of a chunk of nr <= 64 entries, lane l
// of `mybias` holds entry l's item bias.  The score of entry j+r is written into lane j+r of one vector, so x and
// g = d loss / d s are evaluated ONCE per buffer, lane-parallel, instead of once per row in all 64 lanes (expf, the
// IEEE division and the lane selects were 32 of the 56 vector instructions a row cost).  expf and '/' are pure per-lane
// functions and the reduction tree, the operands of the bias add, the order of gsum and of the axpys are what the
// row-by-row loop had: identical bits.  Lanes outside [j, j+R) n [0, nr) carry garbage through expf and the division;
// they reach neither gv / xv (the chunk's per-lane g and x, merged here) nor gsum nor acc.
template <int LOSS, int V, int NCH, int R>
__device__ __forceinline__ void hsk_weigh_rows(const hsk_row<V, NCH>& ur, const hsk_row<V, NCH> (&buf)[R], int j, int nr,
                                               int lane, float mybias, float s0, float inv_norm, hsk_row<V, NCH>& acc,
                                               float& gsum, float& gv, float& xv) {
  static_assert(LOSS == HSK_LOSS_BPR || LOSS == HSK_LOSS_BCE, "the sampled softmax keeps a running max: row by row");
  if (j >= nr) return;
  float sv = 0.f;
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (j + r < nr) sv = hsk_writelane_f(hsk_wave_sum(hsk_row_dot_partial(ur, buf[r])), j + r, sv);
  const float s = sv + mybias;
  float x, g;
  if (LOSS == HSK_LOSS_BPR) {
    x = s0 - s;
    g = inv_norm / (1.f + expf(x));    // sigma(-x)/(B*N) = d loss / d s_neg
  } else {
    x = s;
    g = inv_norm / (1.f + expf(-s));   // sigma(s)/(B*K), label 0
  }
  const bool mine = lane >= j && lane < min(j + R, nr);
  gv = mine ? g : gv;
  xv = mine ? x : xv;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (j + r < nr) {
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
