// hsk_ecf.hip -- the affiliation of a row of similarities to the taste clusters of ECF (algorithms/sgd_alg.py:579-775 of
// the reference; Du et al., "Towards Explainable Collaborative Filtering with Taste Clusters Learning", WWW 2023).
//
// For a row s[0..C) of S [n, C] row-major, 1 <= k <= C <= 64 and a temperature t > 0:
//   p    = softmax(s / t)
//   m_c  = 1 if rank(c) < k else 0,   rank(c) = #{ j : s_j > s_c  or (s_j == s_c and j < c) }   (lower index wins a tie)
//   mh   = p + (m - p)                                           in fp32, in this order
//   A    = sigmoid(s) * mh                                       exactly 0 off the mask
// The gradient passes through p only (the mask is a constant): with G = dL/dA and h_c = G_c * sigmoid(s_c)
//   dS_c = G_c * sigmoid'(s_c) * mh_c + (1 / t) * p_c * (h_c - sum_j p_j h_j)
// The backward recomputes p, m and the sigmoid from S.
//
// One lane holds one cluster.  A row occupies W = the smallest power of two >= C consecutive lanes, so a wave owns
// 64 / W rows (one row for C in 33..64); the row maximum and the row sums are xor butterflies that stay inside the W
// lanes, the rank is counted against each of the row's C values read from its lane.  No LDS, no atomics: two calls give
// the same bits.
#include "hsk_common.h"

#include <limits.h>
#include <math.h>

#define HSK_ECF_MAX_CLUSTERS 64

template <int W>
__device__ __forceinline__ float hsk_seg_max(float v) {
#pragma unroll
  for (int off = W / 2; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, HSK_WAVE));
  return v;
}

template <int W>
__device__ __forceinline__ float hsk_seg_sum(float v) {
#pragma unroll
  for (int off = W / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, HSK_WAVE);
  return v;
}

// value of cluster j of this lane's row: lane j of the wave when the row is the wave (j is wave-uniform)
template <int W>
__device__ __forceinline__ float hsk_seg_read(float v, int lane, int j) {
  if (W == HSK_WAVE) return hsk_readlane_f(v, j);
  return __shfl(v, (lane & ~(W - 1)) + j, HSK_WAVE);
}

struct hsk_ecf_row {
  float p, mh, sig, dsig;
};

// s: this lane's similarity (-inf on a lane that holds no cluster); every lane of the wave takes part
template <int W>
__device__ __forceinline__ hsk_ecf_row hsk_ecf_forward(float s, bool live, int lane, int c, int C, int k, float t) {
  const float z = s / t;
  const float zmax = hsk_seg_max<W>(z);
  const float e = live ? expf(z - zmax) : 0.f;
  const float den = hsk_seg_sum<W>(e);
  int rank = 0;
  for (int j = 0; j < C; ++j) {
    const float sj = hsk_seg_read<W>(s, lane, j);
    rank += (sj > s || (sj == s && j < c)) ? 1 : 0;
  }
  hsk_ecf_row r;
  r.p = e / den;
  const float m = rank < k ? 1.f : 0.f;
  r.mh = r.p + (m - r.p);
  // sigmoid and its derivative from e = exp(-|s|): sigmoid(|s|) = 1 / (1 + e), sigmoid(-|s|) = e / (1 + e),
  // sigmoid' = e / (1 + e)^2 -- no overflow, and no 1 - sigmoid that cancels to 0 where the sigmoid saturates
  const float en = expf(-fabsf(s));
  const float rn = 1.f / (1.f + en);
  r.sig = s >= 0.f ? rn : en * rn;
  r.dsig = en * rn * rn;
  return r;
}

template <int W, bool BWD>
__global__ __launch_bounds__(256) void k_ecf_affiliation(const float* __restrict__ S, const float* __restrict__ G,
                                                         long long n, int C, int k, float t, float* __restrict__ out) {
  constexpr int RPW = HSK_WAVE / W;   // rows per wave
  const int lane = hsk_lane();
  const int c = lane & (W - 1);
  const long long row = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + lane / W;
  const bool live = row < n && c < C;
  const long long at = row * C + c;
  const float s = live ? S[at] : -INFINITY;
  const hsk_ecf_row r = hsk_ecf_forward<W>(s, live, lane, c, C, k, t);
  if (!BWD) {
    if (live) out[at] = r.sig * r.mh;
    return;
  }
  const float g = live ? G[at] : 0.f;
  const float h = g * r.sig;
  const float ph = hsk_seg_sum<W>(live ? r.p * h : 0.f);
  if (live) out[at] = g * r.dsig * r.mh + (1.f / t) * (r.p * (h - ph));
}

template <bool BWD>
static int hsk_ecf_launch(const char* name, const float* S, const float* G, int64_t n, int64_t C, int64_t k, double t,
                          float* out, hsk_stream_t stream_) {
  const float tf = (float)t;
  HSK_REQUIRE(C >= 1 && C <= HSK_ECF_MAX_CLUSTERS, HSK_ERR_INVALID, "%s: %lld clusters, 1..%d are served", name,
              (long long)C, HSK_ECF_MAX_CLUSTERS);
  HSK_REQUIRE(k >= 1 && k <= C, HSK_ERR_INVALID, "%s: top-k %lld outside [1, %lld]", name, (long long)k, (long long)C);
  HSK_REQUIRE(t > 0 && std::isfinite(t) && tf > 0.f && std::isfinite(tf), HSK_ERR_INVALID,
              "%s: the temperature must be positive and finite, got %g", name, t);
  HSK_REQUIRE(n >= 0 && n < INT_MAX, HSK_ERR_INVALID, "%s: bad row count %lld", name, (long long)n);
  if (n == 0) return HSK_OK;
  HSK_REQUIRE(S && out && (G || !BWD), HSK_ERR_INVALID, "%s: NULL pointer argument", name);
  hipStream_t stream = (hipStream_t)stream_;
  int W = 1;
  while (W < C) W <<= 1;
  const unsigned grid = (unsigned)hsk_ceil_div(n, 4 * (HSK_WAVE / W));
#define HSK_ECF_CASE(w)                                                                                       \
  case w:                                                                                                     \
    k_ecf_affiliation<w, BWD><<<grid, 256, 0, stream>>>(S, G, (long long)n, (int)C, (int)k, tf, out);         \
    break;
  switch (W) {
    HSK_ECF_CASE(1)
    HSK_ECF_CASE(2)
    HSK_ECF_CASE(4)
    HSK_ECF_CASE(8)
    HSK_ECF_CASE(16)
    HSK_ECF_CASE(32)
    HSK_ECF_CASE(64)
  }
#undef HSK_ECF_CASE
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}

extern "C" int hsk_ecf_affiliation(const float* S, int64_t n, int64_t C, int64_t k, double t, float* A,
                                   hsk_stream_t stream) {
  return hsk_ecf_launch<false>("hsk_ecf_affiliation", S, nullptr, n, C, k, t, A, stream);
}

extern "C" int hsk_ecf_affiliation_backward(const float* S, const float* G, int64_t n, int64_t C, int64_t k, double t,
                                            float* dS, hsk_stream_t stream) {
  return hsk_ecf_launch<true>("hsk_ecf_affiliation_backward", S, G, n, C, k, t, dS, stream);
}
