// hsk_calib.hip -- calibration metrics of a ranked list (reference eval/eval.py:121-208, eval/metrics.py:108-152):
// how far the bin distribution of the top-k items (tags, popularity buckets) is from the one of the user's train
// history -- Hellinger distance, Jensen-Shannon distance, KL divergence -- at several cut-offs from one pass over
// the list.  DESIGN.md section 5.7.
//
// One wave per row, four rows per 256-thread block (as k_rank_metrics).  The row's ids are staged once in LDS; lanes
// stride over bins, so the wave reads an item's row as consecutive elements.  Each lane keeps the running fp64 sum of
// its bin over the ranks, in rank order; at every cut-off it takes a snapshot q = beta p + (1 - beta) sum / k and adds
// its bin's terms of the three distances to per-cut-off partial sums, which hsk_wave_sum_f64 combines at the end.
// Nothing is guarded: log 0, 0 * inf and a NaN user row give what IEEE arithmetic gives the reference.
#include "hsk_common.h"

#include <limits.h>

#define CALIB_ROWS 4   // rows (waves) per block

// the distinct cut-offs in ascending order: the rank loop runs from one to the next
struct calib_cuts {
  int at[HSK_MAX_KS];
  int n;
};

template <typename T>
__global__ __launch_bounds__(256) void k_calibration_metrics(const int32_t* __restrict__ topk, int n_rows, int k_max,
                                                             const int64_t* __restrict__ u_idx,
                                                             const T* __restrict__ item_mtx, int n_items, int n_bins,
                                                             long long item_ld, const double* __restrict__ user_mtx,
                                                             long long n_users, long long user_ld, double beta,
                                                             hsk_ks ks, calib_cuts cuts, double* __restrict__ out,
                                                             int32_t* __restrict__ status) {
  __shared__ int32_t s_ids[CALIB_ROWS][HSK_KNN_MAX_K];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int r = blockIdx.x * CALIB_ROWS + w;
  const bool live = r < n_rows;
  const int k_used = cuts.at[cuts.n - 1];   // ranks past the largest cut-off are never read
  if (live)
    for (int c = lane; c < k_used; c += 64) s_ids[w][c] = topk[(long long)r * k_max + c];
  __syncthreads();
  if (!live) return;
  long long u = u_idx[r];
  if (u < 0 || u >= n_users) {
    if (lane == 0 && status) atomicOr(status, HSK_STATUS_BAD_INDEX);
    u = 0;
  }
  const double* __restrict__ p_row = user_mtx + u * user_ld;
  const double one_m_beta = 1.0 - beta;
  // per-lane partial sums per cut-off: sum (sqrt p - sqrt q)^2, KL(p|q), KL(p|m), KL(q|m)
  double hel[HSK_MAX_KS], kl[HSK_MAX_KS], jp[HSK_MAX_KS], jq[HSK_MAX_KS];
#pragma unroll
  for (int t = 0; t < HSK_MAX_KS; ++t) hel[t] = kl[t] = jp[t] = jq[t] = 0.0;
  for (int b = lane; b < n_bins; b += 64) {
    const double p = p_row[b];
    const double sp = sqrt(p), lp = log(p);
    const T* __restrict__ col = item_mtx + b;
    double acc = 0.0;
    int rank = 0;
    for (int c = 0; c < cuts.n; ++c) {
      const int k = cuts.at[c];
#pragma unroll 4
      for (; rank < k; ++rank) {
        const int id = s_ids[w][rank];
        // an id outside the catalogue (hsk_topk_merge pads with 0x7fffffff) is a zero row and is never dereferenced
        if ((unsigned)id < (unsigned)n_items) acc += (double)col[(long long)id * item_ld];
      }
      // eval/eval.py:181-186 -- mean over the k rows, then the smoothing; no contraction into an fma, as there
      const double q = __dadd_rn(__dmul_rn(beta, p), __dmul_rn(one_m_beta, acc / (double)k));
      const double lq = log(q);
      const double m = 0.5 * (p + q);
      const double lm = log(m);
      const double d = sp - sqrt(q);
      const double hv = d * d;
      const double kv = __dmul_rn(p, lp - lq);
      const double pv = __dmul_rn(p, lp - lm);
      const double qv = __dmul_rn(q, lq - lm);
#pragma unroll
      for (int t = 0; t < HSK_MAX_KS; ++t) {
        if (t < ks.n && ks.k[t] == k) {
          hel[t] += hv;
          kl[t] += kv;
          jp[t] += pv;
          jq[t] += qv;
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < HSK_MAX_KS; ++t) {
    if (t < ks.n) {
      const double h_ = hsk_wave_sum_f64(hel[t]);
      const double k_ = hsk_wave_sum_f64(kl[t]);
      const double p_ = hsk_wave_sum_f64(jp[t]);
      const double q_ = hsk_wave_sum_f64(jq[t]);
      if (lane == 0) {
        double* o = out + ((long long)r * ks.n + t) * 3;
        o[0] = sqrt(0.5 * h_);
        o[1] = sqrt(0.5 * (p_ + q_));
        o[2] = k_;
      }
    }
  }
}

extern "C" int hsk_calibration_metrics(const int32_t* topk_idx, int64_t n_rows, int64_t k_max, const int64_t* u_idx,
                                       const void* item_mtx, int32_t item_is_f64, int64_t n_items, int64_t n_bins,
                                       int64_t item_ld, const double* user_mtx, int64_t n_users, int64_t user_ld,
                                       double beta, const int32_t* ks, int32_t n_ks, double* out, int32_t* status,
                                       hsk_stream_t stream_) {
  HSK_REQUIRE(topk_idx && u_idx && item_mtx && user_mtx && ks && out, HSK_ERR_INVALID,
              "hsk_calibration_metrics: null pointer");
  HSK_REQUIRE(item_is_f64 == 0 || item_is_f64 == 1, HSK_ERR_INVALID, "hsk_calibration_metrics: item_is_f64 = %d",
              item_is_f64);
  HSK_REQUIRE(n_ks >= 1 && n_ks <= HSK_MAX_KS, HSK_ERR_UNSUPPORTED, "hsk_calibration_metrics: n_ks %d outside [1, %d]",
              n_ks, HSK_MAX_KS);
  HSK_REQUIRE(k_max >= 1 && k_max <= HSK_KNN_MAX_K, HSK_ERR_UNSUPPORTED,
              "hsk_calibration_metrics: k_max = %lld outside [1, %d]", (long long)k_max, HSK_KNN_MAX_K);
  HSK_REQUIRE(n_rows >= 0 && n_rows < INT_MAX && n_items > 0 && n_items < INT_MAX && n_bins > 0 && n_bins < INT_MAX &&
                  item_ld >= n_bins && n_users > 0 && user_ld >= n_bins,
              HSK_ERR_INVALID, "hsk_calibration_metrics: bad shape rows %lld items %lld bins %lld ld %lld users %lld ld %lld",
              (long long)n_rows, (long long)n_items, (long long)n_bins, (long long)item_ld, (long long)n_users,
              (long long)user_ld);
  HSK_REQUIRE(beta >= 0.0 && beta <= 1.0, HSK_ERR_INVALID, "hsk_calibration_metrics: beta %g outside [0, 1]", beta);
  hsk_ks kk;
  calib_cuts cuts;
  kk.n = n_ks;
  cuts.n = 0;
  for (int t = 0; t < HSK_MAX_KS; ++t) kk.k[t] = cuts.at[t] = 0;
  for (int t = 0; t < n_ks; ++t) {
    HSK_REQUIRE(ks[t] >= 1 && ks[t] <= k_max, HSK_ERR_INVALID, "hsk_calibration_metrics: ks[%d]=%d outside [1, k_max=%lld]",
                t, ks[t], (long long)k_max);
    kk.k[t] = ks[t];
    int pos = 0;   // insert into the ascending list of distinct cut-offs
    while (pos < cuts.n && cuts.at[pos] < ks[t]) ++pos;
    if (pos < cuts.n && cuts.at[pos] == ks[t]) continue;
    for (int j = cuts.n; j > pos; --j) cuts.at[j] = cuts.at[j - 1];
    cuts.at[pos] = ks[t];
    ++cuts.n;
  }
  if (n_rows == 0) return HSK_OK;
  const unsigned grid = (unsigned)hsk_ceil_div(n_rows, CALIB_ROWS);
  hipStream_t stream = (hipStream_t)stream_;
  if (item_is_f64)
    k_calibration_metrics<double><<<grid, 256, 0, stream>>>(topk_idx, (int)n_rows, (int)k_max, u_idx,
                                                            (const double*)item_mtx, (int)n_items, (int)n_bins, item_ld,
                                                            user_mtx, n_users, user_ld, beta, kk, cuts, out, status);
  else
    k_calibration_metrics<float><<<grid, 256, 0, stream>>>(topk_idx, (int)n_rows, (int)k_max, u_idx,
                                                           (const float*)item_mtx, (int)n_items, (int)n_bins, item_ld,
                                                           user_mtx, n_users, user_ld, beta, kk, cuts, out, status);
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}
