// hsk_dmf.hip -- the sparse first layer of DeepMatrixFactorization (algorithms/sgd_alg.py:778-880 of the reference).
//
// The reference feeds a dense 0/1 row of the train matrix to the first nn.Linear of each tower.  A 0/1 row times the
// weight is the sum of the weight's columns named by the row's stored entries, so with the weight kept transposed,
// Wt [n_in, dim] row-major, the product is a gather-sum of contiguous rows:
//   forward   out[j, :]     = ((0 + Wt[c1, :]) + Wt[c2, :]) + ...   over the entries c of CSR row idx[j], stored order
//   backward  grad_Wt[c, :] = ((0 + g[j1, :]) + g[j2, :]) + ...     over the batch positions j whose row holds c,
//                                                                     ascending j (a duplicated row id counts each time)
// One wavefront owns one output row in both directions (hsk_rows.h tiles, hsk_dispatch_dim), with R row loads in
// flight.  The backward expands the batch's entries into (column, batch position) pairs in position order, groups them
// by column with the stable key sort (hsk_keysort.h: inside a column the pairs keep ascending position)
// and sums g rows through the pair list -- no gradient row per pair is materialised and no float atomic is used, so two
// calls give the same bits.
#include "hsk_rows.h"
#include "hsk_keysort.h"

#include <limits.h>

template <int V, int NCH>
struct hsk_dmf_inflight {   // row loads in flight per wave: 4, or 2 for the widest tiles (registers)
  static constexpr int R = (V * NCH >= 16) ? 2 : 4;
};

template <int V, int NCH, bool FULL>
__global__ __launch_bounds__(256) void k_sparse_rows_sum(const float* __restrict__ Wt, int n_in, int D,
                                                         const int64_t* __restrict__ indptr,
                                                         const int32_t* __restrict__ indices, int n_rows_csr,
                                                         const int64_t* __restrict__ idx, int n, float* __restrict__ out,
                                                         int32_t* status) {
  constexpr int R = hsk_dmf_inflight<V, NCH>::R;
  const int lane = hsk_lane();
  const int j = blockIdx.x * 4 + hsk_uniform_i(threadIdx.x >> 6);
  if (j >= n) return;
  using Row = hsk_row<V, NCH>;
  const int r = hsk_uniform_i(hsk_clamp_index(idx[j], n_rows_csr, status));
  const long long beg = indptr[r], end = indptr[r + 1];
  Row acc;
  hsk_row_zero(acc);
  for (long long c0 = beg; c0 < end; c0 += 64) {
    const int nr = (int)min((long long)64, end - c0);
    int myc = -1;   // -1: a column id outside [0, n_in), skipped
    if (lane < nr) {
      const int c = indices[c0 + lane];
      myc = (c >= 0 && c < n_in) ? c : -1;
    }
    for (int k = 0; k < nr; k += R) {
      Row buf[R];
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const int c = hsk_readlane_i(myc, min(k + q, 63));
        if (k + q < nr && c >= 0) hsk_row_load<V, NCH, FULL>(buf[q], Wt + (long long)c * D, lane, D);
      }
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const int c = hsk_readlane_i(myc, min(k + q, 63));
        if (k + q < nr && c >= 0) hsk_row_add(acc, buf[q]);
      }
    }
  }
  hsk_row_store<V, NCH, FULL>(acc, out + (long long)j * D, lane, D);
}

// pair_off[j] = number of stored entries of the CSR rows named by idx[0..j), pair_off[n] = the batch's entry count.
// One workgroup walks the batch 1024 positions at a time with a running carry.
__global__ __launch_bounds__(1024) void k_sparse_rows_offsets(const int64_t* __restrict__ indptr, int n_rows_csr,
                                                              const int64_t* __restrict__ idx, int n,
                                                              int64_t* __restrict__ pair_off, int32_t* status) {
  __shared__ long long wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  long long carry = 0;
  for (int base = 0; base < n; base += 1024) {
    const int j = base + tid;
    long long len = 0;
    if (j < n) {
      const int r = hsk_clamp_index(idx[j], n_rows_csr, status);
      len = indptr[r + 1] - indptr[r];
      if (len < 0) len = 0;
    }
    long long incl = len;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const long long t = __shfl_up(incl, off, 64);
      if (lane >= off) incl += t;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    long long wbase = 0, tot = 0;
    for (int ww = 0; ww < 16; ++ww) {
      if (ww < w) wbase += wsum[ww];
      tot += wsum[ww];
    }
    if (j < n) pair_off[j] = carry + wbase + incl - len;
    carry += tot;
    __syncthreads();
  }
  if (tid == 0) pair_off[n] = carry;
}

// pairs of batch position j, in position order: key[p] = column, prow[p] = j for p in [pair_off[j], pair_off[j + 1]).
// An out-of-range column id keeps its slot with key 0 and prow -1 (the segment sum skips it); so do the slots in
// [pair_off[n], n_pairs) if the caller's n_pairs is larger than the batch's entry count, and a slot at or past n_pairs
// is never written.
__global__ __launch_bounds__(256) void k_sparse_rows_expand(const int64_t* __restrict__ indptr,
                                                            const int32_t* __restrict__ indices, int n_rows_csr,
                                                            int n_in, const int64_t* __restrict__ idx, int n,
                                                            const int64_t* __restrict__ pair_off, int n_pairs,
                                                            int* __restrict__ key, int* __restrict__ prow,
                                                            int32_t* status) {
  const int lane = hsk_lane();
  const int j = blockIdx.x * 4 + hsk_uniform_i(threadIdx.x >> 6);
  if (j >= n) return;
  const int r = hsk_uniform_i(hsk_clamp_index(idx[j], n_rows_csr, status));
  const long long beg = indptr[r], len = indptr[r + 1] - beg, p0 = pair_off[j];
  for (long long e = lane; e < len; e += 64) {
    const long long p = p0 + e;
    if (p < 0 || p >= n_pairs) break;
    const int c = indices[beg + e];
    const bool ok = c >= 0 && c < n_in;
    key[p] = ok ? c : 0;
    prow[p] = ok ? j : -1;
  }
  if (j == n - 1) {
    long long t0 = pair_off[n];
    if (t0 < 0) t0 = 0;
    for (long long p = t0 + lane; p < n_pairs; p += 64) {
      key[p] = 0;
      prow[p] = -1;
    }
  }
}

template <int V, int NCH, bool FULL>
__global__ __launch_bounds__(256) void k_sparse_rows_segment_sum(const float* __restrict__ g, int n,
                                                                 const int* __restrict__ prow,
                                                                 const int* __restrict__ perm,
                                                                 const int* __restrict__ offsets, int n_in, int D,
                                                                 float* __restrict__ grad_Wt) {
  constexpr int R = hsk_dmf_inflight<V, NCH>::R;
  const int lane = hsk_lane();
  const int c = blockIdx.x * 4 + hsk_uniform_i(threadIdx.x >> 6);
  if (c >= n_in) return;
  using Row = hsk_row<V, NCH>;
  const int beg = hsk_uniform_i(offsets[c]), end = hsk_uniform_i(offsets[c + 1]);
  Row acc;
  hsk_row_zero(acc);
  for (int c0 = beg; c0 < end; c0 += 64) {
    const int nr = min(64, end - c0);
    int myj = -1;
    if (lane < nr) {
      myj = prow[perm[c0 + lane]];
      if (myj >= n) myj = -1;
    }
    for (int k = 0; k < nr; k += R) {
      Row buf[R];
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const int j = hsk_readlane_i(myj, min(k + q, 63));
        if (k + q < nr && j >= 0) hsk_row_load<V, NCH, FULL>(buf[q], g + (long long)j * D, lane, D);
      }
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const int j = hsk_readlane_i(myj, min(k + q, 63));
        if (k + q < nr && j >= 0) hsk_row_add(acc, buf[q]);
      }
    }
  }
  hsk_row_store<V, NCH, FULL>(acc, grad_Wt + (long long)c * D, lane, D);
}

// n == 0 is a no-op: idx (and the per-position buffers of the callers) may then be NULL
static int hsk_sparse_rows_check(const char* name, const int64_t* indptr, const int32_t* indices, int64_t n_rows_csr,
                                 int64_t n_in, const int64_t* idx, int64_t n, int64_t dim) {
  HSK_REQUIRE(indptr && indices && (idx || n == 0), HSK_ERR_INVALID, "%s: NULL pointer argument", name);
  HSK_REQUIRE(n_rows_csr > 0 && n_rows_csr < INT_MAX && n_in > 0 && n_in < INT_MAX && dim > 0 && n >= 0 && n < INT_MAX,
              HSK_ERR_INVALID, "%s: bad sizes", name);
  return HSK_OK;
}

extern "C" int hsk_sparse_rows_sum(const float* Wt, int64_t n_in, int64_t dim, const int64_t* indptr,
                                   const int32_t* indices, int64_t n_rows_csr, const int64_t* idx, int64_t n, float* out,
                                   int32_t* status, hsk_stream_t stream_) {
  HSK_REQUIRE(Wt && (out || n == 0), HSK_ERR_INVALID, "hsk_sparse_rows_sum: NULL pointer argument");
  int rc = hsk_sparse_rows_check("hsk_sparse_rows_sum", indptr, indices, n_rows_csr, n_in, idx, n, dim);
  if (rc) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  rc = hsk_dispatch_dim(dim, [&](auto v_, auto n_, auto f_) -> int {
    constexpr int V = decltype(v_)::value;
    constexpr int NCH = decltype(n_)::value;
    constexpr bool FULL = decltype(f_)::value;
    HSK_REQUIRE((((uintptr_t)Wt | (uintptr_t)out) & (uintptr_t)(4 * V - 1)) == 0, HSK_ERR_INVALID,
                "hsk_sparse_rows_sum: Wt and out must be %d-byte aligned", 4 * V);
    if (n == 0) return (int)HSK_OK;
    k_sparse_rows_sum<V, NCH, FULL><<<(unsigned)hsk_ceil_div(n, 4), 256, 0, stream>>>(
        Wt, (int)n_in, (int)dim, indptr, indices, (int)n_rows_csr, idx, (int)n, out, status);
    return (int)HSK_OK;
  });
  if (rc) return rc;
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}

extern "C" int hsk_sparse_rows_offsets(const int64_t* indptr, int64_t n_rows_csr, const int64_t* idx, int64_t n,
                                       int64_t* pair_off, int32_t* status, hsk_stream_t stream_) {
  HSK_REQUIRE(indptr && (idx || n == 0) && pair_off, HSK_ERR_INVALID, "hsk_sparse_rows_offsets: NULL pointer argument");
  HSK_REQUIRE(n_rows_csr > 0 && n_rows_csr < INT_MAX && n >= 0 && n < INT_MAX, HSK_ERR_INVALID,
              "hsk_sparse_rows_offsets: bad sizes");
  k_sparse_rows_offsets<<<1, 1024, 0, (hipStream_t)stream_>>>(indptr, (int)n_rows_csr, idx, (int)n, pair_off, status);
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}

struct hsk_dmfw {   // scratch of hsk_sparse_rows_sum_backward: the pairs' batch positions, then the key sort's
  int* prow;
  hsk_keysort sort;
  int64_t total;
};

static hsk_dmfw hsk_dmfw_carve(void* base, int64_t n_in, int64_t n_pairs) {
  hsk_dmfw w;
  const int64_t head = hsk_align_up(n_pairs * 4, 256);
  w.prow = (int*)base;
  w.sort = hsk_keysort_carve(base ? (char*)base + head : nullptr, n_in, n_pairs);
  w.total = head + w.sort.total;
  return w;
}

extern "C" int64_t hsk_sparse_rows_sum_backward_ws_bytes(int64_t n_in, int64_t n_pairs) {
  if (n_in <= 0 || n_in >= INT_MAX || n_pairs < 0 || n_pairs >= INT_MAX) return -1;
  if (n_pairs == 0) return 256;
  if (!hsk_keysort_supported(n_in, n_pairs)) return -1;
  return hsk_dmfw_carve(nullptr, n_in, n_pairs).total;
}

extern "C" int hsk_sparse_rows_sum_backward(const float* g, const int64_t* indptr, const int32_t* indices,
                                            int64_t n_rows_csr, int64_t n_in, const int64_t* idx, int64_t n,
                                            const int64_t* pair_off, int64_t n_pairs, int64_t dim, float* grad_Wt,
                                            void* ws, int64_t ws_bytes, int32_t* status, hsk_stream_t stream_) {
  HSK_REQUIRE(grad_Wt, HSK_ERR_INVALID, "hsk_sparse_rows_sum_backward: NULL pointer argument");
  int rc = hsk_sparse_rows_check("hsk_sparse_rows_sum_backward", indptr, indices, n_rows_csr, n_in, idx, n, dim);
  if (rc) return rc;
  HSK_REQUIRE(n_pairs >= 0 && n_pairs < INT_MAX, HSK_ERR_INVALID, "hsk_sparse_rows_sum_backward: bad n_pairs %lld",
              (long long)n_pairs);
  hipStream_t stream = (hipStream_t)stream_;
  if (n == 0 || n_pairs == 0) {   // nobody touches a row: the dispatch still says whether the width is served
    rc = hsk_dispatch_dim(dim, [&](auto, auto, auto) -> int { return HSK_OK; });
    if (rc) return rc;
    HSK_HIP(hipMemsetAsync(grad_Wt, 0, (size_t)n_in * dim * 4, stream));
    return HSK_OK;
  }
  HSK_REQUIRE(g && pair_off && ws, HSK_ERR_INVALID, "hsk_sparse_rows_sum_backward: NULL pointer argument");
  const int64_t need = hsk_sparse_rows_sum_backward_ws_bytes(n_in, n_pairs);
  HSK_REQUIRE(need > 0, HSK_ERR_UNSUPPORTED, "hsk_sparse_rows_sum_backward: %lld columns too many for the key sort",
              (long long)n_in);
  HSK_REQUIRE(ws_bytes >= need && ((uintptr_t)ws & 255) == 0, HSK_ERR_INVALID,
              "hsk_sparse_rows_sum_backward workspace: %lld bytes needed, %lld given", (long long)need,
              (long long)ws_bytes);
  const hsk_dmfw w = hsk_dmfw_carve(ws, n_in, n_pairs);
  rc = hsk_dispatch_dim(dim, [&](auto v_, auto n_, auto f_) -> int {
    constexpr int V = decltype(v_)::value;
    constexpr int NCH = decltype(n_)::value;
    constexpr bool FULL = decltype(f_)::value;
    HSK_REQUIRE((((uintptr_t)g | (uintptr_t)grad_Wt) & (uintptr_t)(4 * V - 1)) == 0, HSK_ERR_INVALID,
                "hsk_sparse_rows_sum_backward: g and grad_Wt must be %d-byte aligned", 4 * V);
    k_sparse_rows_expand<<<(unsigned)hsk_ceil_div(n, 4), 256, 0, stream>>>(indptr, indices, (int)n_rows_csr, (int)n_in,
                                                                            idx, (int)n, pair_off, (int)n_pairs,
                                                                            w.sort.it32, w.prow, status);
    if (hipGetLastError() != hipSuccess) {
      hsk_set_error("hsk_sparse_rows_sum_backward: kernel launch failed");
      return (int)HSK_ERR_HIP;
    }
    int src = hsk_keysort_run(w.sort, n_in, n_pairs, stream);
    if (src) return src;
    k_sparse_rows_segment_sum<V, NCH, FULL><<<(unsigned)hsk_ceil_div(n_in, 4), 256, 0, stream>>>(
        g, (int)n, w.prow, w.sort.perm, w.sort.offsets, (int)n_in, (int)dim, grad_Wt);
    return (int)HSK_OK;
  });
  if (rc) return rc;
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}
