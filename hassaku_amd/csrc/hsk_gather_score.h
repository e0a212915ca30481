// hsk_gather_score.h -- the fp64 gather-sum scorer of the item x item models (hsk_ease_score_rows, hsk_p3_score_rows):
//   out[q, j] = ((0 + W[i1, j]) + W[i2, j]) + ...  over the items of user u = users[q] in stored (ascending) order,
// and with SCALED  out[q, j] = pow(inv_deg_u[u] * that sum, alpha).  One workgroup per (user, column window),
// HSK_GS_PER columns per thread and pass; the columns of the user's exclusion row come back as -inf; a user id outside
// [0, n_users) sets HSK_STATUS_BAD_INDEX and scores as user 0.
#pragma once
#include "hsk_common.h"

#include <limits.h>
#include <math.h>

#define HSK_GS_THREADS 256
#define HSK_GS_PER 4   // columns per thread and pass

template <bool SCALED>
__global__ void __launch_bounds__(HSK_GS_THREADS) k_gather_score(
    const int64_t* __restrict__ users, int64_t n_users, const int64_t* __restrict__ x_ptr,
    const int32_t* __restrict__ x_idx, const double* __restrict__ W, int64_t n_items, int64_t ldw,
    const double* __restrict__ inv_deg_u, double alpha, int64_t window, const int64_t* __restrict__ e_ptr,
    const int32_t* __restrict__ e_idx, double* __restrict__ out, int64_t ld, int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.y, w0 = (int64_t)blockIdx.x * window;
  const int64_t w1 = w0 + window < n_items ? w0 + window : n_items;
  int64_t u = users[q];
  if (u < 0 || u >= n_users) {
    if (tid == 0) atomicOr(status, HSK_STATUS_BAD_INDEX);
    u = 0;
  }
  const int64_t lo = x_ptr[u], hi = x_ptr[u + 1];
  const double wu = SCALED ? inv_deg_u[u] : 0.0;
  const bool plain = alpha == 1.0;
  for (int64_t c0 = w0; c0 < w1; c0 += HSK_GS_THREADS * HSK_GS_PER) {
    double acc[HSK_GS_PER];
    int64_t col[HSK_GS_PER];
#pragma unroll
    for (int s = 0; s < HSK_GS_PER; ++s) {
      acc[s] = 0.0;
      col[s] = c0 + s * HSK_GS_THREADS + tid;
    }
    for (int64_t e = lo; e < hi; ++e) {
      const int32_t i = x_idx[e];
      if (i < 0 || i >= n_items) continue;
      const double* row = W + (int64_t)i * ldw;
#pragma unroll
      for (int s = 0; s < HSK_GS_PER; ++s)
        if (col[s] < w1) acc[s] = acc[s] + row[col[s]];
    }
#pragma unroll
    for (int s = 0; s < HSK_GS_PER; ++s)
      if (col[s] < w1) {
        if (SCALED) {
          const double p = wu * acc[s];
          out[q * ld + col[s]] = plain ? p : (p == 0.0 ? 0.0 : pow(p, alpha));   // a zero sum gives +0.0
        } else {
          out[q * ld + col[s]] = acc[s];
        }
      }
  }
  if (e_ptr) {
    __syncthreads();   // the window's scores are written before its excluded columns are overwritten
    for (int64_t f = e_ptr[u] + tid; f < e_ptr[u + 1]; f += HSK_GS_THREADS) {
      const int64_t j = e_idx[f];
      if (j >= w0 && j < w1) out[q * ld + j] = -__builtin_inf();
    }
  }
}

// the checks, the window clamp and the launches of both entry points; `name` is the entry point's, for the messages
template <bool SCALED>
static int hsk_gather_score_rows(const char* name, const int64_t* users, int64_t n_rows, int64_t n_users,
                                 const int64_t* x_indptr, const int32_t* x_indices, const double* W, int64_t n_items,
                                 int64_t ldw, const double* inv_deg_u, double alpha, int64_t window,
                                 const int64_t* excl_indptr, const int32_t* excl_indices, double* out, int64_t ld,
                                 int32_t* status, hsk_stream_t stream) {
  HSK_REQUIRE(users && x_indptr && x_indices && W && (inv_deg_u || !SCALED) && out && status, HSK_ERR_INVALID,
              "%s: null pointer", name);
  HSK_REQUIRE((excl_indptr == nullptr) == (excl_indices == nullptr), HSK_ERR_INVALID,
              "%s: exclude CSR needs both arrays", name);
  HSK_REQUIRE(n_rows > 0 && n_users > 0 && n_items > 0 && n_items < INT_MAX && ldw >= n_items && ld >= n_items,
              HSK_ERR_INVALID, "%s: bad shape", name);
  HSK_REQUIRE(!SCALED || (alpha > 0.0 && alpha < __builtin_inf()), HSK_ERR_INVALID, "%s: alpha %g is not in (0, inf)",
              name, alpha);
  HSK_REQUIRE(window >= 1, HSK_ERR_INVALID, "%s: window %lld < 1", name, (long long)window);
  const int64_t wlen = window < n_items ? window : n_items;
  const int64_t nw = hsk_ceil_div(n_items, wlen);
  HSK_REQUIRE(nw < (1ll << 31), HSK_ERR_INVALID, "%s: too many windows", name);
  for (int64_t at = 0; at < n_rows; at += 65535) {   // grid.y limit
    const int64_t part = n_rows - at < 65535 ? n_rows - at : 65535;
    k_gather_score<SCALED><<<dim3((unsigned)nw, (unsigned)part), HSK_GS_THREADS, 0, (hipStream_t)stream>>>(
        users + at, n_users, x_indptr, x_indices, W, n_items, ldw, inv_deg_u, alpha, wlen, excl_indptr, excl_indices,
        out + at * ld, ld, status);
    HSK_LAUNCH_CHECK();
  }
  return HSK_OK;
}
