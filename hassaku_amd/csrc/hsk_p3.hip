// hsk_p3.hip -- P3alpha (reference algorithms/graph_algs.py:9-88): the reciprocal degrees, the weighted fp64 Gram
// S = X^T diag(w_u) X on v_mfma_f64_16x16x4_f64 straight from the int8 image of X^T, and the fp64 gather-sum scorer
// with the element-wise power.  DESIGN.md section 5.3.
//
// Gram geometry: a workgroup of four waves owns 128 x 128 outputs, wave (wm, wn) the 64 x 64 block at (64 wm, 64 wn) in
// 4 x 4 accumulator tiles of 16 x 16 (operand and C/D maps as in k_ease_update).  The k loop walks k_pad in blocks of
// P3_BK = 64 users.  Both operands are rows of the same item-major int8 matrix M; a block's two [128 items][64 B] tiles
// are loaded 16 bytes per lane (as knn_gload does) one block ahead of the MFMAs, and are converted to fp64 once, when
// they are written to LDS as k-major [64][128 + 16 pad] images -- the B side multiplied by col_weight there, which is
// exact (the product is 0 or w_u).  Row tile and column tile walk k in the same order and every product is w_u or 0 on
// both sides of the diagonal, so the unscaled result is bitwise symmetric.
#include "hsk_common.h"

#include <limits.h>
#include <math.h>

#define P3_TILE 128
#define P3_BK 64
#define P3_LDS_ROW 144                          // 128 doubles + 16 pad: rows k and k + 1 start 32 banks apart
#define P3_IMAGE (P3_BK * P3_LDS_ROW)           // doubles of one operand image: 73 728 bytes, two of them 147 456
#define P3_SCORE_THREADS 256
#define P3_SCORE_PER 4                          // columns per thread and pass of the scorer

typedef double hsk_p_f64x4 __attribute__((ext_vector_type(4)));
typedef double hsk_p_f64x2 __attribute__((ext_vector_type(2)));
typedef int hsk_p_i32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------
// w[i] = 1 / degree(i), 0 for degree 0 and for the padding i in [n, n_out)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_p3_inv_degrees(const int64_t* __restrict__ indptr, int64_t n, int64_t n_out,
                                                        double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_out) return;
  const int64_t d = i < n ? indptr[i + 1] - indptr[i] : 0;
  out[i] = d > 0 ? 1.0 / (double)d : 0.0;
}

// ---------------------------------------------------------------------------------------------
// Gram: out[i, j] = row_scale[i] * sum_u M[i, u] col_weight[u] M[j, u] for i in [r0, r1), j in [0, n)
// ---------------------------------------------------------------------------------------------
struct p3_stage {
  hsk_p_i32x4 a[2], b[2];
  hsk_p_f64x2 w[8];   // col_weight of this lane's 16 k of the block
};

__device__ __forceinline__ void p3_gload(p3_stage& s, const int8_t* __restrict__ M, const double* __restrict__ cw,
                                         int64_t k_pad, int64_t m0, int64_t n0, int kt, int tid) {
  const int64_t k0 = (int64_t)kt * P3_BK + (tid & 3) * 16;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int row = (tid + 256 * q) >> 2;
    s.a[q] = *reinterpret_cast<const hsk_p_i32x4*>(M + (m0 + row) * k_pad + k0);
    s.b[q] = *reinterpret_cast<const hsk_p_i32x4*>(M + (n0 + row) * k_pad + k0);
  }
#pragma unroll
  for (int t = 0; t < 8; ++t) s.w[t] = *reinterpret_cast<const hsk_p_f64x2*>(cw + k0 + 2 * t);
}

// int8 -> fp64 once, on the way into the k-major images: sa[k][item] = M[m0 + item, k], sb[k][item] = w_k M[n0 + item, k]
__device__ __forceinline__ void p3_sstore(const p3_stage& s, double* __restrict__ sa, double* __restrict__ sb, int tid) {
#pragma clang fp contract(off)
  const int kc = (tid & 3) * 16;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int row = (tid + 256 * q) >> 2;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const double a = (double)(int8_t)((s.a[q][t >> 2] >> (8 * (t & 3))) & 0xff);
      const double b = (double)(int8_t)((s.b[q][t >> 2] >> (8 * (t & 3))) & 0xff);
      sa[(kc + t) * P3_LDS_ROW + row] = a;
      sb[(kc + t) * P3_LDS_ROW + row] = b * s.w[t >> 1][t & 1];
    }
  }
}

__global__ void __launch_bounds__(256) k_p3_gram(const int8_t* __restrict__ M, int64_t n, int64_t k_pad,
                                                 const double* __restrict__ col_weight,
                                                 const double* __restrict__ row_scale, int64_t r0, int64_t r1,
                                                 double* __restrict__ out, int64_t ld) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* sa = lds;              // rows m0 .. m0 + 128 of M, k-major
  double* sb = lds + P3_IMAGE;   // rows n0 .. n0 + 128 of M times col_weight, k-major
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lc = lane & 15, lq = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t m0 = r0 + (int64_t)blockIdx.y * P3_TILE, n0 = (int64_t)blockIdx.x * P3_TILE;
  const int NK = (int)(k_pad / P3_BK);
  hsk_p_f64x4 acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj)
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[mi][nj][v] = 0.0;
  p3_stage s;
  p3_gload(s, M, col_weight, k_pad, m0, n0, 0, tid);
  p3_sstore(s, sa, sb, tid);
  __syncthreads();
  for (int kt = 0; kt < NK; ++kt) {
    const bool more = kt + 1 < NK;
    if (more) p3_gload(s, M, col_weight, k_pad, m0, n0, kt + 1, tid);   // in flight under this block's MFMAs
    // A operand: lane holds A[row = lane & 15][k = lane >> 4]; B operand: B[k = lane >> 4][col = lane & 15]
#pragma unroll 4
    for (int ks = 0; ks < P3_BK / 4; ++ks) {
      double af[4], bf[4];
      const int k = ks * 4 + lq;
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) af[mi] = sa[k * P3_LDS_ROW + wm * 64 + mi * 16 + lc];
#pragma unroll
      for (int nj = 0; nj < 4; ++nj) bf[nj] = sb[k * P3_LDS_ROW + wn * 64 + nj * 16 + lc];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int nj = 0; nj < 4; ++nj)
          acc[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[mi], bf[nj], acc[mi][nj], 0, 0, 0);
    }
    __syncthreads();   // every wave has read this block's images
    if (more) {
      p3_sstore(s, sa, sb, tid);
      __syncthreads();
    }
  }
  // f64 16x16x4 C/D map: column = lane & 15, row = (lane >> 4) + 4 v
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int64_t gi = m0 + wm * 64 + mi * 16 + lq + 4 * v;
      if (gi >= r1) continue;
      const double sc = row_scale ? row_scale[gi] : 1.0;
#pragma unroll
      for (int nj = 0; nj < 4; ++nj) {
        const int64_t gj = n0 + wn * 64 + nj * 16 + lc;
        if (gj < n) out[gi * ld + gj] = row_scale ? sc * acc[mi][nj][v] : acc[mi][nj][v];
      }
    }
}

// ---------------------------------------------------------------------------------------------
// scoring: out[q, j] = pow(inv_deg_u[u] * (((0 + W[i1, j]) + W[i2, j]) + ...), alpha) over the items of user
// u = users[q] in stored (ascending) order; loop, windows, exclusion and status as in k_ease_score
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(P3_SCORE_THREADS) k_p3_score(
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
  const double wu = inv_deg_u[u];
  const bool plain = alpha == 1.0;
  for (int64_t c0 = w0; c0 < w1; c0 += P3_SCORE_THREADS * P3_SCORE_PER) {
    double acc[P3_SCORE_PER];
    int64_t col[P3_SCORE_PER];
#pragma unroll
    for (int s = 0; s < P3_SCORE_PER; ++s) {
      acc[s] = 0.0;
      col[s] = c0 + s * P3_SCORE_THREADS + tid;
    }
    for (int64_t e = lo; e < hi; ++e) {
      const int32_t i = x_idx[e];
      if (i < 0 || i >= n_items) continue;
      const double* row = W + (int64_t)i * ldw;
#pragma unroll
      for (int s = 0; s < P3_SCORE_PER; ++s)
        if (col[s] < w1) acc[s] = acc[s] + row[col[s]];
    }
#pragma unroll
    for (int s = 0; s < P3_SCORE_PER; ++s)
      if (col[s] < w1) {
        const double p = wu * acc[s];
        out[q * ld + col[s]] = plain ? p : (p == 0.0 ? 0.0 : pow(p, alpha));   // a zero sum gives +0.0
      }
  }
  if (e_ptr) {
    __syncthreads();   // the window's scores are written before its excluded columns are overwritten
    for (int64_t f = e_ptr[u] + tid; f < e_ptr[u + 1]; f += P3_SCORE_THREADS) {
      const int64_t j = e_idx[f];
      if (j >= w0 && j < w1) out[q * ld + j] = -__builtin_inf();
    }
  }
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" int hsk_p3_inv_degrees(const int64_t* indptr, int64_t n, double* out, int64_t n_out, hsk_stream_t stream) {
  HSK_REQUIRE(indptr && out, HSK_ERR_INVALID, "hsk_p3_inv_degrees: null pointer");
  HSK_REQUIRE(n > 0 && n_out >= n && n_out < INT_MAX, HSK_ERR_INVALID, "hsk_p3_inv_degrees: bad shape n %lld n_out %lld",
              (long long)n, (long long)n_out);
  k_p3_inv_degrees<<<(unsigned)hsk_ceil_div(n_out, 256), 256, 0, (hipStream_t)stream>>>(indptr, n, n_out, out);
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}

extern "C" int hsk_p3_gram_f64(const int8_t* M, int64_t n, int64_t rows_pad, int64_t k_pad, const double* col_weight,
                               const double* row_scale, int64_t r0, int64_t r1, double* out, int64_t ld,
                               hsk_stream_t stream) {
  HSK_REQUIRE(M && col_weight && out, HSK_ERR_INVALID, "hsk_p3_gram_f64: null pointer");
  HSK_REQUIRE(n > 0 && n < INT_MAX && rows_pad >= n && rows_pad % P3_TILE == 0 && k_pad > 0 && k_pad % P3_BK == 0 &&
                  k_pad < INT_MAX,
              HSK_ERR_INVALID, "hsk_p3_gram_f64: bad operand shape (n %lld, rows_pad %lld, k_pad %lld)", (long long)n,
              (long long)rows_pad, (long long)k_pad);
  HSK_REQUIRE(r0 >= 0 && r0 % P3_TILE == 0 && r1 > r0 && r1 <= n && ld >= n, HSK_ERR_INVALID,
              "hsk_p3_gram_f64: bad row block [%lld, %lld) (r0 must be a multiple of %d) or ld %lld", (long long)r0,
              (long long)r1, P3_TILE, (long long)ld);
  HSK_REQUIRE(((uintptr_t)M & 15) == 0 && ((uintptr_t)col_weight & 15) == 0, HSK_ERR_INVALID,
              "hsk_p3_gram_f64: M and col_weight must be 16-byte aligned");
  const int lds_bytes = 2 * P3_IMAGE * (int)sizeof(double);
  HSK_HIP(hipFuncSetAttribute((const void*)k_p3_gram, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
  const int64_t gy = hsk_ceil_div(r1 - r0, P3_TILE);
  HSK_REQUIRE(gy <= 65535, HSK_ERR_INVALID, "hsk_p3_gram_f64: row block of %lld rows is too tall (at most %d)",
              (long long)(r1 - r0), 65535 * P3_TILE);
  const dim3 grid((unsigned)hsk_ceil_div(n, P3_TILE), (unsigned)gy);
  k_p3_gram<<<grid, 256, lds_bytes, (hipStream_t)stream>>>(M, n, k_pad, col_weight, row_scale, r0, r1, out, ld);
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}

extern "C" int hsk_p3_score_rows(const int64_t* users, int64_t n_rows, int64_t n_users, const int64_t* x_indptr,
                                 const int32_t* x_indices, const double* W, int64_t n_items, int64_t ldw,
                                 const double* inv_deg_u, double alpha, int64_t window, const int64_t* excl_indptr,
                                 const int32_t* excl_indices, double* out, int64_t ld, int32_t* status,
                                 hsk_stream_t stream) {
  HSK_REQUIRE(users && x_indptr && x_indices && W && inv_deg_u && out && status, HSK_ERR_INVALID,
              "hsk_p3_score_rows: null pointer");
  HSK_REQUIRE((excl_indptr == nullptr) == (excl_indices == nullptr), HSK_ERR_INVALID,
              "hsk_p3_score_rows: exclude CSR needs both arrays");
  HSK_REQUIRE(n_rows > 0 && n_users > 0 && n_items > 0 && n_items < INT_MAX && ldw >= n_items && ld >= n_items,
              HSK_ERR_INVALID, "hsk_p3_score_rows: bad shape");
  HSK_REQUIRE(alpha > 0.0 && alpha < __builtin_inf(), HSK_ERR_INVALID, "hsk_p3_score_rows: alpha %g is not in (0, inf)",
              alpha);
  HSK_REQUIRE(window >= 1, HSK_ERR_INVALID, "hsk_p3_score_rows: window %lld < 1", (long long)window);
  const int64_t wlen = window < n_items ? window : n_items;
  const int64_t nw = hsk_ceil_div(n_items, wlen);
  HSK_REQUIRE(nw < (1ll << 31), HSK_ERR_INVALID, "hsk_p3_score_rows: too many windows");
  for (int64_t at = 0; at < n_rows; at += 65535) {   // grid.y limit
    const int64_t part = n_rows - at < 65535 ? n_rows - at : 65535;
    k_p3_score<<<dim3((unsigned)nw, (unsigned)part), P3_SCORE_THREADS, 0, (hipStream_t)stream>>>(
        users + at, n_users, x_indptr, x_indices, W, n_items, ldw, inv_deg_u, alpha, wlen, excl_indptr, excl_indices,
        out + at * ld, ld, status);
    HSK_LAUNCH_CHECK();
  }
  return HSK_OK;
}
