// hsk_p3.hip -- P3alpha (reference algorithms/graph_algs.py:9-88): the reciprocal degrees, the weighted fp64 Gram
// S = X^T diag(w_u) X on v_mfma_f64_16x16x4_f64 straight from the int8 image of X^T, and the fp64 gather-sum scorer
// with the element-wise power.  DESIGN.md section 5.3.
//
// Gram geometry: a workgroup of four waves owns 128 x 128 outputs, wave (wm, wn) the 64 x 64 block at (64 wm, 64 wn) in
// 4 x 4 accumulator tiles of 16 x 16 (the tile loop and its operand and C/D maps: hsk_f64_tile.h).  The k loop walks k_pad in blocks of
// P3_BK = 64 users.  Both operands are rows of the same item-major int8 matrix M; a block's two [128 items][64 B] tiles
// are loaded 16 bytes per lane (as knn_gload does) one block ahead of the MFMAs, and are converted to fp64 once, when
// they are written to LDS as k-major [64][128 + 16 pad] images -- the B side multiplied by col_weight there, which is
// exact (the product is 0 or w_u).  Row tile and column tile walk k in the same order and every product is w_u or 0 on
// both sides of the diagonal, so the unscaled result is bitwise symmetric.
#include "hsk_f64_tile.h"
#include "hsk_gather_score.h"

#include <limits.h>

#define P3_TILE 128
#define P3_BK 64
#define P3_LDS_ROW 144                          // 128 doubles + 16 pad: rows k and k + 1 start 32 banks apart
#define P3_IMAGE (P3_BK * P3_LDS_ROW)           // doubles of one operand image: 73 728 bytes, two of them 147 456

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
  hsk_f64x2 w[8];   // col_weight of this lane's 16 k of the block
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
  for (int t = 0; t < 8; ++t) s.w[t] = *reinterpret_cast<const hsk_f64x2*>(cw + k0 + 2 * t);
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
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t m0 = r0 + (int64_t)blockIdx.y * P3_TILE, n0 = (int64_t)blockIdx.x * P3_TILE;
  const int NK = (int)(k_pad / P3_BK);
  hsk_f64x4 acc[4][4];
  hsk_f64_tile_zero(acc);
  p3_stage s;
  p3_gload(s, M, col_weight, k_pad, m0, n0, 0, tid);
  p3_sstore(s, sa, sb, tid);
  __syncthreads();
  for (int kt = 0; kt < NK; ++kt) {
    const bool more = kt + 1 < NK;
    if (more) p3_gload(s, M, col_weight, k_pad, m0, n0, kt + 1, tid);   // in flight under this block's MFMAs
    hsk_f64_tile_mma<4, P3_BK, P3_LDS_ROW, 4, false>(acc, sa, wm * 64, sb, wn * 64, lane);
    __syncthreads();   // every wave has read this block's images
    if (more) {
      p3_sstore(s, sa, sb, tid);
      __syncthreads();
    }
  }
  auto store_row = [&](int64_t gi, const int64_t(&gj)[4], const double(&x)[4]) {
    if (gi >= r1) return;
    const double sc = row_scale ? row_scale[gi] : 1.0;
#pragma unroll
    for (int nj = 0; nj < 4; ++nj)
      if (gj[nj] < n) out[gi * ld + gj[nj]] = row_scale ? sc * x[nj] : x[nj];
  };
  hsk_f64_tile_rows(acc, m0 + wm * 64, n0 + wn * 64, lane, store_row);
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
  return hsk_gather_score_rows<true>("hsk_p3_score_rows", users, n_rows, n_users, x_indptr, x_indices, W, n_items, ldw,
                                     inv_deg_u, alpha, window, excl_indptr, excl_indices, out, ld, status, stream);
}
