// hsk_svd.hip -- truncated SVD of the binary train matrix X (reference algorithms/mf_algs.py:13-65) by block subspace
// iteration with Rayleigh-Ritz on A = X^T X, which is never formed.  DESIGN.md section 5.4.  Five entry points:
//   hsk_svd_spmm_f64        out = CSR @ dense block, each sum in stored order from 0.0 (scipy's csr @ dense, bitwise)
//   hsk_svd_gram_f64        H = A^T B of two tall-skinny blocks, split over the rows, partials summed in a fixed order
//   hsk_svd_mul_f64         out = A Q, A tall-skinny, Q small
//   hsk_svd_residuals_f64   res[j] = || Y[:, j] - theta_j V[:, j] ||_2
//   hsk_svd_score_rows      out[q, j] = <UF[users[q]], IF[j]>, excluded columns -inf
// Gram, product and scorer are one tile kernel on v_mfma_f64_16x16x4_f64: a workgroup of four waves owns 64 x 64
// outputs, wave (wm, wn) the 32 x 32 block at (32 wm, 32 wn) in 2 x 2 accumulator tiles of 16 x 16, and walks the inner
// dimension in blocks of SVD_BK = 32.  Both operands of a block sit in LDS as k-major [32][64 + 16 pad] images (rows k
// and k + 1 start 32 banks apart); an operand stored inner-dimension-major in global memory (the rows of A in A^T B,
// the rows of Q) is copied, one stored the other way (the rows of A in A Q, the factor rows of the scorer) is
// transposed on the way in.  Everything outside the operands reads as 0.0, so any 1 <= b <= HSK_SVD_MAX_BLOCK works.
// The next block's global loads are in flight under this block's MFMAs.  The tile loop and its operand and C/D maps
// are hsk_f64_tile.h's.
#include "hsk_f64_tile.h"

#include <limits.h>

#define SVD_TILE 64
#define SVD_BK 32
#define SVD_LDS_ROW 80
#define SVD_IMAGE (SVD_BK * SVD_LDS_ROW)   // doubles of one operand image: 20 480 bytes, two of them 40 960
#define SVD_SPMM_DEPTH 8                    // gathered rows in flight per wave
#define SVD_RES_COLS 16                     // columns per workgroup of the residual kernel
#define SVD_GRAM_TARGET_WGS 1024            // the Gram's grid: tiles x row splits is about this many workgroups

// ---------------------------------------------------------------------------------------------
// sparse x dense: one wave per (CSR row, 128 columns), lane = one pair of columns
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_svd_spmm(const int64_t* __restrict__ indptr,
                                                  const int32_t* __restrict__ indices, int64_t n_rows, int64_t n_cols,
                                                  const double* __restrict__ V, int64_t ldv, int b,
                                                  double* __restrict__ out, int64_t ldo) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  // a wave is the unit of work: no barrier, so a long row holds up its own wave only
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n_rows) return;
  const int c = (int)blockIdx.y * 128 + 2 * lane;
  if (c >= b) return;
  const int64_t lo = indptr[r], hi = indptr[r + 1];
  const double* __restrict__ col = V + c;
  hsk_f64x2 acc = {0.0, 0.0};
  for (int64_t e = lo; e < hi; e += SVD_SPMM_DEPTH) {
    hsk_f64x2 x[SVD_SPMM_DEPTH];
    bool ok[SVD_SPMM_DEPTH];
#pragma unroll
    for (int t = 0; t < SVD_SPMM_DEPTH; ++t) {
      const int32_t i = e + t < hi ? indices[e + t] : -1;
      ok[t] = i >= 0 && i < n_cols;
      // c and ldv are even: the pair (c, c + 1) is inside its row even where c + 1 == b.  A slot past the row's end
      // (or a bad id) loads row 0 and is not added, so the loads carry no branch and all of them are in flight.
      x[t] = *reinterpret_cast<const hsk_f64x2*>(col + (int64_t)(ok[t] ? i : 0) * ldv);
    }
#pragma unroll
    for (int t = 0; t < SVD_SPMM_DEPTH; ++t)
      if (ok[t]) acc = acc + x[t];   // in stored order
  }
  double* o = out + r * ldo + c;
  if (c + 1 < b) {
    *reinterpret_cast<hsk_f64x2*>(o) = acc;
  } else {
    *o = acc[0];
  }
}

// ---------------------------------------------------------------------------------------------
// the tile kernel
// ---------------------------------------------------------------------------------------------
struct svd_stage {
  hsk_f64x2 v[4];
};

// source stored inner-dimension-major: P[k, c], k in [k0, k1), c in [c0, C)
__device__ __forceinline__ void svd_gload_k(svd_stage& s, const double* __restrict__ P, int64_t ld, int64_t k0,
                                            int64_t k1, int64_t c0, int64_t C, int tid) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int t = tid + 256 * q;
    const int64_t k = k0 + (t >> 5), c = c0 + (t & 31) * 2;
    hsk_f64x2 x = {0.0, 0.0};
    if (k < k1 && c < C) {
      x = *reinterpret_cast<const hsk_f64x2*>(P + k * ld + c);
      if (c + 1 >= C) x[1] = 0.0;
    }
    s.v[q] = x;
  }
}

__device__ __forceinline__ void svd_sstore_k(const svd_stage& s, double* __restrict__ img, int tid) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int t = tid + 256 * q;
    *reinterpret_cast<hsk_f64x2*>(img + (t >> 5) * SVD_LDS_ROW + (t & 31) * 2) = s.v[q];
  }
}

// source stored the other way: P[row(c), k]; rows = the ids of the rows (or NULL for c itself), checked against n_src
__device__ __forceinline__ void svd_gload_c(svd_stage& s, const double* __restrict__ P, int64_t ld,
                                            const int64_t* __restrict__ rows, int64_t n_src, int64_t k0, int64_t k1,
                                            int64_t c0, int64_t C, int tid, int32_t* __restrict__ status) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int t = tid + 256 * q;
    const int64_t c = c0 + (t >> 4), k = k0 + (t & 15) * 2;
    hsk_f64x2 x = {0.0, 0.0};
    if (c < C && k < k1) {
      int64_t row = c;
      if (rows) {
        row = rows[c];
        if (row < 0 || row >= n_src) {
          if (k == 0) atomicOr(status, HSK_STATUS_BAD_INDEX);
          row = 0;
        }
      }
      x = *reinterpret_cast<const hsk_f64x2*>(P + row * ld + k);
      if (k + 1 >= k1) x[1] = 0.0;
    }
    s.v[q] = x;
  }
}

__device__ __forceinline__ void svd_sstore_c(const svd_stage& s, double* __restrict__ img, int tid) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int t = tid + 256 * q;
    const int c = t >> 4, k = (t & 15) * 2;
    img[k * SVD_LDS_ROW + c] = s.v[q][0];
    img[(k + 1) * SVD_LDS_ROW + c] = s.v[q][1];
  }
}

// out[z][i, j] = sum_{k in split z} a(i, k) b(k, j), i < M, j < N.  A_K: A is stored [K, M] (else [M, K], its rows
// picked by a_rows if given); B_K: B is stored [K, N] (else [N, K]).  blockIdx = (tile of M, tile of N, split of K).
template <bool A_K, bool B_K>
__global__ void __launch_bounds__(256) k_svd_tile(const double* __restrict__ A, int64_t lda,
                                                  const int64_t* __restrict__ a_rows, int64_t n_a_src,
                                                  const double* __restrict__ B, int64_t ldb, int64_t M, int64_t N,
                                                  int64_t K, int64_t k_per, double* __restrict__ out, int64_t ldo,
                                                  int64_t out_stride, int32_t* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) double sa[SVD_IMAGE];
  __shared__ __attribute__((aligned(16))) double sb[SVD_IMAGE];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t m0 = (int64_t)blockIdx.x * SVD_TILE, n0 = (int64_t)blockIdx.y * SVD_TILE;
  const int64_t kb = (int64_t)blockIdx.z * k_per, ke = kb + k_per < K ? kb + k_per : K;
  hsk_f64x4 acc[2][2];
  hsk_f64_tile_zero(acc);
  svd_stage ra, rb;
  auto gload = [&](int64_t k0) {
    if (A_K) svd_gload_k(ra, A, lda, k0, ke, m0, M, tid);
    else svd_gload_c(ra, A, lda, a_rows, n_a_src, k0, ke, m0, M, tid, status);
    if (B_K) svd_gload_k(rb, B, ldb, k0, ke, n0, N, tid);
    else svd_gload_c(rb, B, ldb, nullptr, 0, k0, ke, n0, N, tid, status);
  };
  auto sstore = [&]() {
    if (A_K) svd_sstore_k(ra, sa, tid);
    else svd_sstore_c(ra, sa, tid);
    if (B_K) svd_sstore_k(rb, sb, tid);
    else svd_sstore_c(rb, sb, tid);
  };
  gload(kb);
  sstore();
  __syncthreads();
  for (int64_t k0 = kb; k0 < ke; k0 += SVD_BK) {
    const bool more = k0 + SVD_BK < ke;
    if (more) gload(k0 + SVD_BK);
    hsk_f64_tile_mma<2, SVD_BK, SVD_LDS_ROW, SVD_BK / 4, false>(acc, sa, wm * 32, sb, wn * 32, lane);
    __syncthreads();   // every wave has read this block's images
    if (more) {
      sstore();
      __syncthreads();
    }
  }
  double* __restrict__ o = out + (int64_t)blockIdx.z * out_stride;
  auto store_row = [&](int64_t gi, const int64_t(&gj)[2], const double(&x)[2]) {
    if (gi >= M) return;
#pragma unroll
    for (int nj = 0; nj < 2; ++nj)
      if (gj[nj] < N) o[gi * ldo + gj[nj]] = x[nj];
  };
  hsk_f64_tile_rows(acc, m0 + wm * 32, n0 + wn * 32, lane, store_row);
}

// H[i, j] = ((0 + P_0[i, j]) + P_1[i, j]) + ... over the row splits in ascending order
__global__ void __launch_bounds__(256) k_svd_gram_sum(const double* __restrict__ ws, int64_t splits, int b,
                                                      double* __restrict__ H, int64_t ldh) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, bb = (int64_t)b * b;
  if (t >= bb) return;
  double acc = 0.0;
  for (int64_t z = 0; z < splits; ++z) acc = acc + ws[z * bb + t];
  H[(t / b) * ldh + t % b] = acc;
}

// ---------------------------------------------------------------------------------------------
// column residuals: a workgroup owns 16 columns, thread (rr, p) = (tid >> 3, tid & 7) the pair p of rows rr + 32 t;
// the 32 partial sums of squares of a column are added in ascending rr: the same order in every run
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_svd_residuals(const double* __restrict__ Y, int64_t ldy,
                                                       const double* __restrict__ V, int64_t ldv,
                                                       const double* __restrict__ theta, int64_t n, int b,
                                                       double* __restrict__ res) {
#pragma clang fp contract(off)
  __shared__ double part[32][SVD_RES_COLS];
  const int tid = threadIdx.x, rr = tid >> 3, p = tid & 7;
  const int c = (int)blockIdx.x * SVD_RES_COLS + 2 * p;
  double s0 = 0.0, s1 = 0.0;
  if (c < b) {
    const bool two = c + 1 < b;
    const double t0 = theta[c], t1 = two ? theta[c + 1] : 0.0;
    for (int64_t r = rr; r < n; r += 32) {
      const hsk_f64x2 y = *reinterpret_cast<const hsk_f64x2*>(Y + r * ldy + c);
      const hsk_f64x2 v = *reinterpret_cast<const hsk_f64x2*>(V + r * ldv + c);
      const double d0 = y[0] - t0 * v[0];
      s0 = s0 + d0 * d0;
      if (two) {
        const double d1 = y[1] - t1 * v[1];
        s1 = s1 + d1 * d1;
      }
    }
  }
  part[rr][2 * p] = s0;
  part[rr][2 * p + 1] = s1;
  __syncthreads();
  if (tid < SVD_RES_COLS && (int)blockIdx.x * SVD_RES_COLS + tid < b) {
    double acc = 0.0;
    for (int i = 0; i < 32; ++i) acc = acc + part[i][tid];
    res[blockIdx.x * SVD_RES_COLS + tid] = sqrt(acc);
  }
}

// the excluded columns of score row q = blockIdx.x (launched after the scores, on the same stream)
__global__ void __launch_bounds__(256) k_svd_exclude(const int64_t* __restrict__ users, int64_t n_users,
                                                     int64_t n_items, const int64_t* __restrict__ e_ptr,
                                                     const int32_t* __restrict__ e_idx, double* __restrict__ out,
                                                     int64_t ld) {
  const int64_t q = blockIdx.x;
  int64_t u = users[q];
  if (u < 0 || u >= n_users) u = 0;   // reported by the score kernel
  for (int64_t f = e_ptr[u] + threadIdx.x; f < e_ptr[u + 1]; f += 256) {
    const int64_t j = e_idx[f];
    if (j >= 0 && j < n_items) out[q * ld + j] = -__builtin_inf();
  }
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
static bool svd_dense_ok(const void* p, int64_t ld, int64_t b) {
  return ((uintptr_t)p & 15) == 0 && ld % 2 == 0 && ld >= b;
}

#define SVD_REQUIRE_BLOCK(b, what) \
  HSK_REQUIRE((b) >= 1 && (b) <= HSK_SVD_MAX_BLOCK, HSK_ERR_INVALID, what ": block width %lld outside [1, %d]", \
              (long long)(b), HSK_SVD_MAX_BLOCK)

extern "C" int hsk_svd_spmm_f64(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols,
                                const double* V, int64_t ldv, int64_t b, double* out, int64_t ldo,
                                hsk_stream_t stream) {
  HSK_REQUIRE(indptr && indices && V && out, HSK_ERR_INVALID, "hsk_svd_spmm_f64: null pointer");
  SVD_REQUIRE_BLOCK(b, "hsk_svd_spmm_f64");
  HSK_REQUIRE(n_rows > 0 && n_cols > 0 && n_cols < INT_MAX && hsk_ceil_div(n_rows, 4) < INT_MAX, HSK_ERR_INVALID,
              "hsk_svd_spmm_f64: bad shape (%lld x %lld)", (long long)n_rows, (long long)n_cols);
  HSK_REQUIRE(svd_dense_ok(V, ldv, b) && svd_dense_ok(out, ldo, b), HSK_ERR_INVALID,
              "hsk_svd_spmm_f64: V and out must be 16-byte aligned with even leading dimensions >= b");
  const dim3 grid((unsigned)hsk_ceil_div(n_rows, 4), (unsigned)hsk_ceil_div(b, 128));
  k_svd_spmm<<<grid, 256, 0, (hipStream_t)stream>>>(indptr, indices, n_rows, n_cols, V, ldv, (int)b, out, ldo);
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}

// rows of one split (a multiple of SVD_BK) and the number of splits
static void svd_gram_split(int64_t n, int64_t b, int64_t* k_per, int64_t* splits) {
  const int64_t tiles = hsk_ceil_div(b, SVD_TILE) * hsk_ceil_div(b, SVD_TILE);
  int64_t want = SVD_GRAM_TARGET_WGS / tiles;
  if (want < 1) want = 1;
  *k_per = hsk_align_up(hsk_ceil_div(n, want), SVD_BK);
  *splits = hsk_ceil_div(n, *k_per);
}

extern "C" int64_t hsk_svd_gram_ws_bytes(int64_t n, int64_t b) {
  if (n < 1 || b < 1 || b > HSK_SVD_MAX_BLOCK) return 0;
  int64_t k_per, splits;
  svd_gram_split(n, b, &k_per, &splits);
  return splits * b * b * (int64_t)sizeof(double);
}

extern "C" int hsk_svd_gram_f64(const double* A, int64_t lda, const double* B, int64_t ldb, int64_t n, int64_t b,
                                double* H, int64_t ldh, void* workspace, int64_t workspace_bytes, hsk_stream_t stream) {
  HSK_REQUIRE(A && B && H && workspace, HSK_ERR_INVALID, "hsk_svd_gram_f64: null pointer");
  SVD_REQUIRE_BLOCK(b, "hsk_svd_gram_f64");
  HSK_REQUIRE(n > 0 && ldh >= b, HSK_ERR_INVALID, "hsk_svd_gram_f64: bad shape (n %lld, ldh %lld)", (long long)n,
              (long long)ldh);
  HSK_REQUIRE(svd_dense_ok(A, lda, b) && svd_dense_ok(B, ldb, b), HSK_ERR_INVALID,
              "hsk_svd_gram_f64: A and B must be 16-byte aligned with even leading dimensions >= b");
  HSK_REQUIRE(((uintptr_t)workspace & 15) == 0 && workspace_bytes >= hsk_svd_gram_ws_bytes(n, b), HSK_ERR_INVALID,
              "hsk_svd_gram_f64: workspace of %lld bytes, needs %lld, 16-byte aligned", (long long)workspace_bytes,
              (long long)hsk_svd_gram_ws_bytes(n, b));
  int64_t k_per, splits;
  svd_gram_split(n, b, &k_per, &splits);
  HSK_REQUIRE(splits <= 65535, HSK_ERR_INVALID, "hsk_svd_gram_f64: too many row splits");
  const unsigned tiles = (unsigned)hsk_ceil_div(b, SVD_TILE);
  double* ws = (double*)workspace;
  k_svd_tile<true, true><<<dim3(tiles, tiles, (unsigned)splits), 256, 0, (hipStream_t)stream>>>(
      A, lda, nullptr, 0, B, ldb, b, b, n, k_per, ws, b, b * b, nullptr);
  HSK_LAUNCH_CHECK();
  k_svd_gram_sum<<<(unsigned)hsk_ceil_div(b * b, 256), 256, 0, (hipStream_t)stream>>>(ws, splits, (int)b, H, ldh);
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}

extern "C" int hsk_svd_mul_f64(const double* A, int64_t lda, int64_t n, int64_t b, const double* Q, int64_t ldq,
                               int64_t b2, double* out, int64_t ldo, hsk_stream_t stream) {
  HSK_REQUIRE(A && Q && out && (const double*)out != A, HSK_ERR_INVALID,
              "hsk_svd_mul_f64: null pointer, or out is A (the product is not in place)");
  SVD_REQUIRE_BLOCK(b, "hsk_svd_mul_f64");
  HSK_REQUIRE(b2 >= 1 && b2 <= b, HSK_ERR_INVALID, "hsk_svd_mul_f64: b2 %lld outside [1, b = %lld]", (long long)b2,
              (long long)b);
  HSK_REQUIRE(n > 0 && hsk_ceil_div(n, SVD_TILE) < INT_MAX && ldo >= b2, HSK_ERR_INVALID,
              "hsk_svd_mul_f64: bad shape (n %lld, ldo %lld)", (long long)n, (long long)ldo);
  HSK_REQUIRE(svd_dense_ok(A, lda, b) && svd_dense_ok(Q, ldq, b2), HSK_ERR_INVALID,
              "hsk_svd_mul_f64: A and Q must be 16-byte aligned with even leading dimensions >= b and >= b2");
  const dim3 grid((unsigned)hsk_ceil_div(n, SVD_TILE), (unsigned)hsk_ceil_div(b2, SVD_TILE));
  k_svd_tile<false, true><<<grid, 256, 0, (hipStream_t)stream>>>(A, lda, nullptr, 0, Q, ldq, n, b2, b, b, out, ldo, 0,
                                                                 nullptr);
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}

extern "C" int hsk_svd_residuals_f64(const double* Y, int64_t ldy, const double* V, int64_t ldv, const double* theta,
                                     int64_t n, int64_t b, double* res, hsk_stream_t stream) {
  HSK_REQUIRE(Y && V && theta && res, HSK_ERR_INVALID, "hsk_svd_residuals_f64: null pointer");
  SVD_REQUIRE_BLOCK(b, "hsk_svd_residuals_f64");
  HSK_REQUIRE(n > 0, HSK_ERR_INVALID, "hsk_svd_residuals_f64: n %lld < 1", (long long)n);
  HSK_REQUIRE(svd_dense_ok(Y, ldy, b) && svd_dense_ok(V, ldv, b), HSK_ERR_INVALID,
              "hsk_svd_residuals_f64: Y and V must be 16-byte aligned with even leading dimensions >= b");
  k_svd_residuals<<<(unsigned)hsk_ceil_div(b, SVD_RES_COLS), 256, 0, (hipStream_t)stream>>>(Y, ldy, V, ldv, theta, n,
                                                                                           (int)b, res);
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}

extern "C" int hsk_svd_score_rows(const int64_t* users, int64_t n_rows, int64_t n_users, const double* UF, int64_t ldu,
                                  const double* IF, int64_t ldi, int64_t n_items, int64_t k,
                                  const int64_t* excl_indptr, const int32_t* excl_indices, double* out, int64_t ld,
                                  int32_t* status, hsk_stream_t stream) {
  HSK_REQUIRE(users && UF && IF && out && status, HSK_ERR_INVALID, "hsk_svd_score_rows: null pointer");
  HSK_REQUIRE((excl_indptr == nullptr) == (excl_indices == nullptr), HSK_ERR_INVALID,
              "hsk_svd_score_rows: exclude CSR needs both arrays");
  SVD_REQUIRE_BLOCK(k, "hsk_svd_score_rows");
  // the row tiles are grid.x, the item tiles grid.y
  HSK_REQUIRE(n_rows > 0 && n_rows < INT_MAX && n_users > 0 && n_items > 0 && ld >= n_items &&
                  hsk_ceil_div(n_items, SVD_TILE) <= 65535,
              HSK_ERR_INVALID, "hsk_svd_score_rows: bad shape (at most %d items)", 65535 * SVD_TILE);
  HSK_REQUIRE(svd_dense_ok(UF, ldu, k) && svd_dense_ok(IF, ldi, k), HSK_ERR_INVALID,
              "hsk_svd_score_rows: UF and IF must be 16-byte aligned with even leading dimensions >= k");
  const dim3 grid((unsigned)hsk_ceil_div(n_rows, SVD_TILE), (unsigned)hsk_ceil_div(n_items, SVD_TILE));
  k_svd_tile<false, false><<<grid, 256, 0, (hipStream_t)stream>>>(UF, ldu, users, n_users, IF, ldi, n_rows, n_items, k,
                                                                  k, out, ld, 0, status);
  HSK_LAUNCH_CHECK();
  if (excl_indptr) {
    k_svd_exclude<<<(unsigned)n_rows, 256, 0, (hipStream_t)stream>>>(users, n_users, n_items, excl_indptr,
                                                                     excl_indices, out, ld);
    HSK_LAUNCH_CHECK();
  }
  return HSK_OK;
}
