// hsk_ease.hip -- EASE (reference algorithms/linear_algs.py:131-176): fp64 Gram from the exact int32 counts, the SPD
// inverse on v_mfma_f64_16x16x4_f64, the column scaling and the fp64 gather-sum scorer.  DESIGN.md section 5.2.
//
// Inverse: blocked Gauss-Jordan without pivoting, in place, block width EASE_NB = 64.  For the diagonal block k
// (rows / columns K = [k0, k0 + b)), with D = A_KK^-1 and R = D A_K,: :
//     A_ij -= A_iK R_Kj  (i, j outside K),   A_K,: = R,   A_:,K = -A_:,K D,   A_KK = D.
// One step is three launches:
//   k_ease_diag_inv   one workgroup inverts A_KK in LDS (unblocked Gauss-Jordan) into the workspace;
//   k_ease_panels     writes the two k-major panels  Rp[r, j] (= R, and D in the columns of K)  and  Ct[c, i] = A[i, k0+c]
//                     (both [EASE_NB, n_pad], zero where r or c >= b and beyond n), so the update reads nothing it writes;
//   k_ease_update     out = (j in K ? 0 : A_ij) - sum_c Ct[c, i] Rp[c, j] on the matrix cores; rows of K take Rp instead.
// The update's workgroup (four waves) owns 128 x 128 outputs, wave (wm, wn) the 64 x 64 block in 4 x 4 tiles of
// 16 x 16 (hsk_f64_tile.h).  The whole inner dimension (64) of both panels sits in LDS at once: no k loop over global
// memory.  The scorer is hsk_gather_score.h's plain instance.
#include "hsk_f64_tile.h"
#include "hsk_gather_score.h"

#include <limits.h>

#define EASE_NB 64
#define EASE_TILE 128
#define EASE_LDS_ROW 144                            // 128 doubles + 16 pad: rows k and k + 1 start 32 banks apart
#define EASE_PANEL_LDS (EASE_NB * EASE_LDS_ROW)     // doubles of one panel image
#define EASE_GRID_ROWS 1024                         // grid.y of the row-wise kernels; each walks its rows in that stride

// ---------------------------------------------------------------------------------------------
// G = (double) counts + lam on the diagonal
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_ease_gram(const int32_t* __restrict__ C, int64_t rows, int64_t n, int64_t ldc,
                                                   int64_t r0, double lam, double* __restrict__ G, int64_t ld) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  for (int64_t i = blockIdx.y; i < rows; i += gridDim.y) {
    const double v = (double)C[i * ldc + j];
    G[(r0 + i) * ld + j] = (r0 + i == j) ? v + lam : v;
  }
}

// ---------------------------------------------------------------------------------------------
// inverse
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_ease_diag_inv(const double* __restrict__ A, int64_t ld, int64_t k0, int b,
                                                       double* __restrict__ D, int32_t* __restrict__ status) {
  __shared__ double a[EASE_NB][EASE_NB + 1];
  __shared__ double colp[EASE_NB];
  const int tid = threadIdx.x;
  for (int t = tid; t < EASE_NB * EASE_NB; t += 256) {
    const int r = t / EASE_NB, c = t % EASE_NB;
    a[r][c] = (r < b && c < b) ? A[(k0 + r) * ld + k0 + c] : (r == c ? 1.0 : 0.0);
  }
  __syncthreads();
  for (int p = 0; p < b; ++p) {
    const double piv = a[p][p];
    if (tid == 0 && !(piv > 0.0 && piv < __builtin_inf())) atomicOr(status, HSK_STATUS_NOT_SPD);
    const double inv = 1.0 / piv;
    if (tid < EASE_NB) colp[tid] = a[tid][p];
    __syncthreads();
    if (tid < EASE_NB) a[p][tid] = (tid == p) ? inv : a[p][tid] * inv;
    __syncthreads();
    for (int t = tid; t < EASE_NB * EASE_NB; t += 256) {
      const int r = t / EASE_NB, c = t % EASE_NB;
      if (r == p) continue;
      const double f = colp[r];
      a[r][c] = (c == p) ? -f * inv : a[r][c] - f * a[p][c];
    }
    __syncthreads();
  }
  for (int t = tid; t < EASE_NB * EASE_NB; t += 256) {
    const int r = t / EASE_NB, c = t % EASE_NB;
    D[t] = (r < b && c < b) ? a[r][c] : 0.0;
  }
}

// 64 columns per workgroup; thread (g, x) = (tid >> 6, tid & 63) computes rows 16 g ... 16 g + 15 of column j0 + x
__global__ void __launch_bounds__(256) k_ease_panels(const double* __restrict__ A, int64_t n, int64_t ld, int64_t n_pad,
                                                     int64_t k0, int b, const double* __restrict__ D,
                                                     double* __restrict__ Rp, double* __restrict__ Ct) {
  __shared__ double d[EASE_NB][EASE_NB];
  const int tid = threadIdx.x, g = tid >> 6, x = tid & 63;
  for (int t = tid; t < EASE_NB * EASE_NB; t += 256) d[t / EASE_NB][t % EASE_NB] = D[t];
  __syncthreads();
  const int64_t j = (int64_t)blockIdx.x * 64 + x;   // < n_pad
  const bool in_k = j >= k0 && j < k0 + b;
  // the column panel, transposed: Ct[c, j] = A[j, k0 + c] (zero on the rows of K, which take Rp)
  for (int c = g * 16; c < g * 16 + 16; ++c)
    Ct[c * n_pad + j] = (c < b && j < n && !in_k) ? A[j * ld + k0 + c] : 0.0;
  double acc[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0;
  if (j < n && !in_k) {
    for (int c = 0; c < b; ++c) {
      const double v = A[(k0 + c) * ld + j];
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = fma(d[g * 16 + r][c], v, acc[r]);
    }
  } else if (in_k) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = d[g * 16 + r][(int)(j - k0)];
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) Rp[(g * 16 + r) * n_pad + j] = acc[r];
}

__global__ void __launch_bounds__(256) k_ease_update(double* __restrict__ A, int64_t n, int64_t ld, int64_t n_pad,
                                                     int64_t k0, int b, const double* __restrict__ Rp,
                                                     const double* __restrict__ Ct) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* sa = lds;                    // Ct[:, i0 .. i0 + 128)
  double* sb = lds + EASE_PANEL_LDS;   // Rp[:, j0 .. j0 + 128)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t i0 = (int64_t)blockIdx.y * EASE_TILE, j0 = (int64_t)blockIdx.x * EASE_TILE;
  hsk_f64x4 acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const int64_t gj = hsk_f64_tile_col(j0 + wn * 64, nj, lane);
      const bool col_k = gj >= k0 && gj < k0 + b;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int64_t gi = hsk_f64_tile_row(i0 + wm * 64, mi, v, lane);
        acc[mi][nj][v] = (gi < n && gj < n && !col_k) ? A[gi * ld + gj] : 0.0;
      }
    }
  for (int t = tid; t < EASE_NB * (EASE_TILE / 2); t += 256) {
    const int k = t / (EASE_TILE / 2), c = (t % (EASE_TILE / 2)) * 2;
    *reinterpret_cast<hsk_f64x2*>(sa + k * EASE_LDS_ROW + c) =
        *reinterpret_cast<const hsk_f64x2*>(Ct + k * n_pad + i0 + c);
    *reinterpret_cast<hsk_f64x2*>(sb + k * EASE_LDS_ROW + c) =
        *reinterpret_cast<const hsk_f64x2*>(Rp + k * n_pad + j0 + c);
  }
  __syncthreads();
  // the product is subtracted: the A operand is negated as it is read
  hsk_f64_tile_mma<4, EASE_NB, EASE_LDS_ROW, 4, true>(acc, sa, wm * 64, sb, wn * 64, lane);
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const int cj = hsk_f64_tile_col(wn * 64, nj, lane);
      const int64_t gj = j0 + cj;
      if (gj >= n) continue;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int64_t gi = hsk_f64_tile_row(i0 + wm * 64, mi, v, lane);
        if (gi >= n) continue;
        const bool row_k = gi >= k0 && gi < k0 + b;
        A[gi * ld + gj] = row_k ? sb[(int)(gi - k0) * EASE_LDS_ROW + cj] : acc[mi][nj][v];
      }
    }
}

// ---------------------------------------------------------------------------------------------
// B = P / (-diag P), zero diagonal
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_ease_neg_diag(const double* __restrict__ P, int64_t n, int64_t ld,
                                                       double* __restrict__ nd) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < n) nd[j] = -P[j * ld + j];
}

__global__ void __launch_bounds__(256) k_ease_weights(double* __restrict__ P, int64_t n, int64_t ld,
                                                      const double* __restrict__ nd) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const double d = nd[j];
  for (int64_t i = blockIdx.y; i < n; i += gridDim.y) P[i * ld + j] = (i == j) ? 0.0 : P[i * ld + j] / d;
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" int hsk_ease_gram_f64(const int32_t* C, int64_t rows, int64_t n, int64_t ldc, int64_t r0, int64_t lam,
                                 double* G, int64_t ld, hsk_stream_t stream) {
  HSK_REQUIRE(C && G, HSK_ERR_INVALID, "hsk_ease_gram_f64: null pointer");
  HSK_REQUIRE(rows > 0 && n > 0 && n < INT_MAX && ldc >= n && ld >= n && r0 >= 0 && r0 + rows <= n,
              HSK_ERR_INVALID, "hsk_ease_gram_f64: bad block shape (rows %lld at %lld of n %lld, ldc %lld, ld %lld)",
              (long long)rows, (long long)r0, (long long)n, (long long)ldc, (long long)ld);
  const dim3 grid((unsigned)hsk_ceil_div(n, 256), (unsigned)(rows < EASE_GRID_ROWS ? rows : EASE_GRID_ROWS));
  k_ease_gram<<<grid, 256, 0, (hipStream_t)stream>>>(C, rows, n, ldc, r0, (double)lam, G, ld);
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}

extern "C" int64_t hsk_ease_inverse_ws_bytes(int64_t n) {
  if (n <= 0) return 0;
  return (2 * EASE_NB * hsk_align_up(n, EASE_TILE) + EASE_NB * EASE_NB) * (int64_t)sizeof(double);
}

extern "C" int hsk_ease_inverse_f64(double* A, int64_t n, int64_t ld, void* workspace, int64_t workspace_bytes,
                                    int32_t* status, hsk_stream_t stream) {
  HSK_REQUIRE(A && workspace && status, HSK_ERR_INVALID, "hsk_ease_inverse_f64: null pointer");
  HSK_REQUIRE(n > 0 && n < INT_MAX && ld >= n, HSK_ERR_INVALID, "hsk_ease_inverse_f64: bad shape n %lld ld %lld",
              (long long)n, (long long)ld);
  HSK_REQUIRE(workspace_bytes >= hsk_ease_inverse_ws_bytes(n), HSK_ERR_INVALID,
              "hsk_ease_inverse_f64: workspace of %lld bytes, needs %lld", (long long)workspace_bytes,
              (long long)hsk_ease_inverse_ws_bytes(n));
  HSK_REQUIRE(((uintptr_t)workspace & 15) == 0, HSK_ERR_INVALID, "hsk_ease_inverse_f64: workspace not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t n_pad = hsk_align_up(n, EASE_TILE);
  double* Rp = (double*)workspace;
  double* Ct = Rp + EASE_NB * n_pad;
  double* D = Ct + EASE_NB * n_pad;
  const int lds_bytes = 2 * EASE_PANEL_LDS * (int)sizeof(double);
  HSK_HIP(hipFuncSetAttribute((const void*)k_ease_update, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
  const dim3 grid((unsigned)(n_pad / EASE_TILE), (unsigned)(n_pad / EASE_TILE));
  for (int64_t k0 = 0; k0 < n; k0 += EASE_NB) {
    const int b = (int)(n - k0 < EASE_NB ? n - k0 : EASE_NB);
    k_ease_diag_inv<<<1, 256, 0, s>>>(A, ld, k0, b, D, status);
    HSK_LAUNCH_CHECK();
    k_ease_panels<<<(unsigned)(n_pad / 64), 256, 0, s>>>(A, n, ld, n_pad, k0, b, D, Rp, Ct);
    HSK_LAUNCH_CHECK();
    k_ease_update<<<grid, 256, lds_bytes, s>>>(A, n, ld, n_pad, k0, b, Rp, Ct);
    HSK_LAUNCH_CHECK();
  }
  return HSK_OK;
}

extern "C" int hsk_ease_weights(double* P, int64_t n, int64_t ld, double* neg_diag, hsk_stream_t stream) {
  HSK_REQUIRE(P && neg_diag, HSK_ERR_INVALID, "hsk_ease_weights: null pointer");
  HSK_REQUIRE(n > 0 && n < INT_MAX && ld >= n, HSK_ERR_INVALID, "hsk_ease_weights: bad shape n %lld ld %lld",
              (long long)n, (long long)ld);
  hipStream_t s = (hipStream_t)stream;
  k_ease_neg_diag<<<(unsigned)hsk_ceil_div(n, 256), 256, 0, s>>>(P, n, ld, neg_diag);
  HSK_LAUNCH_CHECK();
  const dim3 grid((unsigned)hsk_ceil_div(n, 256), (unsigned)(n < EASE_GRID_ROWS ? n : EASE_GRID_ROWS));
  k_ease_weights<<<grid, 256, 0, s>>>(P, n, ld, neg_diag);
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}

extern "C" int hsk_ease_score_rows(const int64_t* users, int64_t n_rows, int64_t n_users, const int64_t* x_indptr,
                                   const int32_t* x_indices, const double* B, int64_t n_items, int64_t ldb,
                                   int64_t window, const int64_t* excl_indptr, const int32_t* excl_indices, double* out,
                                   int64_t ld, int32_t* status, hsk_stream_t stream) {
  return hsk_gather_score_rows<false>("hsk_ease_score_rows", users, n_rows, n_users, x_indptr, x_indices, B, n_items, ldb,
                                      nullptr, 1.0, window, excl_indptr, excl_indices, out, ld, status, stream);
}
