// hsk_als.hip -- implicit-feedback alternating least squares (reference algorithms/mf_algs.py:68-142, which calls the
// `implicit` package; Hu, Koren, Volinsky).  DESIGN.md section 5.9.  One entry point, one half-sweep:
//   hsk_als_solve_f64   x_r = A_r^-1 b_r for every row r of a binary CSR against the other side's factors Y,
//                       A_r = G + reg I + (alpha - 1) sum_{i in row r} y_i y_i^T,   b_r = alpha sum_{i in row r} y_i
// with G = Y^T Y from hsk_svd_gram_f64.  All fp64, solved exactly by Cholesky.
//
// One workgroup of four waves owns one row; T = ceil(k / 32), KP = 32 T, PITCH = KP + 16.
//   1. gather   the row's factor rows, ALS_BK = 32 entries at a time, into one k-major LDS image img[entry][factor];
//               the image is both MFMA operands (S = Y_r^T Y_r) and wave (wm, wn) holds its quarter of S in T x T
//               accumulator tiles through hsk_f64_tile_mma.  The next block's gathers are in flight under this
//               block's MFMAs.  b_r is summed from the same image by thread f in ascending entry order.
//   2. A_r      = coef S + G + reg I is formed in the accumulators (rows and columns >= k: the identity).
//   3. Cholesky right-looking in panels of 16 columns.  The trailing matrix never leaves the accumulators: for panel
//               J the waves that own its columns write them to L[col][row] (the image's storage, dead by now), wave 0
//               factors the 16 x 16 diagonal block in registers (lane i = row i, pivots and multipliers by shuffle)
//               and forward-substitutes b_J on the way, one thread per row below solves its row of the panel against
//               L_JJ and updates its b, and every wave subtracts L_:J L_:J^T from its tiles that are still open on
//               the matrix cores, L_:J read in place as a k-major image.
//   4. solve    the forward substitution is done (step 3); wave 0 substitutes backwards, lane = row, and stores x_r.
// Every sum has a fixed order that depends on the row's own entries and on k alone: not on the grid, on `order` or on
// what other rows hold.
#include "hsk_f64_tile.h"

#include <limits.h>
#include <math.h>

#include <atomic>

#define ALS_BK 32       // entries gathered per block
#define ALS_PANEL 16    // columns of a Cholesky panel

template <int T>
struct als_dims {
  static constexpr int KP = 32 * T;            // padded number of factors
  static constexpr int PITCH = KP + 16;        // doubles per row of the image and of L
  static constexpr int PAIRS = KP / 2;         // f64x2 per gathered row
  static constexpr int NQ = ALS_BK * PAIRS / 256;   // f64x2 per thread per block (= 2 T)
  // L (KP x PITCH; the gather image ALS_BK x PITCH shares its storage), b / z (KP), one flag word
  static constexpr int LDS_BYTES = (KP * PITCH + KP + 2) * (int)sizeof(double);
};

template <int T>
struct als_stage {
  hsk_f64x2 v[als_dims<T>::NQ];
};

// entries [e0, e0 + 32) of the row (entry e of the block = row e of the image); slots past the row's end, bad ids and
// factors >= k read as 0.0
template <int T>
__device__ __forceinline__ void als_gload(als_stage<T>& s, const int32_t* __restrict__ indices, int64_t e0, int64_t hi,
                                          int64_t n_cols, const double* __restrict__ Y, int64_t ldy, int k, int tid,
                                          int32_t* __restrict__ status) {
  using D = als_dims<T>;
#pragma unroll
  for (int q = 0; q < D::NQ; ++q) {
    const int t = tid + 256 * q;
    const int e = t / D::PAIRS, f = (t % D::PAIRS) * 2;
    hsk_f64x2 x = {0.0, 0.0};
    if (e0 + e < hi && f < k) {
      const int32_t i = indices[e0 + e];
      if (i >= 0 && i < n_cols) {
        // f and ldy are even: the pair (f, f + 1) is inside its row even where f + 1 == k
        x = *reinterpret_cast<const hsk_f64x2*>(Y + (int64_t)i * ldy + f);
        if (f + 1 >= k) x[1] = 0.0;
      } else if (f == 0) {
        atomicOr(status, HSK_STATUS_BAD_INDEX);
      }
    }
    s.v[q] = x;
  }
}

template <int T>
__device__ __forceinline__ void als_sstore(const als_stage<T>& s, double* __restrict__ img, int tid) {
  using D = als_dims<T>;
#pragma unroll
  for (int q = 0; q < D::NQ; ++q) {
    const int t = tid + 256 * q;
    *reinterpret_cast<hsk_f64x2*>(img + (t / D::PAIRS) * D::PITCH + (t % D::PAIRS) * 2) = s.v[q];
  }
}

template <int T>
__global__ void __launch_bounds__(256) k_als_solve(const int64_t* __restrict__ indptr,
                                                   const int32_t* __restrict__ indices, int64_t n_rows, int64_t n_cols,
                                                   const int32_t* __restrict__ order, const double* __restrict__ Y,
                                                   int64_t ldy, int k, const double* __restrict__ G, int64_t ldg,
                                                   double alpha, double reg, double* __restrict__ X, int64_t ldx,
                                                   int32_t* __restrict__ status) {
  using D = als_dims<T>;
  constexpr int KP = D::KP, P = D::PITCH;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* L = lds;                 // L[c * P + r] = L_rc (r >= c); first the gather image img[e * P + f]
  double* sb = lds + KP * P;       // b_r, overwritten block by block with z = L^-1 b_r
  int* flag = reinterpret_cast<int*>(sb + KP);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;

  int64_t r = blockIdx.x;
  if (order) {
    r = order[blockIdx.x];
    if (r < 0 || r >= n_rows) {   // not a permutation: nothing is read or written for it
      if (tid == 0) atomicOr(status, HSK_STATUS_BAD_INDEX);
      return;
    }
  }
  double* __restrict__ xr = X + r * ldx;
  const int64_t lo = indptr[r], hi = indptr[r + 1];
  if (lo >= hi) {   // no entries: x_r = 0 exactly, no LDS, no barrier
    if (tid < k) xr[tid] = 0.0;
    return;
  }

  // ---- 1. S = Y_r^T Y_r in the accumulators, b_r = sum y_i in thread f
  const double coef = alpha - 1.0;
  hsk_f64x4 acc[T][T];
  hsk_f64_tile_zero(acc);
  double bsum = 0.0;
  als_stage<T> st;
  als_gload<T>(st, indices, lo, hi, n_cols, Y, ldy, k, tid, status);
  als_sstore<T>(st, L, tid);
  __syncthreads();
  for (int64_t e0 = lo; e0 < hi; e0 += ALS_BK) {
    const bool more = e0 + ALS_BK < hi;
    if (more) als_gload<T>(st, indices, e0 + ALS_BK, hi, n_cols, Y, ldy, k, tid, status);
    if (coef != 0.0) hsk_f64_tile_mma<T, ALS_BK, P, ALS_BK / 4, false>(acc, L, wm * 16 * T, L, wn * 16 * T, lane);
    if (tid < KP) {
#pragma unroll 8
      for (int e = 0; e < ALS_BK; ++e) bsum = bsum + L[e * P + tid];   // ascending entry order
    }
    __syncthreads();   // every wave has read this block's image
    if (more) {
      als_sstore<T>(st, L, tid);
      __syncthreads();
    }
  }

  // ---- 2. A_r in the accumulators; the image is dead: its storage becomes L, zero above the diagonal blocks
#pragma unroll
  for (int mi = 0; mi < T; ++mi)
#pragma unroll
    for (int nj = 0; nj < T; ++nj) {
      const int gj = hsk_f64_tile_col(wn * 16 * T, nj, lane);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int gi = hsk_f64_tile_row(wm * 16 * T, mi, v, lane);
        double a = gi == gj ? 1.0 : 0.0;
        if (gi < k && gj < k) {
          a = fma(coef, acc[mi][nj][v], G[(int64_t)gi * ldg + gj]);
          if (gi == gj) a = a + reg;
        }
        acc[mi][nj][v] = a;
      }
    }
  for (int t = tid; t < KP * P / 2; t += 256) *reinterpret_cast<hsk_f64x2*>(L + 2 * t) = hsk_f64x2{0.0, 0.0};
  if (tid < KP) sb[tid] = alpha * bsum;
  if (tid == 0) *flag = 0;
  __syncthreads();

  // ---- 3. blocked Cholesky, the forward substitution riding along
  const int nb = (k + ALS_PANEL - 1) / ALS_PANEL, k16 = nb * ALS_PANEL;
  const int lc = lane & 15, lq = lane >> 4;
  bool failed = false;
  for (int jb = 0; jb < nb; ++jb) {
    const int j0 = jb * ALS_PANEL;
    double* __restrict__ Lj = L + j0 * P;   // the panel: Lj[c * P + row], c < 16
    // the panel's columns leave the accumulators (rows from the diagonal block down)
#pragma unroll
    for (int mi = 0; mi < T; ++mi)
#pragma unroll
      for (int nj = 0; nj < T; ++nj)
        if (wn * T + nj == jb && wm * T + mi >= jb) {
#pragma unroll
          for (int v = 0; v < 4; ++v) Lj[lc * P + (wm * T + mi) * 16 + lq + 4 * v] = acc[mi][nj][v];
        }
    __syncthreads();
    if (wave == 0) {
      // the diagonal block: lane i (of each 16) holds row i, a[c] = A[j0 + i][j0 + c]; what a lane holds right of its
      // own diagonal (c > i) is never used
      double a[ALS_PANEL];
#pragma unroll
      for (int c = 0; c < ALS_PANEL; ++c) a[c] = Lj[c * P + j0 + lc];
      bool bad = false;
#pragma unroll
      for (int c = 0; c < ALS_PANEL; ++c) {
        const double d = __shfl(a[c], c, 16);
        bad = bad || !(d > 0.0 && d < __builtin_inf());
        const double piv = sqrt(d);
        a[c] = lc == c ? piv : a[c] / piv;
#pragma unroll
        for (int c2 = c + 1; c2 < ALS_PANEL; ++c2) a[c2] = a[c2] - a[c] * __shfl(a[c], c2, 16);
      }
      // z_J = L_JJ^-1 b_J, one value per lane: lane c divides at step c, the lanes after it subtract
      double zv = sb[j0 + lc];
#pragma unroll
      for (int c = 0; c < ALS_PANEL; ++c) {
        const double zc = __shfl(zv / a[c], c, 16);   // in lane c, a[c] = L_cc
        zv = lc == c ? zc : (lc > c ? zv - a[c] * zc : zv);
      }
      if (lane < ALS_PANEL) {
#pragma unroll
        for (int c = 0; c < ALS_PANEL; ++c) Lj[c * P + j0 + lc] = lc >= c ? a[c] : 0.0;
        sb[j0 + lc] = zv;
        if (bad) *flag = 1;
      }
    }
    __syncthreads();
    if (*flag) {   // the same word for every thread: a uniform exit
      failed = true;
      break;
    }
    // one thread per row below the diagonal block: its row of L_:J, then its b
    const int row = j0 + ALS_PANEL + tid;
    if (row < k16) {
      double x[ALS_PANEL];
#pragma unroll
      for (int c = 0; c < ALS_PANEL; ++c) x[c] = Lj[c * P + row];
#pragma unroll
      for (int c = 0; c < ALS_PANEL; ++c) {
        double s = x[c];
#pragma unroll
        for (int m = 0; m < c; ++m) s = s - x[m] * Lj[m * P + j0 + c];
        x[c] = s / Lj[c * P + j0 + c];
      }
      double bb = sb[row];
#pragma unroll
      for (int c = 0; c < ALS_PANEL; ++c) {
        bb = bb - x[c] * sb[j0 + c];
        Lj[c * P + row] = x[c];
      }
      sb[row] = bb;
    }
    __syncthreads();
    // the open tiles (below and right of the panel, lower triangle) lose L_:J L_:J^T; the next panel's columns go to
    // other rows of L, so no barrier is needed before they are written
    if (jb + 1 < nb) {
#pragma unroll
      for (int ks = 0; ks < ALS_PANEL / 4; ++ks) {
        double af[T], bf[T];
        const int kk = ks * 4 + lq;
#pragma unroll
        for (int mi = 0; mi < T; ++mi) af[mi] = -Lj[kk * P + (wm * T + mi) * 16 + lc];
#pragma unroll
        for (int nj = 0; nj < T; ++nj) bf[nj] = Lj[kk * P + (wn * T + nj) * 16 + lc];
#pragma unroll
        for (int mi = 0; mi < T; ++mi)
#pragma unroll
          for (int nj = 0; nj < T; ++nj)
            if (wn * T + nj > jb && wn * T + nj < nb && wm * T + mi >= wn * T + nj)
              acc[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[mi], bf[nj], acc[mi][nj], 0, 0, 0);
      }
    }
  }
  if (wave != 0) return;   // no barrier below

  // ---- 4. L^T x = z in wave 0: lane holds rows lane and lane + 64
  double x0 = 0.0, x1 = 0.0;
  if (!failed) {
    x0 = lane < k ? sb[lane] : 0.0;
    if (KP > 64) x1 = lane + 64 < k ? sb[lane + 64] : 0.0;
    for (int c = k - 1; c >= 0; --c) {
      const double mine = (KP > 64 && c >= 64) ? x1 : x0;
      const double xc = __shfl(mine / L[c * P + c], c & 63);
      if (lane == (c & 63)) {
        if (KP > 64 && c >= 64) x1 = xc;
        else x0 = xc;
      }
      if (lane < c) x0 = x0 - L[lane * P + c] * xc;
      if (KP > 64 && lane + 64 < c) x1 = x1 - L[(lane + 64) * P + c] * xc;
    }
    const bool fin = fabs(x0) < __builtin_inf() && fabs(x1) < __builtin_inf();
    failed = !__all(fin);   // a non-finite solution: non-finite input that met no pivot (alpha == 1)
  }
  if (failed) {
    x0 = x1 = 0.0;
    if (lane == 0) atomicOr(status, HSK_STATUS_NOT_SPD);
  }
  if (lane < k) xr[lane] = x0;
  if (KP > 64 && lane + 64 < k) xr[lane + 64] = x1;
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
static bool als_dense_ok(const void* p, int64_t ld, int64_t k) {
  return ((uintptr_t)p & 15) == 0 && ld % 2 == 0 && ld >= k;
}

template <int T>
static int als_launch(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols,
                      const int32_t* order, const double* Y, int64_t ldy, int k, const double* G, int64_t ldg,
                      double alpha, double reg, double* X, int64_t ldx, int32_t* status, hipStream_t s) {
  const int lds_bytes = als_dims<T>::LDS_BYTES;
  // the dynamic LDS limit of this instance is raised once per device, not at every launch of a fit
  static std::atomic<uint64_t> raised{0};
  int dev = 0;
  HSK_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !((raised.load() >> dev) & 1)) {
    HSK_HIP(hipFuncSetAttribute((const void*)k_als_solve<T>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    if (dev >= 0 && dev < 64) raised.fetch_or(uint64_t(1) << dev);
  }
  k_als_solve<T><<<(unsigned)n_rows, 256, lds_bytes, s>>>(indptr, indices, n_rows, n_cols, order, Y, ldy, k, G, ldg,
                                                          alpha, reg, X, ldx, status);
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}

extern "C" int hsk_als_solve_f64(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols,
                                 const int32_t* order, const double* Y, int64_t ldy, int64_t k, const double* G,
                                 int64_t ldg, double alpha, double reg, double* X, int64_t ldx, int32_t* status,
                                 hsk_stream_t stream) {
  HSK_REQUIRE(indptr && indices && Y && G && X && status, HSK_ERR_INVALID, "hsk_als_solve_f64: null pointer");
  HSK_REQUIRE(k >= 1 && k <= HSK_ALS_MAX_FACTORS, HSK_ERR_INVALID, "hsk_als_solve_f64: k %lld outside [1, %d]",
              (long long)k, HSK_ALS_MAX_FACTORS);
  HSK_REQUIRE(n_rows > 0 && n_rows < INT_MAX && n_cols > 0 && n_cols < INT_MAX, HSK_ERR_INVALID,
              "hsk_als_solve_f64: bad shape (%lld x %lld)", (long long)n_rows, (long long)n_cols);
  HSK_REQUIRE(als_dense_ok(Y, ldy, k) && als_dense_ok(X, ldx, k) && ldg >= k, HSK_ERR_INVALID,
              "hsk_als_solve_f64: Y and X must be 16-byte aligned with even leading dimensions >= k, ldg >= k");
  HSK_REQUIRE(alpha > 0.0 && alpha < (double)INFINITY && reg > 0.0 && reg < (double)INFINITY, HSK_ERR_INVALID,
              "hsk_als_solve_f64: alpha %g and reg %g must be finite and > 0", alpha, reg);
  hipStream_t s = (hipStream_t)stream;
  switch ((k + 31) / 32) {
    case 1:
      return als_launch<1>(indptr, indices, n_rows, n_cols, order, Y, ldy, (int)k, G, ldg, alpha, reg, X, ldx, status, s);
    case 2:
      return als_launch<2>(indptr, indices, n_rows, n_cols, order, Y, ldy, (int)k, G, ldg, alpha, reg, X, ldx, status, s);
    case 3:
      return als_launch<3>(indptr, indices, n_rows, n_cols, order, Y, ldy, (int)k, G, ldg, alpha, reg, X, ldx, status, s);
    default:
      return als_launch<4>(indptr, indices, n_rows, n_cols, order, Y, ldy, (int)k, G, ldg, alpha, reg, X, ldx, status, s);
  }
}
