// hsk_f64_tile.h -- the fp64 matrix-core tile loop of the closed-form models (k_ease_update, k_p3_gram, k_svd_tile).
//
// A wave owns T x T accumulator tiles of 16 x 16, each one hsk_f64x4 per lane, and feeds them with
// v_mfma_f64_16x16x4_f64 from two k-major LDS images sa[k][row] and sb[k][column] of PITCH doubles per k:
//   A operand: the lane holds A[row = lane & 15][k = lane >> 4];  B operand: B[k = lane >> 4][column = lane & 15];
//   C/D:       element v of the lane's accumulator is C[row = (lane >> 4) + 4 v][column = lane & 15].
// How the images are filled, and what the accumulators start from and end in, is the kernel's own business.
#pragma once
#include "hsk_common.h"

typedef double hsk_f64x4 __attribute__((ext_vector_type(4)));
typedef double hsk_f64x2 __attribute__((ext_vector_type(2)));

// row / column of element v of accumulator tile (mi, nj), counted from the row0 / col0 of the wave's tile (0, 0), in
// the type of row0 / col0
template <class I>
__device__ __forceinline__ I hsk_f64_tile_row(I row0, int mi, int v, int lane) {
  return row0 + mi * 16 + (lane >> 4) + 4 * v;
}
template <class I>
__device__ __forceinline__ I hsk_f64_tile_col(I col0, int nj, int lane) {
  return col0 + nj * 16 + (lane & 15);
}

template <int T>
__device__ __forceinline__ void hsk_f64_tile_zero(hsk_f64x4 (&acc)[T][T]) {
#pragma unroll
  for (int mi = 0; mi < T; ++mi)
#pragma unroll
    for (int nj = 0; nj < T; ++nj)
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[mi][nj][v] = 0.0;
}

// acc += (NEG_A ? -a : a) b over one block of BK k.  a0 / b0 = the wave's first row / column in the images; k ascends,
// and within one k step the tiles go mi outer, nj inner.  UNROLL = k steps (of 4) unrolled together.
template <int T, int BK, int PITCH, int UNROLL, bool NEG_A>
__device__ __forceinline__ void hsk_f64_tile_mma(hsk_f64x4 (&acc)[T][T], const double* sa, int a0, const double* sb,
                                                 int b0, int lane) {
  const int lc = lane & 15, lq = lane >> 4;
#pragma unroll UNROLL
  for (int ks = 0; ks < BK / 4; ++ks) {
    double af[T], bf[T];
    const int k = ks * 4 + lq;
#pragma unroll
    for (int mi = 0; mi < T; ++mi) {
      const double a = sa[k * PITCH + a0 + mi * 16 + lc];
      af[mi] = NEG_A ? -a : a;
    }
#pragma unroll
    for (int nj = 0; nj < T; ++nj) bf[nj] = sb[k * PITCH + b0 + nj * 16 + lc];
#pragma unroll
    for (int mi = 0; mi < T; ++mi)
#pragma unroll
      for (int nj = 0; nj < T; ++nj)
        acc[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[mi], bf[nj], acc[mi][nj], 0, 0, 0);
  }
}

// f(row, col, x) for each of the lane's 4 T rows, mi outer and v inner: x[nj] is the row's element in column col[nj].
// Rows and columns count from the row0 / col0 of the wave's tile (0, 0), in their type.  A row at a time, so that what
// depends on the row alone is done once; the columns are formed before the walk (formed at each use, k_p3_gram came out
// of the compiler with 64 more VGPRs live across its k loop).
template <int T, class I, class F>
__device__ __forceinline__ void hsk_f64_tile_rows(const hsk_f64x4 (&acc)[T][T], I row0, I col0, int lane, F f) {
  I col[T];
#pragma unroll
  for (int nj = 0; nj < T; ++nj) col[nj] = hsk_f64_tile_col(col0, nj, lane);
#pragma unroll
  for (int mi = 0; mi < T; ++mi)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      double x[T];
#pragma unroll
      for (int nj = 0; nj < T; ++nj) x[nj] = acc[mi][nj][v];
      f(hsk_f64_tile_row(row0, mi, v, lane), col, x);
    }
}
