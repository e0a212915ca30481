// hsk_slim.hip -- SLIM (reference algorithms/linear_algs.py:14-128): n_items independent non-negative elastic-net
// problems over one shared fp64 Gram G = X^T X, by cyclic coordinate descent on G alone.  DESIGN.md section 5.10.
//
// Per column j, with l1 = n_users alpha rho, l2 = n_users alpha (1 - rho), d_i = G_ii, g_i = G_ij and
// q_i = sum_{k != j} G_ik w_k:
//     t = g_i - (q_i - d_i w_i) - l1;   new = t > 0 ? t / (d_i + l2) : 0;
//     if new != w_i:  q_k += (new - w_i) G_ik for every k,  w_i = new
// over i ascending, i != j, d_i > 0; every operation rounded on its own (nothing contracted into an fma), so the
// iterates depend on no summation order.  After a sweep with wmax == 0, dmax <= tol wmax or it == max_iter sklearn's
// duality gap decides (its sums are the only reductions: per-thread strides, a shuffle tree, the four waves in order).
//
// One workgroup (four waves) per column, columns pulled in order from a counter.  The candidates {i : g_i > l1,
// d_i > 0, i != j} are compacted once in ascending order (with G >= 0 and w >= 0 no other coordinate can leave 0);
// their g, d, q, w and ids live in LDS up to SLIM_LDS_CANDIDATES of them and in the workgroup's slot of the
// workspace beyond.  The sequential law without a barrier per coordinate: every wave evaluates the same 64
// candidates from the position p against the current q (the four waves compute the same bits, so nothing has to be
// exchanged), the first lane whose new != w_i is the ballot's lowest bit, all 256 threads apply that one update to q,
// and the chunk is evaluated again from the coordinate after it.  A chunk without a change costs one pass and no
// barrier; a change costs two barriers.
#include "hsk_common.h"

#include <limits.h>
#include <math.h>

#define SLIM_THREADS 256
#define SLIM_WAVES (SLIM_THREADS / HSK_WAVE)
#define SLIM_LDS_CANDIDATES 4096   // hip_ops.SLIM_LDS_CANDIDATES: g, d, q, w and the ids take 144 KiB of the CU's 160
#define SLIM_GRID 256              // resident workgroups (one per CU); each owns one slot of the workspace
#define SLIM_SCRATCH 32            // doubles of reduction scratch behind the four arrays; the candidates' ids follow
#define SLIM_LDS_BYTES ((4 * SLIM_LDS_CANDIDATES + SLIM_SCRATCH) * 8 + SLIM_LDS_CANDIDATES * 4)

static inline int64_t slim_idx_bytes(int64_t n) { return hsk_align_up(n * 4, 256); }
static inline int64_t slim_slot_bytes(int64_t n) { return slim_idx_bytes(n) + hsk_align_up(4 * n * 8, 256); }
static inline int64_t slim_head_bytes(int64_t n) { return 256 + hsk_align_up(n * 8, 256); }

__global__ void __launch_bounds__(256) k_slim_diag(const double* __restrict__ G, int64_t n, int64_t ld,
                                                   double* __restrict__ diag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) diag[i] = G[i * ld + i];
}

__device__ __forceinline__ bool slim_finite(double v) { return fabs(v) < __builtin_inf(); }

__device__ __forceinline__ double slim_wave_max(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double o = __shfl_xor(v, off, HSK_WAVE);
    v = o > v ? o : v;
  }
  return v;
}

// sum (MAX = false) or maximum of v over the workgroup in a fixed order; every thread gets the result
template <bool MAX>
__device__ __forceinline__ double slim_block_reduce(double v, double* scratch, int wave, int lane) {
  v = MAX ? slim_wave_max(v) : hsk_wave_sum_f64(v);
  __syncthreads();   // the scratch of the previous reduction has been read
  if (lane == 0) scratch[wave] = v;
  __syncthreads();
  double r = scratch[0];
#pragma unroll
  for (int x = 1; x < SLIM_WAVES; ++x) r = MAX ? (scratch[x] > r ? scratch[x] : r) : r + scratch[x];
  return r;
}

// The solve of one column over its C compacted candidates: cg / cd / cq / cw are the candidates' g, d, q, w (LDS or the
// workspace), cidx their item ids.  Returns the sweep count; *gap_out the last gap evaluated.
__device__ __forceinline__ int slim_solve(const double* __restrict__ G, int64_t ld, const int32_t* cidx, int C,
                                          const double* cg, const double* cd, double* cq, double* cw, double yy,
                                          double l1, double l2, double tol, int max_iter, double* scratch,
                                          double* gap_out) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  double gap = 0.0;
  int it = 1;
  for (;; ++it) {
    double dmax = 0.0, wmax_l = 0.0;
    int p = 0;
    while (p < C) {
      const int c = p + lane;
      double old = 0.0, nw = 0.0;
      bool changed = false;
      if (c < C) {
        old = cw[c];
        const double d = cd[c];
        const double t = cg[c] - (cq[c] - d * old) - l1;
        nw = t > 0.0 ? t / (d + l2) : 0.0;
        changed = nw != old;
      }
      const unsigned long long mask = __ballot(changed);
      const int first = mask ? __builtin_ctzll(mask) : HSK_WAVE;
      if (c < C && lane <= first) {   // the coordinates this pass settles: unchanged ones and the first changed
        const double a = fabs(nw);
        wmax_l = a > wmax_l ? a : wmax_l;
      }
      if (!mask) {
        p += HSK_WAVE;
        continue;
      }
      const int ci = p + first;
      const double nwv = __shfl(nw, first, HSK_WAVE);
      const double delta = nwv - __shfl(old, first, HSK_WAVE);
      const double ad = fabs(delta);
      dmax = ad > dmax ? ad : dmax;
      __syncthreads();   // every wave has read q and w of this pass
      if (tid == first) cw[ci] = nwv;
      const double* row = G + (int64_t)cidx[ci] * ld;
      for (int k = tid; k < C; k += SLIM_THREADS) cq[k] = cq[k] + delta * row[cidx[k]];
      __syncthreads();
      p = ci + 1;
    }
    const double wmax = slim_wave_max(wmax_l);
    const bool last = it >= max_iter;
    if (!(wmax == 0.0 || dmax <= tol * wmax || last)) continue;
    // sklearn's duality gap
    double s_wg = 0.0, s_wq = 0.0, s_w = 0.0, s_ww = 0.0, s_max = -__builtin_inf();
    for (int k = tid; k < C; k += SLIM_THREADS) {
      const double w = cw[k], g = cg[k], q = cq[k];
      s_wg = s_wg + w * g;
      s_wq = s_wq + w * q;
      s_w = s_w + w;
      s_ww = s_ww + w * w;
      const double s = g - q - l2 * w;
      s_max = s > s_max ? s : s_max;
    }
    const double wg = slim_block_reduce<false>(s_wg, scratch, wave, lane);
    const double wq = slim_block_reduce<false>(s_wq, scratch, wave, lane);
    const double sw = slim_block_reduce<false>(s_w, scratch, wave, lane);
    const double ww = slim_block_reduce<false>(s_ww, scratch, wave, lane);
    const double D = slim_block_reduce<true>(s_max, scratch, wave, lane);
    const double R2 = yy - 2.0 * wg + wq;
    const double Ry = yy - wg;
    double cc = 1.0;
    if (D > l1) {
      cc = l1 / D;
      gap = 0.5 * R2 * (1.0 + cc * cc);
    } else {
      gap = R2;
    }
    gap = gap + (l1 * sw - cc * Ry + 0.5 * l2 * (1.0 + cc * cc) * ww);
    if (last || (tol > 0.0 && gap <= tol * yy) || (tol == 0.0 && dmax == 0.0)) break;
  }
  *gap_out = gap;
  return it;
}

__global__ void __launch_bounds__(SLIM_THREADS) k_slim_cd(const double* __restrict__ G, int64_t n, int64_t ld,
                                                          int64_t j0, int64_t j1, double l1, double l2, double tol,
                                                          int max_iter, const double* __restrict__ diag,
                                                          unsigned int* __restrict__ counter, char* __restrict__ slots,
                                                          int64_t slot_bytes, int64_t idx_bytes, double* __restrict__ Wt,
                                                          int64_t ldw, int32_t* __restrict__ n_iter,
                                                          double* __restrict__ gap_out, int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* sg = lds;
  double* sd = sg + SLIM_LDS_CANDIDATES;
  double* sq = sd + SLIM_LDS_CANDIDATES;
  double* sw = sq + SLIM_LDS_CANDIDATES;
  double* scratch = sw + SLIM_LDS_CANDIDATES;                      // SLIM_WAVES doubles of the reductions
  int* wcount = reinterpret_cast<int*>(scratch + SLIM_WAVES);      // SLIM_WAVES ints of the compaction
  unsigned int* next = reinterpret_cast<unsigned int*>(scratch + 2 * SLIM_WAVES);
  int32_t* sidx = reinterpret_cast<int32_t*>(scratch + SLIM_SCRATCH);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  char* slot = slots + (int64_t)blockIdx.x * slot_bytes;
  int32_t* cidx = reinterpret_cast<int32_t*>(slot);
  double* gg = reinterpret_cast<double*>(slot + idx_bytes);        // the four arrays of a column beyond the LDS
  double* gd = gg + n;
  double* gq = gd + n;
  double* gw = gq + n;
  const int64_t cols = j1 - j0;
  bool bad = false;
  for (;;) {
    __syncthreads();   // `next` and the slot of the previous column have been read
    if (tid == 0) *next = atomicAdd(counter, 1u);
    __syncthreads();
    const int64_t t = *next;
    if (t >= cols) break;
    const int64_t j = j0 + t;
    const double* grow = G + j * ld;
    // the candidates of column j, ascending
    int C = 0;
    for (int64_t base = 0; base < n; base += SLIM_THREADS) {
      const int64_t i = base + tid;
      bool keep = false;
      if (i < n) {
        const double g = grow[i], d = diag[i];
        bad |= !slim_finite(g) || !slim_finite(d);
        keep = i != j && d > 0.0 && g > l1;
      }
      const unsigned long long mask = __ballot(keep);
      if (lane == 0) wcount[wave] = __popcll(mask);
      __syncthreads();
      int at = C, total = 0;
#pragma unroll
      for (int x = 0; x < SLIM_WAVES; ++x) {
        if (x < wave) at += wcount[x];
        total += wcount[x];
      }
      if (keep) cidx[at + __popcll(mask & ((1ull << lane) - 1ull))] = (int32_t)i;
      C += total;
      __syncthreads();   // wcount is free again; after the last round cidx is visible to the workgroup
    }
    const bool in_lds = C <= SLIM_LDS_CANDIDATES;
    double* cg = in_lds ? sg : gg;
    double* cd = in_lds ? sd : gd;
    double* cq = in_lds ? sq : gq;
    double* cw = in_lds ? sw : gw;
    for (int k = tid; k < C; k += SLIM_THREADS) {
      const int32_t i = cidx[k];
      if (in_lds) sidx[k] = i;
      cg[k] = grow[i];
      cd[k] = diag[i];
      cq[k] = 0.0;
      cw[k] = 0.0;
    }
    double* wrow = Wt + j * ldw;
    for (int64_t i = tid; i < n; i += SLIM_THREADS) wrow[i] = 0.0;
    __syncthreads();
    const double yy = grow[j];
    double gap;
    int it;
    if (in_lds)
      it = slim_solve(G, ld, sidx, C, sg, sd, sq, sw, yy, l1, l2, tol, max_iter, scratch, &gap);
    else
      it = slim_solve(G, ld, cidx, C, gg, gd, gq, gw, yy, l1, l2, tol, max_iter, scratch, &gap);
    __syncthreads();
    for (int k = tid; k < C; k += SLIM_THREADS) {
      const double w = cw[k];
      bad |= !slim_finite(w);
      wrow[cidx[k]] = w;
    }
    if (tid == 0) {
      bad |= !slim_finite(gap);
      n_iter[j] = it;
      gap_out[j] = gap;
    }
  }
  if (bad) atomicOr(status, HSK_STATUS_NOT_FINITE);
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" int64_t hsk_slim_lds_candidates(void) { return SLIM_LDS_CANDIDATES; }

extern "C" int64_t hsk_slim_cd_ws_bytes(int64_t n) {
  if (n <= 0 || n >= INT_MAX) return 0;
  return slim_head_bytes(n) + SLIM_GRID * slim_slot_bytes(n);
}

extern "C" int hsk_slim_cd_f64(const double* G, int64_t n, int64_t ld, int64_t j0, int64_t j1, double l1, double l2,
                               double tol, int64_t max_iter, double* Wt, int64_t ldw, int32_t* n_iter, double* gap,
                               void* workspace, int64_t workspace_bytes, int32_t* status, hsk_stream_t stream) {
  HSK_REQUIRE(G && Wt && n_iter && gap && workspace && status, HSK_ERR_INVALID, "hsk_slim_cd_f64: null pointer");
  HSK_REQUIRE(n > 0 && n < INT_MAX && ld >= n && ldw >= n, HSK_ERR_INVALID,
              "hsk_slim_cd_f64: bad shape n %lld ld %lld ldw %lld", (long long)n, (long long)ld, (long long)ldw);
  HSK_REQUIRE(j0 >= 0 && j0 < j1 && j1 <= n, HSK_ERR_INVALID,
              "hsk_slim_cd_f64: column range [%lld, %lld) outside [0, %lld)", (long long)j0, (long long)j1, (long long)n);
  HSK_REQUIRE(max_iter >= 1 && max_iter < INT_MAX, HSK_ERR_INVALID, "hsk_slim_cd_f64: max_iter %lld below 1",
              (long long)max_iter);
  HSK_REQUIRE(std::isfinite(l1) && l1 >= 0.0 && std::isfinite(l2) && l2 >= 0.0 && std::isfinite(tol) && tol >= 0.0,
              HSK_ERR_INVALID, "hsk_slim_cd_f64: l1 %g, l2 %g, tol %g must be finite and >= 0", l1, l2, tol);
  HSK_REQUIRE(workspace_bytes >= hsk_slim_cd_ws_bytes(n), HSK_ERR_INVALID,
              "hsk_slim_cd_f64: workspace of %lld bytes, needs %lld", (long long)workspace_bytes,
              (long long)hsk_slim_cd_ws_bytes(n));
  HSK_REQUIRE(((uintptr_t)workspace & 255) == 0, HSK_ERR_INVALID, "hsk_slim_cd_f64: workspace not 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  unsigned int* counter = (unsigned int*)ws;
  double* diag = (double*)(ws + 256);
  char* slots = ws + slim_head_bytes(n);
  HSK_HIP(hipMemsetAsync(counter, 0, 256, s));
  k_slim_diag<<<(unsigned)hsk_ceil_div(n, 256), 256, 0, s>>>(G, n, ld, diag);
  HSK_LAUNCH_CHECK();
  const int lds_bytes = SLIM_LDS_BYTES;
  HSK_HIP(hipFuncSetAttribute((const void*)k_slim_cd, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
  const int64_t cols = j1 - j0;
  const unsigned grid = (unsigned)(cols < SLIM_GRID ? cols : SLIM_GRID);
  k_slim_cd<<<grid, SLIM_THREADS, lds_bytes, s>>>(G, n, ld, j0, j1, l1, l2, tol, (int)max_iter, diag, counter, slots,
                                                 slim_slot_bytes(n), slim_idx_bytes(n), Wt, ldw, n_iter, gap, status);
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}
