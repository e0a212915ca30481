// hsk_knn.hip -- ItemKNN / UserKNN (reference algorithms/knn_algs.py, utilities/similarities.py): int8 pack of a binary
// CSR, exact int32 Gram on v_mfma_i32_32x32x32_i8, fp64 similarity + top-k neighbours, fp64 sparse scoring and the
// fp64 top-k of the evaluation.  DESIGN.md section 5 ("KNN") states the exactness argument.
//
// Gram geometry: a workgroup of four waves (one per SIMD) owns 128 x 128 outputs, wave (wm, wn) the 64 x 64 block at
// (64 wm, 64 wn) in 2 x 2 accumulator tiles of 32 x 32.  A k-step is 64 bytes deep (two MFMA k32 steps); both operands
// are rows of the same entity-major int8 matrix M, staged global -> registers -> LDS one step ahead in a double buffer
// of [128 rows][64 B + 16 B pad] images.  A and B fragments take the same k bytes of their rows, so the k order inside a
// fragment (whatever the instruction's lane map is) is the same on both sides and the dot product is exact.
#include "hsk_common.h"

#include <limits.h>

#define KNN_TILE 128
#define KNN_BK 64
#define KNN_LDS_ROW 80                            // 64 data bytes + 16 pad: consecutive rows start 20 banks apart
#define KNN_IMAGE (KNN_TILE * KNN_LDS_ROW)        // 10 240 bytes: one operand, one stage
#define KNN_SEL_CAP 4096                          // candidates sorted in LDS per row
#define KNN_SEL_THREADS 256

typedef int hsk_k_i32x4 __attribute__((ext_vector_type(4)));
typedef int hsk_k_i32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------
// pack: binary CSR -> dense int8 [rows_pad, k_pad] (zeros were written by the caller's memset)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_knn_pack(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                  int64_t n_rows, int64_t n_cols, int64_t k_pad, int8_t* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n_rows) return;
  for (int64_t e = indptr[r] + hsk_lane(); e < indptr[r + 1]; e += HSK_WAVE) {
    const int64_t c = indices[e];
    if (c >= 0 && c < n_cols) out[r * k_pad + c] = 1;
  }
}

// ---------------------------------------------------------------------------------------------
// Gram: C[r - r0, c] = sum_k M[r, k] M[c, k] for r in [r0, r1), c in [0, n_rows)
// ---------------------------------------------------------------------------------------------
struct knn_stage {
  hsk_k_i32x4 a[2], b[2];
};

__device__ __forceinline__ void knn_gload(knn_stage& s, const int8_t* __restrict__ M, int64_t k_pad, int64_t m0,
                                          int64_t n0, int kt, int tid) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int c = tid + 256 * q, row = c >> 2, col = (c & 3) * 16;
    s.a[q] = *reinterpret_cast<const hsk_k_i32x4*>(M + (m0 + row) * k_pad + (int64_t)kt * KNN_BK + col);
    s.b[q] = *reinterpret_cast<const hsk_k_i32x4*>(M + (n0 + row) * k_pad + (int64_t)kt * KNN_BK + col);
  }
}
__device__ __forceinline__ void knn_sstore(const knn_stage& s, unsigned char* stage, int tid) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int c = tid + 256 * q, off = (c >> 2) * KNN_LDS_ROW + (c & 3) * 16;
    *reinterpret_cast<hsk_k_i32x4*>(stage + off) = s.a[q];
    *reinterpret_cast<hsk_k_i32x4*>(stage + KNN_IMAGE + off) = s.b[q];
  }
}

__global__ void __launch_bounds__(256) k_knn_gram_i8(const int8_t* __restrict__ M, int64_t n_rows, int64_t k_pad,
                                                     int64_t r0, int64_t r1, int32_t* __restrict__ C, int64_t ldc) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * 2 * KNN_IMAGE];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t m0 = r0 + (int64_t)blockIdx.y * KNN_TILE, n0 = (int64_t)blockIdx.x * KNN_TILE;
  const int NK = (int)(k_pad / KNN_BK);
  hsk_k_i32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[i][j][v] = 0;
  knn_stage s;
  knn_gload(s, M, k_pad, m0, n0, 0, tid);
  knn_sstore(s, lds, tid);
  __syncthreads();
  for (int kt = 0; kt < NK; ++kt) {
    const bool more = kt + 1 < NK;
    if (more) knn_gload(s, M, k_pad, m0, n0, kt + 1, tid);
    const unsigned char* rd = lds + (kt & 1) * 2 * KNN_IMAGE;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      hsk_k_i32x4 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        a[i] = *reinterpret_cast<const hsk_k_i32x4*>(rd + (wm * 64 + i * 32 + r) * KNN_LDS_ROW + ks * 32 + h * 16);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        b[j] = *reinterpret_cast<const hsk_k_i32x4*>(rd + KNN_IMAGE + (wn * 64 + j * 32 + r) * KNN_LDS_ROW + ks * 32 +
                                                     h * 16);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (more) knn_sstore(s, lds + ((kt + 1) & 1) * 2 * KNN_IMAGE, tid);
    __syncthreads();
  }
  // C/D map of the 32 x 32 forms: column = lane & 31, row = (v & 3) + 8 (v >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t gc = n0 + wn * 64 + j * 32 + r;
      if (gc >= n_rows) continue;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int64_t gr = m0 + wm * 64 + i * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
        if (gr < r1) C[(gr - r0) * ldc + gc] = acc[i][j][v];
      }
    }
}

// ---------------------------------------------------------------------------------------------
// fp64 top-k of one row per workgroup, order (value desc, index asc)
// ---------------------------------------------------------------------------------------------
// monotone 64-bit key of a double: larger double <=> larger key
__device__ __forceinline__ uint64_t knn_key(double v) {
  const uint64_t u = (uint64_t)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | (1ull << 63));
}
__device__ __forceinline__ double knn_unkey(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}
__device__ __forceinline__ bool knn_before(uint64_t ka, int ia, uint64_t kb, int ib) {
  return ka > kb || (ka == kb && ia < ib);
}

struct knn_sel_smem {
  uint64_t key[KNN_SEL_CAP];
  int idx[KNN_SEL_CAP];
  int hist[256];
  int wsum[KNN_SEL_THREADS / HSK_WAVE];
  uint64_t prefix;
  int pbits, above, need, done, nb, na;
};

// GET(c, key&) -> valid.  Radix select on the key, 8 bits per pass from the top, until the elements above the chosen
// prefix plus those on it fit KNN_SEL_CAP (or all 64 bits are fixed: then every element on the prefix has one value and
// the lowest indices are kept); those are collected -- the prefix ones in index order -- and bitonic-sorted in LDS.
template <class GET>
__device__ void knn_block_topk(GET get, int n, int k, knn_sel_smem& sm, int& m_out) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    sm.prefix = 0;
    sm.pbits = 0;
    sm.above = 0;
    sm.need = k;
    sm.done = 0;
  }
  __syncthreads();
  for (;;) {
    const uint64_t prefix = sm.prefix;
    const int pbits = sm.pbits;
    for (int d = tid; d < 256; d += KNN_SEL_THREADS) sm.hist[d] = 0;
    __syncthreads();
    for (int c = tid; c < n; c += KNN_SEL_THREADS) {
      uint64_t key;
      if (!get(c, key)) continue;
      if (pbits > 0 && (key >> (64 - pbits)) != prefix) continue;
      atomicAdd(&sm.hist[(int)((key >> (56 - pbits)) & 255)], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int total = 0;
      for (int d = 0; d < 256; ++d) total += sm.hist[d];
      if (pbits == 0 && total <= KNN_SEL_CAP) {
        sm.done = 1;
      } else {
        int cum = 0, d = 255;
        for (; d > 0; --d) {
          if (cum + sm.hist[d] >= sm.need) break;
          cum += sm.hist[d];
        }
        sm.above += cum;
        sm.need -= cum;
        sm.prefix = (prefix << 8) | (uint64_t)d;
        sm.pbits = pbits + 8;
        if (sm.above + sm.hist[d] <= KNN_SEL_CAP || sm.pbits == 64) sm.done = 1;
      }
    }
    __syncthreads();
    if (sm.done) break;
  }
  // collect: elements above the prefix in any order (fewer than k of them), the prefix's own in index order
  const uint64_t prefix = sm.prefix;
  const int pbits = sm.pbits, above = sm.above;
  if (tid == 0) {
    sm.nb = 0;
    sm.na = 0;
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  for (int base = 0; base < n; base += KNN_SEL_THREADS) {
    const int c = base + tid;
    uint64_t key = 0;
    bool on = false;
    if (c < n && get(c, key)) {
      const uint64_t top = pbits > 0 ? (key >> (64 - pbits)) : 0;
      if (pbits > 0 && top > prefix) {
        const int slot = atomicAdd(&sm.na, 1);
        sm.key[slot] = key;
        sm.idx[slot] = c;
      } else if (pbits == 0 || top == prefix) {
        on = true;
      }
    }
    const uint64_t bal = __ballot(on);
    if (lane == 0) sm.wsum[wave] = __popcll(bal);
    __syncthreads();
    int off = sm.nb;
    for (int w = 0; w < wave; ++w) off += sm.wsum[w];
    const int pos = above + off + __popcll(bal & ((1ull << lane) - 1));
    if (on && pos < KNN_SEL_CAP) {
      sm.key[pos] = key;
      sm.idx[pos] = c;
    }
    __syncthreads();
    if (tid == 0) {
      int t = 0;
      for (int w = 0; w < KNN_SEL_THREADS / HSK_WAVE; ++w) t += sm.wsum[w];
      sm.nb += t;
    }
    __syncthreads();
  }
  const int m = min(KNN_SEL_CAP, above + sm.nb);
  int P = 1;
  while (P < m) P <<= 1;
  for (int t = m + tid; t < P; t += KNN_SEL_THREADS) {
    sm.key[t] = 0;
    sm.idx[t] = INT_MAX;
  }
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (P >> 1); t += KNN_SEL_THREADS) {
        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
        const bool up = (i & size) == 0;
        const uint64_t ki = sm.key[i], kj = sm.key[j];
        const int ii = sm.idx[i], ij = sm.idx[j];
        if (up ? knn_before(kj, ij, ki, ii) : knn_before(ki, ii, kj, ij)) {
          sm.key[i] = kj;
          sm.key[j] = ki;
          sm.idx[i] = ij;
          sm.idx[j] = ii;
        }
      }
      __syncthreads();
    }
  m_out = m;
}

// ---------------------------------------------------------------------------------------------
// similarity of a count block + k neighbours per row (utilities/similarities.py:18-111)
// ---------------------------------------------------------------------------------------------
struct knn_sim_args {
  const int32_t* C;
  int64_t ldc, n, row0;
  const int64_t* deg;
  const double *sq, *pa, *p1a;
  int kind;
  double alpha, beta, shrink;
};

// the reference's expressions in its operation order, with nothing contracted into an FMA
__device__ __forceinline__ double knn_sim(const knn_sim_args& a, int64_t r, int64_t c, int cnt) {
#pragma clang fp contract(off)
  const double cd = (double)cnt;
  const int64_t dr = a.deg[r], dc = a.deg[c];
  double v;
  switch (a.kind) {
    case HSK_KNN_COSINE: v = cd / (a.sq[r] * a.sq[c]); break;
    case HSK_KNN_JACCARD: v = cd / (double)(dr + dc - (int64_t)cnt); break;
    case HSK_KNN_SORENSEN_DICE: v = cd / (double)(dr + dc); v = v * 2.0; break;
    case HSK_KNN_ASYMMETRIC_COSINE: v = cd / (a.pa[r] * a.p1a[c]); break;
    default: v = cd / (cd + a.alpha * (double)(dr - (int64_t)cnt) + a.beta * (double)(dc - (int64_t)cnt)); break;
  }
  const double f = cd / (cd + a.shrink);
  return v * f;
}

__global__ void __launch_bounds__(KNN_SEL_THREADS) k_knn_select(knn_sim_args a, int64_t rows, int k,
                                                                int32_t* __restrict__ out_idx, double* __restrict__ out_val,
                                                                int32_t* __restrict__ out_len) {
  __shared__ knn_sel_smem sm;
  const int64_t rl = blockIdx.x;
  const int64_t r = a.row0 + rl;
  const int32_t* crow = a.C + rl * a.ldc;
  auto get = [&](int c, uint64_t& key) -> bool {
    const int cnt = crow[c];
    if (cnt <= 0 || c == r) return false;
    key = knn_key(knn_sim(a, r, c, cnt));
    return true;
  };
  int m;
  knn_block_topk(get, (int)a.n, k, sm, m);
  const int len = min(m, k);
  for (int t = threadIdx.x; t < k; t += KNN_SEL_THREADS) {
    out_idx[rl * k + t] = t < len ? sm.idx[t] : -1;
    out_val[rl * k + t] = t < len ? knn_unkey(sm.key[t]) : 0.0;
  }
  if (threadIdx.x == 0) out_len[rl] = len;
}

// ---------------------------------------------------------------------------------------------
// scoring: out[q, j] = sum over A-row u = users[q], in stored order, of w_a * B[r, j]; one wave per (user, item window)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_knn_score(const int64_t* __restrict__ users, int64_t n_a_rows,
                                                  const int64_t* __restrict__ a_ptr, const int32_t* __restrict__ a_idx,
                                                  const double* __restrict__ a_val, int64_t n_b_rows,
                                                  const int64_t* __restrict__ b_ptr, const int32_t* __restrict__ b_idx,
                                                  const double* __restrict__ b_val, int64_t n_cols, int64_t window,
                                                  const int64_t* __restrict__ x_ptr, const int32_t* __restrict__ x_idx,
                                                  double* __restrict__ out, int64_t ld, int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  extern __shared__ double acc[];
  const int lane = threadIdx.x;
  const int64_t q = blockIdx.y, w0 = (int64_t)blockIdx.x * window;
  const int wlen = (int)min(window, n_cols - w0);
  int64_t u = users[q];
  if (u < 0 || u >= n_a_rows) {
    if (lane == 0) atomicOr(status, HSK_STATUS_BAD_INDEX);
    u = 0;
  }
  for (int t = lane; t < wlen; t += HSK_WAVE) acc[t] = 0.0;
  for (int64_t e = a_ptr[u]; e < a_ptr[u + 1]; ++e) {
    const int32_t r = a_idx[e];
    if (r < 0 || r >= n_b_rows) continue;
    const double wa = a_val ? a_val[e] : 1.0;
    for (int64_t f = b_ptr[r] + lane; f < b_ptr[r + 1]; f += HSK_WAVE) {
      const int64_t j = (int64_t)b_idx[f] - w0;   // a B-row's columns are distinct: no two lanes meet
      if (j >= 0 && j < wlen) acc[j] = acc[j] + wa * (b_val ? b_val[f] : 1.0);
    }
    __builtin_amdgcn_wave_barrier();   // one wave, LDS in program order: each accumulator adds in A's stored order
  }
  if (x_ptr) {
    for (int64_t f = x_ptr[u] + lane; f < x_ptr[u + 1]; f += HSK_WAVE) {
      const int64_t j = (int64_t)x_idx[f] - w0;
      if (j >= 0 && j < wlen) acc[j] = -__builtin_inf();
    }
    __builtin_amdgcn_wave_barrier();
  }
  for (int t = lane; t < wlen; t += HSK_WAVE) out[q * ld + w0 + t] = acc[t];
}

__global__ void __launch_bounds__(KNN_SEL_THREADS) k_knn_topk_rows(const double* __restrict__ scores, int64_t n_cols,
                                                                   int64_t ld, int k, double* __restrict__ out_vals,
                                                                   int32_t* __restrict__ out_idx) {
  __shared__ knn_sel_smem sm;
  const int64_t q = blockIdx.x;
  const double* row = scores + q * ld;
  auto get = [&](int c, uint64_t& key) -> bool {
    key = knn_key(row[c]);
    return true;
  };
  int m;
  knn_block_topk(get, (int)n_cols, k, sm, m);
  for (int t = threadIdx.x; t < k; t += KNN_SEL_THREADS) {
    out_idx[q * k + t] = sm.idx[t];
    out_vals[q * k + t] = knn_unkey(sm.key[t]);
  }
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" int hsk_knn_pack_dims(int64_t n_rows, int64_t n_cols, int64_t* rows_pad, int64_t* k_pad) {
  HSK_REQUIRE(n_rows > 0 && n_cols > 0 && n_rows < INT_MAX && n_cols < INT_MAX, HSK_ERR_INVALID,
              "hsk_knn_pack_dims: bad shape %lld x %lld", (long long)n_rows, (long long)n_cols);
  HSK_REQUIRE(rows_pad && k_pad, HSK_ERR_INVALID, "hsk_knn_pack_dims: null output");
  *rows_pad = hsk_align_up(n_rows, KNN_TILE);
  *k_pad = hsk_align_up(n_cols, KNN_BK);
  return HSK_OK;
}

extern "C" int hsk_knn_pack_i8(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols,
                               int64_t rows_pad, int64_t k_pad, int8_t* out, hsk_stream_t stream) {
  HSK_REQUIRE(indptr && indices && out, HSK_ERR_INVALID, "hsk_knn_pack_i8: null pointer");
  HSK_REQUIRE(n_rows > 0 && n_cols > 0 && rows_pad >= n_rows && rows_pad % KNN_TILE == 0 && k_pad >= n_cols &&
                  k_pad % KNN_BK == 0,
              HSK_ERR_INVALID, "hsk_knn_pack_i8: bad shape (rows %lld pad %lld, cols %lld pad %lld)", (long long)n_rows,
              (long long)rows_pad, (long long)n_cols, (long long)k_pad);
  hipStream_t s = (hipStream_t)stream;
  HSK_HIP(hipMemsetAsync(out, 0, (size_t)rows_pad * (size_t)k_pad, s));
  k_knn_pack<<<(unsigned)hsk_ceil_div(n_rows, 4), 256, 0, s>>>(indptr, indices, n_rows, n_cols, k_pad, out);
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}

extern "C" int hsk_knn_gram_i8(const int8_t* M, int64_t n_rows, int64_t rows_pad, int64_t k_pad, int64_t r0, int64_t r1,
                               int32_t* C, int64_t ldc, hsk_stream_t stream) {
  HSK_REQUIRE(M && C, HSK_ERR_INVALID, "hsk_knn_gram_i8: null pointer");
  HSK_REQUIRE(n_rows > 0 && rows_pad >= n_rows && rows_pad % KNN_TILE == 0 && k_pad > 0 && k_pad % KNN_BK == 0,
              HSK_ERR_INVALID, "hsk_knn_gram_i8: bad operand shape");
  HSK_REQUIRE(r0 >= 0 && r0 % KNN_TILE == 0 && r1 > r0 && r1 <= n_rows && ldc >= n_rows, HSK_ERR_INVALID,
              "hsk_knn_gram_i8: bad row block [%lld, %lld) (r0 must be a multiple of %d) or ldc %lld", (long long)r0,
              (long long)r1, KNN_TILE, (long long)ldc);
  dim3 grid((unsigned)hsk_ceil_div(n_rows, KNN_TILE), (unsigned)hsk_ceil_div(r1 - r0, KNN_TILE));
  k_knn_gram_i8<<<grid, 256, 0, (hipStream_t)stream>>>(M, n_rows, k_pad, r0, r1, C, ldc);
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}

extern "C" int hsk_knn_select(const int32_t* C, int64_t rows, int64_t n, int64_t ldc, int64_t row0, const int64_t* deg,
                              const double* sqrt_deg, const double* deg_alpha, const double* deg_1m_alpha, int32_t kind,
                              double alpha, double beta, double shrinkage, int64_t k, int32_t* out_idx, double* out_val,
                              int32_t* out_len, hsk_stream_t stream) {
  HSK_REQUIRE(C && deg && out_idx && out_val && out_len, HSK_ERR_INVALID, "hsk_knn_select: null pointer");
  HSK_REQUIRE(kind >= HSK_KNN_COSINE && kind <= HSK_KNN_TVERSKY, HSK_ERR_INVALID, "hsk_knn_select: unknown kind %d",
              (int)kind);
  HSK_REQUIRE(kind != HSK_KNN_COSINE || sqrt_deg, HSK_ERR_INVALID, "hsk_knn_select: cosine needs sqrt_deg");
  HSK_REQUIRE(kind != HSK_KNN_ASYMMETRIC_COSINE || (deg_alpha && deg_1m_alpha), HSK_ERR_INVALID,
              "hsk_knn_select: asymmetric cosine needs deg^alpha and deg^(1-alpha)");
  HSK_REQUIRE(k >= 1 && k <= HSK_KNN_MAX_K, HSK_ERR_UNSUPPORTED, "hsk_knn_select: k = %lld outside [1, %d]",
              (long long)k, HSK_KNN_MAX_K);
  HSK_REQUIRE(rows > 0 && n > 0 && n < INT_MAX && ldc >= n && row0 >= 0 && row0 + rows <= n, HSK_ERR_INVALID,
              "hsk_knn_select: bad block shape");
  knn_sim_args a{C, ldc, n, row0, deg, sqrt_deg, deg_alpha, deg_1m_alpha, (int)kind, alpha, beta, shrinkage};
  k_knn_select<<<(unsigned)rows, KNN_SEL_THREADS, 0, (hipStream_t)stream>>>(a, rows, (int)k, out_idx, out_val, out_len);
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}

extern "C" int hsk_knn_score_rows(const int64_t* users, int64_t n_users, int64_t n_a_rows, const int64_t* a_indptr,
                                  const int32_t* a_indices, const double* a_vals, int64_t n_b_rows,
                                  const int64_t* b_indptr, const int32_t* b_indices, const double* b_vals, int64_t n_cols,
                                  int64_t window, const int64_t* excl_indptr, const int32_t* excl_indices, double* out,
                                  int64_t ld, int32_t* status, hsk_stream_t stream) {
  HSK_REQUIRE(users && a_indptr && a_indices && b_indptr && b_indices && out && status, HSK_ERR_INVALID,
              "hsk_knn_score_rows: null pointer");
  HSK_REQUIRE((excl_indptr == nullptr) == (excl_indices == nullptr), HSK_ERR_INVALID,
              "hsk_knn_score_rows: exclude CSR needs both arrays");
  HSK_REQUIRE(n_users > 0 && n_users < (1ll << 31) && n_a_rows > 0 && n_b_rows > 0 && n_cols > 0 && ld >= n_cols,
              HSK_ERR_INVALID, "hsk_knn_score_rows: bad shape");
  HSK_REQUIRE(window >= 1 && window <= HSK_KNN_MAX_WINDOW, HSK_ERR_INVALID,
              "hsk_knn_score_rows: window %lld outside [1, %d]", (long long)window, HSK_KNN_MAX_WINDOW);
  const int64_t wlen = window < n_cols ? window : n_cols;
  const int64_t nw = hsk_ceil_div(n_cols, wlen);
  HSK_REQUIRE(nw < (1ll << 31), HSK_ERR_INVALID, "hsk_knn_score_rows: too many windows");
  if (wlen * (int64_t)sizeof(double) > 65536)
    HSK_HIP(hipFuncSetAttribute((const void*)k_knn_score, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(wlen * (int64_t)sizeof(double))));
  k_knn_score<<<dim3((unsigned)nw, (unsigned)n_users), 64, (size_t)wlen * sizeof(double), (hipStream_t)stream>>>(
      users, n_a_rows, a_indptr, a_indices, a_vals, n_b_rows, b_indptr, b_indices, b_vals, n_cols, wlen, excl_indptr,
      excl_indices, out, ld, status);
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}

extern "C" int hsk_knn_topk_rows(const double* scores, int64_t rows, int64_t n_cols, int64_t ld, int64_t k,
                                 double* out_vals, int32_t* out_idx, hsk_stream_t stream) {
  HSK_REQUIRE(scores && out_vals && out_idx, HSK_ERR_INVALID, "hsk_knn_topk_rows: null pointer");
  HSK_REQUIRE(k >= 1 && k <= HSK_KNN_MAX_K && k <= n_cols, HSK_ERR_UNSUPPORTED,
              "hsk_knn_topk_rows: k = %lld outside [1, min(%d, n_cols = %lld)]", (long long)k, HSK_KNN_MAX_K,
              (long long)n_cols);
  HSK_REQUIRE(rows > 0 && rows < (1ll << 31) && n_cols < INT_MAX && ld >= n_cols, HSK_ERR_INVALID,
              "hsk_knn_topk_rows: bad shape");
  k_knn_topk_rows<<<(unsigned)rows, KNN_SEL_THREADS, 0, (hipStream_t)stream>>>(scores, n_cols, ld, (int)k, out_vals,
                                                                               out_idx);
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}
