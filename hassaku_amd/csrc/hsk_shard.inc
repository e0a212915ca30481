// hsk_shard.inc -- multi-GPU phases of the fused step (included by hsk_fused.hip; protocol in hassaku_hip.h).
// Items range-sharded (with their AdamW moments), users row-sharded (owner = u % world, local row = u / world).
// Every rank draws the whole global batch's negatives from the same Philox stream and keeps the entries whose item
// it owns; user rows travel by all_gather, their gradients by reduce_scatter; item gradients never leave the rank.

// ---------------------------------------------------------------------------------------------
// extra scratch of the sharded step (per buffer set where the next batch may be prepared a step ahead)
// ---------------------------------------------------------------------------------------------
#define HSK_SHARD_CHUNK 1024        // positives per workgroup of k_shard_count / k_shard_place
#define HSK_SHARD_MAX_CHUNKS 64     // global batches of up to 65 536 positives
struct hsk_shard_ws {
  int* pos_local[2];   // [G]   local id of the positive item if this rank owns it, else -1
  int* offs[2];        // [G+1] kept entries of positive b: [offs[b], offs[b+1])
  int* slot_of_b[2];   // [G]   row of the positive's user in rows_all / dU_all
  int* req[2];         // [C]   local user row requested through slot s of this rank's segment, -1 = unused
  int* erow[2];        // [cap] per kept entry: slot_of_b of its positive (the item pass gathers user rows by entry)
  int* n_entries[2];   // [1]   number of kept entries
  int* wg_tot[2];      // [64]  kept entries per chunk of 1024 positives (k_shard_count -> k_shard_place)
  int* own_cnt[2];     // [64*64] positives per (chunk, owner rank)
  int* ovf[2];         // [1]   != 0: the batch prepared in this set exceeded a capacity (k_shard_place) -- its step must
                       //       not write a table
  int* poison;         // [1]   != 0: a step has been skipped for that reason; sticky: no later step writes a table either
  int* tmp_pad;        // [G*K] kept entries before compaction, stride K
  int64_t total;
};

static hsk_shard_ws hsk_shard_carve(void* base, int64_t G, int64_t K, int64_t C, int64_t cap) {
  hsk_shard_ws w;
  char* p = (char*)base;
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char* r = p ? p + off : nullptr;
    off += hsk_align_up(bytes, 256);
    return (int*)r;
  };
  for (int s = 0; s < 2; ++s) {
    w.pos_local[s] = take(G * 4);
    w.offs[s] = take((G + 1) * 4);
    w.slot_of_b[s] = take(G * 4);
    w.req[s] = take(C * 4);
    w.erow[s] = take(cap * 4);
    w.n_entries[s] = take(256);
    w.wg_tot[s] = take(HSK_SHARD_MAX_CHUNKS * 4);
    w.own_cnt[s] = take(HSK_SHARD_MAX_CHUNKS * 64 * 4);
    w.ovf[s] = take(256);
  }
  w.poison = take(256);
  w.tmp_pad = take(G * K * 4);
  w.total = off;
  return w;
}

// The layout is a function of the state's LIMITS (base.max_batch, base.max_cols), never of the shape of one step: a
// ragged last batch and the full batch prepared a step ahead share this buffer.
extern "C" int64_t hsk_shard_workspace_bytes(int64_t max_batch, int64_t max_cols, int64_t capacity, int64_t entry_cap) {
  if (max_batch < 1 || max_cols < 2 || capacity < 1 || entry_cap < 1) return -1;
  if (max_batch * max_cols >= 0x7fffffff) return -1;
  return hsk_shard_carve(nullptr, max_batch, max_cols, capacity, entry_cap).total;
}

// ---------------------------------------------------------------------------------------------
// prepare: sample + keep, scan, route, compact (+ the item sort and the owner map of hsk_fused.hip)
// ---------------------------------------------------------------------------------------------
// One wave per positive of the GLOBAL batch.  Draws exactly what k_prep_sample draws (counter = global batch position,
// column, attempt), keeps the entries with item in [item_lo, item_lo + n_loc): the positive first (if owned), then the
// owned negatives in column order.  cnt_out[b] = number kept.
__global__ __launch_bounds__(256) void k_shard_sample(const int32_t* __restrict__ coo_user,
                                                      const int32_t* __restrict__ coo_item,
                                                      const int64_t* __restrict__ order, long long start, int G,
                                                      int n_neg, const int64_t* __restrict__ csr_indptr,
                                                      const int32_t* __restrict__ csr_indices, int n_items_global,
                                                      int item_lo, int n_loc, uint64_t seed, uint64_t stream_id,
                                                      int* __restrict__ ug, int* __restrict__ pos_local,
                                                      int* __restrict__ cnt_out, int* __restrict__ tmp_pad,
                                                      int32_t* status, hsk_alias at) {
  const int lane = hsk_lane();
  const int wave = hsk_uniform_i(threadIdx.x >> 6);
  const int b = blockIdx.x * 4 + wave;
  if (b >= G) return;
  const long long pos = order ? (long long)order[start + b] : (start + b);
  const int u = coo_user[pos];
  const int ipos = coo_item[pos];
  const long long lo = csr_indptr[u], hi = csr_indptr[u + 1];
  const int K = n_neg + 1;
  int* row = tmp_pad + (long long)b * K;
  __shared__ int32_t lds_row[4][HSK_SAMPLER_LDS_ROW];
  const int len = (int)(hi - lo);
  const bool staged = len <= HSK_SAMPLER_LDS_ROW;
  if (staged) {
    for (int j = lane; j < len; j += 64) lds_row[wave][j] = csr_indices[lo + j];
    __builtin_amdgcn_wave_barrier();
  }
  const int32_t* set = staged ? lds_row[wave] : csr_indices + lo;
  const bool own_pos = ipos >= item_lo && ipos < item_lo + n_loc;
  int base = own_pos ? 1 : 0;
  for (int n0 = 0; n0 < n_neg; n0 += 64) {
    const int n = n0 + lane;
    int neg = -1;
    if (n < n_neg)
      neg = hsk_draw_negative(set, 0, len, (uint32_t)n_items_global, (uint32_t)b, (uint32_t)n, seed, stream_id, status, at);
    const bool mine = neg >= item_lo && neg < item_lo + n_loc;
    const unsigned long long mask = __ballot(mine);
    if (mine) row[base + __popcll(mask & ((1ull << lane) - 1ull))] = neg - item_lo;
    base += __popcll(mask);
  }
  if (lane == 0) {
    if (own_pos) row[0] = ipos - item_lo;
    ug[b] = u;
    pos_local[b] = own_pos ? ipos - item_lo : -1;
    cnt_out[b] = base;
  }
}

// ---------------------------------------------------------------------------------------------
// routing in two short launches, one workgroup per chunk of 1024 positives (the one-workgroup scans they
// replace walked the whole global batch 1024 positives at a time: 52 us at G = 4096, 250 us at G = 65 536)
//   k_shard_count   per chunk: kept entries, positives per owner rank; clears the request list
//   k_shard_place   per positive: offs[b] (exclusive scan of the counts, clamped to the entry capacity), slot_of_b[b] =
//                   owner*C + position among that owner's positives in batch order (every rank computes the whole map,
//                   so the owners need no request exchange), the request list + owner map of this rank's own rows
//   k_shard_compact the padded -> compact copy of the kept entries, one wave per positive (erow[e] = its slot)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HSK_SHARD_CHUNK) void k_shard_count(const int* __restrict__ cnt_in,
                                                                 const int* __restrict__ ug, int G, int world, int C,
                                                                 int* __restrict__ wg_tot, int* __restrict__ own_cnt,
                                                                 int* __restrict__ req, int* __restrict__ ovf) {
  __shared__ int own[64];
  __shared__ int tot;
  const int tid = threadIdx.x, wg = blockIdx.x;
  const int b = wg * HSK_SHARD_CHUNK + tid;
  if (tid < 64) own[tid] = 0;
  if (tid == 0) tot = 0;
  if (wg == 0 && tid == 0) *ovf = 0;   // (k_shard_place, the next launch of this stream, raises it)
  if (wg == 0)
    for (int i = tid; i < C; i += HSK_SHARD_CHUNK) req[i] = -1;
  __syncthreads();
  const int c = (b < G) ? cnt_in[b] : 0;
  const int csum = hsk_wave_sum_i32(c);
  if ((tid & 63) == 0) atomicAdd(&tot, csum);
  if (b < G) atomicAdd(&own[ug[b] % world], 1);
  __syncthreads();
  if (tid < 64) own_cnt[wg * 64 + tid] = own[tid];
  if (tid == 0) wg_tot[wg] = tot;
}

__global__ __launch_bounds__(HSK_SHARD_CHUNK) void k_shard_place(
    const int* __restrict__ tmp_pad, const int* __restrict__ ug, int G, int K, int world, int rank, int C, int cap,
    int n_rows, const int* __restrict__ wg_tot, const int* __restrict__ own_cnt, int* __restrict__ offs,
    int* __restrict__ slot_of_b, int* __restrict__ req, int* __restrict__ owner, int* __restrict__ cnt_rows,
    int* __restrict__ n_entries, int32_t* status, int* __restrict__ ovf) {
  __shared__ int base_own[64];
  __shared__ int wave_own[HSK_SHARD_CHUNK / 64][64];
  __shared__ int wsum[HSK_SHARD_CHUNK / 64];
  __shared__ int base_s, total_s;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wg = blockIdx.x;
  const int n_wg = (G + HSK_SHARD_CHUNK - 1) / HSK_SHARD_CHUNK;
  const int b = wg * HSK_SHARD_CHUNK + tid;
  const bool valid = b < G;
  // what the chunks before this one hold: entries, and positives per owner
  if (w == 0) {
    const int v = (lane < n_wg) ? wg_tot[lane] : 0;
    const int before = hsk_wave_sum_i32(lane < wg ? v : 0);
    const int total = hsk_wave_sum_i32(v);
    if (lane == 0) {
      base_s = before;
      total_s = total;
    }
  }
  if (tid >= 64 && tid < 128) {
    const int d = tid - 64;
    int acc = 0;
    for (int ww = 0; ww < wg; ++ww) acc += own_cnt[ww * 64 + d];
    base_own[d] = acc;
  }
  for (int i = tid; i < (HSK_SHARD_CHUNK / 64) * 64; i += HSK_SHARD_CHUNK) (&wave_own[0][0])[i] = 0;
  const int c = valid ? offs[b] : 0;                      // offs[0..G) arrives holding the per-positive counts
  const int u = valid ? ug[b] : 0;
  const int d = valid ? u % world : 0;
  const int incl = hsk_wave_incl_scan(c, lane);
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  // same-owner rank inside the wave, per-(wave, owner) counts for the waves behind
  const unsigned long long same = hsk_match_any(d, hsk_bits_for(world), valid);
  const int rank_in_wave = __popcll(same & ((1ull << lane) - 1ull));
  if (valid && rank_in_wave == 0) wave_own[w][d] = __popcll(same);
  int before = base_s;
  for (int ww = 0; ww < w; ++ww) before += wsum[ww];
  __syncthreads();
  int pos = base_own[d] + rank_in_wave;
  for (int ww = 0; ww < w; ++ww) pos += wave_own[ww][d];
  const int beg = min(before + incl - c, cap);
  int slot = d * C;
  if (valid) {
    offs[b] = beg;
    if (pos < C) {
      slot = d * C + pos;
      if (d == rank) {
        const int row = u / world;
        req[pos] = row;
        if (row < n_rows) {
          atomicMin(&owner[row], pos);   // owner[row] = lowest slot that requests it, cnt[row] = requesting slots
          atomicAdd(&cnt_rows[row], 1);
        } else if (status) {
          atomicOr(status, HSK_STATUS_BAD_INDEX);
        }
      }
    } else {                             // keep every index in range; the step is invalid: flagged for the host in
      if (status) atomicOr(status, HSK_STATUS_SHARD_OVERFLOW);   // *status, for the step's own kernels in *ovf (no
      atomicOr(ovf, 1);                                          // table is written on such a batch, hsk_shard_guard)
    }
    slot_of_b[b] = slot;
  }
  if (wg == 0 && tid == 0) {
    if (total_s > cap) {
      if (status) atomicOr(status, HSK_STATUS_SHARD_OVERFLOW);
      atomicOr(ovf, 1);
    }
    offs[G] = min(total_s, cap);
    *n_entries = min(total_s, cap);
  }
}

// padded -> compact entry list; erow[e] = where the entry's user row sits in rows_all.  One wave per positive (inside
// k_shard_place a wave walked its 64 positives one after the other: 113 us at G = 4096 for what takes 15 us here).
__global__ __launch_bounds__(256) void k_shard_compact(const int* __restrict__ tmp_pad, const int* __restrict__ offs,
                                                       const int* __restrict__ slot_of_b, int G, int K,
                                                       int* __restrict__ it32c, int* __restrict__ erow) {
  const int lane = hsk_lane();
  const int b = blockIdx.x * 4 + hsk_uniform_i(threadIdx.x >> 6);
  if (b >= G) return;
  const int beg = hsk_uniform_i(offs[b]), end = hsk_uniform_i(offs[b + 1]);   // (both clamped to the entry capacity)
  const int slot = hsk_uniform_i(slot_of_b[b]);
  for (int j = lane; j < end - beg; j += 64) {
    it32c[beg + j] = tmp_pad[(long long)b * K + j];
    erow[beg + j] = slot;
  }
}

// rows_send[s] = Uw[req[s]] (one wave per slot; unused slots are zero-filled so that the exchange never moves
// uninitialised memory)
template <int V, int NCH, bool FULL>
__global__ __launch_bounds__(256) void k_pack_rows(const float* __restrict__ Uw, const int* __restrict__ req, int R,
                                                   int n_rows, int D, float* __restrict__ rows) {
  const int lane = hsk_lane();
  const int s = blockIdx.x * 4 + hsk_uniform_i(threadIdx.x >> 6);
  if (s >= R) return;
  const int row = hsk_uniform_i(req[s]);
  hsk_row<V, NCH> r;
  if (row < 0 || row >= n_rows)
    hsk_row_zero(r);
  else
    hsk_row_load<V, NCH, FULL>(r, Uw + (long long)row * D, lane, D);
  hsk_row_store<V, NCH, FULL>(r, rows + (long long)s * D, lane, D);
}

// ---------------------------------------------------------------------------------------------
// step kernels
// ---------------------------------------------------------------------------------------------
// s0[b] = <u_b, i_b0> + item_bias for the positives whose item this rank owns, 0 elsewhere (the all_reduce then gives
// every rank every positive score: x + 0 + ... + 0 is exact in any order).  One wave per positive.
template <int V, int NCH, bool FULL>
__global__ __launch_bounds__(256) void k_shard_pos_scores(const float* __restrict__ rows_all, const float* __restrict__ Iw,
                                                          const float* __restrict__ Ib,
                                                          const int* __restrict__ slot_of_b,
                                                          const int* __restrict__ pos_local, int G, int D,
                                                          float* __restrict__ s0) {
  const int lane = hsk_lane();
  const int b = blockIdx.x * 4 + hsk_uniform_i(threadIdx.x >> 6);
  if (b >= G) return;
  const int pl = hsk_uniform_i(pos_local[b]);
  if (pl < 0) {
    if (lane == 0) s0[b] = 0.f;
    return;
  }
  hsk_row<V, NCH> ur, r0;
  hsk_row_load<V, NCH, FULL>(ur, rows_all + (long long)hsk_uniform_i(slot_of_b[b]) * D, lane, D);
  hsk_row_load<V, NCH, FULL>(r0, Iw + (long long)pl * D, lane, D);
  const float s = hsk_wave_sum(hsk_row_dot_partial(ur, r0)) + (Ib ? Ib[pl] : 0.f);
  if (lane == 0) s0[b] = s;
}

// The gather + loss kernel of the sharded step: one wave per positive of the global batch, over the negatives THIS rank
// owns.  Same arithmetic per entry as k_fwd_ugrad<..., LOSS>.  What couples a positive to its negatives across the ranks
// is settled afterwards:
//   HSK_LOSS_BPR  the positive's own term (g_0 = -sum over ALL ranks of the negatives' weights) is added by
//                 k_shard_pos_fix once gsum has been all-reduced;
//   HSK_LOSS_BCE  nothing: every logit is weighed on its own (train/rec_losses.py:27-53), the positive's by its owner;
//   HSK_LOSS_SSM  the softmax normaliser (train/rec_losses.py:91-139): the rank keeps a running max m_r and
//                 l_r = sum exp(z - m_r) over ITS negatives (online softmax, as the single-GPU kernel does), leaves
//                 the unnormalised sum_k exp(z_k - m_r) i_k in dU_all[slot], z_k in g_s, (m_r, l_r) in stats[b], stats[G + b];
//                 k_shard_ssm_fix combines the ranks' pairs once they have been all-gathered.
template <int V, int NCH, bool FULL, int R, int LOSS>
__global__ __launch_bounds__(256) void k_shard_fwd(const float* __restrict__ rows_all, const float* __restrict__ Iw,
                                                   const float* __restrict__ Ib, const int* __restrict__ slot_of_b,
                                                   const int* __restrict__ pos_local, const int* __restrict__ offs,
                                                   const int* __restrict__ it32c, const float* __restrict__ s0all,
                                                   int G, int D, float inv_norm, float ssm_c, float* __restrict__ g_s,
                                                   float* __restrict__ dU_all, float* __restrict__ gsum_out,
                                                   double* __restrict__ loss_b, float* __restrict__ stats) {
  const int lane = hsk_lane();
  const int b = blockIdx.x * 4 + hsk_uniform_i(threadIdx.x >> 6);
  if (b >= G) return;
  using Row = hsk_row<V, NCH>;
  const int slot = hsk_uniform_i(slot_of_b[b]);
  const int beg = hsk_uniform_i(offs[b]) + (hsk_uniform_i(pos_local[b]) >= 0 ? 1 : 0);
  const int end = hsk_uniform_i(offs[b + 1]);
  const float s0 = (LOSS == HSK_LOSS_BPR) ? s0all[b] : 0.f;
  Row ur, acc;
  hsk_row_load<V, NCH, FULL>(ur, rows_all + (long long)slot * D, lane, D);
  hsk_row_zero(acc);
  float gsum = 0.f;
  double lsum = 0.0;
  float smax = -INFINITY, ssum = 0.f;   // SSM: running max and sum of exp(z - smax) over this rank's negatives
  for (int kc = beg; kc < end; kc += 64) {
    const int nr = min(64, end - kc);
    const int myidx = (lane < nr) ? it32c[kc + lane] : 0;
    const float mybias = (Ib && lane < nr) ? Ib[myidx] : 0.f;
    float gv = 0.f, xv = 0.f;
    Row bufA[R], bufB[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (r < nr) hsk_row_load<V, NCH, FULL>(bufA[r], Iw + (long long)hsk_readlane_i(myidx, r) * D, lane, D);
    auto process = [&](Row(&buf)[R], int j) {
      if constexpr (LOSS != HSK_LOSS_SSM) {   // BPR, BCE: the buffer's rows are weighed in one pass
        hsk_weigh_rows<LOSS>(ur, buf, j, nr, lane, mybias, s0, inv_norm, acc, gsum, gv, xv);
      } else {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (j + r < nr) {
            const float s = hsk_wave_sum(hsk_row_dot_partial(ur, buf[r])) + hsk_readlane_f(mybias, j + r);
            const float z = s + ssm_c;
            if (z > smax) {   // wave-uniform: rescale what has been accumulated so far (exp(-inf) = 0 on the first entry)
              const float f = expf(smax - z);
              ssum *= f;
#pragma unroll
              for (int cc = 0; cc < NCH; ++cc)
#pragma unroll
                for (int q = 0; q < V; ++q) acc.c[cc].v[q] *= f;
              smax = z;
            }
            const float e = expf(z - smax);
            ssum += e;
            hsk_row_axpy(acc, e, buf[r]);
            gv = (lane == j + r) ? z : gv;   // finalised by k_shard_ssm_fix
          }
        }
      }
    };
    auto prefetch = [&](Row(&buf)[R], int j) {
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (j + r < nr)
          hsk_row_load<V, NCH, FULL>(buf[r], Iw + (long long)hsk_readlane_i(myidx, j + r) * D, lane, D);
    };
    for (int j = 0; j < nr; j += 2 * R) {
      prefetch(bufB, j + R);
      process(bufA, j);
      prefetch(bufA, j + 2 * R);
      process(bufB, j + R);
    }
    if (lane < nr) {
      g_s[kc + lane] = gv;
      if (LOSS == HSK_LOSS_BPR) lsum += (double)hsk_softplus(-xv);
      if (LOSS == HSK_LOSS_BCE) lsum += (double)hsk_softplus(xv);
    }
  }
  hsk_row_store<V, NCH, FULL>(acc, dU_all + (long long)slot * D, lane, D);
  const double l = hsk_wave_sum_f64(lsum);
  if (lane == 0) {
    if (LOSS == HSK_LOSS_BPR) gsum_out[b] = gsum;
    if (LOSS == HSK_LOSS_SSM) {
      stats[b] = smax;
      stats[G + b] = ssum;
    }
    loss_b[b] = l;   // (SSM: rewritten by k_shard_ssm_fix)
  }
}

// owner of the positive item.  BPR, after gsum has been summed over the ranks: g_0 = -gsum[b] is the weight of the
// positive's entry (item gradient) and dU_all[slot] += g_0 * i_b0 completes this rank's share of the user-row gradient.
// BCE: g_0 = (sigma(s_0) - 1) / (G*K) from the owner's own s_0 (no reduction), + the positive's loss term.
template <int V, int NCH, bool FULL, int LOSS>
__global__ __launch_bounds__(256) void k_shard_pos_fix(const float* __restrict__ Iw, const int* __restrict__ slot_of_b,
                                                       const int* __restrict__ pos_local, const int* __restrict__ offs,
                                                       const float* __restrict__ gsum, const float* __restrict__ s0own,
                                                       int G, int D, float inv_norm, float* __restrict__ g_s,
                                                       float* __restrict__ dU_all, double* __restrict__ loss_b) {
  const int lane = hsk_lane();
  const int b = blockIdx.x * 4 + hsk_uniform_i(threadIdx.x >> 6);
  if (b >= G) return;
  const int pl = hsk_uniform_i(pos_local[b]);
  if (pl < 0) return;
  const int beg = hsk_uniform_i(offs[b]);
  if (beg >= hsk_uniform_i(offs[b + 1])) return;   // entry lost to a capacity overflow (flagged)
  float g0;
  if (LOSS == HSK_LOSS_BCE) {
    const float s0 = s0own[b];
    g0 = -hsk_sigmoid_neg_scaled(inv_norm, s0);
    if (lane == 0) loss_b[b] += (double)hsk_softplus(-s0);
  } else {
    g0 = -gsum[b];
  }
  hsk_row<V, NCH> r0, acc;
  float* drow = dU_all + (long long)hsk_uniform_i(slot_of_b[b]) * D;
  hsk_row_load<V, NCH, FULL>(r0, Iw + (long long)pl * D, lane, D);
  hsk_row_load<V, NCH, FULL>(acc, drow, lane, D);
  hsk_row_axpy(acc, g0, r0);
  hsk_row_store<V, NCH, FULL>(acc, drow, lane, D);
  if (lane == 0) g_s[beg] = g0;
}

// Sampled softmax, after the ranks' (m_r, l_r, s0_r) triples have been all-gathered (stats_all[r][3][G]; s0_r = the
// positive's score on the rank that owns its item, 0 elsewhere).  Every rank, one wave per positive:
//   M = max(s_0, max_r m_r),  L = exp(s_0 - M) + sum_r l_r exp(m_r - M)        (identical bits on every rank)
//   d loss / d s_k = exp(z_k - M) / (L G) for this rank's negatives (z_k was left in g_s), so the rank's unnormalised
//   row in dU_all[slot] is scaled by exp(m_me - M) / (L G); the positive's owner adds g_0 i_0, g_0 = (exp(s_0 - M)/L - 1)/G,
//   and the loss term -s_0 + M + log L (train/rec_losses.py:133-139 of the reference).
template <int V, int NCH, bool FULL>
__global__ __launch_bounds__(256) void k_shard_ssm_fix(const float* __restrict__ Iw, const int* __restrict__ slot_of_b,
                                                       const int* __restrict__ pos_local, const int* __restrict__ offs,
                                                       const float* __restrict__ stats_all, int world, int rank, int G,
                                                       int D, float inv_norm, float* __restrict__ g_s,
                                                       float* __restrict__ dU_all, double* __restrict__ loss_b) {
  const int lane = hsk_lane();
  const int b = blockIdx.x * 4 + hsk_uniform_i(threadIdx.x >> 6);
  if (b >= G) return;
  float m_r = -INFINITY, l_r = 0.f, s_r = 0.f;
  if (lane < world) {
    const float* st = stats_all + (long long)lane * 3 * G;
    m_r = st[b];
    l_r = st[G + b];
    s_r = st[2 * G + b];
  }
  const float s0 = hsk_wave_sum(s_r);            // one non-zero term: exact in any order
  float M = fmaxf(m_r, s0);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) M = fmaxf(M, __shfl_xor(M, off, HSK_WAVE));
  const float Lneg = hsk_wave_sum(l_r * expf(m_r - M));   // (lanes >= world: 0 * exp(-inf) = 0)
  const float L = expf(s0 - M) + Lneg;
  const float rinv = inv_norm / L;
  const float m_me = hsk_readlane_f(m_r, rank);
  const float scale = expf(m_me - M) * rinv;     // 0 for a rank without negatives of this positive (m_me = -inf)
  const int pl = hsk_uniform_i(pos_local[b]);
  const int beg0 = hsk_uniform_i(offs[b]), end = hsk_uniform_i(offs[b + 1]);
  const bool own = pl >= 0 && beg0 < end;        // (an entry lost to a capacity overflow is flagged elsewhere)
  const int beg = beg0 + (own ? 1 : 0);
  for (int k = beg + lane; k < end; k += 64) g_s[k] = expf(g_s[k] - M) * rinv;
  hsk_row<V, NCH> acc;
  float* drow = dU_all + (long long)hsk_uniform_i(slot_of_b[b]) * D;
  hsk_row_load<V, NCH, FULL>(acc, drow, lane, D);
#pragma unroll
  for (int cc = 0; cc < NCH; ++cc)
#pragma unroll
    for (int q = 0; q < V; ++q) acc.c[cc].v[q] *= scale;
  if (own) {
    const float g0 = -Lneg * rinv;   // p_0 / G - 1 / G without the difference
    hsk_row<V, NCH> r0;
    hsk_row_load<V, NCH, FULL>(r0, Iw + (long long)pl * D, lane, D);
    hsk_row_axpy(acc, g0, r0);
    if (lane == 0) g_s[beg0] = g0;
  }
  hsk_row_store<V, NCH, FULL>(acc, drow, lane, D);
  if (lane == 0) loss_b[b] = own ? (double)(-s0 + M + logf(L)) : 0.0;
}

__global__ __launch_bounds__(256) void k_shard_copy_batch(const int* __restrict__ offs, const int* __restrict__ it32c,
                                                          const int* __restrict__ ug, int G, int cap,
                                                          int* __restrict__ offs_out, int* __restrict__ items_out,
                                                          int* __restrict__ u_out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= G) offs_out[i] = offs[i];
  if (i < G) u_out[i] = ug[i];
  if (i < cap) items_out[i] = (i < offs[G]) ? it32c[i] : -1;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
enum { HSK_SHARD_IDLE = 0, HSK_SHARD_PACKED, HSK_SHARD_SCORED, HSK_SHARD_FORWARDED, HSK_SHARD_FIXED, HSK_SHARD_ITEMS };

static int hsk_shard_check(const hsk_bprmf_shard* sh) {
  HSK_REQUIRE(sh != nullptr, HSK_ERR_INVALID, "shard state is NULL");
  int rc = hsk_check_state(&sh->base);
  if (rc) return rc;
  const hsk_bprmf_state* st = &sh->base;
  HSK_REQUIRE(sh->world >= 1 && sh->world <= 64 && sh->rank >= 0 && sh->rank < sh->world, HSK_ERR_INVALID,
              "world %d / rank %d out of range (1..64 ranks)", sh->world, sh->rank);
  HSK_REQUIRE(st->lazy_users == 1, HSK_ERR_UNSUPPORTED, "the sharded step needs lazy_users = 1");
  HSK_REQUIRE(st->loss_kind != HSK_LOSS_SSM || (sh->ssm_send && sh->ssm_all), HSK_ERR_INVALID,
              "the sampled-softmax sharded step needs the ssm_send / ssm_all exchange buffers");
  HSK_REQUIRE(st->loss_kind != HSK_LOSS_BCE || (!st->user_bias && !st->global_bias), HSK_ERR_UNSUPPORTED,
              "bce sends gradient to the user / global bias: not in the sharded step");
  HSK_REQUIRE(st->aux == nullptr, HSK_ERR_INVALID, "the sharded step does its own prefetch: base.aux must be NULL");
  HSK_REQUIRE(sh->n_users_global > 0 && st->n_users == (sh->n_users_global - sh->rank + sh->world - 1) / sh->world,
              HSK_ERR_INVALID, "base.n_users must be the number of users u < n_users_global with u %% world == rank");
  HSK_REQUIRE(sh->n_items_global > 0 && sh->n_items_global < 0x7fffffff && sh->item_lo >= 0 &&
                  sh->item_lo + st->n_items <= sh->n_items_global,
              HSK_ERR_INVALID, "item shard [%lld, +%lld) outside the catalogue of %lld items", (long long)sh->item_lo,
              (long long)st->n_items, (long long)sh->n_items_global);
  HSK_REQUIRE(sh->capacity > 0 && sh->capacity <= st->max_batch, HSK_ERR_INVALID,
              "capacity %lld outside (0, base.max_batch = %lld]", (long long)sh->capacity, (long long)st->max_batch);
  HSK_REQUIRE(sh->entry_cap > 0 && sh->entry_cap <= st->max_batch * st->max_cols, HSK_ERR_INVALID,
              "entry_cap %lld outside (0, max_batch*max_cols]", (long long)sh->entry_cap);
  HSK_REQUIRE(sh->shard_ws && ((uintptr_t)sh->shard_ws & 255) == 0, HSK_ERR_INVALID,
              "shard_ws must be a 256-byte aligned device buffer");
  HSK_REQUIRE(sh->rows_send && sh->rows_all && sh->dU_all && sh->grads_mine && sh->s0 && sh->gsum, HSK_ERR_INVALID,
              "exchange buffers must not be NULL");
  HSK_REQUIRE(st->csr_indptr && st->csr_indices && st->coo_user && st->coo_item, HSK_ERR_INVALID,
              "CSR/COO of the training interactions missing from the state");
  return HSK_OK;
}

// shape-dependent part: G = world*batch positives of n_neg+1 columns must fit what the buffers were sized for
static int hsk_shard_check_batch(const hsk_bprmf_shard* sh, int64_t batch, int64_t n_neg) {
  const hsk_bprmf_state* st = &sh->base;
  const int64_t G = (int64_t)sh->world * batch, K = n_neg + 1;
  HSK_REQUIRE(batch > 0 && G <= st->max_batch, HSK_ERR_INVALID, "global batch %lld outside (0, base.max_batch = %lld]",
              (long long)G, (long long)st->max_batch);
  HSK_REQUIRE(n_neg >= 1 && K <= st->max_cols, HSK_ERR_INVALID, "n_neg %lld outside [1, %lld]", (long long)n_neg,
              (long long)(st->max_cols - 1));
  const int64_t need = hsk_shard_workspace_bytes(st->max_batch, st->max_cols, sh->capacity, sh->entry_cap);
  HSK_REQUIRE(sh->shard_ws_bytes >= need, HSK_ERR_INVALID, "shard_ws too small: %lld < %lld",
              (long long)sh->shard_ws_bytes, (long long)need);
  return HSK_OK;
}

extern "C" int hsk_shard_init(hsk_bprmf_shard* sh, hsk_stream_t stream_) {
  int rc = hsk_shard_check(sh);
  if (rc) return rc;
  sh->cur_batch = sh->cur_cols = 0;
  sh->cur_set = 0;
  sh->phase = HSK_SHARD_IDLE;
  hipStream_t stream = (hipStream_t)stream_;
  HSK_HIP(hipMemsetAsync(sh->dU_all, 0, (size_t)sh->world * sh->capacity * sh->base.dim * sizeof(float), stream));
  HSK_HIP(hipMemsetAsync(sh->rows_send, 0, (size_t)sh->capacity * sh->base.dim * sizeof(float), stream));
  const int64_t need = hsk_shard_workspace_bytes(sh->base.max_batch, sh->base.max_cols, sh->capacity, sh->entry_cap);
  HSK_REQUIRE(sh->shard_ws_bytes >= need, HSK_ERR_INVALID, "shard_ws too small: %lld < %lld",
              (long long)sh->shard_ws_bytes, (long long)need);
  const hsk_shard_ws x = hsk_shard_carve(sh->shard_ws, sh->base.max_batch, sh->base.max_cols, sh->capacity, sh->entry_cap);
  for (int* p : {x.ovf[0], x.ovf[1], x.poison}) HSK_HIP(hipMemsetAsync(p, 0, sizeof(int), stream));   // overflow guard
  return HSK_OK;
}

// steps_ahead: -1 = by the phase (a step in flight: the batch is consumed one step later); 0 / 1 = said by the caller
// (the natively issued step prepares the next batch BEFORE it opens its own step)
static int hsk_shard_prepare_impl(hsk_bprmf_shard* sh, const int64_t* order, int64_t start_global, int64_t batch,
                                  int64_t n_neg, int32_t set, hsk_stream_t stream_, int steps_ahead) {
  int rc = hsk_shard_check(sh);
  if (rc) return rc;
  if ((rc = hsk_shard_check_batch(sh, batch, n_neg))) return rc;
  HSK_REQUIRE(set == 0 || set == 1, HSK_ERR_INVALID, "set must be 0 or 1");
  HSK_REQUIRE(!(sh->phase != HSK_SHARD_IDLE && set == sh->cur_set), HSK_ERR_INVALID,
              "buffer set %d belongs to the step in flight", set);
  hsk_bprmf_state* st = &sh->base;
  const int64_t G = (int64_t)sh->world * batch, K = n_neg + 1;
  HSK_REQUIRE(start_global >= 0 && start_global + G <= st->nnz, HSK_ERR_INVALID,
              "global interaction range [%lld, %lld) outside nnz %lld", (long long)start_global,
              (long long)(start_global + G), (long long)st->nnz);
  hipStream_t stream = (hipStream_t)stream_;
  const hsk_ws w = hsk_select(hsk_carve_st(st), set);
  const hsk_shard_ws x = hsk_shard_carve(sh->shard_ws, st->max_batch, st->max_cols, sh->capacity, sh->entry_cap);
  const int C = (int)sh->capacity, cap = (int)sh->entry_cap;
  // the RNG stream id is the index of the step this batch is consumed at: the step in flight (if any) is st->step
  const uint64_t stream_id = (uint64_t)st->step + (steps_ahead >= 0 ? steps_ahead : sh->phase != HSK_SHARD_IDLE ? 1 : 0);
  k_shard_sample<<<(unsigned)hsk_ceil_div(G, 4), 256, 0, stream>>>(
      st->coo_user, st->coo_item, order, (long long)start_global, (int)G, (int)n_neg, st->csr_indptr, st->csr_indices,
      (int)sh->n_items_global, (int)sh->item_lo, (int)st->n_items, st->seed, stream_id, w.u32, x.pos_local[set],
      x.offs[set], x.tmp_pad, st->status, hsk_alias{st->alias_prob, st->alias_idx});
  HSK_LAUNCH_CHECK();
  HSK_REQUIRE(G <= (int64_t)HSK_SHARD_CHUNK * HSK_SHARD_MAX_CHUNKS, HSK_ERR_UNSUPPORTED,
              "global batch %lld above %d positives", (long long)G, HSK_SHARD_CHUNK * HSK_SHARD_MAX_CHUNKS);
  const unsigned n_chunks = (unsigned)hsk_ceil_div(G, HSK_SHARD_CHUNK);
  k_shard_count<<<n_chunks, HSK_SHARD_CHUNK, 0, stream>>>(x.offs[set], w.u32, (int)G, sh->world, C, x.wg_tot[set],
                                                          x.own_cnt[set], x.req[set], x.ovf[set]);
  k_shard_place<<<n_chunks, HSK_SHARD_CHUNK, 0, stream>>>(x.tmp_pad, w.u32, (int)G, (int)K, sh->world, sh->rank, C, cap,
                                                          (int)st->n_users, x.wg_tot[set], x.own_cnt[set], x.offs[set],
                                                          x.slot_of_b[set], x.req[set], w.owner, w.cnt,
                                                          x.n_entries[set], st->status, x.ovf[set]);
  k_shard_compact<<<(unsigned)hsk_ceil_div(G, 4), 256, 0, stream>>>(x.tmp_pad, x.offs[set], x.slot_of_b[set], (int)G,
                                                                    (int)K, w.it32, x.erow[set]);
  HSK_LAUNCH_CHECK();
  if ((rc = hsk_launch_sort(st, w, cap, stream, x.n_entries[set]))) return rc;
  return HSK_OK;
}

extern "C" int hsk_shard_prepare(hsk_bprmf_shard* sh, const int64_t* order, int64_t start_global, int64_t batch,
                                 int64_t n_neg, int32_t set, hsk_stream_t stream_) {
  return hsk_shard_prepare_impl(sh, order, start_global, batch, n_neg, set, stream_, -1);
}

#define HSK_SHARD_BEGIN(expected, what)                                                                      \
  int rc = hsk_shard_check(sh);                                                                              \
  if (rc) return rc;                                                                                         \
  HSK_REQUIRE(sh->phase == (expected), HSK_ERR_INVALID, what " called out of order (phase %d)", sh->phase);   \
  hsk_bprmf_state* st = &sh->base;                                                                           \
  hipStream_t stream = (hipStream_t)stream_;                                                                 \
  const int set = sh->cur_set;                                                                               \
  const int64_t G = (int64_t)sh->world * sh->cur_batch, K = sh->cur_cols;                                    \
  const hsk_ws w = hsk_select(hsk_carve_st(st), set); \
  const hsk_shard_ws x = hsk_shard_carve(sh->shard_ws, st->max_batch, st->max_cols, sh->capacity, sh->entry_cap); \
  const int C = (int)sh->capacity, D = (int)st->dim;                                                         \
  (void)w; (void)x; (void)C; (void)D; (void)G; (void)K; (void)stream

// owner: bring the user rows requested through the slots of buffer set `set` up to step - 1 (`step` = the step they
// will be trained at).  register_dups: non-owner slots of a row register with the owner slot (once per batch: the call
// that opens the step does it; an ahead-of-time call -- the natively issued step replays the NEXT batch's rows behind the
// current step's user update, off the critical path -- does not).
// opens: this call opens the step of the batch in `set` (hsk_shard_pack): if that batch overflowed a capacity the launch
// raises the sticky guard word; either way a guarded launch touches nothing once a guard word is set (hsk_guard_skip)
static int hsk_shard_catch_up_rows(hsk_bprmf_shard* sh, int set, int64_t step, hipStream_t stream, bool register_dups,
                                   bool opens = false) {
  hsk_bprmf_state* st = &sh->base;
  const hsk_ws w = hsk_select(hsk_carve_st(st), set);
  const hsk_shard_ws x = hsk_shard_carve(sh->shard_ws, st->max_batch, st->max_cols, sh->capacity, sh->entry_cap);
  const hsk_adamw_consts c = hsk_make_adamw_consts(st->lr, st->beta1, st->beta2, st->eps, st->wd, step, st->opt_kind);
  hsk_launch_user_catch_up(st, w, stream, x.req[set], (int)sh->capacity, step, c, register_dups ? w.dupcnt : nullptr,
                           register_dups ? w.duplist : nullptr, x.ovf[set], x.poison, opens ? 1 : 0);
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}

// owner: replay the missed zero-gradient steps of the requested rows and pack them for the all_gather; opens the step
extern "C" int hsk_shard_pack(hsk_bprmf_shard* sh, int64_t batch, int64_t n_neg, int32_t set_, hsk_stream_t stream_) {
  {
    int rc0 = hsk_shard_check(sh);
    if (rc0) return rc0;
    if ((rc0 = hsk_shard_check_batch(sh, batch, n_neg))) return rc0;
    HSK_REQUIRE(set_ == 0 || set_ == 1, HSK_ERR_INVALID, "set must be 0 or 1");
    HSK_REQUIRE(sh->phase == HSK_SHARD_IDLE, HSK_ERR_INVALID, "hsk_shard_pack while a step is in flight");
    sh->cur_batch = batch;
    sh->cur_cols = n_neg + 1;
    sh->cur_set = set_;
  }
  HSK_SHARD_BEGIN(HSK_SHARD_IDLE, "hsk_shard_pack");
  hsk_timing_arm(st);
  if ((rc = hsk_shard_catch_up_rows(sh, set, st->step + 1, stream, true, true))) return rc;
  rc = hsk_dispatch_dim(D, [&](auto v_, auto n_, auto f_) {
    constexpr int V = decltype(v_)::value;
    constexpr int NCH = decltype(n_)::value;
    constexpr bool FULL = decltype(f_)::value;
    k_pack_rows<V, NCH, FULL><<<(unsigned)hsk_ceil_div(C, 4), 256, 0, stream>>>(st->user_emb, x.req[set], C,
                                                                                 (int)st->n_users, D, sh->rows_send);
    return HSK_OK;
  });
  if (rc) return rc;
  HSK_LAUNCH_CHECK();
  sh->phase = HSK_SHARD_PACKED;
  return HSK_OK;
}

extern "C" int hsk_shard_pos_scores(hsk_bprmf_shard* sh, hsk_stream_t stream_) {
  HSK_SHARD_BEGIN(HSK_SHARD_PACKED, "hsk_shard_pos_scores");
  if (st->lazy_items) {
    // the scores must see current item rows: replay the missed zero-gradient steps of this batch's items
    const hsk_adamw_consts c = hsk_make_adamw_consts(st->lr, st->beta1, st->beta2, st->eps, st->wd, st->step + 1, st->opt_kind);
    const unsigned nblk = (unsigned)std::min<int64_t>(st->n_items, sh->entry_cap);
    // (rows of 1024 floats and more, 16-byte aligned: four floats per thread -- a 4 KB row in ONE pass of the workgroup
    // instead of two dependent ones)
    hsk_launch_item_catch_up(st, w, stream, nblk, D % 4 == 0 && D >= 1024, st->step + 1, c, nullptr, 0, x.ovf[set], x.poison);
    HSK_LAUNCH_CHECK();
  }
  rc = hsk_dispatch_dim(D, [&](auto v_, auto n_, auto f_) {
    constexpr int V = decltype(v_)::value;
    constexpr int NCH = decltype(n_)::value;
    constexpr bool FULL = decltype(f_)::value;
    // sampled softmax: the positive's score travels with the (m, l) pair of the forward (third plane of ssm_send)
    float* s0_out = st->loss_kind == HSK_LOSS_SSM ? sh->ssm_send + 2 * G : sh->s0;
    k_shard_pos_scores<V, NCH, FULL><<<(unsigned)hsk_ceil_div(G, 4), 256, 0, stream>>>(
        sh->rows_all, st->item_emb, st->item_bias, x.slot_of_b[set], x.pos_local[set], (int)G, D, s0_out);
    return HSK_OK;
  });
  if (rc) return rc;
  HSK_LAUNCH_CHECK();
  sh->phase = HSK_SHARD_SCORED;
  return HSK_OK;
}

extern "C" int hsk_shard_forward(hsk_bprmf_shard* sh, hsk_stream_t stream_) {
  HSK_SHARD_BEGIN(HSK_SHARD_SCORED, "hsk_shard_forward");
  const float inv_bn = (float)hsk_loss_norm(st->loss_kind, (double)G, (double)K);   // GLOBAL batch
  rc = hsk_dispatch_dim(D, [&](auto v_, auto n_, auto f_) {
    constexpr int V = decltype(v_)::value;
    constexpr int NCH = decltype(n_)::value;
    constexpr bool FULL = decltype(f_)::value;
    constexpr int R = (V * NCH >= 16) ? 2 : 4;
    return hsk_dispatch_loss<true>(st->loss_kind, [&](auto lk_) {
      HSK_STAGE(HSK_STAGE_FWD, (k_shard_fwd<V, NCH, FULL, R, decltype(lk_)::value><<<(unsigned)hsk_ceil_div(G, 4), 256, 0, stream>>>(
                                   sh->rows_all, st->item_emb, st->item_bias, x.slot_of_b[set], x.pos_local[set], x.offs[set],
                                   w.it32, sh->s0, (int)G, D, inv_bn, (float)st->ssm_log_adjust, w.g_s, sh->dU_all, sh->gsum,
                                   w.loss_b, sh->ssm_send)));
      return HSK_OK;
    });
  });
  if (rc) return rc;
  HSK_LAUNCH_CHECK();
  sh->phase = HSK_SHARD_FORWARDED;
  return HSK_OK;
}

extern "C" int hsk_shard_pos_fix(hsk_bprmf_shard* sh, hsk_stream_t stream_) {
  HSK_SHARD_BEGIN(HSK_SHARD_FORWARDED, "hsk_shard_pos_fix");
  rc = hsk_dispatch_dim(D, [&](auto v_, auto n_, auto f_) {
    constexpr int V = decltype(v_)::value;
    constexpr int NCH = decltype(n_)::value;
    constexpr bool FULL = decltype(f_)::value;
    const float inv_bn = (float)hsk_loss_norm(st->loss_kind, (double)G, (double)K);
    const unsigned grid = (unsigned)hsk_ceil_div(G, 4);
    if (st->loss_kind == HSK_LOSS_SSM)
      k_shard_ssm_fix<V, NCH, FULL><<<grid, 256, 0, stream>>>(st->item_emb, x.slot_of_b[set], x.pos_local[set], x.offs[set],
                                                             sh->ssm_all, sh->world, sh->rank, (int)G, D, inv_bn, w.g_s,
                                                             sh->dU_all, w.loss_b);
    else if (st->loss_kind == HSK_LOSS_BCE)
      k_shard_pos_fix<V, NCH, FULL, HSK_LOSS_BCE><<<grid, 256, 0, stream>>>(st->item_emb, x.slot_of_b[set], x.pos_local[set],
                                                                           x.offs[set], sh->gsum, sh->s0, (int)G, D, inv_bn,
                                                                           w.g_s, sh->dU_all, w.loss_b);
    else
      k_shard_pos_fix<V, NCH, FULL, HSK_LOSS_BPR><<<grid, 256, 0, stream>>>(st->item_emb, x.slot_of_b[set], x.pos_local[set],
                                                                           x.offs[set], sh->gsum, sh->s0, (int)G, D, inv_bn,
                                                                           w.g_s, sh->dU_all, w.loss_b);
    return HSK_OK;
  });
  if (rc) return rc;
  HSK_LAUNCH_CHECK();
  sh->phase = HSK_SHARD_FIXED;
  return HSK_OK;
}

// local item shard: item-major gradient reduction over the kept entries + AdamW (dense over the shard, or only the
// touched rows with lazy_items); the user rows are gathered from rows_all through erow
extern "C" int hsk_shard_apply_items(hsk_bprmf_shard* sh, hsk_stream_t stream_) {
  HSK_SHARD_BEGIN(HSK_SHARD_FIXED, "hsk_shard_apply_items");
  // the kernels' `step` is the step being taken; the lazy-item bookkeeping inside reads st->step
  st->step += 1;
  const hsk_adamw_consts c = hsk_make_adamw_consts(st->lr, st->beta1, st->beta2, st->eps, st->wd, st->step, st->opt_kind);
  rc = hsk_dispatch_dim(D, [&](auto v_, auto n_, auto f_) {
    constexpr int V = decltype(v_)::value;
    constexpr int NCH = decltype(n_)::value;
    constexpr bool FULL = decltype(f_)::value;
    constexpr int R = (V * NCH >= 16) ? 2 : 4;
    HSK_STAGE(HSK_STAGE_ITEM, hsk_launch_item_pass<V, NCH, FULL, R, true>(st, w, sh->rows_all, x.erow[set], 1, c, nullptr,
                                                                          nullptr, stream, sh->entry_cap, nullptr, nullptr,
                                                                          1, x.ovf[set], x.poison));
    return HSK_OK;
  });
  st->step -= 1;
  if (rc) return rc;
  HSK_LAUNCH_CHECK();
  sh->phase = HSK_SHARD_ITEMS;
  return HSK_OK;
}

// owner: AdamW on the requested user rows (needs grads_mine); takes the step counter forward and closes the step
// sweep: the periodic sweeps of the lazily updated shards that come due with this step are launched behind the update
// (the natively issued step runs this phase on its communication stream, beside the item pass, and sweeps after the join)
static int hsk_shard_apply_users_impl(hsk_bprmf_shard* sh, hsk_stream_t stream_, bool sweep) {
  HSK_SHARD_BEGIN(HSK_SHARD_ITEMS, "hsk_shard_apply_users");
  st->step += 1;
  const hsk_adamw_consts c = hsk_make_adamw_consts(st->lr, st->beta1, st->beta2, st->eps, st->wd, st->step, st->opt_kind);
  const double inv_bn_d = hsk_loss_norm(st->loss_kind, (double)G, (double)K);
  rc = hsk_dispatch_dim(D, [&](auto v_, auto n_, auto f_) {
    constexpr int V = decltype(v_)::value;
    constexpr int NCH = decltype(n_)::value;
    constexpr bool FULL = decltype(f_)::value;
    // + one workgroup for this rank's share of the loss and the (replicated, gradient-free) global bias
    const hsk_finish_args fin = {w.loss_b, (int)G, inv_bn_d, st->loss_out, st->global_bias, st->m_global_bias,
                                 st->v_global_bias};
    // rows were brought up to date (and written back) by hsk_shard_pack: no replay here (tab = NULL)
    const hsk_user_lazy_args ua = {st->user_emb, st->m_user_emb, st->v_user_emb, st->user_bias, st->m_user_bias,
                                   st->v_user_bias, sh->grads_mine, x.req[set], w.owner, w.cnt, w.last_step, C, D,
                                   (int)st->step, c, fin, w.dupcnt, w.duplist, nullptr, 0, nullptr, nullptr, nullptr};
    return hsk_dispatch_flags([&](auto gen_) {
      HSK_STAGE(HSK_STAGE_USER, (k_user_update_lazy<V, NCH, FULL, decltype(gen_)::value>
                                 <<<(unsigned)hsk_ceil_div(C, 4) + 1, 256, 0, stream>>>(ua, x.ovf[set], x.poison)));
      return HSK_OK;
    }, st->opt_kind != HSK_OPT_ADAMW);
  });
  if (rc) return rc;
  HSK_LAUNCH_CHECK();
  sh->phase = HSK_SHARD_IDLE;
  sh->cur_batch = 0;
  // the periodic sweeps of the local shards (cadence from the shard sizes: a cfg5 shard of 12.5 M user rows is swept
  // every ~150 steps, 300 GB of traffic each time; a small shard never)
  if (!sweep) return HSK_OK;
  return hsk_periodic_flush(st, w, stream, st->step - 1, (double)C, (double)sh->entry_cap, x.poison);
}

extern "C" int hsk_shard_apply_users(hsk_bprmf_shard* sh, hsk_stream_t stream_) {
  return hsk_shard_apply_users_impl(sh, stream_, true);
}

// a batch prepared in `set` that will not be trained on: give its owner map back
__global__ __launch_bounds__(256) void k_shard_release(const int* __restrict__ req, int C, int* __restrict__ owner,
                                                       int* __restrict__ cnt) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= C) return;
  const int row = req[s];
  if (row < 0) return;
  owner[row] = HSK_OWNER_NONE;
  cnt[row] = 0;
}

extern "C" int hsk_shard_discard(hsk_bprmf_shard* sh, int32_t set, hsk_stream_t stream_) {
  int rc = hsk_shard_check(sh);
  if (rc) return rc;
  HSK_REQUIRE(set == 0 || set == 1, HSK_ERR_INVALID, "set must be 0 or 1");
  HSK_REQUIRE(!(sh->phase != HSK_SHARD_IDLE && set == sh->cur_set), HSK_ERR_INVALID,
              "buffer set %d belongs to the step in flight", set);
  hsk_bprmf_state* st = &sh->base;
  const hsk_ws w = hsk_select(hsk_carve_st(st), set);
  const hsk_shard_ws x = hsk_shard_carve(sh->shard_ws, st->max_batch, st->max_cols, sh->capacity, sh->entry_cap);
  k_shard_release<<<(unsigned)hsk_ceil_div(sh->capacity, 256), 256, 0, (hipStream_t)stream_>>>(x.req[set], (int)sh->capacity,
                                                                                              w.owner, w.cnt);
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}

extern "C" int hsk_shard_flush(hsk_bprmf_shard* sh, hsk_stream_t stream_) {
  int rc = hsk_shard_check(sh);
  if (rc) return rc;
  HSK_REQUIRE(sh->phase == HSK_SHARD_IDLE, HSK_ERR_INVALID, "hsk_shard_flush while a step is in flight");
  hsk_bprmf_state* st = &sh->base;
  const hsk_ws w = hsk_carve_st(st);
  const hsk_shard_ws x = hsk_shard_carve(sh->shard_ws, st->max_batch, st->max_cols, sh->capacity, sh->entry_cap);
  return hsk_launch_flush(st, w, (hipStream_t)stream_, 3, x.poison);
}

extern "C" int hsk_shard_last_batch(const hsk_bprmf_shard* sh, int32_t set, int64_t batch, int32_t* offs_out,
                                    int32_t* items_out, int32_t* u_out, hsk_stream_t stream_) {
  int rc = hsk_shard_check(sh);
  if (rc) return rc;
  HSK_REQUIRE(offs_out && items_out && u_out && (set == 0 || set == 1) && batch > 0, HSK_ERR_INVALID, "bad argument");
  const hsk_bprmf_state* st = &sh->base;
  const int64_t G = (int64_t)sh->world * batch;
  HSK_REQUIRE(G <= st->max_batch, HSK_ERR_INVALID, "batch too large");
  const hsk_ws w = hsk_select(hsk_carve_st(st), set);
  const hsk_shard_ws x = hsk_shard_carve(sh->shard_ws, st->max_batch, st->max_cols, sh->capacity, sh->entry_cap);
  const int64_t n = std::max<int64_t>(G + 1, sh->entry_cap);
  k_shard_copy_batch<<<(unsigned)hsk_ceil_div(n, 256), 256, 0, (hipStream_t)stream_>>>(
      x.offs[set], w.it32, w.u32, (int)G, (int)sh->entry_cap, offs_out, items_out, u_out);
  HSK_LAUNCH_CHECK();
  return HSK_OK;
}
