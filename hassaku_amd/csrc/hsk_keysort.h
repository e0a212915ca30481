// hsk_keysort.h -- the stable key sort of hsk_sort.h for the operators outside hsk_fused.hip (whose kernels it shares):
// n keys in [0, n_keys), written by the caller into `it32`, come back as
//   perm    [n]           positions grouped by key, ascending position inside a key
//   offsets [n_keys + 1]  where each key's group starts in perm.
// Deterministic, no atomics on global memory.  hsk_embedding_backward and hsk_sparse_rows_sum_backward sum gradient
// rows in that order.
#pragma once
#include "hsk_common.h"

struct hsk_keysort {
  int* it32;     // in: the keys
  int2* perm1;   // scratch
  int *perm, *hist, *btot, *bstart, *offsets;
  int64_t total;   // bytes carved
};

// false: more keys than the two-level sort holds counters for
bool hsk_keysort_supported(int64_t n_keys, int64_t n);
// base == NULL: only `total` is meaningful; base must be 256-byte aligned
hsk_keysort hsk_keysort_carve(void* base, int64_t n_keys, int64_t n);
int hsk_keysort_run(const hsk_keysort& k, int64_t n_keys, int64_t n, hipStream_t stream);
