// hsk_rccl.inc -- the sharded step issued from C, its collectives called through a table of function pointers
// (included by hsk_fused.hip).
//
// hassaku_amd/dist.py drives the phases of hsk_shard.inc from Python with torch.distributed collectives in between: ten
// Python -> C / torch dispatches per step, ~10 us of host time each, and the GPU idles in the gaps (86 us of a 322 us
// step at the ml10m shape on one rank, profiles/probes r2_shard timeline).  hsk_shard_step issues the whole step from
// one C call: the same kernels in the same order, all_gather / all_reduce / reduce_scatter enqueued between them -- the
// gradients' way home on a communication stream (fork / join by events) so that the item pass overlaps it.  Results
// are identical to the phased path (same kernels, same arithmetic; the collectives move the same bytes).
//
// Two collective tables are built in:
//   RCCL          ncclAllGather / ncclAllReduce / ncclReduceScatter on the library's own communicator.  RCCL is resolved
//                 at run time (dlopen of librccl.so.1, the copy PyTorch has already loaded if there is one): the library
//                 has no load-time dependency on it; where <rccl/rccl.h> is absent at build time only this table is lost.
//   host-staged   ranks that are PROCESSES SHARING ONE GPU (RCCL refuses two ranks of a communicator on one device):
//                 every collective is a device -> shared-memory copy, a host function on the stream (inter-process
//                 barrier + the reduction in rank order), and a copy back.  Slow and exact; it exists so that
//                 hsk_shard_step itself -- fork order, the two-stream use of one communicator, buffer offsets at C*D --
//                 runs at world 2, 3 on a one-GPU box (tests/test_dist.py), not as a way to train.
// A caller may inject any other table (hsk_shard_rt_create_with).
#include <dlfcn.h>
#include <fcntl.h>
#include <sched.h>
#include <sys/mman.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <mutex>
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#define HSK_HAVE_RCCL 1
#else
#define HSK_HAVE_RCCL 0
#endif

// runtime of the natively issued sharded step: the collectives, the side streams, the batch prepared a step ahead
struct hsk_shard_rt {
  hsk_collectives coll = {};
  int world = 0, rank = 0;
  hipStream_t side = nullptr;     // preparation of the next batch
  hipStream_t cs = nullptr;       // the gradients' way home + the owners' user update
  hipEvent_t ev_fork = nullptr, ev_ready = nullptr, ev_rs_in = nullptr, ev_rs = nullptr;
  bool pf_valid = false;          // a batch prepared for the next step sits in set pf_set
  const int64_t* pf_order = nullptr;
  int64_t pf_start = 0, pf_batch = 0, pf_step = 0;
  int pf_set = 0, cur_set = 0;
};

// =============================================================================================
// table 1: RCCL
// =============================================================================================
#if HSK_HAVE_RCCL
struct hsk_rccl_api {
  ncclResult_t (*GetUniqueId)(ncclUniqueId*);
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int);
  ncclResult_t (*CommDestroy)(ncclComm_t);
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t);
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
  ncclResult_t (*ReduceScatter)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
  const char* (*GetErrorString)(ncclResult_t);
  bool ok = false;
};

static const hsk_rccl_api* hsk_rccl() {
  static hsk_rccl_api api;
  static std::once_flag once;
  std::call_once(once, [] {
    void* h = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (h) break;
    }
    if (!h) return;
#define HSK_SYM(field, sym)                         \
  api.field = (decltype(api.field))dlsym(h, sym);   \
  if (!api.field) return
    HSK_SYM(GetUniqueId, "ncclGetUniqueId");
    HSK_SYM(CommInitRank, "ncclCommInitRank");
    HSK_SYM(CommDestroy, "ncclCommDestroy");
    HSK_SYM(AllGather, "ncclAllGather");
    HSK_SYM(AllReduce, "ncclAllReduce");
    HSK_SYM(ReduceScatter, "ncclReduceScatter");
    HSK_SYM(GetErrorString, "ncclGetErrorString");
#undef HSK_SYM
    api.ok = true;
  });
  return api.ok ? &api : nullptr;
}

struct hsk_rccl_ctx {
  const hsk_rccl_api* api;
  ncclComm_t comm;
};
#define HSK_NCCL(call)                                                                                 \
  do {                                                                                                 \
    ncclResult_t r_ = (call);                                                                          \
    if (r_ != ncclSuccess) {                                                                           \
      hsk_set_error("%s failed: %s (%s:%d)", #call, c->api->GetErrorString(r_), __FILE__, __LINE__);    \
      return HSK_ERR_HIP;                                                                              \
    }                                                                                                  \
  } while (0)
static int hsk_rccl_all_gather(void* ctx, const float* send, float* recv, int64_t count, hsk_stream_t s) {
  hsk_rccl_ctx* c = (hsk_rccl_ctx*)ctx;
  HSK_NCCL(c->api->AllGather(send, recv, (size_t)count, ncclFloat, c->comm, (hipStream_t)s));
  return HSK_OK;
}
static int hsk_rccl_all_reduce(void* ctx, float* buf, int64_t count, hsk_stream_t s) {
  hsk_rccl_ctx* c = (hsk_rccl_ctx*)ctx;
  HSK_NCCL(c->api->AllReduce(buf, buf, (size_t)count, ncclFloat, ncclSum, c->comm, (hipStream_t)s));
  return HSK_OK;
}
static int hsk_rccl_reduce_scatter(void* ctx, const float* send, float* recv, int64_t count, hsk_stream_t s) {
  hsk_rccl_ctx* c = (hsk_rccl_ctx*)ctx;
  HSK_NCCL(c->api->ReduceScatter(send, recv, (size_t)count, ncclFloat, ncclSum, c->comm, (hipStream_t)s));
  return HSK_OK;
}
#undef HSK_NCCL
static void hsk_rccl_destroy(void* ctx) {
  hsk_rccl_ctx* c = (hsk_rccl_ctx*)ctx;
  if (c && c->comm) (void)c->api->CommDestroy(c->comm);
  delete c;
}
#endif  // HSK_HAVE_RCCL

extern "C" int hsk_rccl_available(void) {
#if HSK_HAVE_RCCL
  return hsk_rccl() != nullptr;
#else
  return 0;
#endif
}

// rank 0: 128 bytes to hand to every rank (any transport: the caller broadcasts them)
extern "C" int hsk_rccl_unique_id(void* id128) {
#if HSK_HAVE_RCCL
  const hsk_rccl_api* api = hsk_rccl();
  HSK_REQUIRE(api != nullptr, HSK_ERR_UNSUPPORTED, "RCCL (librccl.so.1) could not be loaded");
  HSK_REQUIRE(id128 != nullptr, HSK_ERR_INVALID, "id buffer is NULL");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  ncclUniqueId id;
  const ncclResult_t r = api->GetUniqueId(&id);
  HSK_REQUIRE(r == ncclSuccess, HSK_ERR_HIP, "ncclGetUniqueId failed: %s", api->GetErrorString(r));
  memcpy(id128, &id, sizeof(id));
  return HSK_OK;
#else
  (void)id128;
  hsk_set_error("this build has no RCCL support (<rccl/rccl.h> was absent)");
  return HSK_ERR_UNSUPPORTED;
#endif
}

// =============================================================================================
// table 2: host-staged collectives between processes that share one GPU (test backend)
// =============================================================================================
#define HSK_HOSTCOLL_MAGIC "HSKSHM1"
#define HSK_HOSTCOLL_TIMEOUT_S 60.0
struct hsk_hostcoll_hdr {   // at the head of the shared segment (fresh shared memory is zero-filled)
  std::atomic<uint32_t> arrived;
  std::atomic<uint32_t> gen;
  std::atomic<uint32_t> failed;
  uint32_t pad[61];
};
struct hsk_hostcoll {
  int world = 0, rank = 0;
  int64_t max_floats = 0;       // largest per-rank send of one collective
  void* map = nullptr;
  size_t map_bytes = 0;
  bool registered = false;      // the segment is pinned for the device (async copies); otherwise pageable copies
  hsk_hostcoll_hdr* hdr = nullptr;
  float* slots = nullptr;       // world x max_floats; rank r's send of the running collective at r * (floats sent)
  float* priv = nullptr;        // pinned, max_floats: this rank's reduced result
  struct op_t {                 // what the next host function on the stream completes
    hsk_hostcoll* c;
    int kind;                   // 0: barrier only, 1: all_reduce, 2: reduce_scatter
    int64_t count;
  };
};

// One collective is in flight per rank at any time (hsk_shard_step orders its two streams by events), so the barrier has
// one participant per rank.  A rank that waits longer than the timeout marks the segment failed: everybody errors out
// instead of hanging.
static bool hsk_hostcoll_barrier(hsk_hostcoll* c, double timeout_s) {
  hsk_hostcoll_hdr* h = c->hdr;
  if (h->failed.load()) return false;
  const uint32_t g = h->gen.load();
  if (h->arrived.fetch_add(1) + 1 == (uint32_t)c->world) {
    h->arrived.store(0);
    h->gen.store(g + 1);
    return true;
  }
  const auto t0 = std::chrono::steady_clock::now();
  while (h->gen.load() == g) {
    sched_yield();
    if (h->failed.load() || std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s) {
      h->failed.store(1);
      return false;
    }
  }
  return true;
}

// host function on the stream: all ranks' sends are in the segment -> reduce what this rank needs, in rank order
static void hsk_hostcoll_cb(void* p) {
  hsk_hostcoll::op_t* op = (hsk_hostcoll::op_t*)p;
  hsk_hostcoll* c = op->c;
  if (hsk_hostcoll_barrier(c, HSK_HOSTCOLL_TIMEOUT_S) && op->kind != 0) {
    const int64_t n = op->count;
    const int64_t stride = op->kind == 2 ? (int64_t)c->world * n : n;   // reduce_scatter: every rank sent world * n
    const int64_t off = op->kind == 2 ? (int64_t)c->rank * n : 0;
    for (int64_t j = 0; j < n; ++j) c->priv[j] = c->slots[off + j];
    for (int r = 1; r < c->world; ++r) {
      const float* src = c->slots + (int64_t)r * stride + off;
      for (int64_t j = 0; j < n; ++j) c->priv[j] += src[j];
    }
  }
  delete op;
}

static int hsk_hostcoll_enqueue_cb(hsk_hostcoll* c, int kind, int64_t count, hipStream_t s) {
  hsk_hostcoll::op_t* op = new hsk_hostcoll::op_t{c, kind, count};
  const hipError_t e = hipLaunchHostFunc(s, hsk_hostcoll_cb, op);
  if (e != hipSuccess) {
    delete op;
    hsk_set_error("hipLaunchHostFunc failed: %s", hipGetErrorString(e));
    return HSK_ERR_HIP;
  }
  return HSK_OK;
}

static int hsk_hostcoll_check(hsk_hostcoll* c, int64_t send_floats) {
  HSK_REQUIRE(!c->hdr->failed.load(), HSK_ERR_HIP, "host-staged collective: a rank failed or timed out earlier");
  HSK_REQUIRE(send_floats >= 0 && send_floats <= c->max_floats, HSK_ERR_INVALID,
              "host-staged collective of %lld floats per rank above the %lld the segment was sized for",
              (long long)send_floats, (long long)c->max_floats);
  return HSK_OK;
}

static int hsk_hostcoll_all_gather(void* ctx, const float* send, float* recv, int64_t count, hsk_stream_t s_) {
  hsk_hostcoll* c = (hsk_hostcoll*)ctx;
  hipStream_t s = (hipStream_t)s_;
  int rc = hsk_hostcoll_check(c, count);
  if (rc) return rc;
  HSK_HIP(hipMemcpyAsync(c->slots + (int64_t)c->rank * count, send, (size_t)count * 4, hipMemcpyDeviceToHost, s));
  if ((rc = hsk_hostcoll_enqueue_cb(c, 0, 0, s))) return rc;
  HSK_HIP(hipMemcpyAsync(recv, c->slots, (size_t)c->world * count * 4, hipMemcpyHostToDevice, s));
  return hsk_hostcoll_enqueue_cb(c, 0, 0, s);   // nobody overwrites the segment before everybody has read it
}

static int hsk_hostcoll_all_reduce(void* ctx, float* buf, int64_t count, hsk_stream_t s_) {
  hsk_hostcoll* c = (hsk_hostcoll*)ctx;
  hipStream_t s = (hipStream_t)s_;
  int rc = hsk_hostcoll_check(c, count);
  if (rc) return rc;
  HSK_HIP(hipMemcpyAsync(c->slots + (int64_t)c->rank * count, buf, (size_t)count * 4, hipMemcpyDeviceToHost, s));
  if ((rc = hsk_hostcoll_enqueue_cb(c, 1, count, s))) return rc;
  HSK_HIP(hipMemcpyAsync(buf, c->priv, (size_t)count * 4, hipMemcpyHostToDevice, s));
  return hsk_hostcoll_enqueue_cb(c, 0, 0, s);
}

static int hsk_hostcoll_reduce_scatter(void* ctx, const float* send, float* recv, int64_t count, hsk_stream_t s_) {
  hsk_hostcoll* c = (hsk_hostcoll*)ctx;
  hipStream_t s = (hipStream_t)s_;
  const int64_t total = (int64_t)c->world * count;
  int rc = hsk_hostcoll_check(c, total);
  if (rc) return rc;
  HSK_HIP(hipMemcpyAsync(c->slots + (int64_t)c->rank * total, send, (size_t)total * 4, hipMemcpyDeviceToHost, s));
  if ((rc = hsk_hostcoll_enqueue_cb(c, 2, count, s))) return rc;
  HSK_HIP(hipMemcpyAsync(recv, c->priv, (size_t)count * 4, hipMemcpyHostToDevice, s));
  return hsk_hostcoll_enqueue_cb(c, 0, 0, s);
}

static void hsk_hostcoll_destroy(void* ctx) {
  hsk_hostcoll* c = (hsk_hostcoll*)ctx;
  if (!c) return;
  if (c->priv) (void)hipHostFree(c->priv);
  if (c->registered) (void)hipHostUnregister(c->map);
  if (c->map) munmap(c->map, c->map_bytes);
  delete c;
}

// 128 bytes naming a fresh shared segment: magic, the largest per-rank send in floats, the segment's name
extern "C" int hsk_hostcoll_unique_id(int64_t max_floats, void* id128) {
  HSK_REQUIRE(id128 != nullptr && max_floats > 0, HSK_ERR_INVALID, "bad argument");
  char* p = (char*)id128;
  memset(p, 0, 128);
  memcpy(p, HSK_HOSTCOLL_MAGIC, 8);
  memcpy(p + 8, &max_floats, 8);
  const unsigned long long t = (unsigned long long)std::chrono::steady_clock::now().time_since_epoch().count();
  snprintf(p + 16, 100, "/hsk_coll_%d_%llx", (int)getpid(), t);
  return HSK_OK;
}

static hsk_hostcoll* hsk_hostcoll_open(int world, int rank, const char* id128) {
  int64_t max_floats = 0;
  memcpy(&max_floats, id128 + 8, 8);
  const char* name = id128 + 16;
  if (max_floats <= 0 || name[0] != '/' || memchr(name, 0, 100) == nullptr) {
    hsk_set_error("host-staged collectives: malformed id");
    return nullptr;
  }
  hsk_hostcoll* c = new hsk_hostcoll();
  c->world = world;
  c->rank = rank;
  c->max_floats = max_floats;
  c->map_bytes = sizeof(hsk_hostcoll_hdr) + (size_t)world * (size_t)max_floats * 4;
  const int fd = shm_open(name, O_CREAT | O_RDWR, 0600);
  bool ok = fd >= 0 && ftruncate(fd, (off_t)c->map_bytes) == 0;
  if (ok) {
    c->map = mmap(nullptr, c->map_bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    ok = c->map != MAP_FAILED;
    if (!ok) c->map = nullptr;
  }
  if (fd >= 0) close(fd);
  if (!ok) {
    hsk_set_error("host-staged collectives: cannot map the shared segment %s", name);
    hsk_hostcoll_destroy(c);
    return nullptr;
  }
  c->hdr = (hsk_hostcoll_hdr*)c->map;
  c->slots = (float*)((char*)c->map + sizeof(hsk_hostcoll_hdr));
  c->registered = hipHostRegister(c->map, c->map_bytes, hipHostRegisterDefault) == hipSuccess;
  if (!c->registered) (void)hipGetLastError();   // pageable copies then: slower, same order
  if (hipHostMalloc((void**)&c->priv, (size_t)max_floats * 4, hipHostMallocDefault) != hipSuccess) {
    hsk_set_error("host-staged collectives: cannot allocate the pinned result buffer");
    c->priv = nullptr;
    hsk_hostcoll_destroy(c);
    return nullptr;
  }
  // every rank has the segment mapped before its name goes away
  const bool met = hsk_hostcoll_barrier(c, 2.0 * HSK_HOSTCOLL_TIMEOUT_S);
  if (rank == 0) shm_unlink(name);
  if (!met) {
    hsk_set_error("host-staged collectives: the %d ranks did not all arrive", world);
    hsk_hostcoll_destroy(c);
    return nullptr;
  }
  return c;
}

// =============================================================================================
// runtime handle
// =============================================================================================
extern "C" void hsk_shard_rt_destroy(void* rt_) {
  hsk_shard_rt* rt = (hsk_shard_rt*)rt_;
  if (!rt) return;
  if (rt->side) (void)hipStreamSynchronize(rt->side);
  if (rt->cs) (void)hipStreamSynchronize(rt->cs);
  if (rt->coll.destroy) rt->coll.destroy(rt->coll.ctx);
  for (hipEvent_t e : {rt->ev_fork, rt->ev_ready, rt->ev_rs_in, rt->ev_rs})
    if (e) (void)hipEventDestroy(e);
  if (rt->side) (void)hipStreamDestroy(rt->side);
  if (rt->cs) (void)hipStreamDestroy(rt->cs);
  delete rt;
}

// takes ownership of coll->ctx (destroyed with the handle, or right here on failure)
extern "C" void* hsk_shard_rt_create_with(int32_t world, int32_t rank, const hsk_collectives* coll) {
  if (world < 1 || world > 64 || rank < 0 || rank >= world || !coll || !coll->all_gather || !coll->all_reduce_sum ||
      !coll->reduce_scatter_sum) {
    hsk_set_error("hsk_shard_rt_create_with: bad world / rank / collective table");
    if (coll && coll->destroy) coll->destroy(coll->ctx);
    return nullptr;
  }
  hsk_shard_rt* rt = new hsk_shard_rt();
  rt->coll = *coll;
  rt->world = world;
  rt->rank = rank;
  int lo = 0, hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
  bool ok = hipStreamCreateWithPriority(&rt->side, hipStreamNonBlocking, hi) == hipSuccess;
  ok = ok && hipStreamCreateWithPriority(&rt->cs, hipStreamNonBlocking, hi) == hipSuccess;
  for (hipEvent_t* e : {&rt->ev_fork, &rt->ev_ready, &rt->ev_rs_in, &rt->ev_rs})
    ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    hsk_set_error("hsk_shard_rt_create: could not create the streams / events");
    hsk_shard_rt_destroy(rt);
    return nullptr;
  }
  return rt;
}

// collective over the job: every rank calls it with the same 128 bytes (hsk_rccl_unique_id, or hsk_hostcoll_unique_id for
// ranks sharing one GPU); the current HIP device is the rank's GPU
extern "C" void* hsk_shard_rt_create(int32_t world, int32_t rank, const void* id128) {
  if (world < 1 || rank < 0 || rank >= world || !id128) {
    hsk_set_error("hsk_shard_rt_create: bad world / rank / id");
    return nullptr;
  }
  hsk_collectives t = {};
  if (memcmp(id128, HSK_HOSTCOLL_MAGIC, 8) == 0) {
    hsk_hostcoll* c = hsk_hostcoll_open(world, rank, (const char*)id128);
    if (!c) return nullptr;
    t = hsk_collectives{c, hsk_hostcoll_all_gather, hsk_hostcoll_all_reduce, hsk_hostcoll_reduce_scatter,
                        hsk_hostcoll_destroy, "host-staged"};
    return hsk_shard_rt_create_with(world, rank, &t);
  }
#if HSK_HAVE_RCCL
  const hsk_rccl_api* api = hsk_rccl();
  if (!api) {
    hsk_set_error("RCCL (librccl.so.1) could not be loaded");
    return nullptr;
  }
  hsk_rccl_ctx* c = new hsk_rccl_ctx{api, nullptr};
  ncclUniqueId id;
  memcpy(&id, id128, sizeof(id));
  const ncclResult_t r = api->CommInitRank(&c->comm, world, id, rank);
  if (r != ncclSuccess) {
    hsk_set_error("ncclCommInitRank failed: %s", api->GetErrorString(r));
    delete c;
    return nullptr;
  }
  t = hsk_collectives{c, hsk_rccl_all_gather, hsk_rccl_all_reduce, hsk_rccl_reduce_scatter, hsk_rccl_destroy, "rccl"};
  return hsk_shard_rt_create_with(world, rank, &t);
#else
  hsk_set_error("this build has no RCCL support (<rccl/rccl.h> was absent)");
  return nullptr;
#endif
}

extern "C" const char* hsk_shard_rt_backend(const void* rt_) {
  const hsk_shard_rt* rt = (const hsk_shard_rt*)rt_;
  return rt && rt->coll.name ? rt->coll.name : "";
}

// a prepared batch that the next step does not consume: give its owner map back
static int hsk_shard_rt_discard(hsk_bprmf_shard* sh, hsk_shard_rt* rt, hipStream_t stream) {
  if (!rt->pf_valid) return HSK_OK;
  HSK_HIP(hipStreamWaitEvent(stream, rt->ev_ready, 0));
  rt->pf_valid = false;
  return hsk_shard_discard(sh, rt->pf_set, stream);
}

extern "C" int hsk_shard_rt_cur_set(const void* rt_) { return rt_ ? ((const hsk_shard_rt*)rt_)->cur_set : 0; }

extern "C" int hsk_shard_rt_discard_prefetch(hsk_bprmf_shard* sh, void* rt_, hsk_stream_t stream_) {
  HSK_REQUIRE(sh && rt_, HSK_ERR_INVALID, "NULL argument");
  return hsk_shard_rt_discard(sh, (hsk_shard_rt*)rt_, (hipStream_t)stream_);
}

extern "C" int hsk_shard_rt_flush(hsk_bprmf_shard* sh, void* rt_, hsk_stream_t stream_) {
  hsk_shard_rt* rt = (hsk_shard_rt*)rt_;
  HSK_REQUIRE(sh && rt, HSK_ERR_INVALID, "NULL argument");
  int rc = hsk_shard_rt_discard(sh, rt, (hipStream_t)stream_);
  if (rc) return rc;
  return hsk_shard_flush(sh, stream_);
}

// the enqueued part of hsk_shard_step; *forked_side / *forked_cs: what has to be joined back if it fails half-way
static int hsk_shard_step_enqueue(hsk_bprmf_shard* sh, hsk_shard_rt* rt, const int64_t* order, int64_t start_global,
                                  int64_t batch, int64_t n_neg, int64_t next_start, int64_t nb, hipStream_t stream,
                                  bool* forked_side, bool* forked_cs) {
  hsk_bprmf_state* st = &sh->base;
  const int64_t G = (int64_t)sh->world * batch;
  const int64_t D = st->dim, C = sh->capacity;
  const hsk_collectives& co = rt->coll;
  int rc;
  int set;
  if (rt->pf_valid && rt->pf_order == order && rt->pf_start == start_global && rt->pf_batch == batch &&
      rt->pf_step == st->step) {
    HSK_HIP(hipStreamWaitEvent(stream, rt->ev_ready, 0));   // sampled + sorted during the previous step
    set = rt->pf_set;
    rt->pf_valid = false;
  } else {
    if ((rc = hsk_shard_rt_discard(sh, rt, stream))) return rc;
    set = rt->cur_set ^ 1;
    if ((rc = hsk_shard_prepare(sh, order, start_global, batch, n_neg, set, stream))) return rc;
  }
  rt->cur_set = set;
  // The preparation of the NEXT batch (sample + keep, routing, item sort) is forked onto the side stream FIRST, in front
  // of this step's catch-up / pack / all_gather / positive scores: those are short launches that leave the chip nearly
  // idle, and the routing kernels' 1024-thread workgroups need a whole CU's wave slots at once -- forked behind the pack
  // they met the forward, which refills every slot a finishing workgroup frees, and sat there until it drained (81-87 us
  // for a 7 us kernel in the timeline), which made the side chain as long as the step itself: 281 -> 270 us per step.
  // (Also tried on top of it, tested bit-equal and measured slower, 281 against 270 us: replaying the NEXT batch's user
  // rows -- those this batch does not train on, told apart by a per-row request stamp -- behind the routing on the side
  // stream, so that the catch-up that opens the next step finds them current.)
  if (next_start >= 0) {
    HSK_HIP(hipEventRecord(rt->ev_fork, stream));
    HSK_HIP(hipStreamWaitEvent(rt->side, rt->ev_fork, 0));
    *forked_side = true;
    if ((rc = hsk_shard_prepare_impl(sh, order, next_start, nb, n_neg, set ^ 1, rt->side, 1))) return rc;
    HSK_HIP(hipEventRecord(rt->ev_ready, rt->side));
    *forked_side = false;   // (ev_ready is what the next call joins on)
    rt->pf_valid = true;
    rt->pf_order = order;
    rt->pf_start = next_start;
    rt->pf_batch = nb;
    rt->pf_step = st->step + 1;
    rt->pf_set = set ^ 1;
  }
  if ((rc = hsk_shard_pack(sh, batch, n_neg, set, stream))) return rc;
  // owner -> everyone: the batch's user rows.  On the step's own stream: nothing of the step can run before they have
  // arrived, and a hop to another stream and back costs ~2 x 11 us of cross-stream signalling (measured).
  if ((rc = co.all_gather(co.ctx, sh->rows_send, sh->rows_all, C * D, stream))) return rc;
  if ((rc = hsk_shard_pos_scores(sh, stream))) return rc;
  // what couples a positive to its negatives across the ranks, by loss (hassaku_hip.h): bpr two [G] sums, bce nothing,
  // sampled softmax one all_gather of the ranks' (max, normaliser, s0) triples
  const int loss = st->loss_kind;
  if (loss == HSK_LOSS_BPR && (rc = co.all_reduce_sum(co.ctx, sh->s0, G, stream))) return rc;
  if ((rc = hsk_shard_forward(sh, stream))) return rc;
  if (loss == HSK_LOSS_BPR && (rc = co.all_reduce_sum(co.ctx, sh->gsum, G, stream))) return rc;
  if (loss == HSK_LOSS_SSM && (rc = co.all_gather(co.ctx, sh->ssm_send, sh->ssm_all, 3 * G, stream))) return rc;
  if ((rc = hsk_shard_pos_fix(sh, stream))) return rc;
  // everyone -> owner: the user-row gradients and, behind them on the same (communication) stream, the owners' user
  // update -- both beside the local item pass on the step's stream (different tables; the user update reads the
  // exchanged gradients, the item pass the gathered rows).  One join at the end instead of a hop there and back.
  HSK_HIP(hipEventRecord(rt->ev_rs_in, stream));
  HSK_HIP(hipStreamWaitEvent(rt->cs, rt->ev_rs_in, 0));
  *forked_cs = true;
  if ((rc = co.reduce_scatter_sum(co.ctx, sh->dU_all, sh->grads_mine, C * D, rt->cs))) return rc;
  if ((rc = hsk_shard_apply_items(sh, stream))) return rc;
  const int64_t step_before = st->step;
  if ((rc = hsk_shard_apply_users_impl(sh, rt->cs, false))) return rc;
  // HSK_SHARD_AHEAD=1 (off by default): behind THAT, the pending zero-gradient steps of the NEXT batch's user rows (its
  // request list is ready once its preparation is), so that the next step's pack finds them current; rows of the batch
  // just trained on were rewritten by the update in front and are skipped as current.  Measured on one rank at the
  // ml10m shape, three alternations on one box: 286-288 us per step without, 295-300 with -- the communication stream's
  // chain (exchange + update + replay) then outlasts the item pass it runs beside, and the join waits for it.
  static const int ahead_on = hsk_env_int("HSK_SHARD_AHEAD", 0);
  if (rt->pf_valid && ahead_on) {
    HSK_HIP(hipStreamWaitEvent(rt->cs, rt->ev_ready, 0));
    if ((rc = hsk_shard_catch_up_rows(sh, rt->pf_set, st->step + 1, rt->cs, false))) return rc;
  }
  HSK_HIP(hipEventRecord(rt->ev_rs, rt->cs));
  HSK_HIP(hipStreamWaitEvent(stream, rt->ev_rs, 0));
  *forked_cs = false;
  const hsk_ws w = hsk_carve_st(st);
  const hsk_shard_ws x = hsk_shard_carve(sh->shard_ws, st->max_batch, st->max_cols, sh->capacity, sh->entry_cap);
  return hsk_periodic_flush(st, w, stream, step_before, (double)sh->capacity, (double)sh->entry_cap, x.poison);
}

// ONE global step: positives = interactions order[start_global .. + world*batch).  next_start >= 0 names the batch of
// the following call (next_batch positives per rank): it is sampled, routed and item-sorted on the side stream while
// this step's exchanges run.  Same results as the phase-by-phase sequence of hassaku_hip.h.
// Everything that can be refused is refused BEFORE anything is enqueued (a rank that raises after its peers have
// entered a collective leaves them blocked there); a failure after that point (a launch or collective error) joins the
// forked streams back, drops the step and the prepared batch, and leaves the state idle.
extern "C" int hsk_shard_step(hsk_bprmf_shard* sh, void* rt_, const int64_t* order, int64_t start_global, int64_t batch,
                              int64_t n_neg, int64_t next_start, int64_t next_batch, hsk_stream_t stream_) {
  hsk_shard_rt* rt = (hsk_shard_rt*)rt_;
  HSK_REQUIRE(sh && rt, HSK_ERR_INVALID, "NULL argument");
  HSK_REQUIRE(rt->world == sh->world && rt->rank == sh->rank, HSK_ERR_INVALID, "runtime / state disagree on world, rank");
  int rc = hsk_shard_check(sh);
  if (rc) return rc;
  if ((rc = hsk_shard_check_batch(sh, batch, n_neg))) return rc;
  HSK_REQUIRE(sh->phase == HSK_SHARD_IDLE, HSK_ERR_INVALID, "hsk_shard_step while a step is in flight");
  const hsk_bprmf_state* st = &sh->base;
  const int64_t G = (int64_t)sh->world * batch;
  HSK_REQUIRE(start_global >= 0 && start_global + G <= st->nnz, HSK_ERR_INVALID,
              "global interaction range [%lld, %lld) outside nnz %lld", (long long)start_global,
              (long long)(start_global + G), (long long)st->nnz);
  const int64_t nb = next_batch > 0 ? next_batch : batch;
  if (next_start >= 0) {
    if ((rc = hsk_shard_check_batch(sh, nb, n_neg))) return rc;
    HSK_REQUIRE(next_start + (int64_t)sh->world * nb <= st->nnz, HSK_ERR_INVALID,
                "next batch [%lld, %lld) outside nnz %lld", (long long)next_start,
                (long long)(next_start + (int64_t)sh->world * nb), (long long)st->nnz);
  }
  hipStream_t stream = (hipStream_t)stream_;
  bool forked_side = false, forked_cs = false;
  rc = hsk_shard_step_enqueue(sh, rt, order, start_global, batch, n_neg, next_start, nb, stream, &forked_side, &forked_cs);
  if (rc == HSK_OK) return rc;
  // keep the first error's text; whatever ran on the other streams is ordered in front of the caller's next work
  if (forked_side && hipEventRecord(rt->ev_ready, rt->side) == hipSuccess) (void)hipStreamWaitEvent(stream, rt->ev_ready, 0);
  if (forked_cs && hipEventRecord(rt->ev_rs, rt->cs) == hipSuccess) (void)hipStreamWaitEvent(stream, rt->ev_rs, 0);
  (void)hipGetLastError();
  rt->pf_valid = false;
  sh->phase = HSK_SHARD_IDLE;
  sh->cur_batch = sh->cur_cols = 0;
  return rc;
}
