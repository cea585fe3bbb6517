// api_ctx.cpp — contexts of the C ABI (include/m3d.h): the error text, kernel timers, the device block
// cache and the live-context registry, the context-owned scratch (the arena, the pinned page, the
// preprocessing buffer: api_internal.h), create / destroy, statistics and profiling.
#include <string.h>

#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "api_internal.h"

using namespace m3d;
using namespace m3d::api;

int m3d_fail(m3d_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}

KTimer::KTimer(m3d_ctx* c, int kid, hipStream_t s) : ctx(c), id(kid), st(s) {
  if (!ctx || !ctx->profiling) return;
  auto& v = ctx->ev[id];
  size_t k = ctx->ev_used[id];
  if (k >= 65536) return;  // cap; read regularly
  if (k == v.size()) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess) return;
    if (hipEventCreate(&b) != hipSuccess) {
      hipEventDestroy(a);
      return;
    }
    v.emplace_back(a, b);
  }
  if (hipEventRecord(v[k].first, st) != hipSuccess) return;
  end = v[k].second;
  ctx->ev_used[id] = k + 1;
}

KTimer::~KTimer() {
  if (end) hipEventRecord(end, st);
}

namespace m3d {
// ------------------------------------------------------------------------------- block cache
// Released device blocks (clouds, grids, Morton copies, target records, MFMA tiles) wait in a
// process-wide cache for an allocation of a size in [need, 2·need].  Each carries the RELEASE
// MARK of the object that freed it: an event recorded, on its context's order stream, after
// every stream the context had enqueued work on (ctx_touch) up to the release — so a reuse only
// makes the ALLOCATING stream wait on the device (hipStreamWaitEvent) for the work that could
// still read the block, never the host, and never work on streams the context never used.
// Blocks freed outside a release scope (a rebuild inside a call) have no mark and are reused
// after a hipDeviceSynchronize, as before round 5.  Bounded (M3D_BLOCK_CACHE MiB, default
// 2048; 64 blocks; oldest freed first); trimmed when the last context of a device is destroyed,
// by m3d_trim_block_cache, and before any device allocation of the library is retried after
// an out-of-memory failure (dev_malloc_raw).
namespace {
struct CachedBlock {
  void* p;
  size_t bytes;
  int dev;
  std::shared_ptr<ReleaseMark> mark;  // null: unknown users, device sync before reuse
};
// The cache's state lives in one heap object that is never destroyed: objects (and their
// marks) may still be released while static destructors run at process exit.
struct CacheState {
  std::mutex mu;
  std::vector<CachedBlock> blocks;  // released, oldest first
  std::unordered_map<void*, std::pair<size_t, int>> live;  // from block_alloc: size, device
  std::mutex ev_mu;  // guards ev_retired; taken after mu (a mark may die under mu)
  std::vector<hipEvent_t> ev_retired;  // marks' events, destroyed once complete
  std::unordered_map<int, int> ctx_per_dev;  // live contexts per device
  std::unordered_map<const m3d_ctx*, uint64_t> ctx_ids;  // live contexts and their ids
  uint64_t next_id = 1;
  size_t bytes = 0;
};
CacheState& cache_state() {
  static CacheState* p = new CacheState();
  return *p;
}
std::mutex& g_bc_mu = cache_state().mu;
std::vector<CachedBlock>& g_bc = cache_state().blocks;
std::unordered_map<void*, std::pair<size_t, int>>& g_bc_live = cache_state().live;
std::mutex& g_ev_mu = cache_state().ev_mu;
std::vector<hipEvent_t>& g_ev_retired = cache_state().ev_retired;
std::unordered_map<int, int>& g_ctx_live = cache_state().ctx_per_dev;
size_t& g_bc_bytes = cache_state().bytes;
constexpr size_t kBcMaxCount = 64;
thread_local std::shared_ptr<ReleaseMark> t_mark;  // the active ReleaseScope's mark

size_t bc_cap() {
  static const size_t cap = [] {
    const char* e = getenv("M3D_BLOCK_CACHE");
    const long long mib = e ? atoll(e) : 2048;
    return mib > 0 ? (size_t)mib << 20 : (size_t)0;
  }();
  return cap;
}
bool bc_on() { return bc_cap() > 0; }

void retire_events(bool wait) {
  std::lock_guard<std::mutex> lk(g_ev_mu);
  for (size_t k = 0; k < g_ev_retired.size();) {
    hipEvent_t ev = g_ev_retired[k];
    if (wait) (void)hipEventSynchronize(ev);
    if (hipEventQuery(ev) == hipSuccess) {
      (void)hipEventDestroy(ev);
      g_ev_retired[k] = g_ev_retired.back();
      g_ev_retired.pop_back();
    } else {
      ++k;
    }
  }
  (void)hipGetLastError();
}

// free cached blocks (of device dev, or every device when dev < 0) until the cache holds at most
// max_bytes / max_count; a block is freed only after its release point has passed on the device
size_t bc_trim_locked(int dev, size_t max_bytes, size_t max_count) {
  size_t freed = 0;
  for (size_t k = 0; k < g_bc.size() && (g_bc_bytes > max_bytes || g_bc.size() > max_count);) {
    CachedBlock& b = g_bc[k];
    if (dev >= 0 && b.dev != dev) {
      ++k;
      continue;
    }
    int cur = 0;
    (void)hipGetDevice(&cur);
    if (cur != b.dev) (void)hipSetDevice(b.dev);
    if (b.mark && b.mark->ev) (void)hipEventSynchronize(b.mark->ev);
    (void)hipFree(b.p);  // (hipFree itself waits for the device)
    if (cur != b.dev) (void)hipSetDevice(cur);
    g_bc_bytes -= b.bytes;
    freed += b.bytes;
    g_bc.erase(g_bc.begin() + (ptrdiff_t)k);
  }
  retire_events(false);
  return freed;
}
}  // namespace

ReleaseMark::~ReleaseMark() {
  if (ev == nullptr) return;
  std::lock_guard<std::mutex> lk(g_ev_mu);
  g_ev_retired.push_back(ev);
}

size_t block_cache_trim(int dev) {
  std::lock_guard<std::mutex> lk(g_bc_mu);
  return bc_trim_locked(dev, 0, 0);
}

hipError_t dev_malloc_raw(void** p, size_t bytes) {
  hipError_t e = hipMalloc(p, bytes);
  if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) {
    (void)hipGetLastError();
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (block_cache_trim(dev) > 0) e = hipMalloc(p, bytes);
  }
  if (e != hipSuccess) *p = nullptr;
  return e;
}

hipError_t block_alloc(void** out, size_t bytes, hipStream_t st) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (bc_on()) {
    std::unique_lock<std::mutex> lk(g_bc_mu);
    int best = -1;
    for (int k = 0; k < (int)g_bc.size(); ++k) {
      const CachedBlock& b = g_bc[(size_t)k];
      if (b.dev == dev && b.bytes >= bytes && b.bytes <= 2 * bytes && (best < 0 || b.bytes < g_bc[(size_t)best].bytes))
        best = k;
    }
    if (best >= 0) {
      const CachedBlock b = g_bc[(size_t)best];
      g_bc.erase(g_bc.begin() + best);
      g_bc_bytes -= b.bytes;
      g_bc_live[b.p] = {b.bytes, dev};
      lk.unlock();
      hipError_t e = hipSuccess;
      if (!b.mark)
        e = hipDeviceSynchronize();  // released outside a scope: unknown users
      else if (b.mark->ev != nullptr)
        e = hipStreamWaitEvent(st, b.mark->ev, 0);  // stream order: the allocating stream waits
      if (e != hipSuccess) {
        block_release(b.p);
        return e;
      }
      *out = b.p;
      return hipSuccess;
    }
  }
  void* p = nullptr;
  const hipError_t e = dev_malloc_raw(&p, bytes);
  if (e != hipSuccess) return e;
  if (bc_on()) {
    std::lock_guard<std::mutex> lk(g_bc_mu);
    g_bc_live[p] = {bytes, dev};
  }
  *out = p;
  return hipSuccess;
}

void block_release(void* p) {
  if (p == nullptr) return;
  if (bc_on()) {
    std::lock_guard<std::mutex> lk(g_bc_mu);
    auto it = g_bc_live.find(p);
    if (it != g_bc_live.end()) {
      g_bc.push_back(CachedBlock{p, it->second.first, it->second.second, t_mark});
      g_bc_bytes += it->second.first;
      g_bc_live.erase(it);
      bc_trim_locked(-1, bc_cap(), kBcMaxCount);
      return;
    }
  }
  (void)hipFree(p);
}

void ctx_touch(m3d_ctx* ctx, hipStream_t st) {
  if (ctx == nullptr) return;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
    (void)hipGetLastError();  // a capture: its graph launch is touched when it is replayed
    return;
  }
  std::lock_guard<std::mutex> lk(ctx->uses_mu);
  hipEvent_t ev = nullptr;
  for (auto& u : ctx->uses)
    if (u.first == st) ev = u.second;
  if (ev == nullptr) {
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
      ctx->uses_lost = true;  // no event: releases fall back to a device sync before reuse
      return;
    }
    ctx->uses.emplace_back(st, ev);
  }
  if (hipEventRecord(ev, st) != hipSuccess) ctx->uses_lost = true;
}

ReleaseScope::ReleaseScope(m3d_ctx* ctx, uint64_t ctx_id) {
  prev = t_mark;
  std::shared_ptr<ReleaseMark> m;
  if (ctx != nullptr) {  // a destroyed context (e.g. Python teardown order): no mark, device sync
    std::lock_guard<std::mutex> lk(g_bc_mu);
    auto it = cache_state().ctx_ids.find(ctx);
    if (it == cache_state().ctx_ids.end() || it->second != ctx_id) ctx = nullptr;
  }
  if (ctx != nullptr) {
    std::lock_guard<std::mutex> lk(ctx->uses_mu);  // destroys may run on finaliser threads
    // streams whose last touched work has completed need no wait: drop them (a destroyed
    // stream's entry goes this way too), so the list stays as long as the streams still busy
    for (size_t k = 0; k < ctx->uses.size();) {
      if (hipEventQuery(ctx->uses[k].second) == hipSuccess) {
        (void)hipEventDestroy(ctx->uses[k].second);
        ctx->uses[k] = ctx->uses.back();
        ctx->uses.pop_back();
      } else {
        ++k;
      }
    }
    (void)hipGetLastError();
    if (!ctx->uses_lost) {
      m = std::make_shared<ReleaseMark>();
      if (!ctx->uses.empty()) {
        int cur = 0;
        (void)hipGetDevice(&cur);  // the caller's (e.g. torch's) current device is left as it was
        if (cur != ctx->device) (void)hipSetDevice(ctx->device);
        bool ok = ctx->order != nullptr || hipStreamCreateWithFlags(&ctx->order, hipStreamNonBlocking) == hipSuccess;
        hipEvent_t ev = nullptr;
        ok = ok && hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess;
        for (auto& u : ctx->uses) ok = ok && hipStreamWaitEvent(ctx->order, u.second, 0) == hipSuccess;
        ok = ok && hipEventRecord(ev, ctx->order) == hipSuccess;
        if (ok) {
          m->ev = ev;
        } else {
          if (ev != nullptr) (void)hipEventDestroy(ev);
          m.reset();
          (void)hipGetLastError();
        }
        if (cur != ctx->device) (void)hipSetDevice(cur);
      }
    }
  }
  t_mark = m;
}

ReleaseScope::~ReleaseScope() { t_mark = prev; }

void ctx_register(m3d_ctx* ctx, bool live) {
  std::lock_guard<std::mutex> lk(g_bc_mu);
  if (live) {
    ctx->id = cache_state().next_id++;
    cache_state().ctx_ids[ctx] = ctx->id;
  } else {
    cache_state().ctx_ids.erase(ctx);
  }
}

void ctx_count(int dev, int delta) {
  std::lock_guard<std::mutex> lk(g_bc_mu);
  const int n = (g_ctx_live[dev] += delta);
  if (n <= 0) {
    g_ctx_live.erase(dev);
    bc_trim_locked(dev, 0, 0);  // the last context of the device: give the cache back
  }
}
}  // namespace m3d

namespace {
constexpr size_t kPinBytes = 4096;  // the pinned page (its layout: api_internal.h pin_read)
}  // namespace

namespace m3d {
namespace api {
int hip_fail(m3d_ctx* ctx, const char* what, hipError_t e, const std::string& why) {
  return m3d_fail(ctx, M3D_ERR_HIP, std::string(what) + ": " + (why.empty() ? hipGetErrorString(e) : why.c_str()));
}

int Arena::commit() {
  if (off <= ctx->scratch_bytes) return M3D_OK;
  if (ctx->scratch) {
    hipDeviceSynchronize();
    hipFree(ctx->scratch);
    ctx->scratch = nullptr;
    ctx->scratch_bytes = 0;
  }
  size_t want = std::max(off, ctx->scratch_bytes * 3 / 2);
  hipError_t e = dev_malloc(&ctx->scratch, want);
  if (e != hipSuccess) {
    ctx->scratch = nullptr;
    return m3d_fail(ctx, M3D_ERR_OOM, "scratch hipMalloc failed");
  }
  ctx->scratch_bytes = want;
  return M3D_OK;
}

int pin_ensure(m3d_ctx* ctx) {
  if (ctx->pin != nullptr) return M3D_OK;
  void* h = nullptr;
  if (hipHostMalloc(&h, kPinBytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
    return m3d_fail(ctx, M3D_ERR_OOM, "pinned staging hipHostMalloc failed");
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
    hipHostFree(h);
    return m3d_fail(ctx, M3D_ERR_HIP, "hipHostGetDevicePointer failed");
  }
  uint32_t* tk = nullptr;
  if (dev_malloc(&tk, sizeof(uint32_t)) != hipSuccess || hipMemset(tk, 0, sizeof(uint32_t)) != hipSuccess) {
    if (tk) hipFree(tk);
    hipHostFree(h);
    return m3d_fail(ctx, M3D_ERR_OOM, "ticket hipMalloc failed");
  }
  ctx->pin = h;
  ctx->pin_dev = d;
  ctx->one_ticket = tk;
  return M3D_OK;
}

int prep_buffer(m3d_ctx* ctx, size_t need, char** out) {
  if (need > ctx->prep_bytes) {
    if (ctx->prep) hipFree(ctx->prep);
    ctx->prep = nullptr;
    ctx->prep_bytes = 0;
    if (dev_malloc(&ctx->prep, need) != hipSuccess) {
      ctx->prep = nullptr;
      return m3d_fail(ctx, M3D_ERR_OOM, "hipMalloc: preprocessing scratch");
    }
    ctx->prep_bytes = need;
  }
  *out = static_cast<char*>(ctx->prep);
  return M3D_OK;
}
}  // namespace api
}  // namespace m3d

extern "C" {

int m3d_abi_version(void) { return M3D_ABI_VERSION; }

int m3d_device_count(int* count) {
  if (!count) return M3D_ERR_INVALID;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *count = n;
  return M3D_OK;
}

int m3d_create(int device, m3d_ctx** out) {
  if (!out) return M3D_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return M3D_ERR_NODEVICE;
  if (device < 0 || device >= n) return M3D_ERR_INVALID;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return M3D_ERR_HIP;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return M3D_ERR_NODEVICE;
  if (hipSetDevice(device) != hipSuccess) return M3D_ERR_HIP;
  m3d_ctx* ctx = new m3d_ctx();
  ctx->device = device;
  if (dev_malloc(&ctx->stats, 8 * sizeof(int64_t)) != hipSuccess ||
      dev_malloc(&ctx->rstate, sizeof(RansacState)) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->scratch_ev, hipEventDisableTiming) != hipSuccess ||
      hipMemset(ctx->stats, 0, 8 * sizeof(int64_t)) != hipSuccess) {
    m3d_destroy(ctx);
    return M3D_ERR_OOM;
  }
  ctx_register(ctx, true);
  ctx_count(device, +1);
  ctx->counted = true;
  *out = ctx;
  return M3D_OK;
}

void m3d_destroy(m3d_ctx* ctx) {
  if (!ctx) return;
  hipSetDevice(ctx->device);
  hipDeviceSynchronize();
  for (auto& u : ctx->uses) hipEventDestroy(u.second);
  if (ctx->order) hipStreamDestroy(ctx->order);
  if (ctx->scratch) hipFree(ctx->scratch);
  if (ctx->stats) hipFree(ctx->stats);
  if (ctx->rstate) hipFree(ctx->rstate);
  if (ctx->scratch_ev) hipEventDestroy(ctx->scratch_ev);
  if (ctx->pin) hipHostFree(ctx->pin);
  if (ctx->one_ticket) hipFree(ctx->one_ticket);
  if (ctx->prep) hipFree(ctx->prep);
  ctx->tmp.release();
  ctx->run.release();
  for (auto& v : ctx->ev)
    for (auto& pr : v) {
      hipEventDestroy(pr.first);
      hipEventDestroy(pr.second);
    }
  const int dev = ctx->device;
  const bool counted = ctx->counted;
  if (counted) ctx_register(ctx, false);
  delete ctx;
  if (counted) ctx_count(dev, -1);  // the device's last context gives the block cache back
}

int m3d_trim_block_cache(m3d_ctx* ctx, int64_t* freed_bytes) {
  if (!ctx) return M3D_ERR_INVALID;
  const size_t f = block_cache_trim(ctx->device);
  if (freed_bytes) *freed_bytes = (int64_t)f;
  return M3D_OK;
}

const char* m3d_last_error(const m3d_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int m3d_get_stats(m3d_ctx* ctx, int64_t* out8) {
  CHECK_ARG(ctx, out8 != nullptr, "null output");
  HIPX(ctx, hipMemcpy(out8, ctx->stats, 8 * sizeof(int64_t), hipMemcpyDeviceToHost));
  return M3D_OK;
}

int m3d_profile_enable(m3d_ctx* ctx, int enable) {
  if (!ctx) return M3D_ERR_INVALID;
  ctx->profiling = enable != 0;
  return M3D_OK;
}

int m3d_profile_read(m3d_ctx* ctx, int kernel, double* total_ms, int64_t* launches) {
  if (!ctx) return M3D_ERR_INVALID;
  CHECK_ARG(ctx, kernel >= 0 && kernel < 6 && total_ms && launches, "invalid arguments");
  double tot = 0.0;
  const size_t n = ctx->ev_used[kernel];
  for (size_t k = 0; k < n; ++k) {
    auto& pr = ctx->ev[kernel][k];
    HIPX(ctx, hipEventSynchronize(pr.second));
    float ms = 0.0f;
    HIPX(ctx, hipEventElapsedTime(&ms, pr.first, pr.second));
    tot += ms;
  }
  ctx->ev_used[kernel] = 0;
  *total_ms = tot;
  *launches = (int64_t)n;
  return M3D_OK;
}

int m3d_debug_block_cache_fill(int byte) {
  // synchronous: every idle block's release point has passed before, and the fill is complete
  // after, so the next owner sees exactly these bytes
  int cur = 0;
  (void)hipGetDevice(&cur);
  if (hipDeviceSynchronize() != hipSuccess) return M3D_ERR_HIP;
  std::lock_guard<std::mutex> lk(g_bc_mu);
  int n = 0;
  for (const CachedBlock& b : g_bc) {
    if (b.dev != cur) continue;
    if (hipMemset(b.p, byte & 0xFF, b.bytes) != hipSuccess) return M3D_ERR_HIP;
    ++n;
  }
  if (hipDeviceSynchronize() != hipSuccess) return M3D_ERR_HIP;
  return n;
}

}  // extern "C"
