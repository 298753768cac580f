// fks_cache.cpp -- what libfks.so keeps on the device between calls, guarded by g_cache_mu:
// the plan cache (the MT stream's static headers and the torch_rocm tensor tables, one LRU
// each) and the per-device stream-ordered buffers (window, z-index, reconstruct window cache).
#include <hip/hip_runtime.h>

#include <cctype>
#include <cstdlib>

#include "fks_host.h"

namespace fks {

std::mutex g_cache_mu;

namespace {

constexpr size_t kPlanCacheEntries = 32;
std::vector<CachedPlan*> g_cache;
std::vector<PhxPlan*> g_phx;
uint64_t g_cache_clock = 0;
std::vector<WinCache> g_win;
std::vector<ZCache> g_zc;
std::vector<JWin> g_jw;

int current_device() {
  int dev = 0;
  (void)hipGetDevice(&dev);
  return dev;
}

// Every input a header depends on: device, CU count, each tensor's address/numel/dtype/flags/
// lr/wd, the scales as f32, the delta base, the shard, the chunk policy.  The ZO optimizer's
// calls and repeated reconstructs of one model hit: no host-side layout work, no upload.
std::vector<uint8_t> plan_key(const fks_tensor* t, int nt, const double* scales, uint64_t delta_base, int shard,
                              int nshards, bool small, const DevCaps& dc) {
  std::vector<uint8_t> k;
  k.reserve(64 + (size_t)nt * 40);
  key_put(k, dc.device);
  key_put(k, dc.cus);
  key_put(k, nt);
  key_put(k, delta_base);
  key_put(k, shard);
  key_put(k, nshards);
  key_put(k, (int)small);
  key_put(k, (int)(scales != nullptr));
  for (int i = 0; i < nt; i++) {
    key_put(k, t[i].data);
    key_put(k, t[i].numel);
    key_put(k, t[i].dtype);
    key_put(k, t[i].flags);
    key_put(k, t[i].lr);
    key_put(k, t[i].wd);
    if (scales) key_put(k, (float)scales[i]);
  }
  return k;
}

// Free a cached table after synchronising the device that owns it (which need not be
// the current one: the key holds the device id, so one process may cache plans of
// several GPUs); the current device is restored.
template <class T>
void free_resident(T* C) {
  const int cur = current_device();
  if (C->device != cur) (void)hipSetDevice(C->device);
  (void)hipDeviceSynchronize();
  (void)hipFree(C->dev);
  if (C->device != cur) (void)hipSetDevice(cur);
  delete C;
}

// The entry of `lru` for `key`, built by make() and uploaded on a miss (synchronously: every
// later launch on any stream finds it in place).  The caller holds g_cache_mu while it uses the
// entry.  The least recently used entry makes room, after a device synchronisation.
template <class T, class Make>
const T* lru_get(std::vector<T*>& lru, std::vector<uint8_t> key, const char* what, const char* what_upload,
                 Make&& make) {
  const uint64_t h = fnv1a(key);
  for (T* C : lru)
    if (C->hash == h && C->key == key) {
      C->last_use = ++g_cache_clock;
      return C;
    }
  auto* C = new T();
  const void* bytes = nullptr;
  size_t nbytes = 0;
  try {
    make(*C, bytes, nbytes);
  } catch (...) {
    delete C;
    throw;
  }
  C->key = std::move(key);
  C->hash = h;
  C->last_use = ++g_cache_clock;
  C->device = current_device();
  const size_t alloc = std::max<size_t>(nbytes, 256);
  if (const hipError_t e = hipMalloc(&C->dev, alloc); e != hipSuccess) {
    delete C;
    throw Error(-FKS_ENOMEM, std::string(what) + " hipMalloc: " + hipGetErrorString(e) + " (" + std::to_string(alloc) +
                                 " bytes)");
  }
  if (const hipError_t e = nbytes ? hipMemcpy(C->dev, bytes, nbytes, hipMemcpyHostToDevice) : hipSuccess;
      e != hipSuccess) {
    (void)hipFree(C->dev);
    delete C;
    throw Error(-FKS_EHIP, std::string(what_upload) + " upload: " + hipGetErrorString(e));
  }
  if (lru.size() >= kPlanCacheEntries) {
    auto victim =
        std::min_element(lru.begin(), lru.end(), [](const T* a, const T* b) { return a->last_use < b->last_use; });
    free_resident(*victim);
    lru.erase(victim);
  }
  lru.push_back(C);
  return C;
}

// The entry of the current device in `v` (created on first use with its event), or
// nullptr if the event cannot be created.
template <class T>
T* dev_entry(std::vector<T>& v) {
  const int dev = current_device();
  for (T& x : v)
    if (x.b.device == dev) return x.b.done ? &x : nullptr;
  v.emplace_back();
  T* X = &v.back();
  X->b.device = dev;
  hipEvent_t ev = nullptr;
  if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  X->b.done = ev;
  return X;
}

// order `stream` after the buffer's last user when that was another stream
bool buf_acquire(DevBuf& b, void* stream) {
  const bool other = b.stream && b.stream != stream;
  if (other && hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)b.done, 0) != hipSuccess) return false;
  b.stream = stream;
  return true;
}

}  // namespace

DevCaps device_caps(bool require) {
  DevCaps dc;
  if (hipGetDevice(&dc.device) != hipSuccess && require) throw Error(-FKS_EHIP, "no current HIP device");
  dc.cus = device_cu_count();
  dc.threads_per_cu = device_max_threads_per_cu();
  dc.max_grid = (int64_t)dc.cus * (dc.threads_per_cu / 256);
  return dc;
}

const CachedPlan* get_plan(const fks_tensor* t, int nt, const double* scales, uint64_t delta_base, int shard,
                           int nshards, bool small, const DevCaps& dc) {
  PlanImage img;
  return lru_get(g_cache, plan_key(t, nt, scales, delta_base, shard, nshards, small, dc), "plan cache", "plan",
                 [&](CachedPlan& C, const void*& bytes, size_t& nbytes) {
                   img = plan_image(t, nt, scales, delta_base, shard, nshards, small, dc.cus);
                   static_cast<PlanInfo&>(C) = img.info;
                   bytes = img.bytes.data();
                   nbytes = img.bytes.size();
                 });
}

// same key as the MT plans, with a tag and what torch's grid depends on besides the CU count
const PhxPlan* get_phx_plan(const fks_tensor* t, int nt, const double* scales, uint64_t delta_base, const DevCaps& dc) {
  std::vector<uint8_t> key = plan_key(t, nt, scales, delta_base, 0, 1, false, dc);
  key_put(key, (int)0x7068);  // "ph": not an MT plan key
  key_put(key, dc.threads_per_cu);
  const char* what = "torch_rocm plan";
  return lru_get(g_phx, std::move(key), what, what, [&](PhxPlan& P, const void*& bytes, size_t& nbytes) {
    static_cast<PhxGeo&>(P) = phx_geometry(t, nt, scales, delta_base, dc.max_grid);
    bytes = P.tab.data();
    nbytes = sizeof(PhxTensor) * P.tab.size();
  });
}

void clear_plan_cache() {
  std::lock_guard<std::mutex> lk(g_cache_mu);
  for (CachedPlan* C : g_cache) free_resident(C);
  g_cache.clear();
  for (PhxPlan* P : g_phx) free_resident(P);
  g_phx.clear();
  const int cur = current_device();
  auto sync = [](DevBuf& b) {
    (void)hipSetDevice(b.device);
    (void)hipDeviceSynchronize();
    b.stream = nullptr;
  };
  for (WinCache& W : g_win) {
    sync(W.b);
    if (W.b.buf) (void)hipFree(W.b.buf);
    if (W.b.done) (void)hipEventDestroy((hipEvent_t)W.b.done);
  }
  for (ZCache& Z : g_zc) {  // the caller's buffers stay attached; their contents are dropped
    sync(Z.b);
    Z.valid = false;
  }
  for (JWin& J : g_jw) {  // likewise
    sync(J.b);
    jw_drop(J);
  }
  (void)hipSetDevice(cur);
  g_win.clear();
}

// A boolean switch of the environment: on for 1 / true / yes / on (any case), off when
// unset, empty or anything else -- so FKS_NO_JWIN=0 leaves the cache ON (codec._env_on
// reads the same values).
bool env_on(const char* name) {
  const char* e = std::getenv(name);
  if (!e) return false;
  std::string v(e);
  for (char& ch : v) ch = (char)std::tolower((unsigned char)ch);
  return v == "1" || v == "true" || v == "yes" || v == "on";
}

int buf_record(DevBuf& b, void* stream) { return (int)hipEventRecord((hipEvent_t)b.done, (hipStream_t)stream); }

void buf_attach(DevBuf& b, void* buf, size_t bytes, const char* what) {
  // the last call that used the old buffer may still be running: the caller may free
  // or reuse it once this returns
  if (b.buf && b.stream && hipEventSynchronize((hipEvent_t)b.done) != hipSuccess)
    throw Error(-FKS_EHIP, std::string(what) + ": waiting for the last user");
  b.buf = bytes ? buf : nullptr;
  b.bytes = buf ? bytes : 0;
  b.stream = nullptr;
}

ZCache* z_entry() { return dev_entry(g_zc); }
JWin* jw_entry() { return dev_entry(g_jw); }

// ... if the attached buffer holds `bytes`; nullptr otherwise (the call then generates)
ZCache* z_cache(void* stream, size_t bytes) {
  const char* env = std::getenv("FKS_ZCACHE");
  if (env && env[0] == '0') return nullptr;
  ZCache* Z = z_entry();
  if (!Z || !Z->b.buf || Z->b.bytes < bytes || !buf_acquire(Z->b, stream)) return nullptr;
  return Z;
}

// ... for a call of the plan with bs_hash `key` and `nch` chunk pairs; nullptr when none is
// attached or it is too small for one two-slice pass.  A new key drops every set.
JWin* jw_cache(void* stream, uint64_t key, int nch) {
  if (env_on("FKS_NO_JWIN")) return nullptr;
  JWin* J = jw_entry();
  if (!J || !J->b.buf) return nullptr;
  const size_t set_bytes = sizeof(uint32_t) * (size_t)kMtN * (size_t)nch;
  const uint32_t nsets = (uint32_t)std::min<size_t>(J->b.bytes / set_bytes, UINT32_MAX);
  if (nsets < (uint32_t)kBsPassSeeds) return nullptr;
  if (!buf_acquire(J->b, stream)) return nullptr;
  if (J->key != key || J->nch != nch || J->sets.nsets != nsets) {
    J->key = key;
    J->nch = nch;
    jw_reset(J->sets, nsets);
  }
  return J;
}

// ... for a one-seed call needing `bytes`; nullptr with FKS_NO_WIN_CACHE set or without
// memory (the call then jumps into its workspace)
WinCache* win_cache(void* stream, size_t bytes) {
  if (env_on("FKS_NO_WIN_CACHE")) return nullptr;
  WinCache* W = dev_entry(g_win);
  if (!W) return nullptr;
  if (W->b.bytes < bytes) {
    if (W->b.buf) {
      // the last user may still read the old buffer
      if (hipEventSynchronize((hipEvent_t)W->b.done) != hipSuccess) return nullptr;
      (void)hipFree(W->b.buf);
      W->b.buf = nullptr;
      W->b.bytes = 0;
    }
    W->valid = false;
    if (hipMalloc(&W->b.buf, bytes) != hipSuccess) {
      W->b.buf = nullptr;
      (void)hipGetLastError();
      return nullptr;
    }
    W->b.bytes = bytes;
    W->b.stream = stream;
  } else if (!buf_acquire(W->b, stream)) {  // another stream used the buffer last: wait (on the device)
    return nullptr;
  }
  return W;
}

size_t zindex_bytes(const fks_tensor* t, int nt) {
  if (rocm_stream(t, nt)) return 0;  // the z-index cache serves the CPU stream only
  std::lock_guard<std::mutex> lk(g_cache_mu);
  const CachedPlan* C = get_plan(t, nt, nullptr, 0, 0, 1, true, device_caps());
  return (C->have_reg && C->nsegs[FKS_BF16] > 0) ? (size_t)kSm2ZidxBytesPerBlock * (size_t)(C->reg_hi - C->reg_lo) : 0;
}

size_t jwin_bytes(const fks_tensor* t, int nt, int k, int shard, int nshards) {
  if (rocm_stream(t, nt) || k <= kBsSeeds) return 0;  // the Philox stream jumps nothing
  std::lock_guard<std::mutex> lk(g_cache_mu);
  // the plan the sharded call itself launches with (run() keys jw_cache on its chunks)
  const CachedPlan* C = get_plan(t, nt, nullptr, 0, shard, nshards, false, device_caps());
  if (!C->have_bs) return 0;
  const size_t set_bytes = sizeof(uint32_t) * (size_t)kMtN * (size_t)(C->Z.bs_chunks / kBsChunksPerWg);
  return set_bytes * (size_t)std::max(k, kBsPassSeeds);
}

}  // namespace fks
