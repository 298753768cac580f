// fks_dev_host.h -- once-per-device host setup of a device translation unit.  Every unit that
// includes this gets its own PerDevice flags and its own ensure_tables(), which fills that
// unit's own instances of c_tab_bf16 (fks_dev_zgen.h) and c_tab_f16 (fks_dev_irr.h): there is
// no -fgpu-rdc, so a __constant__ table exists once per unit that uses it.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>

#include "fks_internal.h"
#include "fks_dev_zgen.h"
#include "fks_dev_irr.h"

namespace fks {
namespace {

// Once-per-DEVICE host setup: __constant__ memory and function attributes belong to
// the device a call runs on, and one process may drive several GPUs (the plan cache
// keys on the device id), so every such flag is a bitmask over device ids.
class PerDevice {
 public:
  template <class F>
  int run(F&& f) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -FKS_EINVAL;
    const uint64_t bit = 1ull << dev;
    if (done_.load(std::memory_order_acquire) & bit) return 0;
    std::lock_guard<std::mutex> lk(mu_);
    if (done_.load(std::memory_order_relaxed) & bit) return 0;
    const int e = f();
    if (e == 0) done_.fetch_or(bit, std::memory_order_release);
    return e;
  }

 private:
  std::mutex mu_;
  std::atomic<uint64_t> done_{0};
};

// this translation unit's Box-Muller tables, from fks::tables()
int ensure_tables() {
  static PerDevice once;
  return once.run([] {
    const Tables& t = tables();
    static float buf[sizeof(c_tab_f16) / sizeof(float)];  // used under the PerDevice mutex only
    for (int i = 0; i < 256; i++) {
      buf[i] = t.r_bf16[i];
      buf[256 + i] = t.c_bf16[i];
      buf[512 + i] = t.s_bf16[i];
    }
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_tab_bf16), buf, sizeof(float) * 768, 0, hipMemcpyHostToDevice);
    if (e != hipSuccess) return (int)e;
    for (int i = 0; i < 2048; i++) {
      buf[i] = t.r_f16[i];
      buf[2048 + i] = t.c_f16[i];
      buf[4096 + i] = t.s_f16[i];
    }
    e = hipMemcpyToSymbol(HIP_SYMBOL(c_tab_f16), buf, sizeof(buf), 0, hipMemcpyHostToDevice);
    return (int)e;
  });
}

// hipFuncAttributeMaxDynamicSharedMemorySize for kernel `fn`, once per device
template <class K>
int ensure_lds_attr(PerDevice& once, K* fn, int bytes) {
  return once.run([&] {
    return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    bytes);
  });
}

}  // namespace
}  // namespace fks
