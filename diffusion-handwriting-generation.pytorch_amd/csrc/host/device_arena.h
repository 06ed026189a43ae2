// host/device_arena.h — device allocations that live as long as their owner (a model handle, or one training call's scratch)
// and are freed in one place, plus the two weight uploads.  The only header of csrc/host/ that needs the HIP runtime.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "convert.h"

#pragma GCC visibility push(hidden)

struct DeviceArena {
  std::vector<void*> allocs;
  const char* failed = "";   // the HIP call behind the last error returned: the owner's message names it

  hipError_t alloc(void** p, size_t bytes, bool zero = true) {
    failed = "hipMalloc";
    hipError_t e = hipMalloc(p, bytes ? bytes : 16);
    if (e != hipSuccess) return e;
    allocs.push_back(*p);
    failed = "hipMemset";
    return zero ? hipMemset(*p, 0, bytes ? bytes : 16) : hipSuccess;
  }
  hipError_t copy_in(void* dst, const void* src, size_t bytes) {
    failed = "hipMemcpy";
    return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
  }
  hipError_t upload_f32(const std::vector<float>& v, float** out) {
    hipError_t e = alloc((void**)out, v.size() * 4, false);
    return e != hipSuccess ? e : copy_in(*out, v.data(), v.size() * 4);
  }
  // row-major Wf[N][K] -> MFMA-fragment order (pack_mfma) as fp32, or rounded to bf16
  hipError_t upload_packed(const std::vector<float>& wf, int N, int K, bool bf16, void** out) {
    const std::vector<float> pk = pack_mfma(wf, N, K);
    const size_t n = pk.size();
    hipError_t e = alloc(out, n * (bf16 ? 2 : 4), false);
    if (e != hipSuccess) return e;
    if (!bf16) return copy_in(*out, pk.data(), n * 4);
    std::vector<uint16_t> b(n);
    for (size_t i = 0; i < n; ++i) b[i] = f2bf(pk[i]);
    return copy_in(*out, b.data(), n * 2);
  }
  void free_all() {
    for (void* p : allocs) hipFree(p);
    allocs.clear();
  }
};

#pragma GCC visibility pop
