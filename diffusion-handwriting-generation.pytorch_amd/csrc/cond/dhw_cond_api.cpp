// dhw_cond_api.cpp — C-ABI of conditioned sampling (include/dhw.h: dhw_sample_cond): the sampler's loop (sampler/sample.cpp)
// with a conditioning block.  The argument checks run inside sample_impl, all of them before its first HIP call; the kernels
// are cond.hip's.
#include "../sampler/handle.h"

extern "C" {

int dhw_sample_cond(dhw_handle* h, const int64_t* text, const float* style, int B, int L, int Lt, const int32_t* lens, int T, int mode,
                    const float* noise, uint64_t seed, int64_t first_sample, const float* known, const uint8_t* keep, int t_start,
                    const float* cond_noise, float* out, void* hip_stream) {
  DHW_GUARD(h, "dhw_sample_cond", int, {
    const CondArgs cond{known, keep, t_start, cond_noise};
    return sample_impl(h, "dhw_sample_cond", text, style, B, L, Lt, T, mode, noise, seed, first_sample, out, hip_stream, lens, lens != nullptr, &cond);
  });
}

}  // extern "C"
