// train_common.h — the small device helpers that several units of the training kernels share (csrc/train.hip and csrc/train/).
#pragma once
#include "../dhw_common.h"

namespace dhw_train {

DHW_DEV float sigmoid_f(float x) { return 1.0f / (1.0f + __expf(-x)); }
DHW_DEV float dsilu_f(float x) { const float s = sigmoid_f(x); return s * (1.0f + x * (1.0f - s)); }
DHW_DEV float sum4(const f32x4& v) { return (v[0] + v[1]) + (v[2] + v[3]); }
DHW_DEV f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

inline unsigned nb(long n, int per = 256) { return (unsigned)((n + per - 1) / per); }

}  // namespace dhw_train

// train/batch.hip: the batch of one update drawn and gathered from a dataset resident on the device (include/dhw_train.h)
hipError_t launch_batch_draw(const uint64_t* rng, int N, int B, const float* abar, int T, const int* grp_start, const int* grp_size, const int* grp_pos,
                             const int* members, int* idx, int* style_src, float* alphas, float* sigma, hipStream_t st);
hipError_t launch_batch_gather(const float* strokes, const int64_t* text, const float* style, const int* idx, const int* style_src, int N, int B, int L, int Lt,
                               int S, float* x, float* pen, int64_t* ids, float* mask, float* style_out, hipStream_t st);
// train/cond_drop.hip: conditioning dropout on a step's input buffers (include/dhw_train.h)
hipError_t launch_cond_drop(const uint64_t* rng, int B, int Lt, int S, float p, int64_t* ids, float* mask, float* style, int* dropped, hipStream_t st);
