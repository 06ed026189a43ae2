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
