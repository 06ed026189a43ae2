// attnmap.h — launcher of the attention-map kernel (include/dhw.h: dhw_attention); shared by attnmap.hip and
// dhw_attnmap_api.cpp (the denoiser call, the Q projection and this launch).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

constexpr int ATTNMAP_D = 64;      // head dimension of every cross attention (sampler/weights.cpp pads heads to it)
constexpr int ATTNMAP_ROWS = 16;   // query rows per workgroup
constexpr int ATTNMAP_MAX_LT = 168;   // H * 16 * Lt_pad floats of LDS must fit 64 KiB at H = 6 (6 * 16 * 168 * 4 = 64512 B)

// One cross attention's probabilities: P[b,h,q,:] = softmax_k(Q[b,q,h,:] . K[b,k,h,:] / 8 + (text[b,k] == 0) * -1e9).
struct AttnMapParams {
  const void* Q; int ldq;    // Q[(b*Lq + q)*ldq + h*64 + j], the handle's element type, rows 16-byte aligned
  const void* K; int ldk;    // K[(b*Lt + k)*ldk + h*64 + j]
  const int64_t* text;       // [B, Lt], 0 = pad
  const int* lens; int lsh;  // per-sample lengths at full resolution (device) or null: sample b has lens[b] >> lsh query rows
  int B, H, Lq, Lt;          // H = 3, 4 or 6
  float* probs;              // [B, H, Lq, Lt] or null
  float* mean;               // [B, Lq, Lt] or null (16-byte aligned)
  int32_t* token;            // [B, Lq] or null
};

hipError_t launch_attnmap(int prec, const AttnMapParams& p, hipStream_t st);
