// sampler/plane_tag.h — what the all-steps text plane resident in a handle's ".T" buffers was computed for, and the host half of
// the decision to reuse it.  Pure host logic, no HIP: dhw_debug_plane_tag runs it without a device.
#pragma once
#include <algorithm>
#include <cstdint>

// sampler steps whose text side is precomputed together (bounds the plane's memory for long schedules)
inline int plane_chunk(int T) { return std::min(T, 64); }

// The plane is a function of (text, style, the sigma schedule of T, the weights) and of where its (step, prompt) slots lie.
// The tag holds everything of that the host knows; text and style are compared on the device (stage_compare_kernel, misc.hip).
// NOT in the tag, because the plane does not depend on them: L (ensure_plane sizes the plane by steps x prompts, max_Lt and the
// widths alone, and no text-side kernel reads a stroke length), seed, first_sample, mode, noise, lens, keep masks, DHW_PERSIST.
struct PlaneTag {
  bool valid = false;
  int B = 0, nstreams = 0;   // the batch and its split into sub-batches (one plane per workspace)
  int Lt = 0, S = 0, T = 0;
  int t_start = 0;           // slot k of the plane holds schedule index t_start - 1 - k
  uint64_t weights_gen = 0;  // dhw_finalize after a change
  const void* film = nullptr;   // the FilmT table the launches read
  uint64_t plane_gen = 0;    // ensure_plane re-allocating
};
inline bool plane_tag_equal(const PlaneTag& a, const PlaneTag& b) {
  return a.valid && b.valid && a.B == b.B && a.nstreams == b.nstreams && a.Lt == b.Lt && a.S == b.S && a.T == b.T && a.t_start == b.t_start &&
         a.weights_gen == b.weights_gen && a.film == b.film && a.plane_gen == b.plane_gen;
}
// what else must hold on the handle for a call to reuse the resident plane
struct PlaneGate {
  bool reuse_on;     // DHW_PLANE_REUSE (default on)
  bool plane;        // the all-steps plane is in use (DHW_PLANE)
  bool text_fused;   // textside_supported(...) for this call's shapes, on a bf16 handle with the fused kernels
};
// 1 = the launches of this call may skip the text side IF the device compare finds prompts and styles unchanged.
// A schedule of more than one chunk never reuses: later chunks overwrite earlier ones in the same buffers.
inline unsigned plane_host_ok(const PlaneTag& resident, const PlaneTag& call, const PlaneGate& g) {
  return g.reuse_on && g.plane && g.text_fused && call.T <= plane_chunk(call.T) && plane_tag_equal(resident, call) ? 1u : 0u;
}
