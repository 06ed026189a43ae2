// host/weight_store.h — the strict, by-name state_dict intake both model handles (dhw_handle, dhw_style) hold: the key spec,
// the fp32 host copies and which keys have arrived.  Pure C++ (tests/cpp/hostpack_check.cpp).
#pragma once
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "convert.h"

#pragma GCC visibility push(hidden)

struct KeySpec { std::string key; std::vector<int64_t> shape; };

struct WeightStore {
  std::vector<KeySpec> spec;
  std::map<std::string, int> key_index;
  std::vector<std::vector<float>> host_w;
  std::vector<char> loaded;
  bool lookup_fail = false;   // the packing code asked for a name that does not exist (find / get; the sampler's FiLM lookup): finalize fails

  void init(std::vector<KeySpec> s) {
    spec = std::move(s);
    key_index.clear();
    for (size_t i = 0; i < spec.size(); ++i) key_index[spec[i].key] = (int)i;
    host_w.assign(spec.size(), {});
    loaded.assign(spec.size(), 0);
  }

  // What load() found, in the order it checks; the caller words the message (the two state_dicts name themselves differently).
  enum LoadResult { LOADED = 0, UNKNOWN_KEY, SIZE_MISMATCH, BAD_DTYPE };
  // f16_ok: dhw_load takes IEEE half tensors, dhw_style_load does not.  The refusal sits here, in front of to_f32, and not in
  // dhw_style_load in front of this call, on purpose: both loads check key, then shape, then dtype, and a half tensor under an
  // unknown key must keep answering "unexpected key", as it always has.
  LoadResult load(const char* key, const void* host_ptr, int dtype, const int64_t* shape, int ndim, bool f16_ok = true) {
    auto it = key_index.find(key);
    if (it == key_index.end()) return UNKNOWN_KEY;
    const KeySpec& k = spec[it->second];
    bool ok = ndim == (int)k.shape.size();
    for (int i = 0; ok && i < ndim; ++i) ok = shape[i] == k.shape[i];
    if (!ok) return SIZE_MISMATCH;
    size_t n = 1;
    for (int64_t s : k.shape) n *= (size_t)s;
    std::vector<float>& dst = host_w[it->second];
    dst.resize(n);
    if ((dtype == DHW_F16 && !f16_ok) || !to_f32(dst.data(), host_ptr, dtype, n)) return BAD_DTYPE;
    loaded[it->second] = 1;
    return LOADED;
  }

  // index of the first key of the spec that has not been loaded, or -1
  int first_missing() const {
    for (size_t i = 0; i < spec.size(); ++i)
      if (!loaded[i]) return (int)i;
    return -1;
  }

  // A weight by key (finalize-time only).  The packing code names the same keys the spec declares, so a miss is a programming
  // error: lookup_fail is raised — *first_miss tells the caller to record its message, once — and zeros() comes back: 4096
  // zeros, which covers the per-channel reads (<= 1280 channels) of the StyleExtractor's packing loops and nothing longer, so
  // any other reader checks lookup_fail or the size before it indexes; nothing throws.
  // find: the index (the sampler keeps a second, padded copy of every tensor under the same index); get: the tensor itself.
  int find(const std::string& key, bool* first_miss) {
    auto it = key_index.find(key);
    const bool miss = it == key_index.end();
    if (first_miss) *first_miss = miss && !lookup_fail;
    if (!miss) return it->second;
    lookup_fail = true;
    return -1;
  }
  static const std::vector<float>& zeros() {
    static const std::vector<float> none(4096, 0.f);
    return none;
  }
  const std::vector<float>& get(const std::string& key, bool* first_miss = nullptr) {
    const int i = find(key, first_miss);
    return i < 0 ? zeros() : host_w[i];
  }
};

#pragma GCC visibility pop
