// hostpack_check — stand-alone CPU program behind tests/test_hostpack_cpu.py: runs the pure host code every GEMM kernel's
// weight layout and every state_dict load depend on (csrc/host/convert.h, csrc/host/weight_store.h) and writes what it
// computed into the directory given as argv[1]; the test compares the files with numpy / torch.  No HIP, no GPU.
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <string>

#include "../../diffusion-handwriting-generation.pytorch_amd/csrc/host/convert.h"
#include "../../diffusion-handwriting-generation.pytorch_amd/csrc/host/weight_store.h"

static std::string g_dir;

template <typename T>
static std::vector<T> read_bin(const char* name) {
  std::vector<T> v;
  FILE* f = fopen((g_dir + "/" + name).c_str(), "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", name); exit(2); }
  fseek(f, 0, SEEK_END);
  v.resize((size_t)ftell(f) / sizeof(T));
  fseek(f, 0, SEEK_SET);
  if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
  fclose(f);
  return v;
}
template <typename T>
static void write_bin(const char* name, const std::vector<T>& v) {
  FILE* f = fopen((g_dir + "/" + name).c_str(), "wb");
  if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "cannot write %s\n", name); exit(2); }
  fclose(f);
}
static std::vector<float> arange(size_t n) {
  std::vector<float> v(n);
  std::iota(v.begin(), v.end(), 0.f);
  return v;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  g_dir = argv[1];

  // ---- the MFMA-fragment packing of arange inputs
  write_bin("pack_16_32.f32", pack_mfma(arange(16 * 32), 16, 32));
  write_bin("pack_48_96.f32", pack_mfma(arange(48 * 96), 48, 96));
  const std::vector<float> flat = conv_flat(arange(32 * 32 * 3), 32, 32);   // Conv1d weight [32][32][3]
  write_bin("conv_flat.f32", flat);
  write_bin("pack_conv_32_96.f32", pack_mfma(flat, 32, 3 * 32));

  // ---- number formats
  {
    const std::vector<float> in = read_bin<float>("f2bf_in.f32");
    std::vector<uint16_t> out(in.size());
    for (size_t i = 0; i < in.size(); ++i) out[i] = f2bf(in[i]);
    write_bin("f2bf_out.u16", out);
    std::vector<float> b(65536), h(65536);
    for (uint32_t i = 0; i < 65536; ++i) { b[i] = bf2f((uint16_t)i); h[i] = h2f((uint16_t)i); }
    write_bin("bf2f_all.f32", b);
    write_bin("h2f_all.f32", h);
  }
  {
    const std::vector<float> f32 = read_bin<float>("to_f32_in.f32");
    const std::vector<double> f64 = read_bin<double>("to_f32_in.f64");
    const std::vector<uint16_t> bf = read_bin<uint16_t>("to_f32_in.bf16"), hf = read_bin<uint16_t>("to_f32_in.f16");
    std::vector<float> out(8, -1.f);
    bool ok = to_f32(out.data(), f32.data(), DHW_F32, 8);
    write_bin("to_f32_out_f32.f32", out);
    ok = to_f32(out.data(), f64.data(), DHW_F64, 8) && ok;
    write_bin("to_f32_out_f64.f32", out);
    ok = to_f32(out.data(), bf.data(), DHW_BF16, 8) && ok;
    write_bin("to_f32_out_bf16.f32", out);
    ok = to_f32(out.data(), hf.data(), DHW_F16, 8) && ok;
    write_bin("to_f32_out_f16.f32", out);
    printf("to_f32_known_dtypes %d\n", (int)ok);
    printf("to_f32_unknown_dtype %d\n", (int)to_f32(out.data(), f32.data(), 99, 8));
  }

  // ---- the weight store
  {
    WeightStore s;
    s.init({{"a.weight", {2, 3}}, {"b.bias", {4}}});
    const int64_t sa[2] = {2, 3}, sb[1] = {4}, wrong[2] = {3, 2};
    const float a1[6] = {1, 2, 3, 4, 5, 6}, b1[4] = {7, 8, 9, 10};
    const uint16_t a2[6] = {0x3f80, 0x4000, 0x4040, 0x4080, 0x40a0, 0xc0c0};   // bf16: 1 2 3 4 5 -6
    printf("missing_at_start %d\n", s.first_missing());
    printf("load_a_f32 %d\n", (int)s.load("a.weight", a1, DHW_F32, sa, 2));
    printf("missing_after_a %d\n", s.first_missing());
    printf("load_a_again_bf16 %d\n", (int)s.load("a.weight", a2, DHW_BF16, sa, 2));
    write_bin("store_a.f32", s.host_w[0]);
    printf("load_unknown_key %d\n", (int)s.load("c.weight", a1, DHW_F32, sa, 2));
    printf("load_wrong_shape %d\n", (int)s.load("b.bias", b1, DHW_F32, wrong, 2));
    printf("load_wrong_dim %d\n", (int)s.load("a.weight", a1, DHW_F32, wrong, 2));
    printf("load_bad_dtype %d\n", (int)s.load("b.bias", b1, 99, sb, 1));
    printf("load_f16_refused %d\n", (int)s.load("b.bias", a2, DHW_F16, sb, 1, false));
    printf("missing_after_failures %d\n", s.first_missing());
    printf("load_b_f32 %d\n", (int)s.load("b.bias", b1, DHW_F32, sb, 1));
    printf("missing_at_end %d\n", s.first_missing());
    bool first = true;
    const std::vector<float>& known = s.get("b.bias", &first);
    printf("get_known_first %d size %d fail %d\n", (int)first, (int)known.size(), (int)s.lookup_fail);
    const std::vector<float>& z1 = s.get("nope.weight", &first);
    double sum = 0;
    for (float v : z1) sum += std::fabs(v);
    printf("get_unknown_first %d size_ge_1280 %d abs_sum %g fail %d\n", (int)first, (int)(z1.size() >= 1280), sum, (int)s.lookup_fail);
    s.get("nope.bias", &first);
    printf("get_unknown_again_first %d fail %d\n", (int)first, (int)s.lookup_fail);
  }
  return 0;
}
