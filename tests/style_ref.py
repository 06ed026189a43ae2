"""The four kinds of launch of the StyleExtractor front end (csrc/dhw_style_api.cpp dhw_style_forward: stem, pointwise, depthwise, pools)
stated in float64 on the CPU from the definition of each operation (torch.nn.functional convolutions / pools, a matmul) — not from the
kernels' index arithmetic — with the per-element error bound of DESIGN.md §42, the table of the 53 launches derived from
oracle/mobilenet_ref.blocks(), the float64 BatchNorm fold, and the shapes and input generators for per-launch GPU tests.
tests/test_style_ref_cpu.py ties all of it to oracle/mobilenet_ref.forward without a GPU.  The per-launch GPU tests themselves are not
in the tree yet (DESIGN.md §42 says why); this file is what they will compare against.

Activations are NHWC [B, H, W, C] float64 tensors of the REAL channels (the library's layout without its channel padding).

Bound, per output element of a launch that stores fp32 (every launch of an fp32 handle; the pools of either):

    |got - ref| <= U_F32 |ref| + (K + 4) 2^-23 S,   S = |bias| + |res| + sum_k |a_k w_k|  (float64)

  K       the number of summed terms: cin (pointwise), 9 (stem, depthwise), 9 Hp cols (pools: 3x3 windows x pooled rows x the pooled
          columns of the bin)
  U_F32   2^-24, the unit roundoff of the fp32 store
  2^-23   per term and not 2^-24 (fp32 round to nearest): room for an MFMA adder tree that truncates; the + 4 covers the bias, the residual
          and the pools' two scalings
ReLU6 is 1-Lipschitz, so the bound holds for the clamped values as it does for the pre-activations.

No store term for bf16 outputs is stated here.  The plan for the per-launch tests names 2^-9; a correctly rounded bf16 store is off by
up to 2^-8 / (1 + 2^-8) of the value (8 significant bits: half an ulp is 2^-8 of the lower end of a binade), so that value cannot be
asserted of any correct launch, and this file does not restate the plan by itself.  ``bound`` takes the store's unit
roundoff as an argument; the bf16 INPUT side (activations and pointwise weights rounded to bf16, ties to even) is here and checked."""
import torch
import torch.nn.functional as F

from oracle import mobilenet_ref

STEM, POINTWISE, DEPTHWISE, POOL = 0, 1, 2, 3
KIND_NAME = {STEM: "stem", POINTWISE: "pointwise", DEPTHWISE: "depthwise", POOL: "pool"}
BINS, LAST = 14, 1280
U_F32, U_TERM = 2.0 ** -24, 2.0 ** -23
# features.0.1.weight (the stem's BatchNorm gamma) is multiplied by this for per-launch tests: with synthetic_state_dict(0) as it is the
# stem never reaches the upper clip point; 4 is the smallest power of two with >= 1 % of the stem's outputs at 6 for every shape of
# STEM_SHAPES (tests/test_style_ref_cpu.py test_generators_reach_both_clip_points asserts both halves of this sentence)
STEM_GAMMA_SCALE = 4.0


def padc(c):
    """channel padding of the library: up to 64, 96 as it is, else the next multiple of 64"""
    return 64 if c <= 64 else (96 if c == 96 else (c + 63) // 64 * 64)


def launch_table():
    """The 53 launches in forward order, from mobilenet_ref.blocks(): dicts of kind, stride, cin, cin_p, cout, cout_p, relu6, res,
    key (prefix of the convolution's weight), bn (prefix of its BatchNorm), name."""
    t = []

    def add(kind, cin, cout, stride, relu6, res, key, bn, name, pad_in=True):
        t.append(dict(kind=kind, stride=stride, cin=cin, cin_p=padc(cin) if pad_in else cin, cout=cout, cout_p=padc(cout), relu6=relu6, res=res,
                      key=key, bn=bn, name=name))

    add(STEM, 1, 32, 2, True, False, "features.0.0", "features.0.1", "features.0 stem", pad_in=False)
    for idx, tt, cin, hid, cout, stride, res in mobilenet_ref.blocks():
        p, j = f"features.{idx}.conv.", 0
        if tt != 1:
            add(POINTWISE, cin, hid, 1, True, False, p + "0.0", p + "0.1", f"features.{idx} expand")
            j = 1
        add(DEPTHWISE, hid, hid, stride, True, False, f"{p}{j}.0", f"{p}{j}.1", f"features.{idx} depthwise")
        add(POINTWISE, hid, cout, 1, False, bool(res), f"{p}{j + 1}", f"{p}{j + 2}", f"features.{idx} project")
    add(POINTWISE, 320, LAST, 1, True, False, "features.18.0", "features.18.1", "features.18")
    add(POOL, LAST, LAST, 3, False, False, "", "", "pools", pad_in=False)
    return t


def out_hw(e, H, W):
    if e["kind"] == POOL:
        return 1, BINS
    return ((H + 1) // 2, (W + 1) // 2) if e["stride"] == 2 else (H, W)


# ---- bf16 ---------------------------------------------------------------------------------------------------------------------------
def round_bf16(x):
    """float32 tensor -> the nearest bf16 value, ties to even, returned as float32 (finite inputs).  Integer arithmetic on the bits:
    add 0x7FFF plus the lowest kept bit, clear the 16 low bits."""
    b = x.detach().to(torch.float32).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    b = torch.where(b >= 2 ** 31, b - 2 ** 32, b).to(torch.int32)
    return b.view(torch.float32).reshape(x.shape)


# ---- weights ------------------------------------------------------------------------------------------------------------------------
def fold64(sd, e):
    """Convolution + eval BatchNorm (eps 1e-5) of launch e in float64 -> (w [cout, cin] or [cout, 9], bias [cout]); the stem's kernel is
    summed over its three input channels, which all carry the same grey image."""
    d = lambda k: sd[k].detach().to(torch.float64)
    scale = d(e["bn"] + ".weight") / torch.sqrt(d(e["bn"] + ".running_var") + mobilenet_ref.BN_EPS)
    bias = d(e["bn"] + ".bias") - d(e["bn"] + ".running_mean") * scale
    w = d(e["key"] + ".weight")
    w = w.sum(1).reshape(w.shape[0], 9) if e["kind"] == STEM else w.reshape(w.shape[0], -1)
    return w * scale[:, None], bias


def kernel_weights(e, w, bf16):
    """what the launch multiplies by: pointwise weights are bf16 in bf16 mode, stem / depthwise weights stay fp32"""
    return round_bf16(w.to(torch.float32)).double() if (bf16 and e["kind"] == POINTWISE) else w.double()


# ---- the four operations: (ref, S, K) -------------------------------------------------------------------------------------------------
def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1)


def _relu6(x, on):
    return x.clamp(0.0, 6.0) if on else x


def stem(img, w, b):
    """img [B,1,H,W] grey levels; w [32,9], b [32] -> relu6(conv3x3 stride 2 pad 1 of (img / 127.5 - 1) repeated to 3 channels), NHWC.
    The folded kernel is already summed over the 3 channels, so every channel gets w / 3: the same convolution."""
    x = (img.double() / 127.5 - 1.0).repeat(1, 3, 1, 1)
    w3 = (w.double().reshape(-1, 1, 3, 3) / 3.0).repeat(1, 3, 1, 1)
    y = F.conv2d(x, w3, b.double(), stride=2, padding=1)
    S = F.conv2d(x.abs(), w3.abs(), b.double().abs(), stride=2, padding=1)
    return _nhwc(_relu6(y, True)), _nhwc(S), 9


def depthwise(x, w, b, stride):
    """x [B,H,W,C]; w [C,9], b [C] -> relu6(conv3x3 groups=C, pad 1)"""
    C = x.shape[-1]
    w4 = w.double().reshape(C, 1, 3, 3)
    y = F.conv2d(_nchw(x.double()), w4, b.double(), stride=stride, padding=1, groups=C)
    S = F.conv2d(_nchw(x.double()).abs(), w4.abs(), b.double().abs(), stride=stride, padding=1, groups=C)
    return _nhwc(_relu6(y, True)), _nhwc(S), 9


def pointwise(x, w, b, res, relu6):
    """x [B,H,W,cin]; w [cout,cin], b [cout]; res [B,H,W,cout] or None -> (relu6 of) x w^T + b (+ res)"""
    x, w, b = x.double(), w.double(), b.double()
    y, S = x @ w.T + b, x.abs() @ w.abs().T + b.abs()
    if res is not None:
        y, S = y + res.double(), S + res.double().abs()
    return _relu6(y, relu6), S, w.shape[1]


def pool_cols(Wp):
    """pooled columns in each of the 14 adaptive bins: [floor(j Wp / 14), ceil((j + 1) Wp / 14))"""
    return [-((-(j + 1) * Wp) // BINS) - (j * Wp) // BINS for j in range(BINS)]


def pool(x):
    """x [B,H,W,C] -> AvgPool2d(3, 3), AdaptiveAvgPool2d((1, 14)), squeeze, permute: [B,14,C]; K is per bin: [1,14,1]"""
    def both(v):
        return F.adaptive_avg_pool2d(F.avg_pool2d(_nchw(v), 3, 3), (1, BINS)).squeeze(2).permute(0, 2, 1)
    x = x.double()
    K = 9 * (x.shape[1] // 3) * torch.tensor(pool_cols(x.shape[2] // 3), dtype=torch.float64).reshape(1, BINS, 1)
    return both(x), both(x.abs()), K


def run(e, x, w, b, res=None):
    """launch e on input x (stem: the image [B,1,H,W]) with the weights the launch multiplies by -> (ref, S, K)"""
    if e["kind"] == STEM:
        return stem(x, w, b)
    if e["kind"] == DEPTHWISE:
        return depthwise(x, w, b, e["stride"])
    if e["kind"] == POINTWISE:
        return pointwise(x, w, b, res if e["res"] else None, e["relu6"])
    return pool(x)


def bound(ref, S, K, u_out=U_F32):
    """u_out: the unit roundoff of the store (module docstring)"""
    return u_out * ref.abs() + (K + 4) * U_TERM * S


def clip_fractions(ref):
    """fractions of the outputs exactly at the lower and the upper clip point"""
    return float((ref == 0.0).double().mean()), float((ref == 6.0).double().mean())


# ---- shapes and inputs for per-launch GPU tests -----------------------------------------------------------------------------------------
STEM_SHAPES = ((2, 5, 7), (2, 6, 8), (1, 96, 97))                       # (B, H, W) of the image
DW_SHAPES = ((2, 3, 3), (2, 5, 7), (2, 6, 8))                           # odd / even sizes: ceil(H / 2); 3 x 3: every pixel on the border
PW_B, PW_HW = 3, ((1, 1), (1, 31), (1, 33), (7, 9), (7, 10), (1, 97))   # rows per image 1, 31, 33, 63, 70, 97
POOL_SHAPES = ((2, 3, 3), (1, 4, 44), (2, 3, 45), (1, 5, 100), (1, 3, 41))


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def gen_image(B, H, W):
    """integer grey levels 0..255, both extremes present on the border (the zero padding is of the NORMALISED image: a 0 or a 255 next
    to the padding tells a wrong padding value from the right one)"""
    img = torch.randint(0, 256, (B, 1, H, W), generator=_gen(1, B, H, W)).float()
    img[:, :, 0, 0], img[:, :, -1, -1], img[:, :, 0, -1], img[:, :, -1, 0] = 0.0, 255.0, 255.0, 0.0
    return img


def gen_input(i, e, B, H, W, bf16):
    """input of launch i (index in the table): stem -> gen_image; expansions and features.18 -> N(0, 2^2); depthwise, projections and the
    pools (which read what a ReLU6 wrote) -> U[0, 6]; rounded to bf16 in bf16 mode"""
    if e["kind"] == STEM:
        return gen_image(B, H, W)
    g = _gen(2, i, B, H, W)
    if e["kind"] == POINTWISE and e["relu6"]:
        x = torch.randn(B, H, W, e["cin"], generator=g) * 2.0
    else:
        x = torch.rand(B, H, W, e["cin"], generator=g) * 6.0
    return round_bf16(x) if bf16 else x


def gen_residual(i, e, B, H, W, bf16):
    """N(0, 1) of the output's shape for a launch that adds a residual, else None"""
    if not e["res"]:
        return None
    r = torch.randn(B, H, W, e["cout"], generator=_gen(3, i, B, H, W))
    return round_bf16(r) if bf16 else r


def scaled_state_dict(seed=0):
    """mobilenet_ref.synthetic_state_dict(seed) with the stem's BatchNorm gamma times STEM_GAMMA_SCALE"""
    sd = dict(mobilenet_ref.synthetic_state_dict(seed))
    sd["features.0.1.weight"] = sd["features.0.1.weight"] * STEM_GAMMA_SCALE
    return sd
