// Bilinear resize of channels-last float frames with torch's antialias rule: the `resize(frames, (H, W))` of the DepthCrafter stage-1 warper
// (DepthCrafter/warp_depthcrafter.py:203 -> torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=...)).
// Separable: one kernel writes a weight row per output column and per output row, a column pass [T][h][w][3] -> [T][h][W][3] and a row pass
// -> [T][H][W][3] apply them (torch's order: the last axis first).  HBM bound.  Compiled with -ffp-contract=off: a tap sum is
// ((s0 w0 + s1 w1) + s2 w2) + ... in fp32, one rounding per operation.
#include <stdint.h>

#include "common.h"

using namespace wf;

namespace {

constexpr int RS_MAX_BLOCKS = 2048;

struct RSTap {
  int start, count, step;  // taps start, start + step, ...: step is 0 where the second bilinear tap is clamped onto the first
};

__global__ void k_rs_weights(int in, int out, int aa, int maxk, RSTap* __restrict__ taps, float* __restrict__ wts) {
  for (int o = blockIdx.x * blockDim.x + threadIdx.x; o < out; o += gridDim.x * blockDim.x) {
    float* w = wts + (size_t)o * maxk;
    const float scale = (float)in / (float)out;
    RSTap t;
    if (aa) {
      const float support = scale >= 1.0f ? scale : 1.0f, inv = scale >= 1.0f ? 1.0f / scale : 1.0f;
      const float centre = scale * ((float)o + 0.5f);
      int lo = (int)(centre - support + 0.5f), hi = (int)(centre + support + 0.5f);
      lo = lo < 0 ? 0 : (lo > in - 1 ? in - 1 : lo);
      hi = hi > in ? in : hi;
      int cnt = hi - lo;
      cnt = cnt < 1 ? 1 : (cnt > maxk ? maxk : cnt);
      float total = 0.0f;
      for (int j = 0; j < cnt; ++j) {
        const float x = fabsf(((float)(j + lo) - centre + 0.5f) * inv);
        w[j] = x < 1.0f ? 1.0f - x : 0.0f;
        total += w[j];
      }
      if (total != 0.0f)
        for (int j = 0; j < cnt; ++j) w[j] /= total;
      t.start = lo;
      t.count = cnt;
      t.step = 1;
    } else {
      float src = scale * ((float)o + 0.5f) - 0.5f;
      src = src < 0.0f ? 0.0f : src;
      int i0 = (int)src;
      i0 = i0 > in - 1 ? in - 1 : i0;
      float lam = src - (float)i0;
      lam = lam < 0.0f ? 0.0f : (lam > 1.0f ? 1.0f : lam);
      w[0] = 1.0f - lam;
      w[1] = lam;
      t.start = i0;
      t.count = 2;
      t.step = i0 < in - 1 ? 1 : 0;
    }
    taps[o] = t;
  }
}

// out[r][o][c] = sum_j in[r][start_o + j step_o][c] w_o[j]: rows r = (t, y), elem = 3 floats -- or, for the row pass, r = t, elem = W * 3
__global__ void k_rs_pass(const float* __restrict__ in, float* __restrict__ out, size_t rows, int n_in, int n_out, size_t elem,
                          const RSTap* __restrict__ taps, const float* __restrict__ wts, int maxk) {
  const size_t n = rows * (size_t)n_out * elem;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t c = i % elem, ro = i / elem, o = ro % (size_t)n_out, r = ro / (size_t)n_out;
    const RSTap t = taps[o];
    const float* w = wts + o * maxk;
    const float* src = in + (r * (size_t)n_in + (size_t)t.start) * elem + c;
    float acc = src[0] * w[0];
    for (int j = 1; j < t.count; ++j) acc += src[(size_t)j * t.step * elem] * w[j];
    out[i] = acc;
  }
}

__global__ void k_rs_copy(const float* __restrict__ in, float* __restrict__ out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = in[i];
}

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
inline int max_taps(int in, int out, int aa) {
  if (!aa) return 2;
  const float scale = (float)in / (float)out;
  return (int)ceilf(scale >= 1.0f ? scale : 1.0f) * 2 + 1;
}

}  // namespace

extern "C" size_t wf_resize_bilinear_aa_f32_workspace_bytes(int T, int h, int w, int H, int W, int antialias) {
  if (T <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return 0;
  if (h == H && w == W) return 256;
  return al256((size_t)W * sizeof(RSTap)) + al256((size_t)H * sizeof(RSTap)) + al256((size_t)W * max_taps(w, W, antialias) * 4) +
         al256((size_t)H * max_taps(h, H, antialias) * 4) + al256((size_t)T * h * W * 3 * 4);
}

extern "C" int wf_resize_bilinear_aa_f32(const float* in, float* out, int T, int h, int w, int H, int W, int antialias, void* workspace,
                                         void* stream) {
  WF_CHECK_ARG(T > 0 && h > 0 && w > 0 && H > 0 && W > 0, "wf_resize_bilinear_aa_f32: empty problem");
  WF_CHECK_ARG(in && out && workspace, "wf_resize_bilinear_aa_f32: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (h == H && w == W) {
    const size_t n = (size_t)T * H * W * 3;
    hipLaunchKernelGGL(k_rs_copy, dim3(grid_for(n, 256, RS_MAX_BLOCKS)), dim3(256), 0, s, in, out, n);
    WF_LAUNCH_CHECK("wf_resize_bilinear_aa_f32");
    return WF_OK;
  }
  const int aa = antialias != 0, kw = max_taps(w, W, aa), kh = max_taps(h, H, aa);
  unsigned char* base = (unsigned char*)workspace;
  RSTap* tw = (RSTap*)base;
  RSTap* th = (RSTap*)(base + al256((size_t)W * sizeof(RSTap)));
  float* ww = (float*)((unsigned char*)th + al256((size_t)H * sizeof(RSTap)));
  float* wh = (float*)((unsigned char*)ww + al256((size_t)W * kw * 4));
  float* tmp = (float*)((unsigned char*)wh + al256((size_t)H * kh * 4));
  hipLaunchKernelGGL(k_rs_weights, dim3(grid_for((size_t)W, 256, RS_MAX_BLOCKS)), dim3(256), 0, s, w, W, aa, kw, tw, ww);
  hipLaunchKernelGGL(k_rs_weights, dim3(grid_for((size_t)H, 256, RS_MAX_BLOCKS)), dim3(256), 0, s, h, H, aa, kh, th, wh);
  hipLaunchKernelGGL(k_rs_pass, dim3(grid_for((size_t)T * h * W * 3, 256, RS_MAX_BLOCKS)), dim3(256), 0, s, in, tmp, (size_t)T * h, w, W,
                     (size_t)3, (const RSTap*)tw, (const float*)ww, kw);
  hipLaunchKernelGGL(k_rs_pass, dim3(grid_for((size_t)T * H * W * 3, 256, RS_MAX_BLOCKS)), dim3(256), 0, s, (const float*)tmp, out, (size_t)T, h,
                     H, (size_t)W * 3, (const RSTap*)th, (const float*)wh, kh);
  WF_LAUNCH_CHECK("wf_resize_bilinear_aa_f32");
  return WF_OK;
}
