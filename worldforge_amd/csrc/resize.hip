// Bilinear resize of channels-last float frames with torch's antialias rule: the `resize(frames, (H, W))` of the DepthCrafter stage-1 warper
// (DepthCrafter/warp_depthcrafter.py:203 -> torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=...)).
// Separable: one kernel writes a weight row per output column and per output row, a column pass [T][h][w][3] -> [T][h][W][3] and a row pass
// -> [T][H][W][3] apply them (torch's order: the last axis first).  HBM bound.  Compiled with -ffp-contract=off: a tap sum is
// ((s0 w0 + s1 w1) + s2 w2) + ... in fp32, one rounding per operation.
// Below it, PIL.Image.resize on 8-bit frames (wf_resample_u8: Pillow's fixed-point two-pass resample with host-built tables, integers only)
// and the 256-entry u8 -> f32 table look-up that follows it on the way from stage 1 to the sampler (wf_u8_lut_planar_f32).
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

// ---- Pillow's 8-bit resample (wf_resample_u8): integer arithmetic only ------------------------------------------------------------------
constexpr int RU_BITS = 22;  // Pillow's PRECISION_BITS for 8-bit pixels: 32 - 8 - 2

// One pass over `rows` rows of n_in elements of `elem` bytes each (columns: rows = T h, elem = C; rows: rows = T, elem = W C):
//   out[r][o][e] = clip8((1 << 21) + sum_j in[r][first_o + j][e] * coefs[o][j]).
// The output is walked as one flat byte array in ALIGNED dwords (a row of 3 W bytes starts anywhere): a thread owns the dword at
// out - head + 4 d, head = the pointer's offset in its dword, computes its four bytes from byte loads and stores it whole; the first and
// last dword of the array may be partial and are stored byte by byte.  Neighbouring lanes write neighbouring dwords and read neighbouring
// bytes of each tap row.
__global__ void __launch_bounds__(256) k_ru_pass(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, size_t n, int n_in, int n_out,
                                                 unsigned elem, const int32_t* __restrict__ bounds, const int32_t* __restrict__ coefs,
                                                 int ksize, unsigned head) {
  const size_t nd = (n + head + 3) / 4, rowb = (size_t)n_out * elem;
  for (size_t d = (size_t)blockIdx.x * blockDim.x + threadIdx.x; d < nd; d += (size_t)gridDim.x * blockDim.x) {
    const long long b0 = (long long)(4 * d) - (long long)head;  // byte index of this dword's first byte; < 0 only for d = 0
    const size_t i0 = b0 < 0 ? 0 : (size_t)b0;
    size_t r = i0 / rowb;
    const unsigned rem = (unsigned)(i0 - r * rowb);  // rowb = n_out * elem < 2^32: checked by the entry point
    unsigned o = rem / elem, e = rem - o * elem;
    uint32_t packed = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const long long i = b0 + q;
      if (i < 0 || (size_t)i >= n) continue;
      const int first = bounds[2 * o], count = bounds[2 * o + 1];
      const int32_t* k = coefs + (size_t)o * ksize;
      const uint8_t* src = in + (r * (size_t)n_in + (size_t)first) * elem + e;
      int acc = 1 << (RU_BITS - 1);
      for (int j = 0; j < count; ++j) acc += (int)src[(size_t)j * elem] * k[j];
      int v = acc >> RU_BITS;
      v = v < 0 ? 0 : (v > 255 ? 255 : v);
      packed |= (uint32_t)v << (8 * q);
      if (++e == elem) {
        e = 0;
        if (++o == (unsigned)n_out) {
          o = 0;
          ++r;
        }
      }
    }
    if (b0 >= 0 && (size_t)b0 + 4 <= n) {
      *(uint32_t*)(out + b0) = packed;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const long long i = b0 + q;
        if (i >= 0 && (size_t)i < n) out[i] = (uint8_t)(packed >> (8 * q));
      }
    }
  }
}

// out[c][t][p] = lut[in[t][p][c]]
__global__ void __launch_bounds__(256) k_u8_lut_planar(const uint8_t* __restrict__ in, const float* __restrict__ lut, float* __restrict__ out,
                                                       size_t T, size_t P, int C) {
  const size_t n = (size_t)C * T * P;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t p = i % P, ct = i / P, t = ct % T, c = ct / T;
    out[i] = lut[in[(t * P + p) * (size_t)C + c]];
  }
}

constexpr int RU_MAX_BLOCKS = 16384;  // 256 CUs x 8 blocks of 256 threads, a few rounds of them: the loops above stride over the rest

void ru_launch(const uint8_t* in, uint8_t* out, size_t rows, int n_in, int n_out, size_t elem, const int32_t* bounds, const int32_t* coefs,
               int ksize, hipStream_t s) {
  const size_t n = rows * (size_t)n_out * elem;
  const unsigned head = (unsigned)((uintptr_t)out & 3);
  hipLaunchKernelGGL(k_ru_pass, dim3(grid_for((n + head + 3) / 4, 256, RU_MAX_BLOCKS)), dim3(256), 0, s, in, out, n, n_in, n_out,
                     (unsigned)elem, bounds, coefs, ksize, head);
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

extern "C" size_t wf_resample_u8_workspace_bytes(int T, int h, int w, int H, int W, int C) {
  if (T <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || (C != 1 && C != 3)) return 0;
  if (h == H || w == W) return 256;
  return al256((size_t)T * h * W * C);
}

extern "C" int wf_resample_u8(const uint8_t* in, uint8_t* out, int T, int h, int w, int H, int W, int C, const int32_t* xbounds,
                              const int32_t* xcoefs, int xk, const int32_t* ybounds, const int32_t* ycoefs, int yk, void* workspace,
                              void* stream) {
  WF_CHECK_ARG(T > 0 && h > 0 && w > 0 && H > 0 && W > 0, "wf_resample_u8: empty problem");
  WF_CHECK_ARG(C == 1 || C == 3, "wf_resample_u8: C = %d, 1 or 3 only", C);
  WF_CHECK_ARG(in && out, "wf_resample_u8: null pointer");
  WF_CHECK_ARG((size_t)H * W * C < ((size_t)1 << 32), "wf_resample_u8: an output frame of 2^32 bytes or more");
  const bool xpass = w != W, ypass = h != H;
  WF_CHECK_ARG(!xpass || (xbounds && xcoefs && xk > 0), "wf_resample_u8: the column pass needs its tables");
  WF_CHECK_ARG(!ypass || (ybounds && ycoefs && yk > 0), "wf_resample_u8: the row pass needs its tables");
  WF_CHECK_ARG(!(xpass && ypass) || workspace, "wf_resample_u8: two passes need the workspace");
  hipStream_t s = (hipStream_t)stream;
  if (!xpass && !ypass) {
    hipError_t e = hipMemcpyAsync(out, in, (size_t)T * H * W * C, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return check_hip(e, "wf_resample_u8 (copy)");
    return WF_OK;
  }
  const uint8_t* src = in;
  if (xpass) {
    uint8_t* dst = ypass ? (uint8_t*)workspace : out;
    ru_launch(src, dst, (size_t)T * h, w, W, (size_t)C, xbounds, xcoefs, xk, s);
    src = dst;
  }
  if (ypass) ru_launch(src, out, (size_t)T, h, H, (size_t)W * C, ybounds, ycoefs, yk, s);
  WF_LAUNCH_CHECK("wf_resample_u8");
  return WF_OK;
}

extern "C" int wf_u8_lut_planar_f32(const uint8_t* in, const float* lut, float* out, int T, int h, int w, int C, void* stream) {
  WF_CHECK_ARG(T > 0 && h > 0 && w > 0 && C > 0, "wf_u8_lut_planar_f32: empty problem");
  WF_CHECK_ARG(in && lut && out, "wf_u8_lut_planar_f32: null pointer");
  const size_t P = (size_t)h * w;
  hipLaunchKernelGGL(k_u8_lut_planar, dim3(grid_for((size_t)C * T * P, 256, RU_MAX_BLOCKS)), dim3(256), 0, (hipStream_t)stream, in, lut, out,
                     (size_t)T, P, C);
  WF_LAUNCH_CHECK("wf_u8_lut_planar_f32");
  return WF_OK;
}
