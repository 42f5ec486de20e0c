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

// The row pass of wf_resample_u8_window_f32, the table look-up and the move to planar floats in one kernel:
//   out[t][c][oy][ox] = lut[c][clip8((1 << 21) + sum_j src[t][first_oy + j][xoff + ox][c] * coefs[oy][j])],  oy < Hc, ox < Wc,
// src = the column pass's u8 intermediate or the input itself (fstride / rstride = bytes per frame / per row, xoff = the window's first
// column in it); bounds == NULL is the skipped row pass: one tap of weight 1 on row y0 + oy.  bounds / coefs start at the window's first row.
// A wavefront owns one output row (t, oy) at a time, so the tap window and the coefficients are wave-uniform (scalar loads), and walks the
// row's C planes in ALIGNED groups of four floats: a plane row of Wc floats starts at any phase `a` of a 16-byte line, group g holds the
// elements 4 g - a .. 4 g - a + 3, a lane computes one group and stores it whole, the clipped first and last group element by element.
// The C tables of 256 floats sit in LDS.
__global__ void __launch_bounds__(256) k_ru_window_lut(const uint8_t* __restrict__ src, size_t fstride, size_t rstride, int xoff, int y0,
                                                       const int32_t* __restrict__ bounds, const int32_t* __restrict__ coefs, int ksize,
                                                       const float* __restrict__ lut, float* __restrict__ out, int T, int C, int Hc,
                                                       int Wc) {
  __shared__ float s_lut[3 * 256];
  for (int i = threadIdx.x; i < C * 256; i += 256) s_lut[i] = lut[i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const unsigned phase = (unsigned)(((uintptr_t)out >> 2) & 3);
  const size_t rows = (size_t)T * Hc, step = (size_t)gridDim.x * 4;
  for (size_t row0 = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); row0 < rows; row0 += step) {
    const unsigned row_lo = __builtin_amdgcn_readfirstlane((unsigned)row0), row_hi = __builtin_amdgcn_readfirstlane((unsigned)(row0 >> 32));
    const size_t row = ((size_t)row_hi << 32) | row_lo;  // the same in every lane of the wavefront: everything derived from it is scalar
    const size_t t = row / (size_t)Hc;
    const int oy = (int)(row - t * (size_t)Hc);
    const int first = bounds ? bounds[2 * oy] : y0 + oy, count = bounds ? bounds[2 * oy + 1] : 1;
    const int32_t* k = bounds ? coefs + (size_t)oy * ksize : nullptr;
    const uint8_t* base = src + t * fstride + (size_t)first * rstride + (size_t)xoff * C;
    for (int c = 0; c < C; ++c) {
      const size_t plane = ((t * (size_t)C + c) * Hc + oy) * (size_t)Wc;  // index of out[t][c][oy][0]
      const int a = (int)((phase + (unsigned)(plane & 3)) & 3), ng = (Wc + a + 3) >> 2;
      const float* tab = s_lut + c * 256;
      for (int g = lane; g < ng; g += 64) {
        const int e0 = 4 * g - a;
        int col[4], acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int e = e0 + q;
          col[q] = (e < 0 ? 0 : (e >= Wc ? Wc - 1 : e)) * C + c;  // a clipped element recomputes its neighbour and is not stored
          acc[q] = 1 << (RU_BITS - 1);
        }
        for (int j = 0; j < count; ++j) {
          const uint8_t* r = base + (size_t)j * rstride;
          const int kj = bounds ? k[j] : (1 << RU_BITS);
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[q] += (int)r[col[q]] * kj;
        }
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          int b = acc[q] >> RU_BITS;
          b = b < 0 ? 0 : (b > 255 ? 255 : b);
          v[q] = tab[b];
        }
        float* dst = out + plane + e0;
        if (e0 >= 0 && e0 + 4 <= Wc) {
          *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (e0 + q >= 0 && e0 + q < Wc) dst[q] = v[q];
        }
      }
    }
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

extern "C" size_t wf_resample_u8_window_f32_workspace_bytes(int T, int h, int w, int H, int W, int C, int y0, int x0, int Hc, int Wc) {
  if (T <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || Hc <= 0 || Wc <= 0 || (C != 1 && C != 3)) return 0;
  if (y0 < 0 || x0 < 0 || (long long)y0 + Hc > H || (long long)x0 + Wc > W) return 0;
  if (w == W) return 256;
  return al256((size_t)T * h * Wc * C);  // the column pass's u8 rows [T][h][Wc][C], addressed by source row
}

extern "C" int wf_resample_u8_window_f32(const uint8_t* in, float* out, int T, int h, int w, int H, int W, int C, int y0, int x0, int Hc,
                                         int Wc, const int32_t* xbounds, const int32_t* xcoefs, int xk, const int32_t* ybounds,
                                         const int32_t* ycoefs, int yk, const float* lut, void* workspace, void* stream) {
  WF_CHECK_ARG(T > 0 && h > 0 && w > 0 && H > 0 && W > 0 && Hc > 0 && Wc > 0, "wf_resample_u8_window_f32: empty problem");
  WF_CHECK_ARG(C == 1 || C == 3, "wf_resample_u8_window_f32: C = %d, 1 or 3 only", C);
  WF_CHECK_ARG(y0 >= 0 && x0 >= 0 && (long long)y0 + Hc <= H && (long long)x0 + Wc <= W,
               "wf_resample_u8_window_f32: the window %d x %d at (%d, %d) leaves %d x %d", Hc, Wc, y0, x0, H, W);
  WF_CHECK_ARG(in && out && lut, "wf_resample_u8_window_f32: null pointer");
  WF_CHECK_ARG((size_t)W * C < ((size_t)1 << 31) && (size_t)w * C < ((size_t)1 << 31), "wf_resample_u8_window_f32: a row of 2^31 bytes or more");
  const bool xpass = w != W, ypass = h != H;
  WF_CHECK_ARG(!xpass || (xbounds && xcoefs && xk > 0), "wf_resample_u8_window_f32: the column pass needs its tables");
  WF_CHECK_ARG(!ypass || (ybounds && ycoefs && yk > 0), "wf_resample_u8_window_f32: the row pass needs its tables");
  WF_CHECK_ARG(!xpass || workspace, "wf_resample_u8_window_f32: the column pass needs the workspace");
  hipStream_t s = (hipStream_t)stream;
  const uint8_t* src = in;
  size_t fstride = (size_t)h * w * C, rstride = (size_t)w * C;
  int xoff = x0;
  if (xpass) {
    // Source rows the window's output rows can tap.  The tables live on the device, so the range is taken from the geometry they were
    // built from: a tap window is centred at (i + 0.5) h / H and reaches (yk - 1) / 2 >= the support to either side; one row of slack each
    // way covers the rounding.  A row outside the exact range costs time only; the intermediate is addressed by source row.
    int r0 = 0, r1 = h;
    if (ypass) {
      const double scale = (double)h / (double)H, half = 0.5 * (yk - 1) + 0.5;
      const double lo = floor((y0 + 0.5) * scale - half) - 1.0, hi = ceil((y0 + Hc - 0.5) * scale + half) + 1.0;
      r0 = lo < 0.0 ? 0 : (int)lo;
      r1 = hi > (double)h ? h : (int)hi;
    } else {
      r0 = y0;
      r1 = y0 + Hc;
    }
    uint8_t* mid = (uint8_t*)workspace;
    const size_t mrow = (size_t)Wc * C;
    const int32_t* xb = xbounds + 2 * (size_t)x0;
    const int32_t* xc = xcoefs + (size_t)x0 * xk;
    if (r0 == 0 && r1 == h) {
      ru_launch(in, mid, (size_t)T * h, w, Wc, (size_t)C, xb, xc, xk, s);
    } else {
      for (int t = 0; t < T; ++t)
        ru_launch(in + ((size_t)t * h + r0) * rstride, mid + ((size_t)t * h + r0) * mrow, (size_t)(r1 - r0), w, Wc, (size_t)C, xb, xc, xk, s);
    }
    src = mid;
    fstride = (size_t)h * mrow;
    rstride = mrow;
    xoff = 0;
  }
  const size_t rows = (size_t)T * Hc;
  hipLaunchKernelGGL(k_ru_window_lut, dim3(grid_for((rows + 3) / 4 * 256, 256, RS_MAX_BLOCKS)), dim3(256), 0, s, src, fstride, rstride, xoff, y0,
                     ypass ? ybounds + 2 * (size_t)y0 : (const int32_t*)nullptr, ypass ? ycoefs + (size_t)y0 * yk : (const int32_t*)nullptr, yk,
                     lut, out, T, C, Hc, Wc);
  WF_LAUNCH_CHECK("wf_resample_u8_window_f32");
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
