// VGGT's DPT depth head (vggt/heads/dpt_head.py, DPT below): the reference runs it as an fp32 module outside autocast, so every product
// here is an fp32 product on the fp32-input MFMA v_mfma_f32_32x32x2_f32 (bit for bit a k-ordered fmaf chain, one rounding per product;
// gfx950 has no xf32).  No operand and no partial result is narrower than fp32, there is no atomic and no split of a sum over waves: two
// calls give the same bits.  Activations are channels-last fp32 [n, H, W, C].  The LayerNorm is wf_ln_modulate, the 1x1 convolutions and
// the two ConvTransposes (kernel = stride) are wf_gemm_f32 (worldforge_amd/vggt.py is the host).
//
// k_conv2d_f32: 3x3, pad 1, stride 1 or 2 as an implicit GEMM, out[pixel, co] = sum_tap sum_c in[pixel's tap][c] w[tap][co][c].
// A = weights (output channels -> accumulator rows: a lane owns 4 consecutive channels of ONE pixel per register quad, 16-byte stores),
// B = pixels (operand maps: clip.hip's header).  One workgroup = 4 waves = one [TC channels x TP pixels] tile; both operands of one K
// chunk (one tap, 32 input channels) are staged through LDS: [rows][36] floats (32 + 4 of padding: 144-byte rows keep the 16-byte
// fragment reads aligned and spread eight consecutive rows over all 32 banks).  A thread stages 16 bytes = 4 consecutive channels of a
// row and writes them as two 8-byte pieces so that inside every 8-wide block the k-th channel sits at slot 4 (k & 1) + (k >> 1): lane
// half h then reads slots 4 h .. 4 h + 3 with ONE 16-byte read and owns k = h, 2 + h, 4 + h, 6 + h, and MFMA step e multiplies
// k = 2 e (half 0) and 2 e + 1 (half 1).  The sum of an output element is therefore the chain tap 0 .. 8 outer, channel 0 .. Cin - 1
// inner, ascending, whatever the tile: its bits depend neither on n nor on where the tile edges fall nor on the tile shape chosen.
// The next chunk's global loads are issued into registers before the MFMAs of the current one (one LDS buffer, two barriers per chunk).
// Taps outside the image, rows behind the last pixel / channel and the channels behind Cin in a ragged chunk are staged as zeros
// (fma(0, 0, c) = c) and 8-wide blocks that are all padding are skipped; nothing outside a tensor is ever read, the epilogue stores
// nothing outside it.
// Tile shapes (waves as channels x pixels, accumulators per wave): 128 x 128 (2 x 2 waves, 2 x 2 accumulators: the guide's untuned GEMM
// shape) when that gives at least one workgroup per CU; 64 x 64 (2 x 2 waves, 1 x 1) below that (one frame's maps up to 84 x 148, the
// pyramid's top at any chunk size: 4 x the workgroups; at 84 x 148, 256 -> 256, one frame, 196 large tiles measured 306 us against
// 240 us for 784 small ones); 32 x 256 (1 x 4 waves, 1 x 2) for Cout <= 32 (output_conv2.0), where a 128-wide
// channel tile would run three quarters empty.
#include "common.h"
#include "mfma.h"

namespace wf {
namespace {

__device__ __forceinline__ f32x16 mfma32f(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

constexpr int CV_LD = 36;   // floats per LDS row: one K chunk of 32 + 4 of padding

struct ConvF32Args {
  const float *in, *w, *bias, *resid;
  float* out;
  int M, HoWo, Wo, Hi, Wi, Cin, Cout, stride, relu_in, relu_resid, relu_out, tiles_c;
};

template <int WGC, int WGP, int WC, int WP>
__global__ __launch_bounds__(256) void k_conv2d_f32(ConvF32Args a) {
  static_assert(WGC * WGP == 4, "four waves");
  constexpr int TC = WGC * WC * 32, TP = WGP * WP * 32, NA = TC / 32, NB = TP / 32;
  __shared__ __attribute__((aligned(16))) float As[TC * CV_LD];
  __shared__ __attribute__((aligned(16))) float Bs[TP * CV_LD];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, r31 = lane & 31, hi = lane >> 5;
  const int wc = wid % WGC, wp = wid / WGC;
  const int c_base = ((int)blockIdx.x % a.tiles_c) * TC, p_base = ((int)blockIdx.x / a.tiles_c) * TP;
  const int srow = tid >> 3, sq = tid & 7;   // staging: row srow + 32 i, channels 4 sq .. 4 sq + 3 of the chunk

  int iy0[NB], ix0[NB], boff[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int p = p_base + srow + 32 * i;
    if (p < a.M) {
      const int img = p / a.HoWo, rem = p - img * a.HoWo, oy = rem / a.Wo, ox = rem - oy * a.Wo;
      iy0[i] = oy * a.stride - 1, ix0[i] = ox * a.stride - 1, boff[i] = img * a.Hi * a.Wi;
    } else {
      iy0[i] = -4, ix0[i] = -4, boff[i] = 0;   // every tap of a row behind the last pixel is outside the image
    }
  }

  // The loads are unconditional (a piece that is padding reads the tensor's first 16 bytes instead) and nothing touches their result
  // before stage(): the zeroing of the padding and the ReLU happen there, so the loads stay in flight under the MFMAs of the chunk before.
  f32x4 ra[NA], rb[NB];
  unsigned amask = 0, bmask = 0;   // bit i: piece i is data, not padding
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  auto load = [&](int tap, int c0) {
    const int dy = tap / 3, dx = tap - 3 * dy, c = c0 + 4 * sq;
    const bool cok = c < a.Cin;
    amask = 0, bmask = 0;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int co = c_base + srow + 32 * i;
      const bool ok = cok && co < a.Cout;
      amask |= (unsigned)ok << i;
      ra[i] = *(const f32x4*)(ok ? a.w + ((size_t)tap * a.Cout + co) * a.Cin + c : a.w);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int iy = iy0[i] + dy, ix = ix0[i] + dx;
      const bool ok = cok && (unsigned)iy < (unsigned)a.Hi && (unsigned)ix < (unsigned)a.Wi;
      bmask |= (unsigned)ok << i;
      rb[i] = *(const f32x4*)(ok ? a.in + (size_t)(boff[i] + iy * a.Wi + ix) * a.Cin + c : a.in);
    }
  };
  auto stage = [&]() {
    const int col = 8 * (sq >> 1) + 2 * (sq & 1);
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const f32x4 v = (amask >> i) & 1 ? ra[i] : zero;
      float* d = As + (srow + 32 * i) * CV_LD + col;
      *(float2*)d = make_float2(v[0], v[2]);
      *(float2*)(d + 4) = make_float2(v[1], v[3]);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      f32x4 v = (bmask >> i) & 1 ? rb[i] : zero;
      if (a.relu_in) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
      }
      float* d = Bs + (srow + 32 * i) * CV_LD + col;
      *(float2*)d = make_float2(v[0], v[2]);
      *(float2*)(d + 4) = make_float2(v[1], v[3]);
    }
  };

  f32x16 acc[WC][WP];
#pragma unroll
  for (int i = 0; i < WC; ++i)
#pragma unroll
    for (int j = 0; j < WP; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  int tap = 0, c0 = 0;
  load(0, 0);
  while (tap < 9) {
    stage();
    __syncthreads();
    const int nkb = min(4, (a.Cin - c0 + 7) >> 3);
    c0 += 32;
    if (c0 >= a.Cin) c0 = 0, ++tap;
    if (tap < 9) load(tap, c0);
    for (int kb = 0; kb < nkb; ++kb) {
      f32x4 af[WC], bf[WP];
#pragma unroll
      for (int i = 0; i < WC; ++i) af[i] = *(const f32x4*)(As + ((wc * WC + i) * 32 + r31) * CV_LD + 8 * kb + 4 * hi);
#pragma unroll
      for (int j = 0; j < WP; ++j) bf[j] = *(const f32x4*)(Bs + ((wp * WP + j) * 32 + r31) * CV_LD + 8 * kb + 4 * hi);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < WC; ++i)
#pragma unroll
          for (int j = 0; j < WP; ++j) acc[i][j] = mfma32f(af[i][e], bf[j][e], acc[i][j]);
    }
    __syncthreads();
  }

  // epilogue: registers 4 g .. 4 g + 3 = channels 8 g + 4 hi + 0..3 of the 32-block, pixel = the lane's column
#pragma unroll
  for (int j = 0; j < WP; ++j) {
    const int p = p_base + (wp * WP + j) * 32 + r31;
    if (p >= a.M) continue;
#pragma unroll
    for (int i = 0; i < WC; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int co = c_base + (wc * WC + i) * 32 + 8 * g + 4 * hi;
        if (co >= a.Cout) continue;   // Cout % 4 == 0: a quad is inside or outside
        const size_t o = (size_t)p * a.Cout + co;
        f32x4 y = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
        if (a.bias) y += *(const f32x4*)(a.bias + co);
        if (a.resid) {
          f32x4 r = *(const f32x4*)(a.resid + o);
          if (a.relu_resid) {
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = fmaxf(r[e], 0.f);
          }
          y += r;
        }
        if (a.relu_out) {
#pragma unroll
          for (int e = 0; e < 4; ++e) y[e] = fmaxf(y[e], 0.f);
        }
        *(f32x4*)(a.out + o) = y;
      }
  }
}

// F.interpolate(mode="bilinear", align_corners=True) as PyTorch evaluates it in fp32 (area_pixel_compute_scale: scale = (in - 1) / (out - 1),
// 0 when out == 1; src = scale * dst; i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1; rows blended after columns), one
// thread per output pixel and 4 channels.
struct ResizeArgs {
  const float *in, *col, *row;
  float* out;
  int Hi, Wi, Ho, Wo, C;
  float sy, sx;
  size_t total;   // n Ho Wo C / 4
};

__global__ void k_resize_bilinear_cl(ResizeArgs a) {
  const int C4 = a.C >> 2, half = a.C >> 1;
  const bool same = a.Hi == a.Ho && a.Wi == a.Wo;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4) * 4;
    size_t pix = i / C4;
    const int ox = (int)(pix % a.Wo);
    pix /= a.Wo;
    const int oy = (int)(pix % a.Ho);
    const size_t img = pix / a.Ho;
    const float* src = a.in + img * a.Hi * a.Wi * a.C + c;
    f32x4 v;
    if (same) {
      v = *(const f32x4*)(src + ((size_t)oy * a.Wi + ox) * a.C);
    } else {
      const float fy = a.sy * (float)oy, fx = a.sx * (float)ox;
      const int y0 = min((int)fy, a.Hi - 1), x0 = min((int)fx, a.Wi - 1);   // the clamp never binds: fy <= Hi - 1 up to one rounding
      const int y1 = min(y0 + 1, a.Hi - 1), x1 = min(x0 + 1, a.Wi - 1);
      const float ly1 = fy - (float)y0, lx1 = fx - (float)x0, ly0 = 1.f - ly1, lx0 = 1.f - lx1;
      const f32x4 v00 = *(const f32x4*)(src + ((size_t)y0 * a.Wi + x0) * a.C), v01 = *(const f32x4*)(src + ((size_t)y0 * a.Wi + x1) * a.C);
      const f32x4 v10 = *(const f32x4*)(src + ((size_t)y1 * a.Wi + x0) * a.C), v11 = *(const f32x4*)(src + ((size_t)y1 * a.Wi + x1) * a.C);
      v = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
    }
    if (a.col) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ch = c + e;
        v[e] += ch < half ? a.col[(size_t)ox * half + ch] : a.row[(size_t)oy * half + ch - half];
      }
    }
    *(f32x4*)(a.out + i * 4) = v;
  }
}

// output_conv2.2 (1x1, Cin -> 2) + activate_head("exp", "expp1") (head_act.py): one thread per pixel, the two dot products as fmaf chains
// over ascending channels on top of the bias.
__global__ void k_dpt_depth_out(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ depth,
                                float* __restrict__ conf, size_t npix, int Cin) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (size_t)gridDim.x * blockDim.x) {
    const float* row = x + p * Cin;
    float v0 = b[0], v1 = b[1];
    for (int c = 0; c < Cin; c += 4) {
      const f32x4 xv = *(const f32x4*)(row + c), w0 = *(const f32x4*)(w + c), w1 = *(const f32x4*)(w + Cin + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) v0 = fmaf(xv[e], w0[e], v0), v1 = fmaf(xv[e], w1[e], v1);
    }
    depth[p] = expf(v0);
    conf[p] = 1.f + expf(v1);
  }
}

template <int WGC, int WGP, int WC, int WP>
int launch_conv(ConvF32Args a, hipStream_t st) {
  constexpr int TC = WGC * WC * 32, TP = WGP * WP * 32;
  a.tiles_c = (a.Cout + TC - 1) / TC;
  const int64_t blocks = (int64_t)a.tiles_c * (((int64_t)a.M + TP - 1) / TP);
  if (blocks > ((int64_t)1 << 30)) {
    set_error("wf_conv2d_f32: %lld tiles", (long long)blocks);
    return WF_EINVAL;
  }
  hipLaunchKernelGGL((k_conv2d_f32<WGC, WGP, WC, WP>), dim3((unsigned)blocks), dim3(256), 0, st, a);
  WF_LAUNCH_CHECK("wf_conv2d_f32");
  return WF_OK;
}

}  // namespace
}  // namespace wf

using namespace wf;

extern "C" int wf_conv2d_f32(const float* in, const float* w_packed, const float* bias, const float* resid, float* out, int n, int Hi, int Wi,
                             int Cin, int Cout, int stride, int relu_in, int relu_resid, int relu_out, void* stream) {
  WF_CHECK_ARG(in && w_packed && out, "wf_conv2d_f32: null pointer");
  WF_CHECK_ARG(n >= 1 && Hi >= 1 && Wi >= 1, "wf_conv2d_f32: need n, Hi, Wi >= 1 (n=%d Hi=%d Wi=%d)", n, Hi, Wi);
  WF_CHECK_ARG(Cin >= 4 && Cout >= 4 && Cin % 4 == 0 && Cout % 4 == 0, "wf_conv2d_f32: need Cin %% 4 == 0, Cout %% 4 == 0 (Cin=%d Cout=%d)", Cin, Cout);
  WF_CHECK_ARG(stride == 1 || stride == 2, "wf_conv2d_f32: stride %d is not 1 or 2", stride);
  WF_CHECK_ARG(!relu_resid || resid, "wf_conv2d_f32: relu_resid without resid");
  WF_CHECK_ARG((((uintptr_t)in | (uintptr_t)w_packed | (uintptr_t)bias | (uintptr_t)resid | (uintptr_t)out) & 15) == 0,
               "wf_conv2d_f32: pointers must be 16-byte aligned");
  const int Ho = (Hi - 1) / stride + 1, Wo = (Wi - 1) / stride + 1;
  const int64_t M = (int64_t)n * Ho * Wo;
  WF_CHECK_ARG((int64_t)n * Hi * Wi * Cin < ((int64_t)1 << 31) && M * Cout < ((int64_t)1 << 31) && (int64_t)9 * Cin * Cout < ((int64_t)1 << 31),
               "wf_conv2d_f32: a tensor has 2^31 elements or more (n=%d Hi=%d Wi=%d Cin=%d Cout=%d)", n, Hi, Wi, Cin, Cout);
  ConvF32Args a;
  a.in = in, a.w = w_packed, a.bias = bias, a.resid = resid, a.out = out;
  a.M = (int)M, a.HoWo = Ho * Wo, a.Wo = Wo, a.Hi = Hi, a.Wi = Wi, a.Cin = Cin, a.Cout = Cout, a.stride = stride;
  a.relu_in = relu_in != 0, a.relu_resid = relu_resid != 0, a.relu_out = relu_out != 0, a.tiles_c = 0;
  const hipStream_t st = (hipStream_t)stream;
  if (Cout <= 32) return launch_conv<1, 4, 1, 2>(a, st);
  const int64_t big = ((M + 127) / 128) * (((int64_t)Cout + 127) / 128);
  if (big >= 256) return launch_conv<2, 2, 2, 2>(a, st);
  return launch_conv<2, 2, 1, 1>(a, st);
}

extern "C" int wf_resize_bilinear_cl_f32(const float* in, float* out, int n, int Hi, int Wi, int Ho, int Wo, int C, const float* col_table,
                                         const float* row_table, void* stream) {
  WF_CHECK_ARG(in && out, "wf_resize_bilinear_cl_f32: null pointer");
  WF_CHECK_ARG(n >= 1 && Hi >= 1 && Wi >= 1 && Ho >= 1 && Wo >= 1, "wf_resize_bilinear_cl_f32: need n and every size >= 1");
  WF_CHECK_ARG(C >= 4 && C % 4 == 0, "wf_resize_bilinear_cl_f32: need C %% 4 == 0 (C=%d)", C);
  WF_CHECK_ARG((col_table == nullptr) == (row_table == nullptr), "wf_resize_bilinear_cl_f32: the column and row tables come together");
  WF_CHECK_ARG((((uintptr_t)in | (uintptr_t)out) & 15) == 0 && (((uintptr_t)col_table | (uintptr_t)row_table) & 3) == 0,
               "wf_resize_bilinear_cl_f32: in / out must be 16-byte aligned, the tables 4-byte aligned");
  ResizeArgs a;
  a.in = in, a.out = out, a.col = col_table, a.row = row_table;
  a.Hi = Hi, a.Wi = Wi, a.Ho = Ho, a.Wo = Wo, a.C = C;
  a.sy = Ho > 1 ? (float)(Hi - 1) / (float)(Ho - 1) : 0.f;
  a.sx = Wo > 1 ? (float)(Wi - 1) / (float)(Wo - 1) : 0.f;
  a.total = (size_t)n * Ho * Wo * (C / 4);
  hipLaunchKernelGGL(k_resize_bilinear_cl, dim3(grid_for(a.total, 256, 65536)), dim3(256), 0, (hipStream_t)stream, a);
  WF_LAUNCH_CHECK("wf_resize_bilinear_cl_f32");
  return WF_OK;
}

extern "C" int wf_dpt_depth_out(const float* rows, const float* w, const float* b, float* depth, float* conf, size_t npix, int Cin, void* stream) {
  WF_CHECK_ARG(rows && w && b && depth && conf, "wf_dpt_depth_out: null pointer");
  WF_CHECK_ARG(npix >= 1 && Cin >= 4 && Cin % 4 == 0, "wf_dpt_depth_out: need npix >= 1, Cin %% 4 == 0 (Cin=%d)", Cin);
  WF_CHECK_ARG((((uintptr_t)rows | (uintptr_t)w) & 15) == 0 && (((uintptr_t)b | (uintptr_t)depth | (uintptr_t)conf) & 3) == 0,
               "wf_dpt_depth_out: rows / w must be 16-byte aligned, b / depth / conf 4-byte aligned");
  hipLaunchKernelGGL(k_dpt_depth_out, dim3(grid_for(npix, 256, 65536)), dim3(256), 0, (hipStream_t)stream, rows, w, b, depth, conf, npix, Cin);
  WF_LAUNCH_CHECK("wf_dpt_depth_out");
  return WF_OK;
}
