// Point-cloud renderer + depth-edge point filter of the DepthCrafter stage-1 warper (dynamic scenes: one point cloud per video frame).
//
// Replaces DepthCrafter/utils.py project_points_to_image_pytorch (:103-171: pytorch3d PointsRasterizer with radius 0.005, nearest point per
// pixel, 5 x 5 opening of the coverage mask) and filter_edge_points / detect_depth_edges (:495-567: Sobel magnitude, 7 x 7 dilation, 5 x 5
// min / max depth-jump test) as warp_depthcrafter.py:255-288 runs them for every frame.  HBM / atomic bound: a 64-bit atomicMin z-buffer
// (view depth bits << 32 | point index: nearest wins, ties to the smaller index), a handful of 5 x 5 / 7 x 7 stencils on byte masks.
// pytorch3d and OpenCV are third-party packages absent from the reference tree: their behaviour is restated (oracle/pointrender.py lists the
// statements) and parity with them is UNPINNED.  Compiled with -ffp-contract=off: the projection is the oracle's float32 op sequence.
#include <stdint.h>

#include "common.h"

using namespace wf;

namespace {

struct PRCam {
  float R[9];   // pytorch3d rotation (row vectors: view = p R + T)
  float T[3];
  float focal[2], p0[2];
};

// rasterization_utils.cuh PixToNonSquareNdc
__device__ __forceinline__ float pix_to_ndc(int i, int S1, int S2) {
  const float r = S1 <= S2 ? 2.0f : ((float)S1 * 2.0f) / (float)S2;
  const float o = r / 2.0f;
  return -o + (r * (float)i + o) / (float)S1;
}

__global__ void k_pr_splat(const float* __restrict__ pts, const unsigned char* __restrict__ drop, int n, PRCam c, int H, int W, float radius,
                           unsigned long long* __restrict__ zbuf) {
  const float r2 = radius * radius;
  const float rx = W <= H ? 2.0f : ((float)W * 2.0f) / (float)H, ry = H <= W ? 2.0f : ((float)H * 2.0f) / (float)W;
  const int reach = (int)ceilf(radius * fmaxf((float)W / rx, (float)H / ry)) + 1;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (drop && drop[i]) continue;
    const float px = pts[3 * (size_t)i], py = pts[3 * (size_t)i + 1], pz = pts[3 * (size_t)i + 2];
    float v[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) v[j] = ((px * c.R[j] + py * c.R[3 + j]) + pz * c.R[6 + j]) + c.T[j];
    const float z = v[2];
    if (!(z >= 0.0f)) continue;  // behind the camera (rasterize_points: pz < 0), NaN
    const float x = (c.focal[0] * v[0] + c.p0[0] * z) / z, y = (c.focal[1] * v[1] + c.p0[1] * z) / z;
    if (!isfinite(x) || !isfinite(y)) continue;
    // flipped pixel indices i' = S - 1 - i of the centres around the point
    const int bx = (int)floorf((x + rx * 0.5f) * (float)W / rx - 0.5f), by = (int)floorf((y + ry * 0.5f) * (float)H / ry - 0.5f);
    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)i;
    for (int dy = -reach; dy <= reach + 1; ++dy) {
      const int iy = by + dy;
      if (iy < 0 || iy >= H) continue;
      const float ddy = pix_to_ndc(iy, H, W) - y;
      for (int dx = -reach; dx <= reach + 1; ++dx) {
        const int ix = bx + dx;
        if (ix < 0 || ix >= W) continue;
        const float ddx = pix_to_ndc(ix, W, H) - x;
        if (ddx * ddx + ddy * ddy < r2) atomicMin(&zbuf[(size_t)(H - 1 - iy) * W + (W - 1 - ix)], key);
      }
    }
  }
}

__global__ void k_pr_mask(const unsigned long long* __restrict__ zbuf, unsigned char* __restrict__ m, size_t hw) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += (size_t)gridDim.x * blockDim.x) m[i] = zbuf[i] != ~0ull;
}

// K x K erosion (MIN) or dilation (MAX) of a byte mask, anchor at the centre, pixels outside the image ignored (OpenCV's default border
// value for morphology: +inf for erode, -inf for dilate)
template <bool ERODE>
__global__ void k_morph(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, int H, int W, int K) {
  const int r = K >> 1;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)H * W; i += (size_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
    unsigned char v = ERODE ? 1 : 0;
    for (int dy = -r; dy <= r; ++dy) {
      const int yy = y + dy;
      if (yy < 0 || yy >= H) continue;
      for (int dx = -r; dx <= r; ++dx) {
        const int xx = x + dx;
        if (xx < 0 || xx >= W) continue;
        const unsigned char s = in[(size_t)yy * W + xx] != 0;
        v = ERODE ? (v & s) : (v | s);
      }
    }
    out[i] = v;
  }
}

// image[p] = features[idx[p]] where the final mask is set, else 0 (utils.py:149-169)
__global__ void k_pr_resolve(const unsigned long long* __restrict__ zbuf, const unsigned char* __restrict__ mask,
                             const float* __restrict__ feat, int F, float* __restrict__ img, size_t hw) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += (size_t)gridDim.x * blockDim.x) {
    const bool on = mask[i] != 0;
    const unsigned idx = (unsigned)(zbuf[i] & 0xffffffffull);
    for (int k = 0; k < F; ++k) img[i * F + k] = on ? feat[(size_t)idx * F + k] : 0.0f;
  }
}

// ---- filter_edge_points ----
__device__ __forceinline__ int reflect101(int i, int n) {  // BORDER_REFLECT_101 (n >= 2)
  if (i < 0) i = -i;
  if (i >= n) i = 2 * n - 2 - i;
  return i < 0 ? 0 : i;
}
__device__ __forceinline__ int reflect_edge(int i, int n) {  // scipy.ndimage mode="reflect": d c b a | a b c d | d c b a
  if (i < 0) i = -i - 1;
  if (i >= n) i = 2 * n - 1 - i;
  return i < 0 ? 0 : (i >= n ? n - 1 : i);
}
// Sobel (ksize 3, CV_64F) gradient magnitude, and its maximum as the bits of a non-negative double (atomicMax on the integer image)
__global__ void k_sobel_mag(const float* __restrict__ d, double* __restrict__ mag, unsigned long long* __restrict__ gmax, int H, int W) {
  unsigned long long lm = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)H * W; i += (size_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
    const int ym = reflect101(y - 1, H), yp = reflect101(y + 1, H), xm = reflect101(x - 1, W), xp = reflect101(x + 1, W);
    auto at = [&](int yy, int xx) { return (double)d[(size_t)yy * W + xx]; };
    // correlation in row-major tap order (dy, dx), zero taps skipped
    const double gx = ((((-at(ym, xm) + at(ym, xp)) - 2.0 * at(y, xm)) + 2.0 * at(y, xp)) - at(yp, xm)) + at(yp, xp);
    const double gy = ((((-at(ym, xm) - 2.0 * at(ym, x)) - at(ym, xp)) + at(yp, xm)) + 2.0 * at(yp, x)) + at(yp, xp);
    const double m = sqrt(gx * gx + gy * gy);
    mag[i] = m;
    const unsigned long long b = (unsigned long long)__double_as_longlong(m);
    if (m == m && b > lm) lm = b;
  }
  if (lm && lm > __builtin_nontemporal_load(gmax)) atomicMax(gmax, lm);  // (same-address atomics serialise: only while the maximum still grows)
}
__global__ void k_edge_thresh(const double* __restrict__ mag, const unsigned long long* __restrict__ gmax, double thr, unsigned char* __restrict__ e,
                              size_t hw) {
  const double mx = __longlong_as_double((long long)*gmax);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += (size_t)gridDim.x * blockDim.x) {
    const double m = mx > 0.0 ? mag[i] / mx : mag[i];
    e[i] = m > thr;
  }
}
// drop |= (max - min over the (2 r + 1)^2 window, scipy "reflect" border) > jump
__global__ void k_depth_jump(const float* __restrict__ d, unsigned char* __restrict__ drop, int H, int W, int r, float jump) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)H * W; i += (size_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
    float mn = INFINITY, mx = -INFINITY;
    for (int dy = -r; dy <= r; ++dy) {
      const int yy = reflect_edge(y + dy, H);
      for (int dx = -r; dx <= r; ++dx) {
        const float v = d[(size_t)yy * W + reflect_edge(x + dx, W)];
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
      }
    }
    if (mx - mn > jump) drop[i] = 1;
  }
}

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" size_t wf_points_render_workspace_bytes(int H, int W) {
  if (H <= 0 || W <= 0) return 0;
  const size_t hw = (size_t)H * W;
  return al256(hw * 8) + 2 * al256(hw);  // z-buffer, two byte masks
}

extern "C" int wf_points_render(const float* points, const float* features, const void* drop_u8, int n, int F, const float* camera,
                                int H, int W, float radius, int morph, float* out_image, void* out_mask_u8, void* workspace,
                                void* stream) {
  const unsigned char* drop = (const unsigned char*)drop_u8;
  unsigned char* out_mask = (unsigned char*)out_mask_u8;
  WF_CHECK_ARG(points && features && camera && out_image && out_mask && workspace, "wf_points_render: null pointer");
  WF_CHECK_ARG(n > 0 && F > 0 && H > 0 && W > 0 && radius > 0.0f, "wf_points_render: empty problem");
  hipStream_t s = (hipStream_t)stream;
  const size_t hw = (size_t)H * W;
  unsigned char* base = (unsigned char*)workspace;
  unsigned long long* zbuf = (unsigned long long*)base;
  unsigned char* m0 = base + al256(hw * 8);
  unsigned char* m1 = m0 + al256(hw);
  PRCam c;
  for (int i = 0; i < 9; ++i) c.R[i] = camera[i];
  for (int i = 0; i < 3; ++i) c.T[i] = camera[9 + i];
  c.focal[0] = camera[12]; c.focal[1] = camera[13]; c.p0[0] = camera[14]; c.p0[1] = camera[15];
  if (hipMemsetAsync(zbuf, 0xff, hw * 8, s) != hipSuccess) return check_hip(hipGetLastError(), "wf_points_render");
  hipLaunchKernelGGL(k_pr_splat, dim3(grid_for((size_t)n, 256, 16384)), dim3(256), 0, s, points, drop, n, c, H, W, radius, zbuf);
  const int g = grid_for(hw, 256, 16384);
  hipLaunchKernelGGL(k_pr_mask, dim3(g), dim3(256), 0, s, (const unsigned long long*)zbuf, morph ? m0 : out_mask, hw);
  if (morph) {  // cv2.morphologyEx(mask, MORPH_OPEN, ones(5, 5))
    hipLaunchKernelGGL(k_morph<true>, dim3(g), dim3(256), 0, s, (const unsigned char*)m0, m1, H, W, 5);
    hipLaunchKernelGGL(k_morph<false>, dim3(g), dim3(256), 0, s, (const unsigned char*)m1, out_mask, H, W, 5);
  }
  hipLaunchKernelGGL(k_pr_resolve, dim3(g), dim3(256), 0, s, (const unsigned long long*)zbuf, (const unsigned char*)out_mask, features, F,
                     out_image, hw);
  WF_LAUNCH_CHECK("wf_points_render");
  return WF_OK;
}

extern "C" size_t wf_depth_edge_mask_workspace_bytes(int H, int W) {
  if (H <= 0 || W <= 0) return 0;
  const size_t hw = (size_t)H * W;
  return 256 + al256(hw * 8) + al256(hw);  // maximum, magnitudes, thresholded edges
}

extern "C" int wf_depth_edge_mask(const float* depth, int H, int W, double edge_threshold, int edge_dilation, float jump_threshold,
                                  int neighbor_radius, void* out_drop_u8, void* workspace, void* stream) {
  unsigned char* out_drop = (unsigned char*)out_drop_u8;
  WF_CHECK_ARG(depth && out_drop && workspace, "wf_depth_edge_mask: null pointer");
  WF_CHECK_ARG(H >= 2 && W >= 2, "wf_depth_edge_mask: the image must be at least 2 x 2");
  WF_CHECK_ARG(edge_dilation >= 0 && edge_dilation <= 15 && neighbor_radius >= 0 && neighbor_radius <= 15, "wf_depth_edge_mask: radii in 0..15");
  hipStream_t s = (hipStream_t)stream;
  const size_t hw = (size_t)H * W;
  unsigned char* base = (unsigned char*)workspace;
  unsigned long long* gmax = (unsigned long long*)base;
  double* mag = (double*)(base + 256);
  unsigned char* e = base + 256 + al256(hw * 8);
  if (hipMemsetAsync(gmax, 0, 8, s) != hipSuccess) return check_hip(hipGetLastError(), "wf_depth_edge_mask");
  const int g = grid_for(hw, 256, 16384);
  hipLaunchKernelGGL(k_sobel_mag, dim3(g), dim3(256), 0, s, depth, mag, gmax, H, W);
  hipLaunchKernelGGL(k_edge_thresh, dim3(g), dim3(256), 0, s, (const double*)mag, (const unsigned long long*)gmax, edge_threshold,
                     edge_dilation > 0 ? e : out_drop, hw);
  if (edge_dilation > 0)
    hipLaunchKernelGGL(k_morph<false>, dim3(g), dim3(256), 0, s, (const unsigned char*)e, out_drop, H, W, 2 * edge_dilation + 1);
  if (jump_threshold > 0.0f && neighbor_radius > 0)
    hipLaunchKernelGGL(k_depth_jump, dim3(g), dim3(256), 0, s, depth, out_drop, H, W, neighbor_radius, jump_threshold);
  WF_LAUNCH_CHECK("wf_depth_edge_mask");
  return WF_OK;
}

// ---- wf_dc_warp_frames: the frame loop of warp_depthcrafter.py:257-290 for T frames in one call ------------------------------------------
// Nothing per-point reaches HBM: the depth 1 / (disparity + 0.1) and the un-projected point are recomputed where they are read.  Every
// square-window minimum / maximum runs as a row pass and a column pass (exactly separable, border rules included).  All grids are capped
// at DC_MAX_BLOCKS and stride over T * H * W.
namespace {

constexpr int DC_MAX_BLOCKS = 2048;

__device__ __forceinline__ float dc_depth(const float* __restrict__ disp, size_t i) { return 1.0f / (disp[i] + 0.1f); }

// k_sobel_mag's magnitude on the depth of one frame (f = the frame's disparity)
__device__ __forceinline__ double dc_sobel(const float* __restrict__ f, int y, int x, int H, int W) {
  const int ym = reflect101(y - 1, H), yp = reflect101(y + 1, H), xm = reflect101(x - 1, W), xp = reflect101(x + 1, W);
  auto at = [&](int yy, int xx) { return (double)dc_depth(f, (size_t)yy * W + xx); };
  const double gx = ((((-at(ym, xm) + at(ym, xp)) - 2.0 * at(y, xm)) + 2.0 * at(y, xp)) - at(yp, xm)) + at(yp, xp);
  const double gy = ((((-at(ym, xm) - 2.0 * at(ym, x)) - at(ym, xp)) + at(yp, xm)) + 2.0 * at(yp, x)) + at(yp, xp);
  return sqrt(gx * gx + gy * gy);
}

// per-frame Sobel maximum of the frames [t0, T): blockIdx.y = frame, the blocks of a row of the grid stride over that frame's pixels, and
// one integer atomicMax per block carries the block's maximum (a non-negative double orders as its bits)
__global__ void k_dc_sobel_max(const float* __restrict__ disp, unsigned long long* __restrict__ gmax, int t0, int H, int W) {
  __shared__ double part[4];
  const int t = t0 + (int)blockIdx.y;
  const size_t hw = (size_t)H * W;
  const float* f = disp + (size_t)t * hw;
  double lm = 0.0;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += (size_t)gridDim.x * blockDim.x) {
    const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
    const double m = dc_sobel(f, y, x, H, W);
    if (m == m && m > lm) lm = m;  // NaN magnitudes are skipped, as in k_sobel_mag
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lm = fmax(lm, __shfl_xor(lm, o, 64));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = lm;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) lm = fmax(lm, part[w]);
    if (lm > 0.0) atomicMax(&gmax[t], (unsigned long long)__double_as_longlong(lm));
  }
}
// thresholded edge byte + the row pass of the depth-jump minimum / maximum (scipy "reflect"), frames [t0, T)
__global__ void k_dc_edge_row(const float* __restrict__ disp, const unsigned long long* __restrict__ gmax, double thr, int r, int t0, int T,
                              int H, int W, unsigned char* __restrict__ e, float* __restrict__ rmn, float* __restrict__ rmx) {
  const size_t hw = (size_t)H * W, n = (size_t)(T - t0) * hw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int t = t0 + (int)(i / hw);
    const size_t p = i - (size_t)(t - t0) * hw, g = (size_t)t * hw + p;
    const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
    const float* f = disp + (size_t)t * hw;
    const double mx = __longlong_as_double((long long)gmax[t]);
    const double mag = dc_sobel(f, y, x, H, W);
    e[g] = (mx > 0.0 ? mag / mx : mag) > thr;
    if (r > 0) {
      float mn = INFINITY, mxv = -INFINITY;
      for (int dx = -r; dx <= r; ++dx) {
        const float v = dc_depth(f, (size_t)y * W + reflect_edge(x + dx, W));
        mn = fminf(mn, v);
        mxv = fmaxf(mxv, v);
      }
      rmn[g] = mn;
      rmx[g] = mxv;
    }
  }
}
// drop = column maximum of the row-dilated edges | (column max of the row maxima - column min of the row minima > jump)
__global__ void k_dc_drop(const unsigned char* __restrict__ re, const float* __restrict__ rmn, const float* __restrict__ rmx, int d, int r,
                          float jump, int t0, int T, int H, int W, unsigned char* __restrict__ drop) {
  const size_t hw = (size_t)H * W, n = (size_t)(T - t0) * hw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int t = t0 + (int)(i / hw);
    const size_t p = i - (size_t)(t - t0) * hw, base = (size_t)t * hw;
    const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
    unsigned char v = 0;
    for (int dy = -d; dy <= d; ++dy) {
      const int yy = y + dy;
      if (yy >= 0 && yy < H) v |= re[base + (size_t)yy * W + x];
    }
    if (r > 0) {
      float mn = INFINITY, mx = -INFINITY;
      for (int dy = -r; dy <= r; ++dy) {
        const size_t q = base + (size_t)reflect_edge(y + dy, H) * W + x;
        mn = fminf(mn, rmn[q]);
        mx = fmaxf(mx, rmx[q]);
      }
      if (mx - mn > jump) v = 1;
    }
    drop[base + p] = v;
  }
}

__device__ __forceinline__ unsigned char dc_on(unsigned char v) { return v != 0; }
__device__ __forceinline__ unsigned char dc_on(unsigned long long z) { return z != ~0ull; }  // a z-buffer entry that a point reached
// one row (ROW) or column pass of a (2 r + 1) erosion (MIN) / dilation (MAX) of nf frames' masks, pixels outside the image ignored
template <bool ERODE, bool ROW, typename In>
__global__ void k_dc_morph1(const In* __restrict__ in, unsigned char* __restrict__ out, int nf, int H, int W, int r) {
  const size_t hw = (size_t)H * W, n = (size_t)nf * hw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t t = i / hw, p = i - t * hw;
    const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
    unsigned char v = ERODE ? 1 : 0;
    for (int k = -r; k <= r; ++k) {
      const int yy = ROW ? y : y + k, xx = ROW ? x + k : x;
      if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
      const unsigned char s = dc_on(in[t * hw + (size_t)yy * W + xx]);
      v = ERODE ? (v & s) : (v | s);
    }
    out[i] = v;
  }
}

// k_pr_splat over every pixel of every frame: the point is un-projected in place, key and tie rule as there (view depth bits << 32 | raster
// index of the source pixel in its frame)
__global__ void k_dc_splat(const float* __restrict__ disp, const unsigned char* __restrict__ drop, const float* __restrict__ cams, float fx,
                           float fy, float cx, float cy, int from, int T, int H, int W, float radius, unsigned long long* __restrict__ zbuf) {
  const size_t hw = (size_t)H * W, n = (size_t)T * hw;
  const float r2 = radius * radius;
  const float rx = W <= H ? 2.0f : ((float)W * 2.0f) / (float)H, ry = H <= W ? 2.0f : ((float)H * 2.0f) / (float)W;
  const int reach = (int)ceilf(radius * fmaxf((float)W / rx, (float)H / ry)) + 1;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int t = (int)(i / hw);
    const size_t p = i - (size_t)t * hw;
    if (drop && t >= from && drop[i]) continue;
    const int sy = (int)(p / W), sx = (int)(p - (size_t)sy * W);
    const float pz = dc_depth(disp, i);
    const float px = (((float)sx - cx) * pz) / fx, py = (((float)sy - cy) * pz) / fy;
    const float* c = cams + (size_t)t * 16;
    float v[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) v[j] = ((px * c[j] + py * c[3 + j]) + pz * c[6 + j]) + c[9 + j];
    const float z = v[2];
    if (!(z >= 0.0f)) continue;
    const float x = (c[12] * v[0] + c[14] * z) / z, y = (c[13] * v[1] + c[15] * z) / z;
    if (!isfinite(x) || !isfinite(y)) continue;
    // the casts saturate, and the clamps keep bx + dx / by + dy inside int for points far outside the image
    int bx = (int)floorf((x + rx * 0.5f) * (float)W / rx - 0.5f), by = (int)floorf((y + ry * 0.5f) * (float)H / ry - 0.5f);
    bx = bx < -65536 ? -65536 : (bx > W + 65536 ? W + 65536 : bx);
    by = by < -65536 ? -65536 : (by > H + 65536 ? H + 65536 : by);
    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)p;
    unsigned long long* zb = zbuf + (size_t)t * hw;
    for (int dy = -reach; dy <= reach + 1; ++dy) {
      const int iy = by + dy;
      if (iy < 0 || iy >= H) continue;
      const float ddy = pix_to_ndc(iy, H, W) - y;
      if (!(ddy * ddy < r2)) continue;  // ddx^2 + ddy^2 >= ddy^2 in fp32 as well: no pixel of this row passes
      for (int dx = -reach; dx <= reach + 1; ++dx) {
        const int ix = bx + dx;
        if (ix < 0 || ix >= W) continue;
        const float ddx = pix_to_ndc(ix, W, H) - x;
        if (ddx * ddx + ddy * ddy < r2) atomicMin(&zb[(size_t)(H - 1 - iy) * W + (W - 1 - ix)], key);
      }
    }
  }
}

// final mask (column pass of the opening's dilation, or the raw coverage), the owner's colour, and cv2.imwrite's 8-bit conversion of a
// float32 image: saturate(round-half-even(x * 255.0f))
template <bool MORPH>
__global__ void k_dc_resolve(const unsigned long long* __restrict__ zbuf, const unsigned char* __restrict__ rowdil, const float* __restrict__ frames,
                             int T, int H, int W, unsigned char* __restrict__ out_img, unsigned char* __restrict__ out_mask,
                             float* __restrict__ out_f32) {
  const size_t hw = (size_t)H * W, n = (size_t)T * hw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t t = i / hw, p = i - t * hw;
    const unsigned long long zb = zbuf[i];
    bool on;
    if (MORPH) {
      const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
      unsigned char v = 0;
      for (int dy = -2; dy <= 2; ++dy) {
        const int yy = y + dy;
        if (yy >= 0 && yy < H) v |= rowdil[t * hw + (size_t)yy * W + x];
      }
      on = v != 0 && zb != ~0ull;  // (the opening never adds a pixel: the second term only keeps the owner read in bounds)
    } else {
      on = zb != ~0ull;
    }
    out_mask[i] = on;
    const size_t src = (t * hw + (size_t)(unsigned)(zb & 0xffffffffull)) * 3;
    for (int k = 0; k < 3; ++k) {
      const float c = on ? frames[src + k] : 0.0f;
      if (out_f32) out_f32[i * 3 + k] = c;
      const float q = rintf(c * 255.0f);
      out_img[i * 3 + k] = (unsigned char)(!(q > 0.0f) ? 0.0f : (q > 255.0f ? 255.0f : q));
    }
  }
}

}  // namespace

extern "C" size_t wf_dc_warp_frames_workspace_bytes(int T, int H, int W) {
  if (T <= 0 || H <= 0 || W <= 0) return 0;
  const size_t n = (size_t)T * H * W;
  return al256((size_t)T * 8) + al256(n * 8) + 3 * al256(n);  // Sobel maxima, z-buffers (first the jump row minima / maxima), three byte planes
}

extern "C" int wf_dc_warp_frames(const float* frames, const float* disparity, const float* cameras, float fx, float fy, float cx, float cy,
                                 double edge_threshold, int edge_dilation, float jump_threshold, int neighbor_radius, int edge_filter_from,
                                 float radius, int morph, int T, int H, int W, void* out_images_u8, void* out_masks_u8, float* out_images_f32,
                                 void* workspace, void* stream) {
  WF_CHECK_ARG(T > 0 && H > 0 && W > 0, "wf_dc_warp_frames: T, H and W must be positive");
  WF_CHECK_ARG(T <= 65535, "wf_dc_warp_frames: at most 65535 frames a call");
  WF_CHECK_ARG(frames && disparity && cameras && out_images_u8 && out_masks_u8 && workspace, "wf_dc_warp_frames: null pointer");
  WF_CHECK_ARG(H >= 2 && W >= 2, "wf_dc_warp_frames: the frames must be at least 2 x 2 (reflect-101)");
  WF_CHECK_ARG((size_t)H * W <= 0x7fffffffull, "wf_dc_warp_frames: H * W must fit the 32-bit owner index");
  WF_CHECK_ARG(radius > 0.0f && radius <= 0.05f, "wf_dc_warp_frames: radius in (0, 0.05]");
  WF_CHECK_ARG(edge_dilation >= 0 && edge_dilation <= 15 && neighbor_radius >= 0 && neighbor_radius <= 15,
               "wf_dc_warp_frames: edge_dilation and neighbor_radius in 0..15");
  WF_CHECK_ARG(edge_filter_from >= 0, "wf_dc_warp_frames: edge_filter_from must not be negative");
  hipStream_t s = (hipStream_t)stream;
  const size_t hw = (size_t)H * W, n = (size_t)T * hw;
  unsigned char* base = (unsigned char*)workspace;
  unsigned long long* gmax = (unsigned long long*)base;
  unsigned long long* zbuf = (unsigned long long*)(base + al256((size_t)T * 8));
  unsigned char* b0 = (unsigned char*)zbuf + al256(n * 8);
  unsigned char* b1 = b0 + al256(n);
  unsigned char* b2 = b1 + al256(n);
  unsigned char* out_img = (unsigned char*)out_images_u8;
  unsigned char* out_mask = (unsigned char*)out_masks_u8;
  const int g = grid_for(n, 256, DC_MAX_BLOCKS);
  const unsigned char* drop = nullptr;
  if (edge_filter_from < T) {
    const int t0 = edge_filter_from, gf = grid_for((size_t)(T - t0) * hw, 256, DC_MAX_BLOCKS);
    const int r = jump_threshold > 0.0f ? neighbor_radius : 0;
    float* rmn = (float*)zbuf;  // dead before the z-buffer is initialised
    float* rmx = rmn + n;
    if (hipMemsetAsync(gmax, 0, (size_t)T * 8, s) != hipSuccess) return check_hip(hipGetLastError(), "wf_dc_warp_frames");
    const int per_frame = grid_for(hw, 256, DC_MAX_BLOCKS / (T - t0) > 0 ? DC_MAX_BLOCKS / (T - t0) : 1);
    hipLaunchKernelGGL(k_dc_sobel_max, dim3(per_frame, T - t0), dim3(256), 0, s, disparity, gmax, t0, H, W);
    hipLaunchKernelGGL(k_dc_edge_row, dim3(gf), dim3(256), 0, s, disparity, (const unsigned long long*)gmax, edge_threshold, r, t0, T, H, W, b0,
                       rmn, rmx);
    hipLaunchKernelGGL((k_dc_morph1<false, true, unsigned char>), dim3(gf), dim3(256), 0, s, (const unsigned char*)(b0 + (size_t)t0 * hw),
                       b1 + (size_t)t0 * hw, T - t0, H, W, edge_dilation);
    hipLaunchKernelGGL(k_dc_drop, dim3(gf), dim3(256), 0, s, (const unsigned char*)b1, (const float*)rmn, (const float*)rmx, edge_dilation, r,
                       jump_threshold, t0, T, H, W, b2);
    drop = b2;
  }
  if (hipMemsetAsync(zbuf, 0xff, n * 8, s) != hipSuccess) return check_hip(hipGetLastError(), "wf_dc_warp_frames");
  hipLaunchKernelGGL(k_dc_splat, dim3(g), dim3(256), 0, s, disparity, drop, cameras, fx, fy, cx, cy, edge_filter_from, T, H, W, radius, zbuf);
  if (morph) {  // cv2.morphologyEx(mask, MORPH_OPEN, ones(5, 5)): erosion rows, columns; dilation rows, columns (in k_dc_resolve)
    hipLaunchKernelGGL((k_dc_morph1<true, true, unsigned long long>), dim3(g), dim3(256), 0, s, (const unsigned long long*)zbuf, b0, T, H, W, 2);
    hipLaunchKernelGGL((k_dc_morph1<true, false, unsigned char>), dim3(g), dim3(256), 0, s, (const unsigned char*)b0, b1, T, H, W, 2);
    hipLaunchKernelGGL((k_dc_morph1<false, true, unsigned char>), dim3(g), dim3(256), 0, s, (const unsigned char*)b1, b0, T, H, W, 2);
    hipLaunchKernelGGL(k_dc_resolve<true>, dim3(g), dim3(256), 0, s, (const unsigned long long*)zbuf, (const unsigned char*)b0, frames, T, H, W,
                       out_img, out_mask, out_images_f32);
  } else {
    hipLaunchKernelGGL(k_dc_resolve<false>, dim3(g), dim3(256), 0, s, (const unsigned long long*)zbuf, (const unsigned char*)nullptr, frames, T, H,
                       W, out_img, out_mask, out_images_f32);
  }
  WF_LAUNCH_CHECK("wf_dc_warp_frames");
  return WF_OK;
}
