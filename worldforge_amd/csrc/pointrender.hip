// Point-cloud renderer + depth-edge point filter of the DepthCrafter stage-1 warper (dynamic scenes: one point cloud per video frame).
//
// Replaces DepthCrafter/utils.py project_points_to_image_pytorch (:103-171: pytorch3d PointsRasterizer with radius 0.005, nearest point per
// pixel, 5 x 5 opening of the coverage mask) and filter_edge_points / detect_depth_edges (:495-567: Sobel magnitude, 7 x 7 dilation, 5 x 5
// min / max depth-jump test) as warp_depthcrafter.py:255-288 runs them for every frame.  HBM / atomic bound: a 64-bit atomicMin z-buffer
// (view depth bits << 32 | owner index: nearest wins, ties to the smaller index), a handful of 5 x 5 / 7 x 7 stencils on byte masks.
// pytorch3d and OpenCV are third-party packages absent from the reference tree: their behaviour is restated (oracle/pointrender.py lists the
// statements) and parity with them is UNPINNED.  Compiled with -ffp-contract=off: the projection is the oracle's float32 op sequence.
//
// One kernel set serves the three entry points.  wf_dc_warp_frames is the frame loop of warp_depthcrafter.py:257-290 for T frames in one
// call; wf_depth_edge_mask and wf_points_render are its two halves at T = 1 with another source of depth (a stored plane instead of
// 1 / (disparity + 0.1) recomputed where it is read), of points (a stored array instead of the pixel un-projected in place) and another
// colour sink (F features into an f32 image instead of 3 into the 8-bit frame).  Source and sink are template arguments: no kernel
// branches on a mode.  Every square-window minimum / maximum runs as a row pass and a column pass (exactly separable, border rules
// included).  All grids are capped at MAX_BLOCKS and stride.
#include <stdint.h>

#include "common.h"

using namespace wf;

namespace {

constexpr int MAX_BLOCKS = 2048;

// rasterization_utils.cuh PixToNonSquareNdc
__device__ __forceinline__ float pix_to_ndc(int i, int S1, int S2) {
  const float r = S1 <= S2 ? 2.0f : ((float)S1 * 2.0f) / (float)S2;
  const float o = r / 2.0f;
  return -o + (r * (float)i + o) / (float)S1;
}
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

// ---- depth sources: the depth at raster index i of [T][H][W] --------------------------------------------------------------------------------
struct StoredDepth {
  const float* d;
  __device__ __forceinline__ float operator()(size_t i) const { return d[i]; }
};
struct DisparityDepth {  // warp_depthcrafter.py:259, never stored
  const float* disp;
  __device__ __forceinline__ float operator()(size_t i) const { return 1.0f / (disp[i] + 0.1f); }
};

// ---- filter_edge_points ---------------------------------------------------------------------------------------------------------------------
// Sobel (ksize 3, CV_64F) gradient magnitude at (y, x) of the frame that starts at raster index `base`
template <typename Depth>
__device__ __forceinline__ double sobel_mag(const Depth& depth, size_t base, int y, int x, int H, int W) {
  const int ym = reflect101(y - 1, H), yp = reflect101(y + 1, H), xm = reflect101(x - 1, W), xp = reflect101(x + 1, W);
  auto at = [&](int yy, int xx) { return (double)depth(base + (size_t)yy * W + xx); };
  // correlation in row-major tap order (dy, dx), zero taps skipped
  const double gx = ((((-at(ym, xm) + at(ym, xp)) - 2.0 * at(y, xm)) + 2.0 * at(y, xp)) - at(yp, xm)) + at(yp, xp);
  const double gy = ((((-at(ym, xm) - 2.0 * at(ym, x)) - at(ym, xp)) + at(yp, xm)) + 2.0 * at(yp, x)) + at(yp, xp);
  return sqrt(gx * gx + gy * gy);
}

// per-frame Sobel maximum of the frames [t0, T): blockIdx.y = frame, the blocks of a row of the grid stride over that frame's pixels, and
// one integer atomicMax per block carries the block's maximum (a non-negative double orders as its bits)
template <typename Depth>
__global__ void k_sobel_max(Depth depth, unsigned long long* __restrict__ gmax, int t0, int H, int W) {
  __shared__ double part[4];
  const int t = t0 + (int)blockIdx.y;
  const size_t hw = (size_t)H * W;
  double lm = 0.0;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += (size_t)gridDim.x * blockDim.x) {
    const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
    const double m = sobel_mag(depth, (size_t)t * hw, y, x, H, W);
    if (m == m && m > lm) lm = m;  // NaN magnitudes are skipped
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
template <typename Depth>
__global__ void k_edge_row(Depth depth, const unsigned long long* __restrict__ gmax, double thr, int r, int t0, int T, int H, int W,
                           unsigned char* __restrict__ e, float* __restrict__ rmn, float* __restrict__ rmx) {
  const size_t hw = (size_t)H * W, n = (size_t)(T - t0) * hw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int t = t0 + (int)(i / hw);
    const size_t base = (size_t)t * hw, p = i - (size_t)(t - t0) * hw, g = base + p;
    const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
    const double mx = __longlong_as_double((long long)gmax[t]);
    const double mag = sobel_mag(depth, base, y, x, H, W);
    e[g] = (mx > 0.0 ? mag / mx : mag) > thr;
    if (r > 0) {
      float mn = INFINITY, mxv = -INFINITY;
      for (int dx = -r; dx <= r; ++dx) {
        const float v = depth(base + (size_t)y * W + reflect_edge(x + dx, W));
        mn = fminf(mn, v);
        mxv = fmaxf(mxv, v);
      }
      rmn[g] = mn;
      rmx[g] = mxv;
    }
  }
}
// drop = column maximum of the row-dilated edges | (column max of the row maxima - column min of the row minima > jump)
__global__ void k_drop(const unsigned char* __restrict__ re, const float* __restrict__ rmn, const float* __restrict__ rmx, int d, int r,
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

__device__ __forceinline__ unsigned char mask_on(unsigned char v) { return v != 0; }
__device__ __forceinline__ unsigned char mask_on(unsigned long long z) { return z != ~0ull; }  // a z-buffer entry that a point reached
// one row (ROW) or column pass of a (2 r + 1) erosion (MIN) / dilation (MAX) of nf frames' masks, anchor at the centre, pixels outside the
// image ignored (OpenCV's default border value for morphology: +inf for erode, -inf for dilate)
template <bool ERODE, bool ROW, typename In>
__global__ void k_morph1(const In* __restrict__ in, unsigned char* __restrict__ out, int nf, int H, int W, int r) {
  const size_t hw = (size_t)H * W, n = (size_t)nf * hw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t t = i / hw, p = i - t * hw;
    const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
    unsigned char v = ERODE ? 1 : 0;
    for (int k = -r; k <= r; ++k) {
      const int yy = ROW ? y : y + k, xx = ROW ? x + k : x;
      if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
      const unsigned char s = mask_on(in[t * hw + (size_t)yy * W + xx]);
      v = ERODE ? (v & s) : (v | s);
    }
    out[i] = v;
  }
}

// ---- point sources: point i of n -> false = none, else its frame, its owner index (the low half of the z-buffer key) and its position; ------
// cam(t, k) = float k of frame t's camera {R' (9, row vectors: view = p R' + T'), T' (3), focal' (2), principal' (2)}
struct Camera {
  float v[16];
};
struct ArrayPoints {  // a stored [n][3] array with an optional drop[n], one frame, its camera by value; owner = the point index
  const float* pts;
  const unsigned char* drop;
  size_t n;
  Camera c;
  __device__ __forceinline__ bool point(size_t i, size_t, int, int& t, unsigned& owner, float& px, float& py, float& pz) const {
    if (drop && drop[i]) return false;
    t = 0;
    owner = (unsigned)i;
    px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
    return true;
  }
  __device__ __forceinline__ float cam(int, int k) const { return c.v[k]; }
};
struct PixelPoints {  // every pixel of T frames un-projected in place (:262-266); owner = its raster index in the frame
  DisparityDepth depth;
  const unsigned char* drop;  // [T][H][W] or null, read for the frames t >= from
  const float* cams;          // [T][16]
  float fx, fy, cx, cy;
  int from;
  size_t n;
  __device__ __forceinline__ bool point(size_t i, size_t hw, int W, int& t, unsigned& owner, float& px, float& py, float& pz) const {
    t = (int)(i / hw);
    const size_t p = i - (size_t)t * hw;
    if (drop && t >= from && drop[i]) return false;
    const int sy = (int)(p / W), sx = (int)(p - (size_t)sy * W);
    owner = (unsigned)p;
    pz = depth(i);
    px = (((float)sx - cx) * pz) / fx, py = (((float)sy - cy) * pz) / fy;
    return true;
  }
  __device__ __forceinline__ float cam(int t, int k) const { return cams[(size_t)t * 16 + k]; }
};

template <typename Points>
__global__ void k_splat(Points src, int H, int W, float radius, unsigned long long* __restrict__ zbuf) {
  const size_t hw = (size_t)H * W;
  const float r2 = radius * radius;
  const float rx = W <= H ? 2.0f : ((float)W * 2.0f) / (float)H, ry = H <= W ? 2.0f : ((float)H * 2.0f) / (float)W;
  const int reach = (int)ceilf(radius * fmaxf((float)W / rx, (float)H / ry)) + 1;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < src.n; i += (size_t)gridDim.x * blockDim.x) {
    int t;
    unsigned owner;
    float px, py, pz;
    if (!src.point(i, hw, W, t, owner, px, py, pz)) continue;
    float v[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) v[j] = ((px * src.cam(t, j) + py * src.cam(t, 3 + j)) + pz * src.cam(t, 6 + j)) + src.cam(t, 9 + j);
    const float z = v[2];
    if (!(z >= 0.0f)) continue;  // behind the camera (rasterize_points: pz < 0), NaN
    const float x = (src.cam(t, 12) * v[0] + src.cam(t, 14) * z) / z, y = (src.cam(t, 13) * v[1] + src.cam(t, 15) * z) / z;
    if (!isfinite(x) || !isfinite(y)) continue;
    // flipped pixel indices i' = S - 1 - i of the centres around the point; the casts saturate, and the clamps keep bx + dx / by + dy
    // inside int for points far outside the image
    int bx = (int)floorf((x + rx * 0.5f) * (float)W / rx - 0.5f), by = (int)floorf((y + ry * 0.5f) * (float)H / ry - 0.5f);
    bx = bx < -65536 ? -65536 : (bx > W + 65536 ? W + 65536 : bx);
    by = by < -65536 ? -65536 : (by > H + 65536 ? H + 65536 : by);
    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | owner;
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

// ---- colour sinks: pixel i takes the colour of source element src where the final mask is set (on), else 0 (utils.py:149-169) --------------
struct FeatureSink {  // F floats into an f32 image
  const float* feat;
  int F;
  float* img;
  __device__ __forceinline__ void operator()(size_t i, size_t src, bool on) const {
    for (int k = 0; k < F; ++k) img[i * F + k] = on ? feat[src * F + k] : 0.0f;
  }
};
struct FrameSink {  // 3 floats into the optional f32 image and, as cv2.imwrite converts it (saturate(round-half-even(x * 255.0f))), the 8-bit frame
  const float* frames;
  unsigned char* out_img;
  float* out_f32;
  __device__ __forceinline__ void operator()(size_t i, size_t src, bool on) const {
    for (int k = 0; k < 3; ++k) {
      const float c = on ? frames[src * 3 + k] : 0.0f;
      if (out_f32) out_f32[i * 3 + k] = c;
      const float q = rintf(c * 255.0f);
      out_img[i * 3 + k] = (unsigned char)(!(q > 0.0f) ? 0.0f : (q > 255.0f ? 255.0f : q));
    }
  }
};

// final mask (column pass of the opening's dilation, or the raw coverage) and the owner's colour
template <bool MORPH, typename Sink>
__global__ void k_resolve(const unsigned long long* __restrict__ zbuf, const unsigned char* __restrict__ rowdil, Sink sink, int T, int H, int W,
                          unsigned char* __restrict__ out_mask) {
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
    sink(i, t * hw + (size_t)(unsigned)(zb & 0xffffffffull), on);
  }
}

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// drop[t0 .. T) = the edge filter of those frames.  gmax [T]; rmn, rmx f32 [T * hw]; e, re byte planes [T * hw].  false = a HIP error.
template <typename Depth>
bool edge_filter(Depth depth, double thr, int d, float jump, int nr, int t0, int T, int H, int W, unsigned long long* gmax, float* rmn, float* rmx,
                 unsigned char* e, unsigned char* re, unsigned char* drop, hipStream_t s) {
  const size_t hw = (size_t)H * W;
  const int gf = grid_for((size_t)(T - t0) * hw, 256, MAX_BLOCKS);
  const int r = jump > 0.0f ? nr : 0;
  if (hipMemsetAsync(gmax, 0, (size_t)T * 8, s) != hipSuccess) return false;
  const int per_frame = grid_for(hw, 256, MAX_BLOCKS / (T - t0) > 0 ? MAX_BLOCKS / (T - t0) : 1);
  hipLaunchKernelGGL(k_sobel_max<Depth>, dim3(per_frame, T - t0), dim3(256), 0, s, depth, gmax, t0, H, W);
  hipLaunchKernelGGL(k_edge_row<Depth>, dim3(gf), dim3(256), 0, s, depth, (const unsigned long long*)gmax, thr, r, t0, T, H, W, e, rmn, rmx);
  hipLaunchKernelGGL((k_morph1<false, true, unsigned char>), dim3(gf), dim3(256), 0, s, (const unsigned char*)(e + (size_t)t0 * hw),
                     re + (size_t)t0 * hw, T - t0, H, W, d);
  hipLaunchKernelGGL(k_drop, dim3(gf), dim3(256), 0, s, (const unsigned char*)re, (const float*)rmn, (const float*)rmx, d, r, jump, t0, T, H, W,
                     drop);
  return true;
}

// z-buffer splat of pts, the 5 x 5 opening (morph), masks and colours of T frames.  zbuf [T * hw]; b0, b1 byte planes [T * hw].
template <typename Points, typename Sink>
bool render(Points pts, Sink sink, int morph, int T, int H, int W, float radius, unsigned long long* zbuf, unsigned char* b0, unsigned char* b1,
            unsigned char* out_mask, hipStream_t s) {
  const size_t n = (size_t)T * H * W;
  const int g = grid_for(n, 256, MAX_BLOCKS);
  const unsigned long long* z = zbuf;
  if (hipMemsetAsync(zbuf, 0xff, n * 8, s) != hipSuccess) return false;
  hipLaunchKernelGGL(k_splat<Points>, dim3(grid_for(pts.n, 256, MAX_BLOCKS)), dim3(256), 0, s, pts, H, W, radius, zbuf);
  if (morph) {  // cv2.morphologyEx(mask, MORPH_OPEN, ones(5, 5)): erosion rows, columns; dilation rows, columns (in k_resolve)
    hipLaunchKernelGGL((k_morph1<true, true, unsigned long long>), dim3(g), dim3(256), 0, s, z, b0, T, H, W, 2);
    hipLaunchKernelGGL((k_morph1<true, false, unsigned char>), dim3(g), dim3(256), 0, s, (const unsigned char*)b0, b1, T, H, W, 2);
    hipLaunchKernelGGL((k_morph1<false, true, unsigned char>), dim3(g), dim3(256), 0, s, (const unsigned char*)b1, b0, T, H, W, 2);
    hipLaunchKernelGGL((k_resolve<true, Sink>), dim3(g), dim3(256), 0, s, z, (const unsigned char*)b0, sink, T, H, W, out_mask);
  } else {
    hipLaunchKernelGGL((k_resolve<false, Sink>), dim3(g), dim3(256), 0, s, z, (const unsigned char*)nullptr, sink, T, H, W, out_mask);
  }
  return true;
}

}  // namespace

extern "C" size_t wf_points_render_workspace_bytes(int H, int W) {
  if (H <= 0 || W <= 0) return 0;
  const size_t hw = (size_t)H * W;
  return al256(hw * 8) + 2 * al256(hw);  // z-buffer, two byte masks
}

extern "C" int wf_points_render(const float* points, const float* features, const void* drop_u8, int n, int F, const float* camera,
                                int H, int W, float radius, int morph, float* out_image, void* out_mask_u8, void* workspace,
                                void* stream) {
  WF_CHECK_ARG(points && features && camera && out_image && out_mask_u8 && workspace, "wf_points_render: null pointer");
  WF_CHECK_ARG(n > 0 && F > 0 && H > 0 && W > 0 && radius > 0.0f, "wf_points_render: empty problem");
  const size_t hw = (size_t)H * W;
  unsigned char* base = (unsigned char*)workspace;
  unsigned char* b0 = base + al256(hw * 8);
  ArrayPoints pts{points, (const unsigned char*)drop_u8, (size_t)n, {}};
  for (int i = 0; i < 16; ++i) pts.c.v[i] = camera[i];
  if (!render(pts, FeatureSink{features, F, out_image}, morph, 1, H, W, radius, (unsigned long long*)base, b0, b0 + al256(hw),
              (unsigned char*)out_mask_u8, (hipStream_t)stream))
    return check_hip(hipGetLastError(), "wf_points_render");
  WF_LAUNCH_CHECK("wf_points_render");
  return WF_OK;
}

extern "C" size_t wf_depth_edge_mask_workspace_bytes(int H, int W) {
  if (H <= 0 || W <= 0) return 0;
  const size_t hw = (size_t)H * W;
  return 256 + al256(hw * 8) + 2 * al256(hw);  // maximum, jump row minima / maxima, two byte planes
}

extern "C" int wf_depth_edge_mask(const float* depth, int H, int W, double edge_threshold, int edge_dilation, float jump_threshold,
                                  int neighbor_radius, void* out_drop_u8, void* workspace, void* stream) {
  WF_CHECK_ARG(depth && out_drop_u8 && workspace, "wf_depth_edge_mask: null pointer");
  WF_CHECK_ARG(H >= 2 && W >= 2, "wf_depth_edge_mask: the image must be at least 2 x 2");
  WF_CHECK_ARG(edge_dilation >= 0 && edge_dilation <= 15 && neighbor_radius >= 0 && neighbor_radius <= 15, "wf_depth_edge_mask: radii in 0..15");
  const size_t hw = (size_t)H * W;
  unsigned char* base = (unsigned char*)workspace;
  float* rmn = (float*)(base + 256);
  unsigned char* b0 = base + 256 + al256(hw * 8);
  if (!edge_filter(StoredDepth{depth}, edge_threshold, edge_dilation, jump_threshold, neighbor_radius, 0, 1, H, W, (unsigned long long*)base, rmn,
                   rmn + hw, b0, b0 + al256(hw), (unsigned char*)out_drop_u8, (hipStream_t)stream))
    return check_hip(hipGetLastError(), "wf_depth_edge_mask");
  WF_LAUNCH_CHECK("wf_depth_edge_mask");
  return WF_OK;
}

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
  const size_t n = (size_t)T * H * W;
  unsigned char* base = (unsigned char*)workspace;
  unsigned long long* zbuf = (unsigned long long*)(base + al256((size_t)T * 8));
  unsigned char* b0 = (unsigned char*)zbuf + al256(n * 8);
  unsigned char* b1 = b0 + al256(n);
  unsigned char* b2 = b1 + al256(n);
  const DisparityDepth depth{disparity};
  const unsigned char* drop = nullptr;
  if (edge_filter_from < T) {
    float* rmn = (float*)zbuf;  // dead before the z-buffer is initialised
    if (!edge_filter(depth, edge_threshold, edge_dilation, jump_threshold, neighbor_radius, edge_filter_from, T, H, W, (unsigned long long*)base,
                     rmn, rmn + n, b0, b1, b2, s))
      return check_hip(hipGetLastError(), "wf_dc_warp_frames");
    drop = b2;
  }
  if (!render(PixelPoints{depth, drop, cameras, fx, fy, cx, cy, edge_filter_from, n},
              FrameSink{frames, (unsigned char*)out_images_u8, out_images_f32}, morph, T, H, W, radius, zbuf, b0, b1, (unsigned char*)out_masks_u8, s))
    return check_hip(hipGetLastError(), "wf_dc_warp_frames");
  WF_LAUNCH_CHECK("wf_dc_warp_frames");
  return WF_OK;
}
