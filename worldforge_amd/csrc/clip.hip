// CLIP vision-encoder kernels (transformers/models/clip/modeling_clip.py, CLIPVisionModel): the reference loads this model in float32, so
// every product here is an fp32 product on the fp32-input MFMA v_mfma_f32_32x32x2_f32 (bit for bit a k-ordered fmaf chain, one rounding
// per product; gfx950 has no xf32).  No operand and no partial result is narrower than fp32; there is no atomic: a sum over waves is
// added in the order wave 0, 1, 2, 3, so two runs give the same bits.  The LayerNorms of the encoder are wf_ln_modulate (dit_ops.hip).
//
// Operand maps of __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c): lane l gives A[i = l & 31][k = l >> 5] and B[k = l >> 5][n = l & 31], ONE
// float each; C/D as every 32x32 MFMA (mfma.h): column n = l & 31, row i = (r & 3) + 8 (r >> 2) + 4 (l >> 5).  The order of k inside a sum
// is free as long as A and B agree, so a lane fetches FOUR consecutive k with one 16-byte load (lane half hi takes k = 8 b + 4 hi + j of
// the 8-wide block b) and step j of the block multiplies the two halves' j-th elements.
//
// k_gemm_f32: out[M, N] = epi(X[M, K] . W[N, K]^T + bias).  A = W (output features -> accumulator rows: a lane owns 4 consecutive features
// of ONE token row per register quad, 16-byte stores), B = X.  One workgroup = 4 waves = one [32 tokens x 64 features] tile (two
// accumulators per wave, one X fragment feeds both); the FOUR WAVES SPLIT K (wave w takes the 8-wide blocks [nb w / 4, nb (w + 1) / 4), nb
// = ceil(K / 8): a function of K alone), leave their partial tiles in LDS (32 KB) and wave w adds registers 8 w .. 8 w + 7 of the four
// partials in wave order and runs the epilogue.  Operands go global -> registers (no LDS staging: the four waves of a workgroup read
// disjoint k ranges, there is nothing to share) through two register buffers of four blocks = 32 k each: the 12 loads of one buffer are
// issued before the 32 MFMAs (2048 cycles) that consume the other.  A ragged K (588 = 8 * 73 + 4) is padded with zeros in registers
// (fma(0, 0, c) = c; the load itself reads the row's last fragment, never outside the row); rows behind M or N read the last row again
// and store nothing.
// Why this tiling.  The MFMA issues every 64 cycles per SIMD, so the chip is full with ONE wave per SIMD and the question is only how
// many SIMDs have one.  The encoder's M is 257 tokens = 9 row tiles of 32 (288 rows, 89 % used; 64-row tiles would use 80 %, 128-row
// tiles 67 %).  At N = 1280 a 128 x 128 tiling has 30 workgroups for 256 CUs; 32 x 64 tiles without a K split have 9 * 20 = 180 waves
// for 1024 SIMDs.  With the 4-way K split inside the workgroup every one of the 180 workgroups fills the four SIMDs of its CU: 180 of
// 256 CUs busy (70 %) at N = 1280, 9 * 60 = 540 workgroups = 2.1 rounds at N = 3840, 9 * 80 = 720 = 2.8 rounds at N = 5120.  A split over
// workgroups would need a workspace and a second pass; this one needs neither.  Traffic: a tile step of 32 k reads 96 rows x 128 B for
// 131 kFLOP = 10.7 FLOP / byte, 14.7 TB/s chip-wide at the 157 TF peak, which the L2s serve when the workgroups that share weight rows
// run on one XCD: workgroup b works on item (b % 8) * ceil(items / 8) + b / 8 (token tile fastest), so the 9 token tiles of a weight
// block are neighbours on one XCD and each weight row comes from HBM about once.
//
// k_clip_attn: O = softmax_j(scale q_i . k_j) V, unmasked, fp32 throughout.  One workgroup = 4 waves = (head, 32 query rows); the waves
// split the KEY tiles of 32 (wave w takes tiles [nt w / 4, nt (w + 1) / 4)) and read K and V straight from global memory (a head's K and
// V in fp32 do not fit the LDS at L 257, D 80 and nothing is read twice by one wave that another could share).  Scores are computed
// TRANSPOSED, S^T = K . Q^T (A = K rows, B = the lane's query row held in registers), so a lane owns ONE query and 16 keys of the tile,
// and register r of the score tile IS the B operand of step r of O^T = V^T . P^T: lane half hi holds key (r & 3) + 8 (r >> 2) + 4 hi, the A
// operand is V[that key][channel 32 db + (l & 31)].  p never leaves its fp32 register.  Two sweeps: sweep 1 finds the exact row maximum
// (per wave, then over the four waves through LDS), sweep 2 recomputes the same scores (same instructions, same bits), p = expf(s - m),
// the row sum in fp32; the partial O and sums of waves 1..3 go through LDS (48 KB at D 128) and wave 0 adds them in wave order,
// multiplies by 1 / sum and stores.  D = 80 is 2.5 channel blocks of 32: the third block runs half empty (zeros as A operand).
#include "common.h"
#include "mfma.h"

namespace wf {
namespace {

__device__ __forceinline__ f32x16 mfma32f(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

__device__ __forceinline__ f32x4 ld4_or_zero(const float* p, bool ok) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  return ok ? *(const f32x4*)p : z;
}

constexpr int GF_TM = 32;   // tokens per tile
constexpr int GF_TN = 64;   // features per tile

struct GemmF32Args {
  const float *X, *W, *bias;
  float* out;
  int M, N, K, ldx, ldw, ldo, epi, tiles_m, total, per_xcd;
};

__device__ __forceinline__ float epi_f32(int epi, float v, float old) {
  switch (epi) {
    case WF_EPI_F32_ACC: return old + v;
    case WF_EPI_F32_GELU: return 0.5f * v * (1.f + erff(v * 0.70710678118654752f));
    case WF_EPI_F32_QUICK_GELU: return v * (1.f / (1.f + expf(-1.702f * v)));
    default: return v;
  }
}

__global__ __launch_bounds__(256) void k_gemm_f32(GemmF32Args a) {
  __shared__ float part[4][32][64];   // [wave][register of the two accumulators][lane]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, r31 = lane & 31, hi = lane >> 5;
  const int item = (int)(blockIdx.x & 7) * a.per_xcd + (int)(blockIdx.x >> 3);
  if (item >= a.total) return;                                   // uniform over the workgroup, before any barrier
  const int m0 = (item % a.tiles_m) * GF_TM, n0 = (item / a.tiles_m) * GF_TN;
  const int M = a.M, N = a.N, K = a.K;
  const int xr = min(m0 + r31, M - 1), w0r = min(n0 + r31, N - 1), w1r = min(n0 + 32 + r31, N - 1);
  const float* xp = a.X + (size_t)xr * a.ldx;
  const float* w0p = a.W + (size_t)w0r * a.ldw;
  const float* w1p = a.W + (size_t)w1r * a.ldw;
  const int nb = (K + 7) / 8;
  const int b0 = (int)((int64_t)nb * wid / 4), b1 = (int)((int64_t)nb * (wid + 1) / 4);

  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc0[r] = 0.f, acc1[r] = 0.f;
  // Two register buffers of four blocks each, filled in turn.  Every load is UNCONDITIONAL (a fragment behind the wave's range or behind
  // K reads the row's last fragment instead and is replaced by zeros when it is used), so the compiler counts the loads in flight
  // and waits for the older buffer only (s_waitcnt vmcnt(12)) while the younger one is still on its way under 32 MFMAs.
  f32x4 ax[4], aw0[4], aw1[4], bx[4], bw0[4], bw1[4];
  auto load = [&](int b, f32x4* x, f32x4* w0, f32x4* w1) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = min(8 * (b + u) + 4 * hi, K - 4);            // 0 <= k <= K - 4 (K >= 4): always inside the row
      x[u] = *(const f32x4*)(xp + k);
      w0[u] = *(const f32x4*)(w0p + k);
      w1[u] = *(const f32x4*)(w1p + k);
    }
  };
  auto compute = [&](int b, const f32x4* x, const f32x4* w0, const f32x4* w1) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (b + u >= b1) break;                                    // wave-uniform
      const bool ok = 8 * (b + u) + 4 * hi < K;                  // K % 4 == 0: a fragment is inside the row or outside it
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float xv = ok ? x[u][j] : 0.f;
        acc0 = mfma32f(ok ? w0[u][j] : 0.f, xv, acc0);
        acc1 = mfma32f(ok ? w1[u][j] : 0.f, xv, acc1);
      }
    }
  };
  load(b0, ax, aw0, aw1);
  for (int b = b0; b < b1; b += 8) {
    load(b + 4, bx, bw0, bw1);
    compute(b, ax, aw0, aw1);
    load(b + 8, ax, aw0, aw1);
    compute(b + 4, bx, bw0, bw1);
  }

#pragma unroll
  for (int r = 0; r < 16; ++r) part[wid][r][lane] = acc0[r], part[wid][16 + r][lane] = acc1[r];
  __syncthreads();
  // wave w finishes registers 8 w .. 8 w + 7: accumulator w >> 1, quads 2 (w & 1) and 2 (w & 1) + 1
  const int token = m0 + r31;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int r0 = 8 * wid + 4 * q;                              // first register of the quad among the 32
    const int feat = n0 + 32 * (r0 >> 4) + 8 * ((r0 & 15) >> 2) + 4 * hi;
    if (token >= M || feat >= N) continue;                       // N % 4 == 0, feat % 4 == 0: a quad is inside N or outside it
    float* op = a.out + (size_t)token * a.ldo + feat;
    f32x4 old = {0.f, 0.f, 0.f, 0.f}, bias = {0.f, 0.f, 0.f, 0.f}, y;
    if (a.epi == WF_EPI_F32_ACC) old = *(const f32x4*)op;
    if (a.bias) bias = *(const f32x4*)(a.bias + feat);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float s = ((part[0][r0 + e][lane] + part[1][r0 + e][lane]) + part[2][r0 + e][lane]) + part[3][r0 + e][lane];
      y[e] = epi_f32(a.epi, s + bias[e], old[e]);
    }
    *(f32x4*)op = y;
  }
}

struct ClipAttnArgs {
  const float *Q, *K, *V;
  float* O;
  int ldqkv, ldo, L, D;
  float scale;
};

template <int DB>   // 32-channel blocks of a head: ceil(D / 32)
__global__ __launch_bounds__(256) void k_clip_attn(ClipAttnArgs a) {
  __shared__ float opart[3][DB * 16][64];
  __shared__ float lpart[3][64];
  __shared__ float mpart[4][32];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, r31 = lane & 31, hi = lane >> 5;
  const int h = blockIdx.y, L = a.L, D = a.D;
  const size_t hc = (size_t)h * D;
  const int qi = blockIdx.x * 32 + r31, qic = min(qi, L - 1);     // rows behind L compute row L - 1 again and store nothing

  // this lane's query row as the B operand of S^T = K . Q^T: block t = channels 8 t + 4 hi + j
  f32x4 qf[4 * DB];
#pragma unroll
  for (int t = 0; t < 4 * DB; ++t) qf[t] = ld4_or_zero(a.Q + (size_t)qic * a.ldqkv + hc + 8 * t + 4 * hi, 8 * t < D);

  const int nt = (L + 31) / 32;
  const int t0 = nt * wid / 4, t1 = nt * (wid + 1) / 4;
  auto scores = [&](int kt, f32x16& acc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* kp = a.K + (size_t)min(kt * 32 + r31, L - 1) * a.ldqkv + hc + 4 * hi;
#pragma unroll
    for (int t = 0; t < 4 * DB; ++t) {
      if (8 * t < D) {
        const f32x4 kf = *(const f32x4*)(kp + 8 * t);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = mfma32f(kf[j], qf[t][j], acc);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
      acc[r] = key < L ? acc[r] * a.scale : -INFINITY;
    }
  };

  // ---- sweep 1: the exact row maximum (L >= 1: some wave sees a finite score)
  float m = -INFINITY;
  for (int kt = t0; kt < t1; ++kt) {
    f32x16 acc;
    scores(kt, acc);
#pragma unroll
    for (int r = 0; r < 16; ++r) m = fmaxf(m, acc[r]);
  }
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  if (hi == 0) mpart[wid][r31] = m;
  __syncthreads();
  m = fmaxf(fmaxf(mpart[0][r31], mpart[1][r31]), fmaxf(mpart[2][r31], mpart[3][r31]));

  // ---- sweep 2: p = exp(s - m) in fp32, its row sum, O^T += V^T . P^T with p as it stands in the score registers
  f32x16 o[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
  float lsum = 0.f;
  for (int kt = t0; kt < t1; ++kt) {
    f32x16 acc;
    scores(kt, acc);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc[r] = expf(acc[r] - m);       // exp(-inf) = 0 for the keys that do not exist
      lsum += acc[r];
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = min(kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi, L - 1);
      const float* vp = a.V + (size_t)key * a.ldqkv + hc;
#pragma unroll
      for (int d = 0; d < DB; ++d) {
        const int c = 32 * d + r31;
        o[d] = mfma32f(c < D ? vp[c] : 0.f, acc[r], o[d]);
      }
    }
  }
  lsum += __shfl_xor(lsum, 32, 64);

  if (wid > 0) {
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) opart[wid - 1][16 * d + r][lane] = o[d][r];
    lpart[wid - 1][lane] = lsum;
  }
  __syncthreads();
  if (wid == 0 && qi < L) {
    const float inv = 1.f / (((lsum + lpart[0][lane]) + lpart[1][lane]) + lpart[2][lane]);
    float* orow = a.O + (size_t)qi * a.ldo + hc;
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
      for (int g = 0; g < 4; ++g) {    // registers 4 g .. 4 g + 3 = channels 32 d + 8 g + 4 hi + 0..3
        const int c = 32 * d + 8 * g + 4 * hi;
        if (c >= D) continue;          // D % 8 == 0: a quad is inside the head or outside it
        f32x4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 16 * d + 4 * g + e;
          y[e] = (((o[d][4 * g + e] + opart[0][r][lane]) + opart[1][r][lane]) + opart[2][r][lane]) * inv;
        }
        *(f32x4*)(orow + c) = y;
      }
  }
}

// pixel_values [3][S][S] -> the rows of the patch convolution as a GEMM operand: rows[(py G + px)][c p^2 + ph p + pw], G = S / p
__global__ void k_clip_patch_rows(const float* __restrict__ px, float* __restrict__ rows, int S, int p, size_t n) {
  const int pp = p * p, kk = 3 * pp, G = S / p;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / kk;
    const int k = (int)(i - row * kk);
    const int c = k / pp, ph = (k - c * pp) / p, pw = k - c * pp - ph * p;
    const int py = (int)(row / G), pxx = (int)(row - (size_t)py * G);
    rows[i] = px[((size_t)c * S + (size_t)py * p + ph) * S + (size_t)pxx * p + pw];
  }
}

}  // namespace
}  // namespace wf

using namespace wf;

extern "C" int wf_gemm_f32(const float* X, const float* W, const float* bias, float* out, int M, int N, int K, int ldx, int ldw, int ldo,
                           int epilogue, void* stream) {
  WF_CHECK_ARG(X && W && out, "wf_gemm_f32: null pointer");
  WF_CHECK_ARG(M >= 1 && N >= 4 && K >= 4 && N % 4 == 0 && K % 4 == 0, "wf_gemm_f32: need M >= 1, N %% 4 == 0, K %% 4 == 0 (M=%d N=%d K=%d)", M, N, K);
  WF_CHECK_ARG(ldx % 4 == 0 && ldw % 4 == 0 && ldo % 4 == 0 && ldx >= K && ldw >= K && ldo >= N,
               "wf_gemm_f32: leading dimensions %% 4, ldx >= K, ldw >= K, ldo >= N (ldx=%d ldw=%d ldo=%d)", ldx, ldw, ldo);
  WF_CHECK_ARG((((uintptr_t)X | (uintptr_t)W | (uintptr_t)bias | (uintptr_t)out) & 15) == 0, "wf_gemm_f32: pointers must be 16-byte aligned");
  WF_CHECK_ARG(epilogue == WF_EPI_F32 || epilogue == WF_EPI_F32_ACC || epilogue == WF_EPI_F32_GELU || epilogue == WF_EPI_F32_QUICK_GELU,
               "wf_gemm_f32: epilogue %d is not WF_EPI_F32, _F32_ACC, _F32_GELU or _F32_QUICK_GELU", epilogue);
  const int64_t tiles_m = ((int64_t)M + GF_TM - 1) / GF_TM, tiles_n = ((int64_t)N + GF_TN - 1) / GF_TN;
  const int64_t total = tiles_m * tiles_n;
  WF_CHECK_ARG(total <= (int64_t)1 << 30, "wf_gemm_f32: %lld tiles", (long long)total);
  GemmF32Args a;
  a.X = X, a.W = W, a.bias = bias, a.out = out;
  a.M = M, a.N = N, a.K = K, a.ldx = ldx, a.ldw = ldw, a.ldo = ldo, a.epi = epilogue;
  a.tiles_m = (int)tiles_m, a.total = (int)total, a.per_xcd = (int)((total + 7) / 8);
  hipLaunchKernelGGL(k_gemm_f32, dim3(8 * a.per_xcd), dim3(256), 0, (hipStream_t)stream, a);
  WF_LAUNCH_CHECK("wf_gemm_f32");
  return WF_OK;
}

extern "C" int wf_clip_attn_fwd(const float* Q, const float* K, const float* V, int ldqkv, float* O, int ldo, int H, int L, int D, float scale,
                                void* stream) {
  WF_CHECK_ARG(Q && K && V && O, "wf_clip_attn_fwd: null pointer");
  WF_CHECK_ARG(H >= 1 && H <= 65535 && L >= 1 && L <= 1024, "wf_clip_attn_fwd: need 1 <= H <= 65535, 1 <= L <= 1024 (H=%d L=%d)", H, L);
  WF_CHECK_ARG(D >= 8 && D <= 128 && D % 8 == 0, "wf_clip_attn_fwd: head width %d: need D %% 8 == 0, 8 <= D <= 128", D);
  WF_CHECK_ARG(ldqkv % 4 == 0 && ldo % 4 == 0 && (int64_t)ldqkv >= (int64_t)H * D && (int64_t)ldo >= (int64_t)H * D,
               "wf_clip_attn_fwd: ldqkv %% 4, ldo %% 4, both >= H * D");
  WF_CHECK_ARG((((uintptr_t)Q | (uintptr_t)K | (uintptr_t)V | (uintptr_t)O) & 15) == 0, "wf_clip_attn_fwd: pointers must be 16-byte aligned");
  WF_CHECK_ARG(scale > 0.f && scale < INFINITY, "wf_clip_attn_fwd: scale must be positive and finite");
  ClipAttnArgs a;
  a.Q = Q, a.K = K, a.V = V, a.O = O, a.ldqkv = ldqkv, a.ldo = ldo, a.L = L, a.D = D, a.scale = scale;
  const dim3 grid((L + 31) / 32, H), block(256);
  hipStream_t s = (hipStream_t)stream;
  switch ((D + 31) / 32) {
    case 1: hipLaunchKernelGGL(k_clip_attn<1>, grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(k_clip_attn<2>, grid, block, 0, s, a); break;
    case 3: hipLaunchKernelGGL(k_clip_attn<3>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(k_clip_attn<4>, grid, block, 0, s, a); break;
  }
  WF_LAUNCH_CHECK("wf_clip_attn_fwd");
  return WF_OK;
}

extern "C" int wf_clip_patch_rows(const float* pixels, float* rows, int S, int p, void* stream) {
  WF_CHECK_ARG(pixels && rows, "wf_clip_patch_rows: null pointer");
  WF_CHECK_ARG(p >= 1 && p <= 64 && S >= p && S <= 4096 && S % p == 0, "wf_clip_patch_rows: need 1 <= p <= 64, p <= S <= 4096, S %% p == 0 (S=%d p=%d)", S, p);
  const size_t n = (size_t)3 * S * S;
  hipLaunchKernelGGL(k_clip_patch_rows, dim3(grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, pixels, rows, S, p, n);
  WF_LAUNCH_CHECK("wf_clip_patch_rows");
  return WF_OK;
}
