// UMT5 text-encoder kernels (transformers/models/umt5/modeling_umt5.py): T5 self-attention with a bucketed relative-position bias,
// the gated-GELU gate, T5LayerNorm and the embedding gather.  The GEMMs of the encoder are wf_gemm_bf16 (gemm.hip).
//
// k_t5_attn: one workgroup = 2 waves = (head, 64 query rows), each wave 32 query rows.  The head's K [kvp][64] (rows padded to 72
// elements: conflict-free 16-byte fragment reads) and V^T [64][kvp + 4] live in LDS for the whole workgroup (kvp = kv_len rounded up
// to 32 <= 512: 73,728 + 66,048 bytes at most), beside the head's bias by relative position (bias[h][lut[rel]], <= 1023 floats).
// Scores are computed TRANSPOSED, S^T = K . Q^T on v_mfma_f32_32x32x16_bf16 (A = K from LDS, B = Q held in registers): a lane then owns
// ONE query (column l & 31) and 16 keys of the 32-key tile in its accumulator registers, so the softmax statistics are a chain over
// registers plus one exchange with lane ^ 32, and the accumulator tile converted to bf16 is directly the B operand of O^T = V^T . P^T
// (mfma.h: the k order inside a step is rows 16 s + 8 (j >> 2) + 4 hi + (j & 3); the V^T fragment is read in that order).
// Two sweeps over the keys instead of an online softmax: sweep 1 finds each row's exact maximum, sweep 2 recomputes the same scores
// (same instructions, same bits), p = exp(s - m) in fp32, row sum of the un-rounded p in fp32, P rounded once to bf16 for the PV product,
// O = acc / l rounded once.  The encoder runs once per video on <= 512 tokens: the second QK^T costs nothing that matters and there is
// no rescaling to reason about.
#include "common.h"
#include "mfma.h"

namespace wf {
namespace {

constexpr int T5_D = 64;          // head dimension
constexpr int T5_LMAX = 512;      // longest sequence
constexpr int T5_KLD = 72;        // K row stride in LDS (elements): 144 bytes, 16-byte aligned, 36 dwords -> conflict-free b128 reads
constexpr int T5_VPAD = 4;        // V^T row stride = kvp + 4 elements: (kvp / 2 + 2) dwords, 8-byte aligned rows, conflict-free b64 reads

struct T5AttnArgs {
  const uint16_t *Q, *K, *V;
  uint16_t* O;
  const float* bias;        // [H][num_buckets]
  const uint8_t* lut;       // [2 * lmax - 1]
  int ldqkv, ldo, L, kv_len, kvp, lmax, num_buckets;
};

__global__ __launch_bounds__(128) void k_t5_attn(T5AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int h = blockIdx.y, L = a.L, kvp = a.kvp, kv_len = a.kv_len;
  const int vld = kvp + T5_VPAD;
  uint16_t* Ks = (uint16_t*)smem;                                  // [kvp][72]
  uint16_t* Vt = Ks + (size_t)kvp * T5_KLD;                        // [64][kvp + 4]
  float* brel = (float*)(Vt + (size_t)T5_D * vld);                 // [2 L - 1]: bias of key - query + (L - 1)
  static_assert((T5_KLD * 2) % 16 == 0, "K rows 16-byte aligned");

  // ---- fill: K rows (16-byte chunks), V transposed (one key column per thread, 8 channels), the head's bias by relative position
  for (int i = tid; i < kvp * 8; i += 128) {
    const int c = i / kvp, key = i - c * kvp;     // consecutive threads = consecutive keys: the transposed 2-byte stores are adjacent
    u32x4 kq = {0, 0, 0, 0}, vq = {0, 0, 0, 0};
    if (key < kv_len) {
      const size_t g = (size_t)key * a.ldqkv + (size_t)h * T5_D + 8 * c;
      kq = *(const u32x4*)(a.K + g);
      vq = *(const u32x4*)(a.V + g);
    }
    *(u32x4*)(Ks + (size_t)key * T5_KLD + 8 * c) = kq;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      Vt[(size_t)(8 * c + 2 * e) * vld + key] = (uint16_t)(vq[e] & 0xffffu);
      Vt[(size_t)(8 * c + 2 * e + 1) * vld + key] = (uint16_t)(vq[e] >> 16);
    }
  }
  for (int i = tid; i < 2 * L - 1; i += 128) {
    const int b = a.lut[i - (L - 1) + (a.lmax - 1)];   // a byte outside the table would read outside `bias`: clamped, never trusted
    brel[i] = a.bias[(size_t)h * a.num_buckets + (b < a.num_buckets ? b : a.num_buckets - 1)];
  }

  // ---- this lane's query row as the B operand of S^T = K . Q^T: 4 k-steps of 16 channels, elements 16 s + 8 hi + j
  const int qi = blockIdx.x * 64 + wid * 32 + l31;
  const int qic = qi < L ? qi : L - 1;            // rows behind L (last tile) compute row L - 1 again and store nothing
  bf16x8 qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
    qf[s] = as_bf16x8(*(const u32x4*)(a.Q + (size_t)qic * a.ldqkv + (size_t)h * T5_D + 16 * s + 8 * hi));
  __syncthreads();

  const int nt = kvp / 32;
  const float* bq = brel + (L - 1) - qic;         // bq[key] = bias of (key - query), key < L
  auto scores = [&](int kt, f32x16& acc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const uint16_t* kr = Ks + (size_t)(kt * 32 + l31) * T5_KLD + 8 * hi;
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = mfma32(as_bf16x8(*(const u32x4*)(kr + 16 * s)), qf[s], acc);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
      acc[r] = key < kv_len ? acc[r] + bq[key] : -INFINITY;   // kv_len <= L: bq is only read inside its 2 L - 1 entries
    }
  };

  // ---- sweep 1: the row maximum (kv_len >= 1: finite)
  float m = -INFINITY;
  for (int kt = 0; kt < nt; ++kt) {
    f32x16 acc;
    scores(kt, acc);
#pragma unroll
    for (int r = 0; r < 16; ++r) m = fmaxf(m, acc[r]);
  }
  m = fmaxf(m, __shfl_xor(m, 32, 64));

  // ---- sweep 2: p = exp(s - m), l = sum p (fp32), O^T += V^T . bf16(P^T)
  f32x16 o[2];
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
  float lsum = 0.f;
  for (int kt = 0; kt < nt; ++kt) {
    f32x16 acc;
    scores(kt, acc);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc[r] = expf(acc[r] - m);     // exp(-inf) = 0 for the keys that do not exist
      lsum += acc[r];
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      u32x4 pw;
#pragma unroll
      for (int e = 0; e < 4; ++e) pw[e] = pack_bf16x2(acc[8 * s + 2 * e], acc[8 * s + 2 * e + 1]);
      const bf16x8 pf = as_bf16x8(pw);
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        // element j of lane half hi = key 16 s + 8 (j >> 2) + 4 hi + (j & 3) of the tile: two 8-byte reads of channel row 32 d + l31
        const uint16_t* vr = Vt + (size_t)(32 * d + l31) * vld + kt * 32 + 16 * s + 4 * hi;
        const u32x2 v0 = *(const u32x2*)vr, v1 = *(const u32x2*)(vr + 8);
        const u32x4 vf = {v0[0], v0[1], v1[0], v1[1]};
        o[d] = mfma32(as_bf16x8(vf), pf, o[d]);
      }
    }
  }
  lsum += __shfl_xor(lsum, 32, 64);

  if (qi < L) {
    const float inv = 1.f / lsum;
    uint16_t* orow = a.O + (size_t)qi * a.ldo + (size_t)h * T5_D;
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int g = 0; g < 4; ++g) {   // registers 4 g .. 4 g + 3 = channels 32 d + 8 g + 4 hi + 0..3
        const u32x2 w = {pack_bf16x2(o[d][4 * g] * inv, o[d][4 * g + 1] * inv), pack_bf16x2(o[d][4 * g + 2] * inv, o[d][4 * g + 3] * inv)};
        *(u32x2*)(orow + 32 * d + 8 * g + 4 * hi) = w;
      }
  }
}

// gelu_new(g) * u, one rounding.  tanhf saturates to +-1 for large arguments (g^3 stays finite in fp32 up to |g| ~ 7e12).
__global__ void k_t5_gated_gelu(const float* __restrict__ in, int64_t ld, uint16_t* __restrict__ out, int F, size_t n4) {
  const int f4 = F / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / f4;
    const int c = (int)(i - row * f4) * 4;
    const f32x4 g = *(const f32x4*)(in + row * ld + c), u = *(const f32x4*)(in + row * ld + F + c);
    float y[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x = g[e];
      const float t = tanhf(0.7978845608028654f * (x + 0.044715f * x * x * x));
      y[e] = 0.5f * x * (1.f + t) * u[e];
    }
    const u32x2 w = {pack_bf16x2(y[0], y[1]), pack_bf16x2(y[2], y[3])};
    *(u32x2*)(out + row * (size_t)F + c) = w;
  }
}

// T5LayerNorm: one workgroup of 256 per row; the sum of squares in fp32 in a fixed order (lane chain, wave tree, 4 waves in order).
__global__ __launch_bounds__(256) void k_t5_rmsnorm(const float* __restrict__ x, const float* __restrict__ w, uint16_t* __restrict__ out,
                                                    int C, float eps) {
  __shared__ float part[4];
  const size_t row = blockIdx.x;
  const float* xr = x + row * (size_t)C;
  float ss = 0.f;
  for (int c = threadIdx.x * 4; c < C; c += 1024) {
    const f32x4 v = *(const f32x4*)(xr + c);
    ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  ss = wave_sum(ss);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = ss;
  __syncthreads();
  const float r = rsqrtf((part[0] + part[1] + part[2] + part[3]) / (float)C + eps);
  for (int c = threadIdx.x * 4; c < C; c += 1024) {
    const f32x4 v = *(const f32x4*)(xr + c), g = *(const f32x4*)(w + c);
    const u32x2 o = {pack_bf16x2(v[0] * r * g[0], v[1] * r * g[1]), pack_bf16x2(v[2] * r * g[2], v[3] * r * g[3])};
    *(u32x2*)(out + row * (size_t)C + c) = o;
  }
}

__global__ void k_t5_embed(const int* __restrict__ ids, const uint16_t* __restrict__ table, float* __restrict__ out, int V, int C,
                           size_t n8) {
  const int c8 = C / 8;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / c8;
    const int c = (int)(i - row * c8) * 8;
    int id = ids[row];
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);   // the host has refused such ids already; never read outside the table
    const u32x4 v = *(const u32x4*)(table + (size_t)id * C + c);
    f32x4 lo, hi;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      lo[2 * e] = __uint_as_float(v[e] << 16);
      lo[2 * e + 1] = __uint_as_float(v[e] & 0xffff0000u);
      hi[2 * e] = __uint_as_float(v[2 + e] << 16);
      hi[2 * e + 1] = __uint_as_float(v[2 + e] & 0xffff0000u);
    }
    *(f32x4*)(out + row * (size_t)C + c) = lo;
    *(f32x4*)(out + row * (size_t)C + c + 4) = hi;
  }
}

}  // namespace
}  // namespace wf

using namespace wf;

extern "C" int wf_t5_attn_fwd(const void* Q, const void* K, const void* V, int ldqkv, void* O, int ldo, const float* bias,
                              const void* bucket_lut, int lmax, int num_buckets, int H, int L, int kv_len, void* stream) {
  WF_CHECK_ARG(Q && K && V && O && bias && bucket_lut, "wf_t5_attn_fwd: null pointer");
  WF_CHECK_ARG(H >= 1 && H <= 65535 && kv_len >= 1 && kv_len <= L && L <= T5_LMAX && L <= lmax,
               "wf_t5_attn_fwd: need H >= 1, 1 <= kv_len <= L <= min(512, lmax) (H=%d L=%d kv_len=%d lmax=%d)", H, L, kv_len, lmax);
  WF_CHECK_ARG(num_buckets >= 1 && num_buckets <= 256, "wf_t5_attn_fwd: 1 <= num_buckets <= 256");
  WF_CHECK_ARG(ldqkv % 8 == 0 && ldo % 4 == 0 && (int64_t)ldqkv >= (int64_t)H * T5_D && (int64_t)ldo >= (int64_t)H * T5_D,
               "wf_t5_attn_fwd: ldqkv %% 8, ldo %% 4, both >= H * 64");
  WF_CHECK_ARG((((uintptr_t)Q | (uintptr_t)K | (uintptr_t)V) & 15) == 0 && ((uintptr_t)O & 7) == 0 && ((uintptr_t)bias & 3) == 0,
               "wf_t5_attn_fwd: Q, K, V 16-byte, O 8-byte aligned");
  T5AttnArgs a;
  a.Q = (const uint16_t*)Q, a.K = (const uint16_t*)K, a.V = (const uint16_t*)V, a.O = (uint16_t*)O;
  a.bias = bias, a.lut = (const uint8_t*)bucket_lut;
  a.ldqkv = ldqkv, a.ldo = ldo, a.L = L, a.kv_len = kv_len, a.kvp = (kv_len + 31) / 32 * 32, a.lmax = lmax, a.num_buckets = num_buckets;
  const size_t lds = (size_t)a.kvp * T5_KLD * 2 + (size_t)T5_D * (a.kvp + T5_VPAD) * 2 + (size_t)(2 * L - 1) * 4;
  hipLaunchKernelGGL(k_t5_attn, dim3((L + 63) / 64, H), dim3(128), lds, (hipStream_t)stream, a);
  WF_LAUNCH_CHECK("wf_t5_attn_fwd");
  return WF_OK;
}

extern "C" int wf_t5_gated_gelu(const float* in, int64_t ld, void* out, int M, int F, void* stream) {
  WF_CHECK_ARG(in && out, "wf_t5_gated_gelu: null pointer");
  WF_CHECK_ARG(M >= 0 && F > 0 && F % 4 == 0 && ld % 4 == 0 && ld >= 2 * (int64_t)F, "wf_t5_gated_gelu: F %% 4, ld %% 4, ld >= 2 F");
  WF_CHECK_ARG(((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 7) == 0, "wf_t5_gated_gelu: in 16-byte, out 8-byte aligned");
  const size_t n4 = (size_t)M * (F / 4);
  if (n4 == 0) return WF_OK;
  hipLaunchKernelGGL(k_t5_gated_gelu, dim3(grid_for(n4, 256, 8192)), dim3(256), 0, (hipStream_t)stream, in, ld, (uint16_t*)out, F, n4);
  WF_LAUNCH_CHECK("wf_t5_gated_gelu");
  return WF_OK;
}

extern "C" int wf_t5_rmsnorm(const float* x, const float* weight, void* out, int L, int C, float eps, void* stream) {
  WF_CHECK_ARG(x && weight && out, "wf_t5_rmsnorm: null pointer");
  WF_CHECK_ARG(L >= 0 && C > 0 && C % 4 == 0, "wf_t5_rmsnorm: C %% 4");
  WF_CHECK_ARG((((uintptr_t)x | (uintptr_t)weight) & 15) == 0 && ((uintptr_t)out & 7) == 0, "wf_t5_rmsnorm: x, weight 16-byte, out 8-byte aligned");
  if (L == 0) return WF_OK;
  hipLaunchKernelGGL(k_t5_rmsnorm, dim3(L), dim3(256), 0, (hipStream_t)stream, x, weight, (uint16_t*)out, C, eps);
  WF_LAUNCH_CHECK("wf_t5_rmsnorm");
  return WF_OK;
}

extern "C" int wf_t5_embed(const int* ids, const void* table, float* out, int L, int V, int C, void* stream) {
  WF_CHECK_ARG(ids && table && out, "wf_t5_embed: null pointer");
  WF_CHECK_ARG(L >= 0 && V > 0 && C > 0 && C % 8 == 0, "wf_t5_embed: V > 0, C %% 8");
  WF_CHECK_ARG((((uintptr_t)table | (uintptr_t)out) & 15) == 0 && ((uintptr_t)ids & 3) == 0, "wf_t5_embed: table, out 16-byte aligned");
  const size_t n8 = (size_t)L * (C / 8);
  if (n8 == 0) return WF_OK;
  hipLaunchKernelGGL(k_t5_embed, dim3(grid_for(n8, 256, 8192)), dim3(256), 0, (hipStream_t)stream, ids, (const uint16_t*)table, out, V, C, n8);
  WF_LAUNCH_CHECK("wf_t5_embed");
  return WF_OK;
}
