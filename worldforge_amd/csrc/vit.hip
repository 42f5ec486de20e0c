// ViT kernels of the VGGT front-end (vggt/layers/attention.py, rope.py; vggt/models/aggregator.py): attention over 64-wide heads at
// any sequence length, the per-head LayerNorm + 2D RoPE on q and k, and the patch-embedding rows.  The linears are wf_gemm_bf16.
//
// k_vit_attn: one workgroup = 2 waves = (sequence, head, 64 query rows), each wave 32 query rows -- the frame of k_t5_attn (t5.hip):
// scores TRANSPOSED, S^T = K . Q^T on v_mfma_f32_32x32x16_bf16 (A = K from LDS, B = Q held in registers), so a lane owns ONE query
// (column l & 31) and 16 keys of a 32-key sub-tile; the accumulator tile converted to bf16 is directly the B operand of O^T = V^T . P^T.
// Instead of the whole head in LDS and two sweeps, the keys stream through a ring of two 64-key tiles -- K [64][72] (144-byte rows:
// conflict-free 16-byte fragment reads) and V^T [64][68] (136-byte rows, 8-byte fragment reads) per slot, 35,840 bytes in all -- with
// an online softmax: per tile m' = max(m, tile max), o and l are multiplied by exp2(m - m') (exactly 0 at the first tile, m = -inf),
// p = exp2(s - m') in fp32, l += p (un-rounded), P rounded once to bf16 for the PV product, O = o / l rounded once.  The scores are kept
// in exp2 units: s = acc * (scale * log2 e), one fp32 product.  Tile t + 1 is fetched into registers before tile t is computed and
// written to the other slot afterwards: one barrier per tile.  The last tile is masked here: keys >= L are zero-filled in LDS (never
// read from memory: no row of another sequence is touched) and their scores are -inf; every tile holds at least one key, so m' is finite.
#include "common.h"
#include "mfma.h"

namespace wf {
namespace {

constexpr int VA_D = 64;      // head dimension
constexpr int VA_T = 64;      // keys per tile
constexpr int VA_KLD = 72;    // K row stride in LDS (elements), as T5_KLD
constexpr int VA_VLD = 68;    // V^T row stride (elements): 34 dwords, 8-byte aligned rows, as t5's kvp + 4
constexpr int VA_SLOT = VA_T * VA_KLD + VA_D * VA_VLD;   // elements per ring slot

struct VitAttnArgs {
  const uint16_t *Q, *K, *V;
  uint16_t* O;
  int ldqkv, ldo, L;
  float sl;   // scale * log2(e)
};

__global__ __launch_bounds__(128) void k_vit_attn(VitAttnArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t smem[2 * VA_SLOT];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int h = blockIdx.y, L = a.L;
  const size_t row0 = (size_t)blockIdx.z * L;                     // first row of this sequence
  const uint16_t* Kg = a.K + row0 * a.ldqkv + (size_t)h * VA_D;
  const uint16_t* Vg = a.V + row0 * a.ldqkv + (size_t)h * VA_D;
  static_assert((VA_KLD * 2) % 16 == 0 && (VA_SLOT * 2) % 16 == 0 && (VA_T * VA_KLD * 2) % 8 == 0, "slot alignment");

  // staging: K in row order (thread = 16-byte chunk c of key i >> 3: a key's 128 bytes are read by 8 neighbouring lanes), V with
  // consecutive threads = consecutive keys (the transposed 2-byte LDS stores of a wave are adjacent)
  u32x4 kq[4], vq[4];
  auto fetch = [&](int t) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = tid + 128 * j;
      const int kk = t * VA_T + (i >> 3), vk = t * VA_T + (i & 63);
      kq[j] = u32x4{0, 0, 0, 0};
      vq[j] = u32x4{0, 0, 0, 0};
      if (kk < L) kq[j] = *(const u32x4*)(Kg + (size_t)kk * a.ldqkv + 8 * (i & 7));
      if (vk < L) vq[j] = *(const u32x4*)(Vg + (size_t)vk * a.ldqkv + 8 * (i >> 6));
    }
  };
  auto stash = [&](int slot) {
    uint16_t* Ks = smem + slot * VA_SLOT;
    uint16_t* Vt = Ks + VA_T * VA_KLD;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = tid + 128 * j;
      *(u32x4*)(Ks + (i >> 3) * VA_KLD + 8 * (i & 7)) = kq[j];
      const int key = i & 63, c = i >> 6;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        Vt[(8 * c + 2 * e) * VA_VLD + key] = (uint16_t)(vq[j][e] & 0xffffu);
        Vt[(8 * c + 2 * e + 1) * VA_VLD + key] = (uint16_t)(vq[j][e] >> 16);
      }
    }
  };

  // this lane's query row as the B operand of S^T = K . Q^T: 4 k-steps of 16 channels, elements 16 s + 8 hi + j
  const int qi = blockIdx.x * 64 + wid * 32 + l31;
  const int qic = qi < L ? qi : L - 1;            // rows behind L (last block) compute row L - 1 again and store nothing
  bf16x8 qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
    qf[s] = as_bf16x8(*(const u32x4*)(a.Q + (row0 + qic) * a.ldqkv + (size_t)h * VA_D + 16 * s + 8 * hi));

  f32x16 o[2];
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
  float m = -INFINITY, lsum = 0.f;   // lsum: this lane's 32 of the tile's 64 keys; the halves are added at the end

  const int nt = (L + VA_T - 1) / VA_T;
  fetch(0);
  stash(0);
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) fetch(t + 1);
    const uint16_t* Ks = smem + (t & 1) * VA_SLOT;
    const uint16_t* Vt = Ks + VA_T * VA_KLD;
    f32x16 sc[2];
    float tm = -INFINITY;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[u][r] = 0.f;
      const uint16_t* kr = Ks + (u * 32 + l31) * VA_KLD + 8 * hi;
#pragma unroll
      for (int s = 0; s < 4; ++s) sc[u] = mfma32(as_bf16x8(*(const u32x4*)(kr + 16 * s)), qf[s], sc[u]);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = t * VA_T + u * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        sc[u][r] = key < L ? sc[u][r] * a.sl : -INFINITY;
        tm = fmaxf(tm, sc[u][r]);
      }
    }
    tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
    const float mn = fmaxf(m, tm);                 // finite: key t * 64 exists
    const float alpha = __builtin_amdgcn_exp2f(m - mn);   // exp2(-inf) = 0 at the first tile
    m = mn;
    lsum *= alpha;
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sc[u][r] = __builtin_amdgcn_exp2f(sc[u][r] - mn);    // 0 for the keys that do not exist
        lsum += sc[u][r];
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        u32x4 pw;
#pragma unroll
        for (int e = 0; e < 4; ++e) pw[e] = pack_bf16x2(sc[u][8 * s + 2 * e], sc[u][8 * s + 2 * e + 1]);
        const bf16x8 pf = as_bf16x8(pw);
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          // element j of lane half hi = key 16 s + 8 (j >> 2) + 4 hi + (j & 3) of the sub-tile: two 8-byte reads of channel row 32 d + l31
          const uint16_t* vr = Vt + (32 * d + l31) * VA_VLD + u * 32 + 16 * s + 4 * hi;
          const u32x2 v0 = *(const u32x2*)vr, v1 = *(const u32x2*)(vr + 8);
          const u32x4 vf = {v0[0], v0[1], v1[0], v1[1]};
          o[d] = mfma32(as_bf16x8(vf), pf, o[d]);
        }
      }
    }
    if (t + 1 < nt) stash((t + 1) & 1);   // the other slot was last read in iteration t - 1, behind that iteration's barrier
    __syncthreads();
  }
  lsum += __shfl_xor(lsum, 32, 64);

  if (qi < L) {
    const float inv = 1.f / lsum;
    uint16_t* orow = a.O + (row0 + qi) * a.ldo + (size_t)h * VA_D;
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int g = 0; g < 4; ++g) {   // registers 4 g .. 4 g + 3 = channels 32 d + 8 g + 4 hi + 0..3
        const u32x2 w = {pack_bf16x2(o[d][4 * g] * inv, o[d][4 * g + 1] * inv), pack_bf16x2(o[d][4 * g + 2] * inv, o[d][4 * g + 3] * inv)};
        *(u32x2*)(orow + 32 * d + 8 * g + 4 * hi) = w;
      }
  }
}

// Per (row, head, q | k): LayerNorm over the 64 channels, then the 2D rotation.  8 lanes per item; lane j = 4 hf + t owns channels
// 32 hf + 4 t + 0..3 and their rotate-half partners 32 hf + 16 + 4 t + 0..3 (half hf = 0 turns with the y position, 1 with x): the
// rotation stays inside the lane, the LayerNorm sums cross 8 lanes (xor 1, 2, 4: a fixed order).
struct VitNormArgs {
  uint16_t *Q, *K;
  const float *qw, *qb, *kw, *kb, *cs, *sn;
  const int* pos;
  int ld, L, H, max_pos;
  float eps, out_scale;
  size_t items;   // rows * H * 2
};

__global__ __launch_bounds__(256) void k_vit_qk_norm_rope(VitNormArgs a) {
  const int j = threadIdx.x & 7, hf = j >> 2, t = j & 3;
  const int c0 = 32 * hf + 4 * t;
  const size_t stride = (size_t)gridDim.x * 32;
  const size_t n_up = (a.items + 31) / 32 * 32;       // whole 8-lane groups stay together; a block's 32 items stay in one wave set
  for (size_t it = (size_t)blockIdx.x * 32 + (threadIdx.x >> 3); it < n_up; it += stride) {
    const bool live = it < a.items;
    const size_t itc = live ? it : a.items - 1;
    const int which = (int)(itc & 1);
    const size_t rh = itc >> 1;
    const int h = (int)(rh % a.H);
    const size_t row = rh / a.H;
    uint16_t* p = (which ? a.K : a.Q) + row * a.ld + (size_t)h * 64 + c0;
    const u32x2 lo = *(const u32x2*)p, up = *(const u32x2*)(p + 16);
    float x[8];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      x[2 * e] = __uint_as_float(lo[e] << 16), x[2 * e + 1] = __uint_as_float(lo[e] & 0xffff0000u);
      x[4 + 2 * e] = __uint_as_float(up[e] << 16), x[5 + 2 * e] = __uint_as_float(up[e] & 0xffff0000u);
    }
    const float* w = which ? a.kw : a.qw;
    const float* b = which ? a.kb : a.qb;
    if (w) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) s += x[e];
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) s += __shfl_xor(s, o, 64);
      const float mean = s * (1.f / 64.f);
      float q = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        x[e] -= mean;
        q += x[e] * x[e];
      }
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) q += __shfl_xor(q, o, 64);
      const float r = rsqrtf(q * (1.f / 64.f) + a.eps);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        x[e] = x[e] * r * w[c0 + e] + b[c0 + e];
        x[4 + e] = x[4 + e] * r * w[c0 + 16 + e] + b[c0 + 16 + e];
      }
    }
    if (a.cs) {
      int ps = a.pos[(row % a.L) * 2 + hf];
      ps = ps < 0 ? 0 : (ps > a.max_pos ? a.max_pos : ps);   // the host has refused such positions already; never read outside the tables
      const f32x4 c = *(const f32x4*)(a.cs + (size_t)ps * 16 + 4 * t), s = *(const f32x4*)(a.sn + (size_t)ps * 16 + 4 * t);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float x1 = x[e], x2 = x[4 + e];
        x[e] = x1 * c[e] - x2 * s[e];
        x[4 + e] = x2 * c[e] + x1 * s[e];
      }
    }
    const float g = which ? 1.f : a.out_scale;
    if (live) {
      const u32x2 wl = {pack_bf16x2(x[0] * g, x[1] * g), pack_bf16x2(x[2] * g, x[3] * g)};
      const u32x2 wu = {pack_bf16x2(x[4] * g, x[5] * g), pack_bf16x2(x[6] * g, x[7] * g)};
      *(u32x2*)p = wl;
      *(u32x2*)(p + 16) = wu;
    }
  }
}

// (x - mean_c) / std_c in fp32, one rounding to bf16, in the conv weight's flattening order; 2 columns per thread, 296 threads' worth
// per patch row (columns 588..591 are zero).
__global__ void k_vit_patch_rows(const float* __restrict__ img, uint16_t* __restrict__ rows, int Hh, int Ww, size_t n2) {
  const int gw = Ww / 14, gh = Hh / 14;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / 296;
    const int col = (int)(i - row * 296) * 2;
    const int px = (int)(row % gw), py = (int)((row / gw) % gh);
    const size_t im = row / ((size_t)gw * gh);
    float v[2] = {0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int k = col + e;
      if (k < 588) {
        const int c = k / 196, r = k - c * 196, ph = r / 14, pw = r - ph * 14;
        const float x = img[((im * 3 + c) * Hh + (size_t)py * 14 + ph) * Ww + (size_t)px * 14 + pw];
        const float mean = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f), sd = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);   // ResNet statistics
        v[e] = (x - mean) / sd;
      }
    }
    *(uint32_t*)(rows + row * 592 + col) = pack_bf16x2(v[0], v[1]);
  }
}

}  // namespace
}  // namespace wf

using namespace wf;

extern "C" int wf_vit_attn_fwd(const void* Q, const void* K, const void* V, int ldqkv, void* O, int ldo, int nseq, int H, int L, float scale,
                               void* stream) {
  WF_CHECK_ARG(Q && K && V && O, "wf_vit_attn_fwd: null pointer");
  WF_CHECK_ARG(nseq >= 1 && nseq <= 65535 && H >= 1 && H <= 65535 && L >= 1,
               "wf_vit_attn_fwd: need 1 <= nseq <= 65535, 1 <= H <= 65535, L >= 1 (nseq=%d H=%d L=%d)", nseq, H, L);
  WF_CHECK_ARG((int64_t)nseq * L <= 0x7fffffff, "wf_vit_attn_fwd: nseq * L must fit 31 bits");
  WF_CHECK_ARG(scale > 0.f && scale < INFINITY, "wf_vit_attn_fwd: scale must be positive and finite");
  WF_CHECK_ARG(ldqkv % 8 == 0 && ldo % 4 == 0 && (int64_t)ldqkv >= (int64_t)H * VA_D && (int64_t)ldo >= (int64_t)H * VA_D,
               "wf_vit_attn_fwd: ldqkv %% 8, ldo %% 4, both >= H * 64");
  WF_CHECK_ARG((((uintptr_t)Q | (uintptr_t)K | (uintptr_t)V) & 15) == 0 && ((uintptr_t)O & 7) == 0,
               "wf_vit_attn_fwd: Q, K, V 16-byte, O 8-byte aligned");
  VitAttnArgs a;
  a.Q = (const uint16_t*)Q, a.K = (const uint16_t*)K, a.V = (const uint16_t*)V, a.O = (uint16_t*)O;
  a.ldqkv = ldqkv, a.ldo = ldo, a.L = L, a.sl = scale * 1.4426950408889634f;
  hipLaunchKernelGGL(k_vit_attn, dim3((L + 63) / 64, H, nseq), dim3(128), 0, (hipStream_t)stream, a);
  WF_LAUNCH_CHECK("wf_vit_attn_fwd");
  return WF_OK;
}

extern "C" int wf_vit_qk_norm_rope(void* Q, void* K, int ldqkv, const float* q_weight, const float* q_bias, const float* k_weight,
                                   const float* k_bias, float eps, const float* cos_tab, const float* sin_tab, int max_pos, const int* pos,
                                   int nseq, int L, int H, float out_scale, void* stream) {
  WF_CHECK_ARG(Q && K, "wf_vit_qk_norm_rope: null pointer");
  WF_CHECK_ARG(nseq >= 1 && L >= 1 && H >= 1 && H <= 65535 && (int64_t)nseq * L <= 0x7fffffff,
               "wf_vit_qk_norm_rope: need nseq >= 1, L >= 1, 1 <= H <= 65535, nseq * L in 31 bits (nseq=%d L=%d H=%d)", nseq, L, H);
  const bool norm = q_weight || q_bias || k_weight || k_bias, rope = cos_tab || sin_tab || pos;
  WF_CHECK_ARG(!norm || (q_weight && q_bias && k_weight && k_bias), "wf_vit_qk_norm_rope: the four norm pointers come together or not at all");
  WF_CHECK_ARG(!rope || (cos_tab && sin_tab && pos && max_pos >= 0), "wf_vit_qk_norm_rope: cos, sin and pos come together, max_pos >= 0");
  WF_CHECK_ARG(!norm || (eps > 0.f && eps < INFINITY), "wf_vit_qk_norm_rope: eps must be positive and finite");
  WF_CHECK_ARG(out_scale > 0.f && out_scale < INFINITY, "wf_vit_qk_norm_rope: out_scale must be positive and finite (1 = none)");
  WF_CHECK_ARG(ldqkv % 4 == 0 && (int64_t)ldqkv >= (int64_t)H * 64, "wf_vit_qk_norm_rope: ldqkv %% 4, >= H * 64");
  WF_CHECK_ARG((((uintptr_t)Q | (uintptr_t)K) & 7) == 0 && (((uintptr_t)cos_tab | (uintptr_t)sin_tab) & 15) == 0 && ((uintptr_t)pos & 3) == 0 &&
                   (((uintptr_t)q_weight | (uintptr_t)q_bias | (uintptr_t)k_weight | (uintptr_t)k_bias) & 3) == 0,
               "wf_vit_qk_norm_rope: Q, K 8-byte, tables 16-byte aligned");
  VitNormArgs a;
  a.Q = (uint16_t*)Q, a.K = (uint16_t*)K, a.qw = q_weight, a.qb = q_bias, a.kw = k_weight, a.kb = k_bias, a.cs = cos_tab, a.sn = sin_tab;
  a.pos = pos, a.ld = ldqkv, a.L = L, a.H = H, a.max_pos = max_pos, a.eps = eps, a.out_scale = out_scale;
  a.items = (size_t)nseq * L * H * 2;
  hipLaunchKernelGGL(k_vit_qk_norm_rope, dim3(grid_for((a.items + 31) / 32 * 32, 32, 16384)), dim3(256), 0, (hipStream_t)stream, a);
  WF_LAUNCH_CHECK("wf_vit_qk_norm_rope");
  return WF_OK;
}

extern "C" int wf_vit_patch_rows(const float* images, void* rows, int n, int Hh, int Ww, void* stream) {
  WF_CHECK_ARG(images && rows, "wf_vit_patch_rows: null pointer");
  WF_CHECK_ARG(n >= 1 && Hh >= 14 && Ww >= 14 && Hh % 14 == 0 && Ww % 14 == 0, "wf_vit_patch_rows: n >= 1, H and W positive multiples of 14 (n=%d H=%d W=%d)",
               n, Hh, Ww);
  WF_CHECK_ARG((int64_t)n * (Hh / 14) * (Ww / 14) <= 0x7fffffff, "wf_vit_patch_rows: the row count must fit 31 bits");
  WF_CHECK_ARG(((uintptr_t)images & 3) == 0 && ((uintptr_t)rows & 3) == 0, "wf_vit_patch_rows: 4-byte aligned pointers");
  const size_t n2 = (size_t)n * (Hh / 14) * (Ww / 14) * 296;
  hipLaunchKernelGGL(k_vit_patch_rows, dim3(grid_for(n2, 256, 8192)), dim3(256), 0, (hipStream_t)stream, images, (uint16_t*)rows, Hh, Ww, n2);
  WF_LAUNCH_CHECK("wf_vit_patch_rows");
  return WF_OK;
}
