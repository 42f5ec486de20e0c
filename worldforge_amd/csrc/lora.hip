// Switchable LoRA adapters on resident weights: wf_lora_fold re-derives one bf16 matrix (or a contiguous row slice of one) from its
// untouched base and up to four low-rank adapters,
//
//   out[n, k] = bf16_rne( base[n, k] + sum_j scale_j * sum_r U_j[n, r] * D_j[blk_j(n) * rank_j + r, k] ),   blk_j(n) = n / (N / nsep_j)
//
// (the reference's run-time side path, longcat_video_dit.py:194-247 + lora_utils.py:15-78, turned into a weight switch: the forward keeps
// running on plain bf16 matrices).  Row block b of a fused qkv / kv weight uses rank slice b of the down-projection (LoRAUPParallel,
// lora_utils.py:15-24); no block-diagonal U is ever built.  Products on the bf16 MFMA with fp32 accumulation, each adapter's product
// scaled in fp32, the base added in fp32, ONE rounding to bf16.
//
// HBM-bound (4 bytes of weight traffic per element), so shaped as a streaming kernel:
//   * a workgroup owns a 128-column tile and walks row tiles of it; the D panels of that column tile ([rank][128] per adapter) are
//     transposed into LDS once ([column][rank], so that an MFMA operand fragment is one 16-byte LDS read) and stay there for the walk;
//   * a wave's tile is 32 rows x 128 columns = 4 MFMA tiles; the MFMA's "row" index is the matrix COLUMN (A = D^T, B = U^T in the maps of
//     mfma.h), permuted so that a lane's accumulator registers 8g..8g+7 are 8 consecutive columns of one matrix row: base is read and out
//     written in 16-byte pieces, 256 contiguous bytes per row over the tile;
//   * U fragments ([row][8 ranks] = 16 bytes) come straight from global memory (L2: neighbouring workgroups share the rows).
// Rows are cut into segments on which every adapter's row block is constant (N / lcm(nsep_j) rows), then into chunks that give the grid
// about four workgroups per CU; a workgroup never crosses a segment, so its LDS panels hold one rank slice per adapter.
// base is only read; out may be base (every element is read and written by the same lane, read first).
#include "common.h"
#include "mfma.h"

using namespace wf;

namespace {

constexpr int KT = 128;          // columns per workgroup
constexpr int RT = 32;           // rows per wave tile
constexpr int NWAVE = 4;
constexpr int MAXA = 4;
constexpr int MAX_RANK = 256;
constexpr int MAX_LDS = 128 * 1024;
constexpr int TARGET_BLOCKS = 1024;  // ~4 workgroups of 4 waves per CU

struct Adapter {
  const uint16_t* U;  // [N, rank]
  const uint16_t* D;  // [nsep * rank, K]
  float scale;
  int rank;
  int blk_rows;   // N / nsep
  int lds_off;    // byte offset of this adapter's panel
  int row_bytes;  // bytes per LDS row (one matrix column): slots of 8 ranks, a multiple of swz + 1 slots
  int swz;        // the 16-byte slot s of LDS row c is stored at slot s ^ ((c ^ (c >> 3)) & swz): spreads both the transposing writes
                  // (lanes along c / 8) and the fragment reads (lanes along c) over the banks
};

struct LoraArgs {
  const uint16_t* base;
  uint16_t* out;
  int N, K;
  int seg_rows, chunk_rows, chunks_per_seg, ctiles;
  Adapter a[MAXA];
};

__device__ __forceinline__ int swz_of(int c, int swz) { return (c ^ (c >> 3)) & swz; }

template <int NA>
__global__ __launch_bounds__(NWAVE * 64, NA == 1 ? 3 : NA == 2 ? 2 : 1) void k_lora_fold(LoraArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const int ct = blockIdx.x % p.ctiles;  // column tiles fastest: workgroups in flight together share their U rows in L2
  const int rc = blockIdx.x / p.ctiles;
  const int seg = rc / p.chunks_per_seg, chunk = rc % p.chunks_per_seg;
  const int seg_lo = seg * p.seg_rows;
  const int row_lo = seg_lo + chunk * p.chunk_rows;
  const int row_hi = min(row_lo + p.chunk_rows, seg_lo + p.seg_rows);
  const int k0 = ct * KT;
  const int K = p.K;

  // ---- D panels -> LDS, transposed: a thread takes rank rows 2q, 2q+1 at 8 columns and writes 8 dwords (one per column) ----
  for_const<NA>([&](auto J) {
    const Adapter& a = p.a[J.value];
    const int blk = row_lo / a.blk_rows;
    const uint16_t* Dp = a.D + (size_t)blk * a.rank * K;
    unsigned char* panel = smem + a.lds_off;
    const int ntask = (a.rank >> 1) * (KT / 8);
    for (int task = tid; task < ntask; task += NWAVE * 64) {
      const int ch = task & (KT / 8 - 1), q = task / (KT / 8);
      const int col = k0 + ch * 8;
      u32x4 v0 = {0u, 0u, 0u, 0u}, v1 = {0u, 0u, 0u, 0u};
      if (col < K) {
        v0 = *reinterpret_cast<const u32x4*>(Dp + (size_t)(2 * q) * K + col);
        v1 = *reinterpret_cast<const u32x4*>(Dp + (size_t)(2 * q + 1) * K + col);
      }
      const int slot = q >> 2, sub = (q & 3) * 4;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint32_t w0 = v0[e >> 1], w1 = v1[e >> 1];
        const uint32_t d = (e & 1) ? ((w0 >> 16) | (w1 & 0xffff0000u)) : ((w0 & 0xffffu) | (w1 << 16));
        const int c = ch * 8 + e;
        *reinterpret_cast<uint32_t*>(panel + c * a.row_bytes + ((slot ^ swz_of(c, a.swz)) << 4) + sub) = d;
      }
    }
  });
  __syncthreads();

  // MFMA row i = 8g + 4h + x  <->  tile column 16 (g >> 1) + 8 h + 4 (g & 1) + x: a lane's accumulator registers 8G .. 8G+7 are then the 8
  // consecutive columns 16 G + 8 hi .. of its matrix row (C/D map of mfma.h)
  const int kk = 16 * (l31 >> 4) + 8 * ((l31 >> 2) & 1) + 4 * ((l31 >> 3) & 1) + (l31 & 3);

  for (int r0 = row_lo + wid * RT; r0 < row_hi; r0 += NWAVE * RT) {
    const int n = r0 + l31;
    const int nc = min(n, row_hi - 1);  // loads of the rows past the chunk are clamped, their results dropped
    // base first: its latency hides under the products
    u32x4 bv[4][2];
    const uint16_t* brow = p.base + (size_t)nc * K;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int G = 0; G < 2; ++G) bv[t][G] = *reinterpret_cast<const u32x4*>(brow + min(k0 + 32 * t + 16 * G + 8 * hi, K - 8));

    // the adapters but the last are summed (scaled, fp32) in tot; the last one's accumulators go straight into the epilogue
    f32x16 tot[4], acc[4];
    for_const<NA>([&](auto J) {
      const Adapter& a = p.a[J.value];
      const unsigned char* panel = smem + a.lds_off;
      const uint16_t* Up = a.U + (size_t)nc * a.rank;
      const int nslots = a.rank >> 3;
      int rowoff[4], rsw[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        rowoff[t] = (32 * t + kk) * a.row_bytes;
        rsw[t] = swz_of(32 * t + kk, a.swz);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
      for (int s = 0; 2 * s < nslots; ++s) {
        // k-step s: ranks 16 s + 8 hi + j; a rank that is no multiple of 16 leaves the last step's upper half empty (zero operands)
        const bool ok = 2 * s + hi < nslots;
        const int slot = ok ? 2 * s + hi : 0;
        u32x4 bu = *reinterpret_cast<const u32x4*>(Up + slot * 8);
        if (!ok) bu = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          u32x4 ad = *reinterpret_cast<const u32x4*>(panel + rowoff[t] + ((slot ^ rsw[t]) << 4));
          if (!ok) ad = u32x4{0u, 0u, 0u, 0u};
          acc[t] = mfma32(as_bf16x8(ad), as_bf16x8(bu), acc[t]);
        }
      }
      if constexpr (J.value + 1 < NA) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            if constexpr (J.value == 0)
              tot[t][r] = a.scale * acc[t][r];
            else
              tot[t][r] += a.scale * acc[t][r];
          }
      }
    });
    const float sl = p.a[NA - 1].scale;
    auto val = [&](int t, int r) { return NA == 1 ? sl * acc[t][r] : tot[t][r] + sl * acc[t][r]; };

    if (n < row_hi) {
      uint16_t* orow = p.out + (size_t)n * K;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int G = 0; G < 2; ++G) {
          const int col = k0 + 32 * t + 16 * G + 8 * hi;
          if (col < K) {
            const u32x4 b = bv[t][G];
            u32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e)
              o[e] = pack_bf16x2(__uint_as_float(b[e] << 16) + val(t, 8 * G + 2 * e), __uint_as_float(b[e] & 0xffff0000u) + val(t, 8 * G + 2 * e + 1));
            *reinterpret_cast<u32x4*>(orow + col) = o;
          }
        }
    }
  }
}

long gcd_l(long a, long b) {
  while (b) {
    const long t = a % b;
    a = b;
    b = t;
  }
  return a;
}

}  // namespace

extern "C" int wf_lora_fold(const void* base, void* out, int N, int K, int n_adapters, const void* U0, const void* D0, int rank0, int nsep0,
                            float scale0, const void* U1, const void* D1, int rank1, int nsep1, float scale1, const void* U2, const void* D2,
                            int rank2, int nsep2, float scale2, const void* U3, const void* D3, int rank3, int nsep3, float scale3,
                            void* stream) {
  WF_CHECK_ARG(base && out, "wf_lora_fold: null pointer");
  WF_CHECK_ARG(N > 0 && K > 0, "wf_lora_fold: empty problem N=%d K=%d", N, K);
  WF_CHECK_ARG(K % 8 == 0, "wf_lora_fold: K (%d) must be a multiple of 8", K);
  WF_CHECK_ARG((((uintptr_t)base | (uintptr_t)out) & 15) == 0, "wf_lora_fold: base and out must be 16-byte aligned");
  WF_CHECK_ARG(n_adapters >= 1 && n_adapters <= MAXA, "wf_lora_fold: n_adapters (%d) must be 1..%d", n_adapters, MAXA);
  const void* Us[MAXA] = {U0, U1, U2, U3};
  const void* Ds[MAXA] = {D0, D1, D2, D3};
  const int ranks[MAXA] = {rank0, rank1, rank2, rank3}, nseps[MAXA] = {nsep0, nsep1, nsep2, nsep3};
  const float scales[MAXA] = {scale0, scale1, scale2, scale3};
  LoraArgs a;
  a.base = (const uint16_t*)base;
  a.out = (uint16_t*)out;
  a.N = N;
  a.K = K;
  long lcm = 1;
  int lds = 0;
  for (int j = 0; j < MAXA; ++j) {
    Adapter& ad = a.a[j];
    if (j >= n_adapters) {
      ad = a.a[0];
      continue;
    }
    WF_CHECK_ARG(Us[j] && Ds[j], "wf_lora_fold: null factor pointer (adapter %d)", j);
    WF_CHECK_ARG((((uintptr_t)Us[j] | (uintptr_t)Ds[j]) & 15) == 0, "wf_lora_fold: U and D must be 16-byte aligned (adapter %d)", j);
    WF_CHECK_ARG(ranks[j] >= 8 && ranks[j] <= MAX_RANK && ranks[j] % 8 == 0, "wf_lora_fold: rank (%d) must be a multiple of 8 in 8..%d (adapter %d)",
                 ranks[j], MAX_RANK, j);
    WF_CHECK_ARG(nseps[j] >= 1 && N % nseps[j] == 0, "wf_lora_fold: N (%d) must be a multiple of nsep (%d) (adapter %d)", N, nseps[j], j);
    const int nslots = ranks[j] / 8;
    int m = 1;
    while (m < 8 && 2 * m <= nslots) m *= 2;
    ad.U = (const uint16_t*)Us[j];
    ad.D = (const uint16_t*)Ds[j];
    ad.scale = scales[j];
    ad.rank = ranks[j];
    ad.blk_rows = N / nseps[j];
    ad.swz = m - 1;
    ad.row_bytes = (nslots + m - 1) / m * m * 16;
    ad.lds_off = lds;
    lds += KT * ad.row_bytes;
    lcm = lcm / gcd_l(lcm, nseps[j]) * nseps[j];  // every nsep divides N, so does their lcm
  }
  WF_CHECK_ARG(lds <= MAX_LDS, "wf_lora_fold: the adapters' ranks need %d bytes of LDS (limit %d)", lds, MAX_LDS);
  a.seg_rows = (int)(N / lcm);
  a.ctiles = ceil_div(K, KT);
  const long nseg = lcm;
  // rows per workgroup: whole wave rounds (128 rows), about TARGET_BLOCKS workgroups in all, never across a segment
  const long want_chunks = TARGET_BLOCKS / a.ctiles > 0 ? TARGET_BLOCKS / a.ctiles : 1;
  long rows = ((long)N + want_chunks - 1) / want_chunks;
  rows = (rows + NWAVE * RT - 1) / (NWAVE * RT) * (NWAVE * RT);
  if (rows > a.seg_rows) rows = a.seg_rows;
  a.chunks_per_seg = ceil_div(a.seg_rows, rows);
  a.chunk_rows = (ceil_div(a.seg_rows, a.chunks_per_seg) + RT - 1) / RT * RT;
  a.chunks_per_seg = ceil_div(a.seg_rows, a.chunk_rows);
  const long grid = (long)a.ctiles * nseg * a.chunks_per_seg;
  WF_CHECK_ARG(grid < (1L << 31), "wf_lora_fold: problem too large");
  hipStream_t s = (hipStream_t)stream;
  switch (n_adapters) {
    case 1: hipLaunchKernelGGL(k_lora_fold<1>, dim3((unsigned)grid), dim3(NWAVE * 64), lds, s, a); break;
    case 2: hipLaunchKernelGGL(k_lora_fold<2>, dim3((unsigned)grid), dim3(NWAVE * 64), lds, s, a); break;
    case 3: hipLaunchKernelGGL(k_lora_fold<3>, dim3((unsigned)grid), dim3(NWAVE * 64), lds, s, a); break;
    default: hipLaunchKernelGGL(k_lora_fold<4>, dim3((unsigned)grid), dim3(NWAVE * 64), lds, s, a); break;
  }
  WF_LAUNCH_CHECK("wf_lora_fold");
  return WF_OK;
}
