// Opt-in MX-fp8 linear layers (OCP MX: e4m3fn elements, one E8M0 scale 2^e per 32 consecutive K elements of a row).
//
//   wf_mx_quant_e4m3: bf16 [M, K] (row stride ldx) -> Q e4m3 [M, K] + S E8M0 [M, K/32].  HBM-bound; the same kernel quantizes the
//                     weights at load (rows = output features) and the activations in front of every GEMM.
//   wf_gemm_mxfp8:    out = epi(dequant(X) . dequant(W)^T + bias) on v_mfma_scale_f32_32x32x64_f8f6f4 (2x the bf16 MFMA rate per clock),
//                     fp32 accumulation.
//
// The GEMM is the ping-pong kernel of gemm.hip with the operand bytes halved: a K tile is 128 e4m3 elements = the same 128-byte LDS row as
// the 64 bf16 elements of k_gemm_pp.  From gemm_pp.h, shared with that kernel: the tile geometry (PPGeom), the XCD-aware rasteriser, the
// wave decomposition, the LDS-DMA piece addressing and its read-phase / MFMA-gap split (PPDma), the barrier helpers and the transposed
// epilogue (pp_epilogue, with gelu_tanh).  Written here: the scale handling, the fragment read, the scaled MFMA call and the K loop, where
// each half-tile phase is ONE k-step of 64 (NI x NJ scaled MFMAs of twice the bf16 cycles: the same matrix-pipe time per phase, for twice the K).
//
// Operand maps of the scaled 32x32x64 MFMA (e4m3 A and B, 32 bytes = 8 VGPRs per lane), pinned on the device with exact-integer data and
// distinct per-block scales (tests/test_gpu_mxfp8.py::test_gemm_layout_exact):
//   lane l (r = l & 31, h = l >> 5) holds row r of A (column r of B) at k = 16 h + j in bytes j = 0..15 and k = 32 + 16 h + (j - 16) in
//   bytes 16..31; the scale of block 0 (k 0..31) is byte 0 of the scale operand of lanes h = 0, that of block 1 (k 32..63) byte 0 of
//   lanes h = 1 (OPSEL left 0).  Loading each lane's 32 bytes as ONE contiguous run put k 16..31 under block 0's scale (measured).
//   C/D: the bf16 32x32 map (mfma.h).
// Scales reach the lanes as one dword per fragment row and K tile (the 4 block scales of the row's 128 elements) through ordinary global
// loads issued a K tile ahead; their wait is forced behind the tile's vmcnt(0) drain, where it costs nothing.
#include "gemm_pp.h"

using namespace wf;

namespace {

// ---- quantizer ---------------------------------------------------------------------------------------------------------------------------
// One lane per 16-byte chunk (8 elements), four lanes per block: the block amax is two xor-shuffles.  amax is taken on the bf16 magnitude
// bits (for non-negative finite values the integer order is the float order; NaN / Inf are >= 0x7f80).  With amax = 1.m * 2^E,
// amax / 2^(E-8) = 1.m * 256 <= 448 iff m <= 0.75 (mantissa field <= 96): e = E - 8 + (field > 96), clamped to the E8M0 range [-127, 127];
// bf16 denormals and zero blocks clamp to e = -127 (scale byte 0).  A block holding a NaN or an Inf gets the E8M0 NaN scale (0xff) and
// e4m3 NaN elements (0x7f): a non-finite input gives a non-finite product, never a clamped one.
__global__ __launch_bounds__(256) void k_mx_quant(const uint16_t* __restrict__ X, uint8_t* __restrict__ Q, uint8_t* __restrict__ S, int M,
                                                  int K, int ldx) {
  const int cpr = K >> 3;  // chunks per row (a multiple of 4: whole blocks never straddle a row or a wave)
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)M * cpr) return;  // the 4 lanes of a block leave together
  const int row = (int)(t / cpr), c = (int)(t % cpr);
  const u32x4 v = *reinterpret_cast<const u32x4*>(X + (size_t)row * ldx + (size_t)c * 8);
  uint32_t amax = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) amax = max(amax, max(v[q] & 0x7fffu, (v[q] >> 16) & 0x7fffu));
  amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1, 64));
  amax = max(amax, (uint32_t)__shfl_xor((int)amax, 2, 64));
  u32x2 pk;
  int sbyte;
  if (amax >= 0x7f80u) {
    sbyte = 0xff;
    pk = u32x2{0x7f7f7f7fu, 0x7f7f7f7fu};
  } else {
    const int eb = (int)(amax >> 7), mb = (int)(amax & 0x7f);
    const int e = eb == 0 ? -127 : max(eb - 135 + (mb > 96 ? 1 : 0), -127);
    sbyte = e + 127;
    const float inv = __uint_as_float((uint32_t)(127 - e) << 23);  // 2^-e, exact (127 - e in [7, 254])
    float f[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f[2 * q] = __uint_as_float(v[q] << 16) * inv;
      f[2 * q + 1] = __uint_as_float(v[q] & 0xffff0000u) * inv;
    }
    // v_cvt_pk_fp8_f32: two f32 -> two e4m3fn (round to nearest even) into the low (false) or high (true) 16 bits of the old value
    int w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w0, true);
    int w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], w1, true);
    pk = u32x2{(uint32_t)w0, (uint32_t)w1};
  }
  *reinterpret_cast<u32x2*>(Q + (size_t)row * K + (size_t)c * 8) = pk;
  if ((c & 3) == 0) S[(size_t)row * (K >> 5) + (c >> 2)] = (uint8_t)sbyte;
}

// ---- GEMM --------------------------------------------------------------------------------------------------------------------------------
struct MxArgs {
  const uint8_t* X;   // [M, ldx] e4m3
  const uint8_t* Xs;  // [M, K/32] E8M0
  const uint8_t* W;   // [N, ldw] e4m3
  const uint8_t* Ws;  // [N, K/32] E8M0
  const float* bias;  // [N] or null
  void* out;          // bf16 / f32 [M, ldo]
  const float* gate;  // [N] f32 (EPI_RESID) or null
  int M, N, K, ldx, ldw, ldo;
  int mt, nt;
};

typedef __attribute__((ext_vector_type(8))) int i32x8;

constexpr int PKB = PP_ROW;  // K elements (= bytes) per K tile

template <int EPI, int NI>
__global__ __launch_bounds__(PP_THREADS, 2) void k_gemm_mx(MxArgs a) {
  using G = PPGeom<NI>;
  constexpr int NJ = G::NJ, W_TILE = G::W_TILE, BUF = G::BUF;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int tm, tn;
  if (!tile_of<PP_SUPER>(a.mt, a.nt, tm, tn)) return;
  const int m0 = tm * PP_M, n0 = tn * G::PNT;
  const PPWave<NI> w;
  const int l31 = w.l31, hi = w.hi, wf0 = w.wf0, wt0 = w.wt0;
  const int nk = a.K / PKB;
  const PPDma<NI> dma(a.W, a.X, a.N, a.M, a.ldw, a.ldx, n0, m0, nk, smem, w);

  // ---- block scales: per fragment row one dword per K tile (blocks 4kt .. 4kt+3 of the row) ----------------------------------------
  const int srow = a.K >> 5;  // scale bytes per row (K % 128 == 0: dword aligned)
  const uint32_t* sptrW[NI];
  const uint32_t* sptrX[NJ];
#pragma unroll
  for (int i = 0; i < NI; ++i) sptrW[i] = reinterpret_cast<const uint32_t*>(a.Ws + (size_t)min(n0 + wf0 + i * 32 + l31, a.N - 1) * srow);
#pragma unroll
  for (int jx = 0; jx < NJ; ++jx) sptrX[jx] = reinterpret_cast<const uint32_t*>(a.Xs + (size_t)min(m0 + wt0 + jx * 32 + l31, a.M - 1) * srow);
  uint32_t scW[NI], scX[NJ], snW[NI], snX[NJ];
  auto load_scales = [&](int kt) {
    const int k = min(kt, nk - 1);
#pragma unroll
    for (int i = 0; i < NI; ++i) snW[i] = sptrW[i][k];
#pragma unroll
    for (int jx = 0; jx < NJ; ++jx) snX[jx] = sptrX[jx][k];
  };
  // the next tile's scales are complete behind a vmcnt(0) drain: a register use here makes the compiler place its wait for them at this
  // point (free), not in front of the next MFMA phase (where it would also wait for the LDS-DMA pieces in flight)
  auto settle_scales = [&]() {
#pragma unroll
    for (int i = 0; i < NI; ++i) asm volatile("" ::"v"(snW[i]));
#pragma unroll
    for (int jx = 0; jx < NJ; ++jx) asm volatile("" ::"v"(snX[jx]));
  };
  auto take_scales = [&]() {
#pragma unroll
    for (int i = 0; i < NI; ++i) scW[i] = snW[i];
#pragma unroll
    for (int jx = 0; jx < NJ; ++jx) scX[jx] = snX[jx];
  };

  const int sw = (l31 >> 1) & 7;
  const int offW = (wf0 + l31) * 128, offX = W_TILE + (wt0 + l31) * 128;
  f32x16 acc[NI][NJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int jx = 0; jx < NJ; ++jx)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][jx][r] = 0.f;

  // half `half` of a K tile = k-step of 64 elements = 16-byte chunks 4h .. 4h+3 of the row: lane (l31, hi) takes chunk 4h + hi into bytes
  // 0..15 and chunk 4h + 2 + hi into bytes 16..31 (the instruction's k order above), so that k 0..31 of the step is memory block 2h
  i32x8 fw[NI], fx[NJ];
  auto read_half = [&](int kt, int half) {
    const unsigned char* base = smem + (kt & 1) * BUF;
    const int c0 = 4 * half + hi;
    const int o0 = (c0 ^ sw) << 4, o1 = ((c0 + 2) ^ sw) << 4;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const u32x4 p0 = *reinterpret_cast<const u32x4*>(base + offW + i * 4096 + o0);
      const u32x4 p1 = *reinterpret_cast<const u32x4*>(base + offW + i * 4096 + o1);
      fw[i] = i32x8{(int)p0[0], (int)p0[1], (int)p0[2], (int)p0[3], (int)p1[0], (int)p1[1], (int)p1[2], (int)p1[3]};
    }
#pragma unroll
    for (int jx = 0; jx < NJ; ++jx) {
      const u32x4 p0 = *reinterpret_cast<const u32x4*>(base + offX + jx * 4096 + o0);
      const u32x4 p1 = *reinterpret_cast<const u32x4*>(base + offX + jx * 4096 + o1);
      fx[jx] = i32x8{(int)p0[0], (int)p0[1], (int)p0[2], (int)p0[3], (int)p1[0], (int)p1[1], (int)p1[2], (int)p1[3]};
    }
  };
  // lanes hi = 0 / 1 supply the scale of the step's first / second block, memory block 2*half + hi of the tile's four: shifted into byte 0
  auto mma = [&](int i, int jx, int half) {
    const int sh = 16 * half + 8 * hi;
    acc[i][jx] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fw[i], fx[jx], acc[i][jx], 0, 0, 0, (int)(scW[i] >> sh), 0,
                                                                 (int)(scX[jx] >> sh));
  };
  auto mma_half_dma = [&](int half, int kt_next) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int jx = 0; jx < NJ; ++jx) {
        mma(i, jx, half);
        dma.gap(i * NJ + jx, kt_next);
      }
    __builtin_amdgcn_s_setprio(0);
  };
  auto mma_half = [&](int half) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int jx = 0; jx < NJ; ++jx) mma(i, jx, half);
    __builtin_amdgcn_s_setprio(0);
  };
  static_assert(NI * NJ >= 2 * (G::NP - PPDma<NI>::RS), "not enough MFMA gaps for the DMA pieces");

  load_scales(0);
  dma.tile(0);
  pp_drain();
  settle_scales();
  pp_bar();
  // Phases as k_gemm_pp (gemm.hip): group A runs R0 M0 R1 M1 per K tile, group B the same one phase later, phase-locked by barriers
  if (!w.groupB) {
    for (int kt = 0; kt < nk; ++kt) {
      take_scales();
      read_half(kt, 0);
      dma.rphase(kt + 1);
      load_scales(kt + 1);
      pp_bar();  // 4kt+1
      mma_half_dma(0, kt + 1);
      pp_bar();  // 4kt+2
      read_half(kt, 1);
      pp_bar();  // 4kt+3
      mma_half(1);
      pp_drain();
      settle_scales();
      pp_bar();  // 4kt+4
    }
    pp_bar();
  } else {
    if (nk > 1) dma.tile(1);
    pp_bar();  // 1
    for (int kt = 0; kt < nk; ++kt) {
      take_scales();
      read_half(kt, 0);
      if (kt > 0) dma.rphase(kt + 1);
      load_scales(kt + 1);
      pp_bar();  // 4kt+2
      mma_half(0);
      pp_bar();  // 4kt+3
      read_half(kt, 1);
      pp_drain();
      settle_scales();
      pp_bar();  // 4kt+4
      mma_half_dma(1, kt + 2);
      pp_bar();  // 4kt+5
    }
    pp_drain();
  }

  pp_epilogue<EPI, NI, false>(acc, smem + w.wid * G::STG, m0 + wt0, n0 + wf0, PPEpiArgs{a.bias, a.gate, a.out, a.M, a.N, a.ldo, 1.0f});
}

template <int EPI, int NI>
void launch_mx(MxArgs a, hipStream_t s) {
  using G = PPGeom<NI>;
  a.mt = ceil_div(a.M, PP_M);
  a.nt = ceil_div(a.N, G::PNT);
  hipLaunchKernelGGL((k_gemm_mx<EPI, NI>), dim3(tile_grid<PP_SUPER>(a.mt, a.nt)), dim3(PP_THREADS), G::LDS, s, a);
}

// The 256-feature tile only: the 320-feature geometry (NI = 5) needs more than the 256 VGPRs of two waves per SIMD once the scale
// registers are added (it spilled), so every N takes NI = 2.
template <int EPI>
void launch_mx_any(const MxArgs& a, hipStream_t s) {
  launch_mx<EPI, 2>(a, s);
}

}  // namespace

extern "C" int wf_mx_quant_e4m3(const void* X, void* Q, void* S, int M, int K, int ldx, void* stream) {
  WF_CHECK_ARG(X && Q && S, "wf_mx_quant_e4m3: null pointer");
  WF_CHECK_ARG(M > 0 && K > 0, "wf_mx_quant_e4m3: empty problem M=%d K=%d", M, K);
  WF_CHECK_ARG(K % 32 == 0 && ldx % 8 == 0 && ldx >= K, "wf_mx_quant_e4m3: K (%d) must be a multiple of 32, ldx (%d) a multiple of 8 >= K", K, ldx);
  WF_CHECK_ARG(((uintptr_t)X & 15) == 0 && ((uintptr_t)Q & 7) == 0, "wf_mx_quant_e4m3: X must be 16-byte and Q 8-byte aligned");
  const long threads = (long)M * (K / 8);
  WF_CHECK_ARG(threads / 256 < (1L << 31), "wf_mx_quant_e4m3: problem too large");
  hipLaunchKernelGGL(k_mx_quant, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)X, (uint8_t*)Q,
                     (uint8_t*)S, M, K, ldx);
  WF_LAUNCH_CHECK("wf_mx_quant_e4m3");
  return WF_OK;
}

extern "C" int wf_gemm_mxfp8(const void* Xq, const void* Xs, const void* Wq, const void* Ws, const float* bias, void* out, const float* gate,
                             int M, int N, int K, int ldx, int ldw, int ldo, int epilogue, void* stream) {
  WF_CHECK_ARG(Xq && Xs && Wq && Ws && out, "wf_gemm_mxfp8: null pointer");
  WF_CHECK_ARG(epilogue >= EPI_BF16 && epilogue <= EPI_RESID, "wf_gemm_mxfp8: unknown epilogue %d (0..3)", epilogue);
  WF_CHECK_ARG(M > 0 && N > 0 && K > 0, "wf_gemm_mxfp8: empty problem M=%d N=%d K=%d", M, N, K);
  WF_CHECK_ARG(K % PKB == 0, "wf_gemm_mxfp8: K (%d) must be a multiple of 128", K);
  WF_CHECK_ARG(ldx % 16 == 0 && ldw % 16 == 0 && ldx >= K && ldw >= K, "wf_gemm_mxfp8: ldx (%d), ldw (%d) must be multiples of 16 with ld >= K", ldx,
               ldw);
  WF_CHECK_ARG(N % 4 == 0 && ldo % 4 == 0 && ldo >= N, "wf_gemm_mxfp8: N (%d) and ldo (%d) must be multiples of 4 with ldo >= N", N, ldo);
  WF_CHECK_ARG((((uintptr_t)Xq | (uintptr_t)Wq | (uintptr_t)out | (uintptr_t)bias | (uintptr_t)gate) & 15) == 0,
               "wf_gemm_mxfp8: operand, output, bias and gate pointers must be 16-byte aligned");
  WF_CHECK_ARG((((uintptr_t)Xs | (uintptr_t)Ws) & 3) == 0, "wf_gemm_mxfp8: scale pointers must be 4-byte aligned");
  // the LDS-DMA addresses a row's bytes by a 32-bit offset from Xq / Wq
  WF_CHECK_ARG((size_t)M * ldx < (1ull << 32) && (size_t)N * ldw < (1ull << 32), "wf_gemm_mxfp8: operand larger than 4 GiB");
  MxArgs a;
  a.X = (const uint8_t*)Xq;
  a.Xs = (const uint8_t*)Xs;
  a.W = (const uint8_t*)Wq;
  a.Ws = (const uint8_t*)Ws;
  a.bias = bias;
  a.out = out;
  a.gate = gate;
  a.M = M; a.N = N; a.K = K; a.ldx = ldx; a.ldw = ldw; a.ldo = ldo;
  a.mt = a.nt = 0;
  hipStream_t s = (hipStream_t)stream;
  switch (epilogue) {
    case EPI_BF16: launch_mx_any<EPI_BF16>(a, s); break;
    case EPI_BF16_GELU: launch_mx_any<EPI_BF16_GELU>(a, s); break;
    case EPI_F32: launch_mx_any<EPI_F32>(a, s); break;
    default: launch_mx_any<EPI_RESID>(a, s); break;
  }
  WF_LAUNCH_CHECK("wf_gemm_mxfp8");
  return WF_OK;
}
