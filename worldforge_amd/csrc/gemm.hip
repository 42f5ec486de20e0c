// bf16 MFMA GEMM for the DiT / VAE linear layers:  out[M,N] = epilogue( X[M,K] . W[N,K]^T + bias[N] )
//
// Replaces every nn.Linear of wan/modules/model.py (q/k/v/o :123-126, ffn :271-273, embeddings :456-464, head :332) and
// the 1x1 convolutions of wan/modules/vae.py (:199, :234-235).  MFMA-bound (2*M*N*K flop).
//
// Design (gfx950, 64-lane waves):
//   * workgroup tile 128(tokens) x 128(features), BK = 64, 4 waves in a 2x2 grid, each wave 64x64 = 2x2 MFMA 32x32x16 tiles;
//     the WEIGHT rows are the MFMA A operand and the TOKEN rows the B operand, so each lane ends up owning one token row
//     and quads of consecutive output features (see mfma.h) -> 8/16-byte epilogue stores and vector bias / gate loads;
//   * both operands are K-contiguous (nn.Linear stores W as [N,K]); tiles are staged global -> VGPR -> LDS with 16-byte
//     accesses, next tile's global loads issued before the current tile's MFMAs and written to the other LDS buffer
//     after them (one barrier per K tile);
//   * LDS rows are 128 B; 16-byte chunk c of row r lives at chunk c ^ ((r >> 1) & 7): conflict-free for the
//     ds_read_b128 lane groups of the fragment reads and for the ds_write_b128 staging writes;
//   * XCD-aware rasterisation: workgroups of one XCD (blockIdx % 8) walk 8x8 super-tiles so that the 32 CUs sharing an
//     L2 re-use the same 8 token panels and 8 weight panels;
//   * ragged M / N are handled by clamping load rows and predicating stores; K tail chunks are zero-filled (K % 8 == 0).
#include "common.h"
#include "gemm_pp.h"
#include "mfma.h"
#include <stdlib.h>

using namespace wf;

namespace {

constexpr int BM = 128;  // token rows per workgroup tile
constexpr int BN = 128;  // output features per workgroup tile
constexpr int BK = 64;
constexpr int NTHREADS = 256;
constexpr int ROW_BYTES = BK * 2;             // 128
constexpr int TILE_BYTES = BM * ROW_BYTES;    // 16 KiB per operand tile
constexpr int CHUNKS_PER_THREAD = (BM * 8) / NTHREADS;  // 4 x 16-byte chunks per operand per thread

struct GemmArgs {
  const uint16_t* X;  // [M, ldx] bf16
  const uint16_t* W;  // [N, K] bf16
  const float* bias;  // [N] or null
  void* out;          // bf16 / f32 [M, ldo]
  const float* gate;  // [N] f32 (EPI_RESID) or null
  int M, N, K, ldx, ldw, ldo;
  int mt, nt;  // tile counts
  // batched launches of k_gemm (blockIdx.y = batch b): X, W, out of problem b start b * bsx / bsw / bso ELEMENTS further (0 = not batched)
  long bsx, bsw, bso;
  int f16;  // X, W and a 16-bit output are fp16 instead of bf16 (wf_gemm_f16: the VAE's fp16 operand formats)
  int batch;  // gridDim.y of a batched launch (1 otherwise)
  float acc_scale;  // F16 instantiations only: out = epilogue(acc * acc_scale + bias) -- 2^-k when the fp16 weight operand is stored scaled by 2^k
};

__device__ __forceinline__ int swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

template <int EPI, bool F16 = false>
__global__ __launch_bounds__(NTHREADS, 2) void k_gemm(GemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int tm, tn;
  if (!tile_of<8>(a.mt, a.nt, tm, tn)) return;  // 8 x 8 super-tiles
  const int m0 = tm * BM, n0 = tn * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int wn = wid >> 1, wm = wid & 1;  // wave's 64x64 sub-tile: features wn*64.., tokens wm*64..
  const int l31 = lane & 31, hi = lane >> 5;

  // LDS: [buf0: W tile | X tile][buf1: W tile | X tile]

  // ---- staging geometry: chunk id = tid + 256*i -> (row = id >> 3, chunk = id & 7) ----------------------------------
  const int kchunks = a.K >> 3;
  u32x4 rW[CHUNKS_PER_THREAD], rX[CHUNKS_PER_THREAD];
  const uint16_t* pW[CHUNKS_PER_THREAD];
  const uint16_t* pX[CHUNKS_PER_THREAD];
  int ldsoff[CHUNKS_PER_THREAD];
  const int ck = tid & 7;
#pragma unroll
  for (int i = 0; i < CHUNKS_PER_THREAD; ++i) {
    int row = (tid >> 3) + 32 * i;
    int wr = min(n0 + row, a.N - 1);
    int xr = min(m0 + row, a.M - 1);
    pW[i] = a.W + (size_t)blockIdx.y * a.bsw + (size_t)wr * a.ldw + ck * 8;
    pX[i] = a.X + (size_t)blockIdx.y * a.bsx + (size_t)xr * a.ldx + ck * 8;
    ldsoff[i] = row * ROW_BYTES + swz(row, ck) * 16;
  }
  bool stage_ok = true;
  auto gload = [&](int kt) {
    // K-tail chunks (only in the last K tile of a K % 64 != 0 problem) must read as zero.  The load always targets a valid
    // (clamped) address and the zero-select is applied when the registers are written to LDS, AFTER the MFMAs of the current
    // tile: neither exec-mask branches nor an early use of the load result sit between the load issue and those MFMAs.
    const int kc = kt * 8 + ck;
    stage_ok = kc < kchunks;
    const size_t koff = (size_t)min(kc, kchunks - 1) * 8 - (size_t)ck * 8;
#pragma unroll
    for (int i = 0; i < CHUNKS_PER_THREAD; ++i) {
      rW[i] = *reinterpret_cast<const u32x4*>(pW[i] + koff);
      rX[i] = *reinterpret_cast<const u32x4*>(pX[i] + koff);
    }
  };
  auto lstore = [&](int buf) {
    const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < CHUNKS_PER_THREAD; ++i) {
      *reinterpret_cast<u32x4*>(smem + buf * (2 * TILE_BYTES) + ldsoff[i]) = stage_ok ? rW[i] : z;
      *reinterpret_cast<u32x4*>(smem + buf * (2 * TILE_BYTES) + TILE_BYTES + ldsoff[i]) = stage_ok ? rX[i] : z;
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int jn = 0; jn < 2; ++jn)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][jn][r] = 0.f;

  // fragment row offsets (constant over K)
  int offW[2], offX[2], rswW[2], rswX[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int rw = wn * 64 + i * 32 + l31;
    int rx = wm * 64 + i * 32 + l31;
    offW[i] = rw * ROW_BYTES;
    offX[i] = rx * ROW_BYTES;
    rswW[i] = (rw >> 1) & 7;
    rswX[i] = (rx >> 1) & 7;
  }

  const int nk = (a.K + BK - 1) / BK;
  gload(0);
  lstore(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    const unsigned char* sWb = smem + buf * (2 * TILE_BYTES);
    const unsigned char* sXb = sWb + TILE_BYTES;
    if (kt + 1 < nk) gload(kt + 1);
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      const int c = 2 * s + hi;
      u32x4 fw[2], fx[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fw[i] = *reinterpret_cast<const u32x4*>(sWb + offW[i] + ((c ^ rswW[i]) << 4));
        fx[i] = *reinterpret_cast<const u32x4*>(sXb + offX[i] + ((c ^ rswX[i]) << 4));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jn = 0; jn < 2; ++jn) acc[i][jn] = mfma32t<F16>(fw[i], fx[jn], acc[i][jn]);
    }
    if (kt + 1 < nk) lstore(buf ^ 1);
    __syncthreads();
  }

  // ---- epilogue: lane owns token row (m) and feature quads -----------------------------------------------------------
#pragma unroll
  for (int jn = 0; jn < 2; ++jn) {
    const int m = m0 + wm * 64 + jn * 32 + l31;
    if (m >= a.M) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + wn * 64 + i * 32 + 8 * g + 4 * hi;
        if (n >= a.N) continue;
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = F16 ? acc[i][jn][4 * g + q] * a.acc_scale : acc[i][jn][4 * g + q];
        if (a.bias) {
          const f32x4 bb = *reinterpret_cast<const f32x4*>(a.bias + n);
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] += bb[q];
        }
        const size_t o = (size_t)m * a.ldo + n;
        if constexpr (EPI == EPI_BF16 || EPI == EPI_BF16_GELU) {
          if constexpr (EPI == EPI_BF16_GELU) {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = gelu_tanh(v[q]);
          }
          u32x2 pk;
          if constexpr (F16)
            pk = u32x2{pack_f16x2(v[0], v[1]), pack_f16x2(v[2], v[3])};
          else
            pk = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
          *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(a.out) + (size_t)blockIdx.y * a.bso + o) = pk;
        } else if constexpr (EPI == EPI_F32) {
          f32x4 ov = {v[0], v[1], v[2], v[3]};
          *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.out) + (size_t)blockIdx.y * a.bso + o) = ov;
        } else if constexpr (EPI == EPI_F32_ACC) {
          float* po = reinterpret_cast<float*>(a.out) + (size_t)blockIdx.y * a.bso + o;
          f32x4 old = *reinterpret_cast<const f32x4*>(po);
          f32x4 ov = {old[0] + v[0], old[1] + v[1], old[2] + v[2], old[3] + v[3]};
          *reinterpret_cast<f32x4*>(po) = ov;
        } else {  // EPI_RESID: x += (acc + bias) * gate   (model.py:306, 310, 313)
          float* po = reinterpret_cast<float*>(a.out) + (size_t)blockIdx.y * a.bso + o;
          f32x4 old = *reinterpret_cast<const f32x4*>(po);
          f32x4 gg = {1.f, 1.f, 1.f, 1.f};
          if (a.gate) gg = *reinterpret_cast<const f32x4*>(a.gate + n);
          f32x4 ov = {old[0] + v[0] * gg[0], old[1] + v[1] * gg[1], old[2] + v[2] * gg[2], old[3] + v[3] * gg[3]};
          *reinterpret_cast<f32x4*>(po) = ov;
        }
      }
    }
  }
}


// ------------------------------------------------------------------------------------------------------------------
// Large-problem variant: 256 x 256 tile, 8 waves (2 token-halves x 4 feature-quarters, wave tile 128 tokens x 64 features =
// 4 x 2 MFMA 32x32x16 tiles), BK = 64, LDS-DMA staging into a double buffer (128 KiB), two-group ping-pong schedule.
//
// Each K tile is processed in four phases per wave: R0 (LDS reads of k-steps 0,1 -> 12 fragment quads), M0 (16 MFMAs, registers
// only), R1, M1.  Waves 0-3 (group A) and 4-7 (group B, one wave of each group per SIMD) run the same phase sequence ONE PHASE
// APART, phase-locked by raw s_barrier, so that on every SIMD one wave's MFMA phase always coincides with the other wave's
// LDS-read / DMA-issue phase: the matrix pipe never waits for LDS latency.  All waves issue the LDS-DMA of tile t+1 right after
// barrier 4t (its buffer was last read two intervals earlier) and drain it (vmcnt(0)) before barrier 4t+4.
// Requirements: K % 64 == 0 (no K tail in the DMA path); ragged M / N handled by clamped source rows + predicated stores.
// ------------------------------------------------------------------------------------------------------------------
#ifndef WF_GEMM_ABLATE
#define WF_GEMM_ABLATE 0  // lab only (tools/gemm_pp_cycles.py, wrong results): 1 no LDS-DMA pieces in the K loop of k_gemm_pp, 2 only the K tile's
#endif                    // last barrier (no phase hand-over barriers), 4 no LDS fragment reads in the loop, 8 no s_setprio around the MFMA phases
// Removed: WF_GEMM_DMA_PHASE 0 and 1, two rejected placements of a wave's LDS-DMA pieces of the next K tile (what is built: PPDma, gemm_pp.h).
// 0 (rounds 1-3): all in the gaps of its MFMA phase through the builtin, ~60 issue cycles per piece where an MFMA leaves ~12 free -- 42 pipe
// cycles lost per piece, 12.7 % of the K loop.  1: all in the wave's own READ phase, which then outlasts the partner's MFMA phase (K loop
// 84.5 -> 70 % of the pipe).  Both are measured in profiles/r4_f_gemm_ablate.md; source last present at ab940ba.
#ifdef WF_GEMM_TIMING
// lab builds (WF_EXTRA_HIPCC_FLAGS=-DWF_GEMM_TIMING): slots [0..7] belonged to k_gemm_w4 (removed in round 5); k_gemm_pp adds, per workgroup (its
// wave 0): [8] prologue, [9] K loop, [10] epilogue shader cycles, [11] workgroups, [12] cycles of wave 4 (group B) K loop
__device__ unsigned long long g_gemm_cycles[16];
#endif
constexpr int PK = 64;  // K elements per K tile (PP_ROW bytes)

template <int EPI, int NI, bool F16 = false>
__global__ __launch_bounds__(PP_THREADS, 2) void k_gemm_pp(GemmArgs a) {
  using G = PPGeom<NI>;
  constexpr int NJ = G::NJ, W_TILE = G::W_TILE, BUF = G::BUF;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // batched launch (wf_gemm_*_batched): problem blockIdx.y starts bsx / bsw / bso ELEMENTS further (all zero, and gridDim.y = 1, otherwise)
  a.X += (size_t)blockIdx.y * a.bsx;
  a.W += (size_t)blockIdx.y * a.bsw;
  a.out = reinterpret_cast<unsigned char*>(a.out) + (size_t)blockIdx.y * a.bso * ((EPI == EPI_BF16 || EPI == EPI_BF16_GELU) ? 2 : 4);
  int tm, tn;
  if (!tile_of<PP_SUPER>(a.mt, a.nt, tm, tn)) return;
  const int m0 = tm * PP_M, n0 = tn * G::PNT;
  const PPWave<NI> w;
  const int nk = a.K / PK;
  const PPDma<NI> dma(a.W, a.X, a.N, a.M, a.ldw * 2, a.ldx * 2, n0, m0, nk, smem, w);

  // ---- fragment addressing ------------------------------------------------------------------------------------------------
  // every fragment row of a wave is its lane's row l31 plus a multiple of 32: one swizzle term serves all of them
  const int sw = (w.l31 >> 1) & 7;
  const int offW = (w.wf0 + w.l31) * 128, offX = W_TILE + (w.wt0 + w.l31) * 128;
  f32x16 acc[NI][NJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int jx = 0; jx < NJ; ++jx)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][jx][r] = 0.f;

  u32x4 fw[2][NI], fx[2][NJ];
  auto read_half = [&](int kt, int half) {
    const unsigned char* base = smem + (kt & 1) * BUF;
    if ((WF_GEMM_ABLATE & 4) && kt > 0) return;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int c = ((2 * (2 * half + ks) + w.hi) ^ sw) << 4;
#pragma unroll
      for (int i = 0; i < NI; ++i) fw[ks][i] = *reinterpret_cast<const u32x4*>(base + offW + i * 4096 + c);
#pragma unroll
      for (int jx = 0; jx < NJ; ++jx) fx[ks][jx] = *reinterpret_cast<const u32x4*>(base + offX + jx * 4096 + c);
    }
  };
  // 2*NI*NJ MFMAs on register operands; in mma_half_dma the pieces of tile `kt_next` that the read phase left over ride in the gaps.  Each
  // phase is compile-time ONE code path: the caller does not branch between the two
  auto mma_half_dma = [&](int kt_next) {
    if (!(WF_GEMM_ABLATE & 8)) __builtin_amdgcn_s_setprio(1);  // the MFMA phase outranks the co-resident wave's LDS phase at the issue arbiter
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int jx = 0; jx < NJ; ++jx) {
          acc[i][jx] = mfma32t<F16>(fw[ks][i], fx[ks][jx], acc[i][jx]);
          if (!(WF_GEMM_ABLATE & 1)) dma.gap((ks * NI + i) * NJ + jx, kt_next);
        }
    __builtin_amdgcn_s_setprio(0);
  };
  auto mma_half = [&]() {
    if (!(WF_GEMM_ABLATE & 8)) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int jx = 0; jx < NJ; ++jx) acc[i][jx] = mfma32t<F16>(fw[ks][i], fx[ks][jx], acc[i][jx]);
    __builtin_amdgcn_s_setprio(0);
  };
  auto rphase_pieces = [&](int kt_next) {
    if (!(WF_GEMM_ABLATE & 1)) dma.rphase(kt_next);
  };
  auto pbar = [&]() {  // a phase hand-over barrier (lab: WF_GEMM_ABLATE & 2 drops them, keeping the K tile's buffer hand-over)
    if (!(WF_GEMM_ABLATE & 2)) pp_bar();
  };

#ifdef WF_GEMM_TIMING
  const unsigned long long tt0 = __builtin_readcyclecounter();
#endif
  dma.tile(0);
  pp_drain();
  pp_bar();
#ifdef WF_GEMM_TIMING
  const unsigned long long tt1 = __builtin_readcyclecounter();
#endif
  if (!w.groupB) {
    for (int kt = 0; kt < nk; ++kt) {
      read_half(kt, 0);
      rphase_pieces(kt + 1);
      pbar();  // 4kt+1
      mma_half_dma(kt + 1);  // the pieces of tile kt+1 ride in the MFMA gaps (its buffer is free since barrier 4kt)
      pbar();  // 4kt+2
      read_half(kt, 1);
      pbar();  // 4kt+3
      mma_half();
      pp_drain();
      pp_bar();  // 4kt+4
    }
    pp_bar();
  } else {
    if (nk > 1) dma.tile(1);
    pp_bar();  // 1
    for (int kt = 0; kt < nk; ++kt) {
      read_half(kt, 0);
      if (kt > 0) rphase_pieces(kt + 1);  // group B's share of tile kt+1 that its previous MFMA phase (in phase 1) left over; tile 1 came whole from the prologue
      pbar();  // 4kt+2
      mma_half();
      pbar();  // 4kt+3
      read_half(kt, 1);
      pp_drain();
      pp_bar();  // 4kt+4
      mma_half_dma(kt + 2);
      pbar();  // 4kt+5
    }
    pp_drain();  // the dummy pieces of the last two phases
  }

#ifdef WF_GEMM_TIMING
  const unsigned long long tt2 = __builtin_readcyclecounter();
#endif
  pp_epilogue<EPI, NI, F16>(acc, smem + w.wid * G::STG, m0 + w.wt0, n0 + w.wf0, PPEpiArgs{a.bias, a.gate, a.out, a.M, a.N, a.ldo, a.acc_scale});
#ifdef WF_GEMM_TIMING
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the epilogue's stores have left the wave
  const unsigned long long tt3 = __builtin_readcyclecounter();
  if (w.lane == 0 && w.wid == 0) {
    atomicAdd(&g_gemm_cycles[8], tt1 - tt0);
    atomicAdd(&g_gemm_cycles[9], tt2 - tt1);
    atomicAdd(&g_gemm_cycles[10], tt3 - tt2);
    atomicAdd(&g_gemm_cycles[11], 1ull);
  }
  if (w.lane == 0 && w.wid == 4) atomicAdd(&g_gemm_cycles[12], tt2 - tt1);
#endif
}

// ------------------------------------------------------------------------------------------------------------------
// Removed in round 5 (superseded kernels kept alive behind environment switches): `k_gemm_pp16`, the same ping-pong
// kernel on v_mfma_f32_16x16x32_bf16 (round 3, WF_GEMM_MFMA=16: +3 ... +5 % in isolated back-to-back launches, nothing in the model,
// profiles/r3_i_gemm_mfma16.md), and `k_gemm_w4`, the one-wave-per-SIMD 256 x 256 tile with all 256 accumulators in AGPRs (round 2,
// WF_GEMM_KERNEL=w4: a better K loop, the same 1200-1300 TFLOP/s, bench 0.234 vs 0.242).  Both are measured negatives documented in
// DESIGN.md section 4; their source is in the history (last present at 57ab8ba).
// ------------------------------------------------------------------------------------------------------------------

template <int EPI, int NI>
static void launch_pp(GemmArgs a, hipStream_t s) {
  using G = PPGeom<NI>;
  a.mt = ceil_div(a.M, PP_M);
  a.nt = ceil_div(a.N, G::PNT);
  const dim3 grid(tile_grid<PP_SUPER>(a.mt, a.nt), a.batch);
  if (a.f16) {  // fp16 operands: the epilogues the VAE uses (the others are rejected by wf_gemm_f16)
    if constexpr (EPI == EPI_BF16 || EPI == EPI_F32 || EPI == EPI_F32_ACC) hipLaunchKernelGGL((k_gemm_pp<EPI, NI, true>), grid, dim3(PP_THREADS), G::LDS, s, a);
  } else
    hipLaunchKernelGGL((k_gemm_pp<EPI, NI>), grid, dim3(PP_THREADS), G::LDS, s, a);
}

// 256- or 320-feature tiles: whichever leaves fewer idle workgroup slots in the last round of `n_cu` concurrent workgroups
// (ties go to the wider tile).  The result does not depend on the choice: every output element is the same sequence of MFMA
// accumulations over K in both.
static int pp_wide(int M, int N) {
  if (N % 320 != 0) return 0;
#ifdef WF_GEMM_LAB_TILE  // lab builds only: WF_GEMM_TILE=256|320 read per call, so that one process can launch both tile widths (tools/gemm_dephase.py, gemm_tiles.py)
  const char* e_ = getenv("WF_GEMM_TILE");
  const int force = e_ ? atoi(e_) : 0;
#else
  const int force = 0;
#endif
  if (force == 256) return 0;
  if (force == 320) return 1;
  static const int n_cu = [] {
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) == hipSuccess) hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    return n > 0 ? n : 256;
  }();
  const long mt = ceil_div(M, PP_M);
  const long t256 = mt * ceil_div(N, 256), t320 = mt * (N / 320);
  const long r256 = (t256 + n_cu - 1) / n_cu, r320 = (t320 + n_cu - 1) / n_cu;
  // cost ~ rounds x tile width
  return r320 * 320 <= r256 * 256;
}

// Large problems with a whole number of 64-wide K tiles take the ping-pong kernel; a batch (blockIdx.y) counts as one problem that is large
// TOGETHER (the VAE mid-block's P . V products: 6240 x 384 x 18 720 per frame, 21 frames).
// INVARIANTS relied on by k_gemm_pp: N >= 4 and N % 4 == 0 for the clamped unconditional loads of its epilogue (pp_epilogue, gemm_pp.h)
// -- a future relaxation of this gate must keep them -- and a row's bytes within a 32-bit offset from X / W for its LDS-DMA.
static bool pp_eligible(const GemmArgs& a) {
  return a.K % PK == 0 && a.M >= 1024 && a.N >= 256 && a.N % 4 == 0 && (long)a.M * a.N * a.batch >= (1L << 22) &&
         (size_t)a.M * a.ldx * 2 < (1ull << 32) && (size_t)a.N * a.ldw * 2 < (1ull << 32);
}

// The ping-pong family, 256- or 320-feature tiles (pp_wide), or the 128 x 128 register-staged k_gemm.
template <int EPI>
static void launch(const GemmArgs& a, hipStream_t s) {
  if (pp_eligible(a)) {
    pp_wide(a.M, a.N) ? launch_pp<EPI, 5>(a, s) : launch_pp<EPI, 2>(a, s);
    return;
  }
  const dim3 grid(tile_grid<8>(a.mt, a.nt), a.batch);
  if (a.f16) {  // as in launch_pp
    if constexpr (EPI == EPI_BF16 || EPI == EPI_F32 || EPI == EPI_F32_ACC) hipLaunchKernelGGL((k_gemm<EPI, true>), grid, dim3(NTHREADS), 4 * TILE_BYTES, s, a);
  } else
    hipLaunchKernelGGL(k_gemm<EPI>, grid, dim3(NTHREADS), 4 * TILE_BYTES, s, a);
}

static bool launch_epilogue(int epilogue, const GemmArgs& a, hipStream_t s) {  // false: no such epilogue
  switch (epilogue) {
    case EPI_BF16: launch<EPI_BF16>(a, s); return true;
    case EPI_BF16_GELU: launch<EPI_BF16_GELU>(a, s); return true;
    case EPI_F32: launch<EPI_F32>(a, s); return true;
    case EPI_RESID: launch<EPI_RESID>(a, s); return true;
    case EPI_F32_ACC: launch<EPI_F32_ACC>(a, s); return true;
  }
  return false;
}

static GemmArgs make_args(const void* X, const void* W, const float* bias, void* out, const float* gate, int M, int N, int K, int ldx, int ldw,
                          int ldo, int batch, long bsx, long bsw, long bso, int f16, float acc_scale) {
  return GemmArgs{(const uint16_t*)X, (const uint16_t*)W, bias, out, gate, M, N, K, ldx, ldw, ldo, ceil_div(M, BM), ceil_div(N, BN),
                  bsx, bsw, bso, f16, batch, acc_scale};
}

}  // namespace

static int gemm_impl(const void* X, const void* W, const float* bias, void* out, const float* gate, int M, int N,
                     int K, int ldx, int ldw, int ldo, int epilogue, void* stream, int f16, float acc_scale = 1.0f) {
  WF_CHECK_ARG(acc_scale > 0.0f && acc_scale < 3.0e38f, "wf_gemm_f16: acc_scale must be a positive finite number (1 = none)");
  WF_CHECK_ARG(X && W && out, "wf_gemm_bf16: null pointer");
  WF_CHECK_ARG(!f16 || epilogue == EPI_BF16 || epilogue == EPI_F32 || epilogue == EPI_F32_ACC,
               "wf_gemm_f16: epilogue %d is not built for fp16 operands (0 = 16-bit out, 2 = f32, 4 = f32 accumulate)", epilogue);
  WF_CHECK_ARG(M > 0 && N > 0 && K > 0, "wf_gemm_bf16: empty problem M=%d N=%d K=%d", M, N, K);
  WF_CHECK_ARG(K % 8 == 0 && ldx % 8 == 0 && ldw % 8 == 0 && ldw >= K && ldx >= K,
               "wf_gemm_bf16: K (%d), ldx (%d), ldw (%d) must be multiples of 8 with ld >= K", K, ldx, ldw);
  WF_CHECK_ARG(N % 4 == 0 && ldo % 4 == 0, "wf_gemm_bf16: N (%d) and ldo (%d) must be multiples of 4", N, ldo);
  WF_CHECK_ARG((((uintptr_t)X | (uintptr_t)W | (uintptr_t)out | (uintptr_t)bias | (uintptr_t)gate) & 15) == 0,
               "wf_gemm_bf16: pointers must be 16-byte aligned");
  const GemmArgs a = make_args(X, W, bias, out, gate, M, N, K, ldx, ldw, ldo, 1, 0, 0, 0, f16, acc_scale);
  WF_CHECK_ARG(launch_epilogue(epilogue, a, (hipStream_t)stream), "wf_gemm_bf16: unknown epilogue %d", epilogue);
  WF_LAUNCH_CHECK(f16 && !pp_eligible(a) ? "wf_gemm_f16" : "wf_gemm_bf16");
  return WF_OK;
}

extern "C" int wf_gemm_bf16(const void* X, const void* W, const float* bias, void* out, const float* gate, int M, int N,
                            int K, int ldx, int ldw, int ldo, int epilogue, void* stream) {
  return gemm_impl(X, W, bias, out, gate, M, N, K, ldx, ldw, ldo, epilogue, stream, 0);
}

// The same GEMM on fp16 operands (X, W fp16; epilogue 0 writes fp16): v_mfma_f32_32x32x16_f16, fp32 accumulation.  Epilogues 0 / 2 / 4.
extern "C" int wf_gemm_f16(const void* X, const void* W, const float* bias, void* out, int M, int N, int K, int ldx, int ldw, int ldo,
                           int epilogue, float acc_scale, void* stream) {
  return gemm_impl(X, W, bias, out, nullptr, M, N, K, ldx, ldw, ldo, epilogue, stream, 1, acc_scale);
}

#ifdef WF_GEMM_TIMING
extern "C" int wf_debug_gemm_cycles(unsigned long long* out16, int reset) {
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_gemm_cycles), sizeof(unsigned long long) * 16) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[16] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_gemm_cycles), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif

// `batch` independent small GEMMs in ONE launch (blockIdx.y = problem): out_b[M,N] = X_b[M,K] . W_b[N,K]^T, problem b at X + b*bsx,
// W + b*bsw, out + b*bso (elements).  Epilogue EPI_BF16 or EPI_F32, no bias / gate.
static int gemm_batched_impl(const void* X, const void* W, void* out, int batch, int M, int N, int K, int ldx, int ldw, int ldo, int64_t bsx,
                             int64_t bsw, int64_t bso, int epilogue, void* stream, int f16) {
  WF_CHECK_ARG(X && W && out, "wf_gemm_bf16_batched: null pointer");
  WF_CHECK_ARG(batch > 0 && batch <= 65535 && M > 0 && N > 0 && K > 0, "wf_gemm_bf16_batched: empty problem batch=%d M=%d N=%d K=%d", batch, M, N, K);
  WF_CHECK_ARG(K % 8 == 0 && ldx % 8 == 0 && ldw % 8 == 0 && ldw >= K && ldx >= K && bsx % 8 == 0 && bsw % 8 == 0,
               "wf_gemm_bf16_batched: K, ldx, ldw, bsx, bsw must be multiples of 8 with ld >= K");
  WF_CHECK_ARG(N % 4 == 0 && ldo % 4 == 0 && bso % 4 == 0, "wf_gemm_bf16_batched: N, ldo, bso must be multiples of 4");
  WF_CHECK_ARG((((uintptr_t)X | (uintptr_t)W | (uintptr_t)out) & 15) == 0, "wf_gemm_bf16_batched: pointers must be 16-byte aligned");
  WF_CHECK_ARG(epilogue == EPI_BF16 || epilogue == EPI_F32, "wf_gemm_bf16_batched: epilogue must be 0 (16-bit out) or 2 (f32)");
  const GemmArgs a = make_args(X, W, nullptr, out, nullptr, M, N, K, ldx, ldw, ldo, batch, bsx, bsw, bso, f16, 1.0f);
  launch_epilogue(epilogue, a, (hipStream_t)stream);
  WF_LAUNCH_CHECK("wf_gemm_bf16_batched");
  return WF_OK;
}

extern "C" int wf_gemm_bf16_batched(const void* X, const void* W, void* out, int batch, int M, int N, int K, int ldx, int ldw, int ldo,
                                    int64_t bsx, int64_t bsw, int64_t bso, int epilogue, void* stream) {
  return gemm_batched_impl(X, W, out, batch, M, N, K, ldx, ldw, ldo, bsx, bsw, bso, epilogue, stream, 0);
}

// wf_gemm_bf16_batched on fp16 operands (epilogue 0 writes fp16): the per-frame P.V products of the VAE mid-block attention in its fp16
// three-term mode, all frames in one launch (each is 147 workgroups of the 128 x 128 kernel: alone it fills a fraction of the chip)
extern "C" int wf_gemm_f16_batched(const void* X, const void* W, void* out, int batch, int M, int N, int K, int ldx, int ldw, int ldo,
                                   int64_t bsx, int64_t bsw, int64_t bso, int epilogue, void* stream) {
  return gemm_batched_impl(X, W, out, batch, M, N, K, ldx, ldw, ldo, bsx, bsw, bso, epilogue, stream, 1);
}