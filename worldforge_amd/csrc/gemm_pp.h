// What the two ping-pong GEMM kernels share: k_gemm_pp (gemm.hip, bf16 / fp16 operands) and k_gemm_mx (mxfp8.hip, MX-fp8 operands).
//
// Both run a 256-token x 256- (or 320-) feature workgroup tile on 8 waves, stage operand tiles by LDS-DMA into a double buffer and write
// the result through a transposed, wave-private LDS epilogue.  A K tile row is 128 BYTES in both (64 bf16 or 128 e4m3 elements), so the
// geometry, the swizzle and the DMA piece addressing are expressed in bytes here and know nothing of the element type.  The K loops (phase
// order, fragment reads, MFMA calls) differ in substance and stay written out in their own files.
#pragma once
#include "common.h"
#include "mfma.h"

namespace wf {

enum { EPI_BF16 = WF_EPI_BF16, EPI_BF16_GELU = WF_EPI_BF16_GELU, EPI_F32 = WF_EPI_F32, EPI_RESID = WF_EPI_RESID, EPI_F32_ACC = WF_EPI_F32_ACC };

__device__ __forceinline__ float gelu_tanh(float x) {
  // nn.GELU(approximate='tanh') (model.py:272): 0.5 x (1 + tanh(u)), u = sqrt(2/pi) (x + 0.044715 x^3).  0.5 (1 + tanh u) is the logistic
  // function of 2u, so gelu = x / (1 + exp(-2u)) = x * rcp(1 + exp2(c x (1 + 0.044715 x^2))) with c = -2 sqrt(2/pi) log2(e): six VALU and
  // two transcendentals per value where the textbook form took about twelve and two (round 4: the GELU was 13 k of the 22 k cycles of
  // the FFN-up epilogue, profiles/r4_c_gemm_pp_cycles.md).  x -> +inf: exp2 -> 0, result x; x -> -inf: exp2 -> inf, rcp -> 0, result -0.
  const float c = -2.0f * 0.7978845608028654f * 1.4426950408889634f, k1 = 0.044715f;
  const float p = __builtin_fmaf(k1, x * x, 1.0f);
  const float e = __builtin_amdgcn_exp2f((c * x) * p);
  return x * __builtin_amdgcn_rcpf(1.0f + e);
}

// ---- XCD-aware tile rasteriser ------------------------------------------------------------------------------------------------------
// Workgroups of one XCD (blockIdx.x % 8) walk super-tiles of S x S workgroup tiles (S a power of two), so that the CUs sharing an L2
// re-use the same token and weight panels.  tile_grid is the launch's gridDim.x; tile_of maps workgroup blockIdx.x to its tile (false: none, the workgroup leaves).
template <int S>
static inline int tile_grid(int mt, int nt) {
  const int nsuper = ((mt + S - 1) / S) * ((nt + S - 1) / S);
  return ((nsuper + 7) / 8) * 8 * S * S;
}
template <int S>
__device__ __forceinline__ bool tile_of(int mt, int nt, int& tm, int& tn) {
  constexpr int LG = __builtin_ctz(S);
  static_assert(S == 1 << LG, "super-tile edge must be a power of two");
  const int smt = (mt + S - 1) >> LG, snt = (nt + S - 1) >> LG;
  const int nsuper = smt * snt;
  const int b = blockIdx.x;
  const int xcd = b & 7, j = b >> 3;
  const int gid = (j >> (2 * LG)) * 8 + xcd;
  if (gid >= nsuper) return false;
  const int within = j & (S * S - 1);
  tm = (gid / snt) * S + (within >> LG);
  tn = (gid % snt) * S + (within & (S - 1));
  return tm < mt && tn < nt;
}

// ---- geometry of a ping-pong workgroup tile, in bytes ---------------------------------------------------------------------------------
// NI = 32-feature MFMA tiles per wave, NJ = 32-token MFMA tiles per wave:
//   NI = 2, NJ = 4: 256 tokens x 256 features; waves = 2 token halves (= ping-pong group) x 4 feature quarters;
//   NI = 5, NJ = 2: 256 tokens x 320 features; waves = 4 token quarters x 2 feature halves (= ping-pong group).  N = 5120 is
//   16 x 320: with 4096 / 8192 tokens per rank (8 / 4 ranks) that is exactly 1 / 2 rounds of 256 workgroups where the 256-wide tile
//   needs 1.25 / 2.5; the wider tile also reads 0.70 fragment quads per MFMA instead of 0.75.
constexpr int PP_M = 256;        // token rows per workgroup tile
constexpr int PP_ROW = 128;      // bytes of a K tile row: the LDS row, and the step of the operand pointers per K tile
constexpr int PP_THREADS = 512;
constexpr int PP_SUPER = 4;      // 4 x 4 super-tiles
template <int NI>
struct PPGeom {
  static constexpr int NJ = NI == 2 ? 4 : 2;
  static constexpr int TSPLIT = PP_M / (NJ * 32);     // waves along tokens
  static constexpr int FSPLIT = 8 / TSPLIT;           // waves along features
  static constexpr int PNT = FSPLIT * NI * 32;        // features per workgroup tile
  static constexpr int W_TILE = PNT * PP_ROW;
  static constexpr int X_TILE = PP_M * PP_ROW;
  static constexpr int BUF = W_TILE + X_TILE;
  static constexpr int NWP = PNT / 64;                // 1 KiB W pieces per wave
  static constexpr int NP = NWP + 4;                  // LDS-DMA pieces per wave per K tile
  static constexpr int STG_ROW = 144;                 // epilogue staging row stride (see pp_epilogue)
  static constexpr int STG = NJ * 32 * STG_ROW;       // epilogue staging bytes per wave
  // + a 1 KiB dummy LDS-DMA target per wave BEHIND both uses of the rest: for NI = 2 the epilogue staging (8 x 18 KiB) is larger than the
  // operand buffers, and a dummy region at 2 * BUF lay inside wave 7's staging rows -- a group-B wave's last dummy pieces could land
  // there after wave 7 had begun its epilogue (seen as a rare wrong tile when several streams shared the GPU)
  static constexpr int DUMMY = 2 * BUF > 8 * STG ? 2 * BUF : 8 * STG;
  static constexpr int LDS = DUMMY + 8 * 1024;        // the launch's dynamic LDS request
};

// ---- a wave's place in the workgroup tile ---------------------------------------------------------------------------------------------
template <int NI>
struct PPWave {
  int lane, wid, l31, hi;
  bool groupB;   // waves 4-7: the ping-pong group that runs one phase behind (one wave of each group per SIMD)
  int wf0, wt0;  // wave tile origin inside the workgroup tile: features, tokens
  __device__ __forceinline__ PPWave() {
    constexpr int NJ = PPGeom<NI>::NJ;
    const int tid = threadIdx.x;
    lane = tid & 63;
    wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    l31 = lane & 31;
    hi = lane >> 5;
    groupB = wid >= 4;
    const int wfi = NJ == 4 ? (wid & 3) : (wid >> 2);  // wave index along features
    const int wti = NJ == 4 ? (wid >> 2) : (wid & 3);  // wave index along tokens
    wf0 = wfi * NI * 32;
    wt0 = wti * NJ * 32;
  }
};

__device__ __forceinline__ void pp_bar() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}
__device__ __forceinline__ void pp_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// ---- LDS-DMA piece addressing -----------------------------------------------------------------------------------------------------------
// An operand tile = rows x 128 B = pieces of 1 KiB (8 rows); wave w moves pieces NWP*w.. of W and 4w..4w+3 of X.
// lane -> (row = 8*piece + lane/8, slot = lane%8) receives source chunk slot ^ ((row >> 1) & 7): the fragment reads undo the swizzle.
// saddr form: wave-uniform 64-bit base + per-lane BYTE offsets that are constant over K (the launcher guarantees rows * row stride < 4 GiB).
#ifndef WF_GEMM_DMA_RSPLIT
#define WF_GEMM_DMA_RSPLIT 5  // lab knob: how many of a wave's 9 (8) pieces go to the tail of its first READ phase instead of the MFMA gaps (0 -> 89.2 %, 3 -> 90.8, 5 -> 92-93.5, 6 / 7 -> 92.4, 9 -> 86.6 % of the pipe in k_gemm_pp)
#endif
template <int NI>
struct PPDma {
  using G = PPGeom<NI>;
  static constexpr int NWP = G::NWP, NP = G::NP;
  static constexpr int RS = WF_GEMM_DMA_RSPLIT < NP ? WF_GEMM_DMA_RSPLIT : NP;
  const unsigned char *W, *X;
  uint32_t voffW[NWP], voffX[4];
  uint32_t smem_base;
  int nk, wid;

  // W [N rows, ldw_bytes apart], X [M rows, ldx_bytes apart]; the workgroup tile starts at rows n0 / m0 (rows past the end are clamped)
  __device__ __forceinline__ PPDma(const void* W_, const void* X_, int N, int M, int ldw_bytes, int ldx_bytes, int n0, int m0, int nk_,
                                   const unsigned char* smem, const PPWave<NI>& w)
      : W((const unsigned char*)W_), X((const unsigned char*)X_), nk(nk_), wid(w.wid) {
    const int slot = w.lane & 7, rowW = 8 * wid * NWP + (w.lane >> 3), rowX = 8 * wid * 4 + (w.lane >> 3);  // the lane's row of piece 0
#pragma unroll
    for (int i = 0; i < NWP; ++i) {
      const int row = rowW + 8 * i;
      voffW[i] = (uint32_t)((size_t)min(n0 + row, N - 1) * ldw_bytes + (slot ^ ((row >> 1) & 7)) * 16);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = rowX + 8 * i;
      voffX[i] = (uint32_t)((size_t)min(m0 + row, M - 1) * ldx_bytes + (slot ^ ((row >> 1) & 7)) * 16);
    }
    smem_base = __builtin_amdgcn_readfirstlane(lds_offset(smem));
  }
  // Piece i (a constant after unrolling: W pieces first, then the 4 X pieces) of K tile kt.  Past the last K tile the pieces are still
  // issued (no branch in the MFMA stream, and ONE code path for the MFMA phase: two copies of it behind a branch made the register
  // allocator spill accumulators): they re-read tile nk-1 into the wave's 1 KiB of the dummy region, which nobody reads.
  __device__ __forceinline__ void piece(int i, int kt) const {
    const bool live = kt < nk;
    const int ks_ = live ? kt : nk - 1;
    const uint32_t buf = smem_base + (uint32_t)((kt & 1) * G::BUF);
    static_assert(G::DUMMY >= 2 * G::BUF && G::DUMMY >= 8 * G::STG && G::LDS >= G::DUMMY + 8 * 1024, "the dummy LDS-DMA targets overlap live LDS");
    const uint32_t dummy = smem_base + (uint32_t)(G::DUMMY + wid * 1024);
    if (i < NWP)
      glds16_saddr(W + (size_t)ks_ * PP_ROW, voffW[i], live ? buf + (uint32_t)((wid * NWP + i) * 1024) : dummy);
    else
      glds16_saddr(X + (size_t)ks_ * PP_ROW, voffX[i - NWP], live ? buf + (uint32_t)(G::W_TILE + (wid * 4 + i - NWP) * 1024) : dummy);
  }
  __device__ __forceinline__ void tile(int kt) const {  // all of the wave's pieces (the prologue)
#pragma unroll
    for (int i = 0; i < NP; ++i) piece(i, kt);
  }
  __device__ __forceinline__ void rphase(int kt_next) const {  // the first RS pieces, behind a read phase's LDS reads
#pragma unroll
    for (int i = 0; i < RS; ++i) piece(i, kt_next);
  }
  // the rest ride in the gaps of an MFMA phase, one behind every second MFMA (idx = the MFMA's index in its phase): the matrix pipe hides
  // their issue cost
  __device__ __forceinline__ void gap(int idx, int kt_next) const {
    if ((idx & 1) && (idx >> 1) < NP - RS) {
      piece(RS + (idx >> 1), kt_next);
      __builtin_amdgcn_sched_barrier(0);  // the piece stays in this gap
    }
  }
};

// ---- epilogue through LDS: row-contiguous global accesses -------------------------------------------------------------------------------
// In the accumulator layout a lane owns one token row and quads of features, so a store instruction touches 32-64 different rows
// (8 / 16 bytes each): 64 such instructions per lane made the epilogue ~20 k cycles per tile, 9 % of a K = 5120 GEMM.  Each wave
// therefore transposes its tile through a private LDS region `stg` (G::STG bytes; the operand buffers are free behind the last barrier)
// in passes of [NJ*32 tokens][128 B]  (64 16-bit features = two MFMA tiles, or 32 fp32 features = one; an odd last 16-bit tile makes a
// 64-byte pass) and reads / writes global memory in whole rows of a pass.  Rows are padded by 16 B (144-byte stride) so that neither the
// column-wise writes nor the row-wise reads conflict.  No workgroup barrier: the region is wave-private.
//
// INVARIANT: bias / gate / old-value quads are loaded UNCONDITIONALLY at clamped addresses `min(n, N - 4)` (a guard per load would put
// every load in its own basic block with its own wait), which needs N >= 4 and N % 4 == 0.  The launchers guarantee both (gemm.hip: the
// ping-pong gate; mxfp8.hip: its argument checks); a relaxation of either must keep them.
struct PPEpiArgs {
  const float* bias;  // [N] or null
  const float* gate;  // [N] (EPI_RESID) or null
  void* out;          // 16-bit / f32 [M, ldo]
  int M, N, ldo;
  float acc_scale;    // F16 only: out = epilogue(acc * acc_scale + bias)
};
// (mw, nw) = the wave tile's first token row / feature in the problem (workgroup tile origin + PPWave::wt0 / wf0)
template <int EPI, int NI, bool F16>
__device__ __forceinline__ void pp_epilogue(const f32x16 (&acc)[NI][PPGeom<NI>::NJ], unsigned char* stg, int mw, int nw, const PPEpiArgs a) {
  constexpr int NJ = PPGeom<NI>::NJ;
  constexpr int RS = PPGeom<NI>::STG_ROW;
  constexpr int ROWS = NJ * 32;
  const int lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  if constexpr (EPI == EPI_BF16 || EPI == EPI_BF16_GELU) {
#pragma unroll
    for (int i0 = 0; i0 < NI; i0 += 2) {
      const int nti = (NI - i0) >= 2 ? 2 : 1;  // feature tiles in this pass (compile-time after unrolling)
      // the pass's bias quads in one batch (one wait) -- per store group they were serialized L2 round trips; features >= N are never
      // stored, so their (clamped) bias value does not matter
      f32x4 bq[2][4];
#pragma unroll
      for (int ii = 0; ii < 2; ++ii)
#pragma unroll
        for (int g = 0; g < 4; ++g) bq[ii][g] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (a.bias) {
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
          for (int g = 0; g < 4; ++g)
            if (ii < nti) bq[ii][g] = *reinterpret_cast<const f32x4*>(a.bias + min(nw + (i0 + ii) * 32 + 8 * g + 4 * hi, a.N - 4));
      }
#pragma unroll
      for (int jx = 0; jx < NJ; ++jx)
#pragma unroll
        for (int ii = 0; ii < 2; ++ii) {
          if (ii >= nti) continue;
          const int i = i0 + ii;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int nl = ii * 32 + 8 * g + 4 * hi;  // feature within the pass
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = (F16 ? acc[i][jx][4 * g + q] * a.acc_scale : acc[i][jx][4 * g + q]) + bq[ii][g][q];
            if constexpr (EPI == EPI_BF16_GELU) {
#pragma unroll
              for (int q = 0; q < 4; ++q) v[q] = gelu_tanh(v[q]);
            }
            u32x2 pk;
            if constexpr (F16)
              pk = u32x2{pack_f16x2(v[0], v[1]), pack_f16x2(v[2], v[3])};
            else
              pk = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
            *reinterpret_cast<u32x2*>(stg + (jx * 32 + l31) * RS + nl * 2) = pk;
          }
        }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      // row phase: 8 (4) lanes x 16 B per token row, 8 (16) rows per instruction
      const int lpr = nti * 4;
      const int lrow = lane / lpr, lch = lane % lpr;
#pragma unroll
      for (int r8 = 0; r8 < ROWS * nti / 16; ++r8) {
        const int row = r8 * (64 / lpr) + lrow;
        const int m = mw + row;
        const int n = nw + i0 * 32 + lch * 8;
        const u32x4 val = *reinterpret_cast<const u32x4*>(stg + row * RS + lch * 16);
        if (m < a.M && n < a.N) {  // N % 4 == 0: a chunk of 8 features may straddle the edge -> the half-chunk store
          uint16_t* op = reinterpret_cast<uint16_t*>(a.out) + (size_t)m * a.ldo + n;
          if (n + 8 <= a.N)
            *reinterpret_cast<u32x4*>(op) = val;
          else
            *reinterpret_cast<u32x2*>(op) = u32x2{val[0], val[1]};
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the next pass overwrites the staging rows
    }
  } else {
    const int lrow = lane >> 3, lch = lane & 7;  // row phase: 8 rows x 8 chunks of 16 B per instruction
    // fp32 outputs: one pass of [NJ*32 tokens][32 features] f32 = 128 B per row for every feature tile
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      // the pass's four bias quads in one batch (one wait): tested and loaded per store group they were four serialized L2 round trips.
      // Features >= N are never stored, so their (clamped) bias value does not matter.
      f32x4 bq[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      if (a.bias) {
#pragma unroll
        for (int g = 0; g < 4; ++g) bq[g] = *reinterpret_cast<const f32x4*>(a.bias + min(nw + i * 32 + 8 * g + 4 * hi, a.N - 4));
      }
#pragma unroll
      for (int jx = 0; jx < NJ; ++jx)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int nl = 8 * g + 4 * hi;
          const float sc = F16 ? a.acc_scale : 1.0f;  // (folds away in the bf16 / MX instantiations)
          f32x4 v = {acc[i][jx][4 * g + 0] * sc + bq[g][0], acc[i][jx][4 * g + 1] * sc + bq[g][1], acc[i][jx][4 * g + 2] * sc + bq[g][2],
                     acc[i][jx][4 * g + 3] * sc + bq[g][3]};
          *reinterpret_cast<f32x4*>(stg + (jx * 32 + l31) * RS + nl * 4) = v;
        }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      // Read-modify-write epilogues: ALL the old values of a chunk of rows are loaded before the first store.  Written as one loop
      // (load, add, store per row) the compiler must keep every load behind the previous row's store -- it cannot know they do not
      // alias -- and each row waited a full HBM round trip: 40 serialized round trips per wave and tile.  The gate row (the same
      // features for every row of the pass) is loaded once per pass for the same reason.
      const int n = nw + i * 32 + lch * 4;
      f32x4 gg = {1.f, 1.f, 1.f, 1.f};
      if constexpr (EPI == EPI_RESID) {
        if (a.gate) gg = *reinterpret_cast<const f32x4*>(a.gate + min(n, a.N - 4));
      }
      constexpr int CH = 4;  // rows-of-8 per chunk: 4 x 16 B per lane in flight (8 spill: the accumulators of the later passes are still live)
#pragma unroll
      for (int c0 = 0; c0 < ROWS / 8; c0 += CH) {
        f32x4 oldv[CH];
        if constexpr (EPI != EPI_F32) {
#pragma unroll
          for (int r8 = 0; r8 < CH; ++r8) {  // unconditional, clamped: a guard per load would put each in its own block with its own wait
            const int m = min(mw + (c0 + r8) * 8 + lrow, a.M - 1);
            oldv[r8] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(a.out) + (size_t)m * a.ldo + min(n, a.N - 4));
          }
        }
#pragma unroll
        for (int r8 = 0; r8 < CH; ++r8) {
          const int row = (c0 + r8) * 8 + lrow;
          const int m = mw + row;
          f32x4 v = *reinterpret_cast<const f32x4*>(stg + row * RS + lch * 16);
          if (m < a.M && n < a.N) {
            float* po = reinterpret_cast<float*>(a.out) + (size_t)m * a.ldo + n;
            if constexpr (EPI == EPI_F32) {
              *reinterpret_cast<f32x4*>(po) = v;
            } else if constexpr (EPI == EPI_F32_ACC) {
              const f32x4 old = oldv[r8];
              *reinterpret_cast<f32x4*>(po) = f32x4{old[0] + v[0], old[1] + v[1], old[2] + v[2], old[3] + v[3]};
            } else {  // EPI_RESID: x += (acc + bias) * gate   (model.py:306, 310, 313)
              const f32x4 old = oldv[r8];
              *reinterpret_cast<f32x4*>(po) =
                  f32x4{old[0] + v[0] * gg[0], old[1] + v[1] * gg[1], old[2] + v[2] * gg[2], old[3] + v[3] * gg[3]};
            }
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the next pass overwrites the staging rows
    }
  }
}

}  // namespace wf
