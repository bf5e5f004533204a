// Dense projection kernels for gfx950 (MI355X): C = epilogue(A[M,K] * W[N,K]^T), f16 operands, f32 accumulate.
//
// Two kernel families share one accumulator set-up / epilogue (init_wave_tile, store_wave_tile):
//   gemm_f16_nt_pp  ping-pong: 256x320 tile, 8 waves in two groups staggered by one barrier, ring of four K32
//                   granules with counted vmcnt - the SAM ViT-H projections (see its comment);
//   gemm_f16_nt     generic BMxBN tile, WMxWN waves of (BM/WM)x(BN/WN), two LDS stages with one drain + barrier per
//                   K-tile - 16-wave 256x256 for the other large shapes, 128x128 (K step 64 or 32) for the rest.
// Common to both (cdna_hip_programming.md §5):
//   - operands staged HBM -> LDS by LDS-DMA (global_load_lds_dwordx4); the LDS image is lane-linear (DMA
//     constraint), so the bank-conflict swizzle is applied to the per-lane SOURCE address and to the ds_read address:
//     16-B chunk c of row r lives at chunk c ^ swz(r);
//   - MFMA 16x16x32 f16 issued "swapped" (W fragment as the A operand) so each lane ends up with 4 CONSECUTIVE
//     output columns of one row;
//   - workgroup ids are remapped so each XCD (private 4 MiB L2) works on a contiguous band of tiles, GROUP_M
//     M-tiles x all N-tiles at a time, and re-reads its A / W panels from L2;
//   - epilogue (fused, f32): +bias, GELU/ReLU, *col_scale, +residual (preloaded into the accumulators for linear
//     GEMMs), optional row scatter (window-unpartition / crop / un-shift), f32 or f16 store as whole row segments.
// The direct 3x3 convolution of the DPT head (conv3x3_f16_nt, ink_conv3x3_f16) is the generic 128x128 kernel with another
// A-address generator and shares the accumulator set-up / epilogue; it lives at the end of the namespace.
// Tile choice: ink_gemm_query_variant (shape heuristic); ink_gemm_set_variant forces one of its tile families (tests).
#include <stdlib.h>

#include "mfma_util.h"
#include "../../include/inklayer_hip.h"

namespace {

template <int BK> struct Swz;
template <> struct Swz<64> {  // 128-B rows, 8 chunks
  static __device__ __forceinline__ int f(int row) { return row & 7; }
};
template <> struct Swz<32> {  // 64-B rows, 4 chunks
  static __device__ __forceinline__ int f(int row) { return (-(row >> 2)) & 3; }
};

// ---------------------------------------------------------------------------------------------------------
// Accumulator set-up and epilogue of one wave tile (TM x TN MFMA tiles of 16x16; the lane holds
// C[m = mw + 16*ti + fr][n = nw + 16*j + 4*fq + 0..3]), shared by every kernel in this file.
//
// Loads and stores share vmcnt and retire in issue order in the counter, so a load issued AFTER a store can only
// be waited for with vmcnt(0) - i.e. by waiting for that store to reach memory (and the compiler has to assume
// the worst over all paths, so "counted" waits degrade to 0 as soon as a store may be skipped).  Measured with
// s_memrealtime stamps (instrumented build, commit 8926174): with the row_map / residual / bias loads inside the slab
// loop each of the 8 slabs of a 256x256 tile paid a full store round trip, 7.5 us per tile against a 31 us main loop.
// So the slab loop contains NO load:
//   * the residual of the linear case (no activation, no layer scale - every large GEMM of the pipeline) is
//     loaded straight into the accumulators before the K loop, row-mapped, and the MFMAs accumulate on top of it
//     (the four j-loads of a row cover 256 contiguous bytes; they overlap the pipeline fill);
//   * the output rows (wave_rows, one per accumulator row, redistributed with ds_bpermute) and the bias are
//     loaded before the first store;
//   * the rare non-linear residual / layer-scale loads stay in the loop, each used inside its own branch.
__device__ __forceinline__ bool residual_preloaded(const InkGemm& p) {
  return p.residual && p.act == INK_ACT_NONE && !p.col_scale;
}

// Output row of every accumulator row of the wave tile (lane & 15 = row within the 16-row slab), -1 = outside M or
// dropped by the row map.  Loaded ONCE, before the first K-tile DMA: the residual preload indexes the residual
// with it and the epilogue redistributes it across lanes with ds_bpermute (no load next to the stores).
template <int TM>
__device__ __forceinline__ void wave_rows(int (&rows)[TM], const InkGemm& p, int mw, int lane) {
#pragma unroll
  for (int ti = 0; ti < TM; ++ti) {
    const int m = mw + ti * 16 + (lane & 15);
    int r = -1;
    if (m < p.M) r = p.row_map ? p.row_map[m] : m;
    rows[ti] = r;
  }
}

template <int TM, int TN>
__device__ __forceinline__ void init_wave_tile(f32x4 (&acc)[TM][TN], const InkGemm& p, const int (&rows)[TM], int nw,
                                               int lane) {
  const int fq = lane >> 4;
  const bool pre = residual_preloaded(p);
#pragma unroll
  for (int ti = 0; ti < TM; ++ti) {
    const int r = pre ? rows[ti] : -1;
    const float* rp = p.residual + (size_t)max(r, 0) * p.ldr + nw + fq * 4;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      acc[ti][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (r >= 0 && nw + j * 16 + fq * 4 < p.N) acc[ti][j] = *(const f32x4*)(rp + j * 16);
    }
  }
}

// Each 16-row slab goes through a wave-private LDS patch so that HBM sees whole row segments (16 B per lane,
// 128 B (f16) / 256 B (f32) contiguous per row); bias / activation / layer-scale are applied on the way in.
// MODE: -1 = activation / layer scale / late residual decided at run time (the generic kernels);  0, 1, 2 = compile-time
// "no activation" / GELU / ReLU with no layer scale and no late residual - the ping-pong kernel dispatches on it ONCE per
// workgroup, so that the 20 activations of a slab form one basic block (the per-group run-time branches cut the GELU
// into 4-element dependent chains: transcendental latency instead of throughput).
// OUT: 0 = f32 C, 1 = f16 C.
// add_bias_wave_tile: the bias add (a function of its own: with its loop written inline, hipcc schedules the epilogue's
// bias loads differently).
template <int TM, int TN>
__device__ __forceinline__ void add_bias_wave_tile(f32x4 (&acc)[TM][TN], const InkGemm& p, int nw, int lane) {
  const int fq = lane >> 4;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = nw + j * 16 + fq * 4;
    f32x4 bv = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (p.bias && n < p.N) bv = *(const f32x4*)(p.bias + n);
#pragma unroll
    for (int ti = 0; ti < TM; ++ti) acc[ti][j] += bv;     // unconditional: no copy of the array at a join
  }
}

template <int TM, int TN, int OUT, int MODE = -1>
__device__ __forceinline__ void store_wave_tile(f32x4 (&acc)[TM][TN], const InkGemm& p, char* er,
                                                const int (&rows)[TM], int nw, int lane) {
  constexpr bool F16O = OUT == 1;
  constexpr int WNC = TN * 16, EP = WNC * 4 + 16;
  constexpr int ES = OUT == 0 ? 4 : 8;             // elements per 16-B chunk of the output row(s)
  constexpr int CPRW = WNC / ES;                   // chunks per patch row
  constexpr int NIT = (16 * CPRW + 63) / 64;       // chunk rounds per slab
  const int fr = lane & 15, fq = lane >> 4;
  const bool wide16 = OUT != 0 && (p.ldc % 8 == 0);
  const bool res_late = MODE < 0 && p.residual && !residual_preloaded(p);
  const int act = MODE < 0 ? p.act : MODE;
  const bool scaled = MODE < 0 && p.col_scale != nullptr;
  // chunk c = it*64 + lane of a slab: patch row c / CPRW, chunk column c % CPRW (the same for every slab)
  int row_of[NIT], n_of[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int c = it * 64 + lane;
    row_of[it] = c < 16 * CPRW ? c / CPRW : 16;
    n_of[it] = nw + (c % CPRW) * ES;
  }

  // the only loads of the epilogue, before the first store: the bias
  add_bias_wave_tile<TM, TN>(acc, p, nw, lane);

#pragma unroll
  for (int ti = 0; ti < TM; ++ti) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      f32x4 v = acc[ti][j];
      if (act == INK_ACT_GELU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = gelu_erf(v[r]);
      } else if (act == INK_ACT_RELU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
      }
      if (scaled) {
        const int n = nw + j * 16 + fq * 4;
        if (n < p.N) v *= *(const f32x4*)(p.col_scale + n);
      }
      if (F16O) {
        *(f16x4*)(er + fr * EP + (j * 16 + fq * 4) * 2) = (f16x4){(f16)v[0], (f16)v[1], (f16)v[2], (f16)v[3]};
      } else {
        *(f32x4*)(er + fr * EP + (j * 16 + fq * 4) * 4) = v;
      }
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      // output row of patch row row_of[it]: held by the lanes with (lane & 15) == that row
      int r = __builtin_amdgcn_ds_bpermute((row_of[it] & 15) << 2, rows[ti]);
      if (row_of[it] >= 16 || n_of[it] >= p.N) r = -1;
      if (r >= 0) {
        const int c_n = n_of[it];
        const char* src = er + row_of[it] * EP + (c_n - nw) * (F16O ? 2 : 4);
        if (F16O) {
          f16x8 d = *(const f16x8*)src;
          f16* dst = (f16*)p.C + (size_t)r * p.ldc + c_n;
          if (res_late) {
            const float* rp = p.residual + (size_t)r * p.ldr + c_n;
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (c_n + e < p.N) d[e] = (f16)((float)d[e] + rp[e]);
          }
          if (wide16 && c_n + 8 <= p.N) {
            *(f16x8*)dst = d;
          } else {
            *(f16x4*)dst = (f16x4){d[0], d[1], d[2], d[3]};
            if (c_n + 8 <= p.N) *(f16x4*)(dst + 4) = (f16x4){d[4], d[5], d[6], d[7]};
          }
        } else {
          f32x4 d = *(const f32x4*)src;
          if (res_late) d += *(const f32x4*)(p.residual + (size_t)r * p.ldr + c_n);
          *(f32x4*)((float*)p.C + (size_t)r * p.ldc + c_n) = d;
        }
      }
    }
  }
}

// Tile coordinates of workgroup id (after xcd_remap) in the grouped order inside the XCD-contiguous id space:
// group_m consecutive M-tiles x all N-tiles, M fastest, so the ~32 tiles an XCD runs concurrently share group_m
// A-panels and 32/group_m W-panels (L2 = 4 MiB per XCD); group_m = 1: row-major.
__device__ __forceinline__ void tile_of(int id, int ntm, int ntn, int group_m, int& mt, int& nt) {
  if (group_m > 1) {
    const int per = group_m * ntn;
    const int first = (id / per) * group_m;
    const int gsz = min(ntm - first, group_m);
    mt = first + (id % per) % gsz;
    nt = (id % per) / gsz;
  } else {
    mt = id / ntn;
    nt = id % ntn;
  }
}

// Generic tile: BM x BN output per workgroup, WM x WN waves (each (BM/WM) x (BN/WN)), K step BK, NS = 2 LDS stages:
// one K-tile in flight, plain __syncthreads (drains the DMA).
constexpr int NS = 2;
template <int BM, int BN, int BK, int WM, int WN>
__global__ __launch_bounds__(WM * WN * 64) void gemm_f16_nt(InkGemm p, int group_m) {
  constexpr int NT = WM * WN * 64;
  constexpr int CPR = BK / 8;          // 16-B chunks per tile row
  constexpr int ROWB = BK * 2;         // bytes per tile row
  constexpr int TILE_A = BM * ROWB, TILE_W = BN * ROWB;
  constexpr int STAGE = TILE_A + TILE_W;
  constexpr int IT_A = (BM * CPR) / NT, IT_W = (BN * CPR) / NT;
  constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
  static_assert((BM * CPR) % NT == 0 && (BN * CPR) % NT == 0, "tile/threads mismatch");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;

  const int ntn = (p.N + BN - 1) / BN;
  const int ntm = (p.M + BM - 1) / BM;
  int mt, nt;
  tile_of(xcd_remap(blockIdx.x, ntm * ntn), ntm, ntn, group_m, mt, nt);
  const int m0 = mt * BM;
  const int n0 = nt * BN;

  const f16* __restrict__ A = (const f16*)p.A;
  const f16* __restrict__ W = (const f16*)p.W;

  const f16* srcA[IT_A];
  const f16* srcW[IT_W];
#pragma unroll
  for (int it = 0; it < IT_A; ++it) {
    const int pch = it * NT + tid;
    const int row = pch / CPR;
    const int lch = (pch % CPR) ^ Swz<BK>::f(row);
    srcA[it] = A + (size_t)min(m0 + row, p.M - 1) * p.lda + lch * 8;
  }
#pragma unroll
  for (int it = 0; it < IT_W; ++it) {
    const int pch = it * NT + tid;
    const int row = pch / CPR;
    const int lch = (pch % CPR) ^ Swz<BK>::f(row);
    srcW[it] = W + (size_t)min(n0 + row, p.N - 1) * p.ldw + lch * 8;
  }

  auto stage = [&](int buf, int kt) {
    char* base = smem + buf * STAGE;
#pragma unroll
    for (int it = 0; it < IT_A; ++it)
      __builtin_amdgcn_global_load_lds((gptr_t)(srcA[it] + kt * BK), (lptr_t)(base + (it * NT + wave * 64) * 16), 16, 0, 0);
#pragma unroll
    for (int it = 0; it < IT_W; ++it)
      __builtin_amdgcn_global_load_lds((gptr_t)(srcW[it] + kt * BK), (lptr_t)(base + TILE_A + (it * NT + wave * 64) * 16), 16, 0, 0);
  };

  int rows[TM];
  wave_rows<TM>(rows, p, m0 + wm * (BM / WM), lane);
  f32x4 acc[TM][TN];

  const int fr = lane & 15, fq = lane >> 4;
  const int offA = (wm * (BM / WM) + fr) * ROWB;
  const int offW = (wn * (BN / WN) + fr) * ROWB;
  const int swz = Swz<BK>::f(fr);      // tile-row bases are multiples of 16 -> swz depends on fr only

  const int nk = p.K / BK;
  auto compute = [&](int cur) {
    const char* bA = smem + cur * STAGE;
    const char* bW = bA + TILE_A;
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      constexpr int AG = TM > 4 ? 4 : TM;    // A fragments live at a time (big wave tiles: registers)
      f16x8 a[AG], w[TN];
      const int co = ((kk * 4 + fq) ^ swz) << 4;
#pragma unroll
      for (int j = 0; j < TN; ++j) w[j] = *(const f16x8*)(bW + offW + j * 16 * ROWB + co);
#pragma unroll
      for (int i0 = 0; i0 < TM; i0 += AG) {
#pragma unroll
        for (int i = 0; i < AG; ++i) a[i] = *(const f16x8*)(bA + offA + (i0 + i) * 16 * ROWB + co);
#pragma unroll
        for (int i = 0; i < AG; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i0 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[j], a[i], acc[i0 + i][j], 0, 0, 0);
      }
    }
  };

  stage(0, 0);
  init_wave_tile<TM, TN>(acc, p, rows, n0 + wn * (BN / WN), lane);
  for (int kt = 0; kt < nk; ++kt) {
    // the LDS-DMA of tile kt is tracked by vmcnt only: drain it EXPLICITLY before the barrier (whether
    // __syncthreads() alone emits the vmcnt wait depends on what else the compiler sees in flight)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < nk) stage((kt + 1) & 1, kt + 1);
    compute(kt & 1);
  }

  // ---- epilogue: lane holds C[m = .. + fr][n = .. + 4*fq + 0..3] for each (i,j)
  constexpr int WNC = BN / WN;                 // columns of the wave tile
  constexpr int EP = WNC * 4 + 16;             // patch row pitch in bytes (f32 worst case + pad)
  static_assert(WM * WN * 16 * EP <= NS * STAGE, "epilogue patch must fit in the staging LDS");
  __syncthreads();                             // every wave is done reading the last K-tile
  char* er = smem + wave * (16 * EP);
  if (p.c_f16 == 1) {
    store_wave_tile<TM, TN, 1>(acc, p, er, rows, n0 + wn * WNC, lane);
  } else {
    store_wave_tile<TM, TN, 0>(acc, p, er, rows, n0 + wn * WNC, lane);
  }
}

// ---------------------------------------------------------------------------------------------------------
// Ping-pong kernel: 256x320 tile, 8 waves = two groups of 4 (group = wave / 4 owns 128 rows, wave = 128 x 80, 160
// accumulator VGPRs; one wave of each group per SIMD), K streamed as a ring of PP_RING = 4 granules of 32 (36 KiB
// each: A 256x32 + W 320x32 f16).  The groups run the same program staggered by ONE barrier, so in every slot one
// group issues its 40 MFMAs while the other reads its fragments from LDS and issues the LDS-DMA of the granule
// AHEAD = 2 ahead:
//     slot      2g          2g+1        2g+2
//     group 0   LOAD(g)     MFMA(g)     LOAD(g+1)
//     group 1   MFMA(g-1)   LOAD(g)     MFMA(g)
// Only four of the eight A fragments are live: the LOAD slot reads rows 0-3 (and the five W fragments), rows 4-7 are
// read DURING the MFMA slot into the registers of rows 0-3 as soon as those have issued their MFMAs.  A granule is
// therefore still read in its MFMA slot, so its ring slot (g % PP_RING) may only be refilled one granule later than
// without the late reads: the DMA runs PP_RING-2 granules ahead, not PP_RING-1.  Every wave ends its LOAD slot with a
// COUNTED vmcnt (one granule stays in flight) and every slot ends with a raw s_barrier, so a granule is only read after
// the wait + barrier that retire it (cdna_hip_programming.md §5 "Read a staged buffer one phase AFTER the wait").
// 8 waves x <=256 VGPRs leave room for the load-free epilogue (store_wave_tile), which the 16-wave tiles lack.
// The epilogue is chosen at run time (bias / activation / layer scale / f32 residual, f32 or f16 C), with ONE compiled
// form for each of the SAM ViT-H block's projections.
constexpr int PP_RING = 4, PP_TN = 5;
__global__ __launch_bounds__(512) void gemm_f16_nt_pp(InkGemm p, int group_m) {
  constexpr int RING = PP_RING, TN = PP_TN;
  constexpr int BM = 256, BN = 64 * TN, BK = 32, NT = 512;
  constexpr int CPR = BK / 8, ROWB = BK * 2;
  constexpr int TILE_A = BM * ROWB, TILE_W = BN * ROWB, GRAN = TILE_A + TILE_W;   // 36 KiB
  constexpr int IT_A = (BM * CPR) / NT, IT_W = (BN * CPR) / NT;                    // 2 + 2 DMA per thread
  constexpr bool W_TAIL = (BN * CPR) % NT != 0;       // 320 rows: a third, half-populated round (waves 0-3 = group 0)
  static_assert(!W_TAIL || (BN * CPR) % NT == NT / 2, "tail is exactly the first four waves");
  constexpr int LOADS = IT_A + IT_W;                  // per wave of group 1; group 0 issues one more with W_TAIL
  constexpr int TM = 8, WNC = 16 * TN;
  constexpr int AHEAD = RING - 2;                     // granules the DMA runs ahead of the LOAD slot
  constexpr int AG = 4;                               // A fragments live at a time
  constexpr int EP = WNC * 4 + 16;
  static_assert(8 * 16 * EP <= RING * GRAN, "patch fits");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave >> 2, wn = wave & 3;         // grp = wave row (128 rows each), wn = wave column (80 cols)
  const int fr = lane & 15, fq = lane >> 4;

  const int ntn = (p.N + BN - 1) / BN, ntm = (p.M + BM - 1) / BM;
  int mt, nt;
  tile_of(xcd_remap(blockIdx.x, ntm * ntn), ntm, ntn, group_m, mt, nt);
  const int m0 = mt * BM, n0 = nt * BN;
  const int G = p.K / BK;
  const f16* __restrict__ A = (const f16*)p.A;
  const f16* __restrict__ W = (const f16*)p.W;
  const f16* srcA[IT_A];
  const f16* srcW[IT_W + (W_TAIL ? 1 : 0)];
#pragma unroll
  for (int it = 0; it < IT_A; ++it) {
    const int pch = it * NT + tid, row = pch / CPR, lch = (pch % CPR) ^ Swz<BK>::f(row);
    srcA[it] = A + (size_t)min(m0 + row, p.M - 1) * p.lda + lch * 8;
  }
#pragma unroll
  for (int it = 0; it < IT_W + (W_TAIL ? 1 : 0); ++it) {
    const int pch = it * NT + tid, row = min(pch / CPR, BN - 1), lch = (pch % CPR) ^ Swz<BK>::f(row);
    srcW[it] = W + (size_t)min(n0 + row, p.N - 1) * p.ldw + lch * 8;
  }
  auto dma = [&](int g, int slot) {
    char* base = smem + slot * GRAN;
#pragma unroll
    for (int it = 0; it < IT_A; ++it)
      __builtin_amdgcn_global_load_lds((gptr_t)(srcA[it] + g * BK), (lptr_t)(base + (it * NT + wave * 64) * 16), 16, 0, 0);
#pragma unroll
    for (int it = 0; it < IT_W; ++it)
      __builtin_amdgcn_global_load_lds((gptr_t)(srcW[it] + g * BK), (lptr_t)(base + TILE_A + (it * NT + wave * 64) * 16), 16, 0, 0);
    if (W_TAIL && grp == 0)
      __builtin_amdgcn_global_load_lds((gptr_t)(srcW[IT_W] + g * BK), (lptr_t)(base + TILE_A + (IT_W * NT + wave * 64) * 16), 16, 0, 0);
  };
  // counted wait that leaves the AHEAD - 1 most recent granules of THIS wave in flight
  auto wait_ahead = [&]() {
    if (W_TAIL && grp == 0) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"((AHEAD - 1) * (LOADS + 1)) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"((AHEAD - 1) * LOADS) : "memory");
    }
  };
  auto slot_end = [&]() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };

  // prologue: residual row indices, then AHEAD granules in flight (the launcher guarantees G >= PP_RING), then the
  // residual preload behind them; with a preload everything is drained once (the counted waits of the loop assume
  // only DMA in flight), without one only granule 0 is waited for
  int rows[TM];
  wave_rows<TM>(rows, p, m0 + grp * 128, lane);
#pragma unroll
  for (int g = 0; g < AHEAD; ++g) dma(g, g);
  f32x4 acc[TM][TN];
  init_wave_tile<TM, TN>(acc, p, rows, n0 + wn * WNC, lane);
  if (residual_preloaded(p)) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
    wait_ahead();
  }
  slot_end();
  if (grp == 1) slot_end();                         // the stagger: group 1 idles through slot 0

  const int offA = (grp * 128 + fr) * ROWB;
  const int offW = (wn * WNC + fr) * ROWB;
  const int co = (fq ^ Swz<BK>::f(fr)) << 4;        // one k-step of 32 per granule: logical chunk = fq
  f16x8 a[AG], w[TN];
  int cslot = 0, islot = AHEAD % RING;
  // one granule (a lambda, not a plain loop body: written as one, hipcc allocates the accumulators differently)
  auto iter = [&](int g) __attribute__((always_inline)) {
    const char* bA = smem + cslot * GRAN;
    const char* bW = bA + TILE_A;
    // ---- LOAD slot
#pragma unroll
    for (int i = 0; i < AG; ++i) a[i] = *(const f16x8*)(bA + offA + i * 16 * ROWB + co);
#pragma unroll
    for (int j = 0; j < TN; ++j) w[j] = *(const f16x8*)(bW + offW + j * 16 * ROWB + co);
    if (g + AHEAD < G) {
      dma(g + AHEAD, islot);
      wait_ahead();                                 // granule g+1 of this wave landed
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    slot_end();
    // ---- MFMA slot
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i0 = 0; i0 < TM; i0 += AG) {
#pragma unroll
      for (int i = 0; i < AG; ++i) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i0 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[j], a[i], acc[i0 + i][j], 0, 0, 0);
        if (i0 + AG < TM) {                         // this fragment register is free: fetch the row AG further down
          a[i] = *(const f16x8*)(bA + offA + (i0 + AG + i) * 16 * ROWB + co);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
    slot_end();
    cslot = (cslot + 1 == RING) ? 0 : cslot + 1;
    islot = (islot + 1 == RING) ? 0 : islot + 1;
  };
  for (int g = 0; g < G; ++g) iter(g);
  if (grp == 0) slot_end();                         // group 0 idles through the last slot (same barrier count)

  // ---- epilogue: the drained ring is the patch space
  char* er = smem + wave * (16 * EP);
  const bool plain = !p.col_scale && !(p.residual && !residual_preloaded(p));
  if (p.c_f16) {
    if (plain && p.act == INK_ACT_GELU) {          // lin1 of the ViT-H MLP
      store_wave_tile<TM, TN, 1, INK_ACT_GELU>(acc, p, er, rows, n0 + wn * WNC, lane);
    } else if (plain && p.act == INK_ACT_NONE) {   // qkv
      store_wave_tile<TM, TN, 1, INK_ACT_NONE>(acc, p, er, rows, n0 + wn * WNC, lane);
    } else {
      store_wave_tile<TM, TN, 1>(acc, p, er, rows, n0 + wn * WNC, lane);
    }
  } else {
    if (plain && p.act == INK_ACT_NONE) {          // proj, lin2 (residual preloaded into the accumulators)
      store_wave_tile<TM, TN, 0, INK_ACT_NONE>(acc, p, er, rows, n0 + wn * WNC, lane);
    } else {
      store_wave_tile<TM, TN, 0>(acc, p, er, rows, n0 + wn * WNC, lane);
    }
  }
}

static int launch_gemm_pp(const InkGemm& p, hipStream_t s, int group_m) {
  if (p.K / 32 < PP_RING) return INK_ERR_ARG;
  constexpr int BN = 64 * PP_TN;
  constexpr int lds = PP_RING * (256 + BN) * 32 * 2;
  static_assert(lds <= 160 * 1024, "LDS budget");
  ink_dyn_lds<gemm_f16_nt_pp>(lds);
  const int ntiles = ((p.M + 255) / 256) * ((p.N + BN - 1) / BN);
  hipLaunchKernelGGL(gemm_f16_nt_pp, dim3(ntiles), dim3(512), lds, s, p, group_m);
  return ink_launch_status();
}

template <int BM, int BN, int BK, int WM, int WN>
static int launch_gemm(const InkGemm& p, hipStream_t s, int group_m = 1) {
  constexpr int lds = NS * (BM + BN) * BK * 2;
  static_assert(lds <= 160 * 1024, "LDS budget");
  ink_dyn_lds<gemm_f16_nt<BM, BN, BK, WM, WN>>(lds);
  const int ntm = (p.M + BM - 1) / BM, ntn = (p.N + BN - 1) / BN;
  hipLaunchKernelGGL((gemm_f16_nt<BM, BN, BK, WM, WN>), dim3(ntm * ntn), dim3(WM * WN * 64), lds, s, p, group_m);
  return ink_launch_status();
}

// ---------------------------------------------------------------------------------------------------------
// Direct 3x3 / pad 1 convolution on an NHWC f16 map (ink_conv3x3_f16): gemm_f16_nt<128, 128, BK, 2, 2> with another
// A-address generator - the im2col matrix [B*OH*OW, 9*C] is never written.  M = B*OH*OW output pixels, K = 9*C in
// (ky, kx, c) order; BK divides C, so a K-tile lies inside ONE tap and is a contiguous BK-channel run of one input
// pixel.  A lane's staging chunk belongs to one output pixel for the whole K loop: (b, oy, ox) is decoded once into the
// pointer of the centre input pixel (with the lane's swizzled chunk folded in, exactly as gemm_f16_nt does) and a
// 9-bit mask of the taps that fall inside the image; per K-tile the LDS-DMA source is centre + tap offset, or a row of
// zeros for a padding tap.  RELU_IN applies ResidualConvUnit's activation(x) to the A fragments after the LDS read
// (packed max with 0; the padding zeros are fixed points).  Accumulators and epilogue are the GEMM's.
struct ConvGeom {
  int H, W, C, OH, OW, stride;
};
__device__ __attribute__((aligned(128))) const uint32_t g_conv_zero_row[32] = {};   // 64 f16 zeros: one padding tap

template <int BK, bool RELU_IN>
__global__ __launch_bounds__(256) void conv3x3_f16_nt(InkGemm p, ConvGeom g) {
  constexpr int BM = 128, BN = 128, WM = 2, WN = 2;
  constexpr int NT = WM * WN * 64;
  constexpr int CPR = BK / 8;
  constexpr int ROWB = BK * 2;
  constexpr int TILE_A = BM * ROWB, TILE_W = BN * ROWB;
  constexpr int STAGE = TILE_A + TILE_W;
  constexpr int IT_A = (BM * CPR) / NT, IT_W = (BN * CPR) / NT;
  constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;

  const int ntn = (p.N + BN - 1) / BN;
  const int ntm = (p.M + BM - 1) / BM;
  int mt, nt;
  tile_of(xcd_remap(blockIdx.x, ntm * ntn), ntm, ntn, 1, mt, nt);
  const int m0 = mt * BM;
  const int n0 = nt * BN;

  const f16* __restrict__ A = (const f16*)p.A;
  const f16* __restrict__ W = (const f16*)p.W;

  const f16* ctrA[IT_A];      // centre input pixel of the chunk's output pixel, + the lane's (swizzled) chunk
  const f16* zeroA[IT_A];     // the same chunk of the zero row
  int maskA[IT_A];            // bit ky*3+kx: that tap lies inside the image
  const f16* srcW[IT_W];
#pragma unroll
  for (int it = 0; it < IT_A; ++it) {
    const int pch = it * NT + tid;
    const int row = pch / CPR;
    const int lch = (pch % CPR) ^ Swz<BK>::f(row);
    const int m = min(m0 + row, p.M - 1);
    const int b = m / (g.OH * g.OW);
    const int rem = m - b * (g.OH * g.OW);
    const int oy = rem / g.OW;
    const int iy = oy * g.stride, ix = (rem - oy * g.OW) * g.stride;
    ctrA[it] = A + (((size_t)b * g.H + iy) * g.W + ix) * g.C + lch * 8;
    zeroA[it] = (const f16*)g_conv_zero_row + lch * 8;
    const int rowok = (iy > 0 ? 1 : 0) | 2 | (iy + 1 < g.H ? 4 : 0);
    const int colok = (ix > 0 ? 1 : 0) | 2 | (ix + 1 < g.W ? 4 : 0);
    int mask = 0;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
      if ((rowok >> ky) & 1) mask |= colok << (ky * 3);
    maskA[it] = mask;
  }
#pragma unroll
  for (int it = 0; it < IT_W; ++it) {
    const int pch = it * NT + tid;
    const int row = pch / CPR;
    const int lch = (pch % CPR) ^ Swz<BK>::f(row);
    srcW[it] = W + (size_t)min(n0 + row, p.N - 1) * p.ldw + lch * 8;
  }

  // K-tiles are staged in order; (tap, c0) of the next one to stage: k = tap * C + c0
  int s_tap = 0, s_c0 = 0;
  auto stage = [&](int buf, int kt) {
    char* base = smem + buf * STAGE;
    const int ky = s_tap / 3, kx = s_tap - ky * 3;
    const ptrdiff_t doff = ((ptrdiff_t)(ky - 1) * g.W + (kx - 1)) * g.C + s_c0;
#pragma unroll
    for (int it = 0; it < IT_A; ++it) {
      const f16* src = ((maskA[it] >> s_tap) & 1) ? ctrA[it] + doff : zeroA[it];
      __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(base + (it * NT + wave * 64) * 16), 16, 0, 0);
    }
#pragma unroll
    for (int it = 0; it < IT_W; ++it)
      __builtin_amdgcn_global_load_lds((gptr_t)(srcW[it] + kt * BK), (lptr_t)(base + TILE_A + (it * NT + wave * 64) * 16), 16, 0, 0);
    s_c0 += BK;
    if (s_c0 == g.C) {
      s_c0 = 0;
      ++s_tap;
    }
  };

  int rows[TM];
  wave_rows<TM>(rows, p, m0 + wm * (BM / WM), lane);
  f32x4 acc[TM][TN];

  const int fr = lane & 15, fq = lane >> 4;
  const int offA = (wm * (BM / WM) + fr) * ROWB;
  const int offW = (wn * (BN / WN) + fr) * ROWB;
  const int swz = Swz<BK>::f(fr);

  const int nk = p.K / BK;
  auto compute = [&](int cur) {
    const char* bA = smem + cur * STAGE;
    const char* bW = bA + TILE_A;
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      f16x8 a[TM], w[TN];
      const int co = ((kk * 4 + fq) ^ swz) << 4;
#pragma unroll
      for (int j = 0; j < TN; ++j) w[j] = *(const f16x8*)(bW + offW + j * 16 * ROWB + co);
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        a[i] = *(const f16x8*)(bA + offA + i * 16 * ROWB + co);
        if (RELU_IN) a[i] = __builtin_elementwise_max(a[i], (f16x8)(f16)0);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[j], a[i], acc[i][j], 0, 0, 0);
    }
  };

  stage(0, 0);
  init_wave_tile<TM, TN>(acc, p, rows, n0 + wn * (BN / WN), lane);
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the LDS-DMA of tile kt (see gemm_f16_nt)
    __syncthreads();
    if (kt + 1 < nk) stage((kt + 1) & 1, kt + 1);
    compute(kt & 1);
  }

  constexpr int WNC = BN / WN;
  constexpr int EP = WNC * 4 + 16;
  static_assert(WM * WN * 16 * EP <= NS * STAGE, "epilogue patch must fit in the staging LDS");
  __syncthreads();
  char* er = smem + wave * (16 * EP);
  if (p.c_f16 == 1) {
    store_wave_tile<TM, TN, 1>(acc, p, er, rows, n0 + wn * WNC, lane);
  } else {
    store_wave_tile<TM, TN, 0>(acc, p, er, rows, n0 + wn * WNC, lane);
  }
}

template <int BK, bool RELU_IN>
static int launch_conv3x3(const InkGemm& p, const ConvGeom& g, hipStream_t s) {
  constexpr int lds = NS * (128 + 128) * BK * 2;
  ink_dyn_lds<conv3x3_f16_nt<BK, RELU_IN>>(lds);
  const int ntm = (p.M + 127) / 128, ntn = (p.N + 127) / 128;
  hipLaunchKernelGGL((conv3x3_f16_nt<BK, RELU_IN>), dim3(ntm * ntn), dim3(256), lds, s, p, g);
  return ink_launch_status();
}

}  // namespace

extern "C" int ink_conv3x3_f16(const void* in_f16, int32_t B, int32_t H, int32_t W, int32_t C, const void* wt_f16,
                               int32_t N, const float* bias, int32_t stride, int32_t relu_in, int32_t act,
                               const float* residual, void* out, int32_t out_f16, void* stream) {
  INK_CHECK_ARG(in_f16 && wt_f16 && out);
  INK_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && N > 0);
  INK_CHECK_ARG(C % 32 == 0 && N % 4 == 0);
  INK_CHECK_ARG(stride == 1 || stride == 2);
  INK_CHECK_ARG(ink_aligned<16>(in_f16, wt_f16, out, residual, bias));
  INK_CHECK_ARG(relu_in == 0 || relu_in == 1);
  INK_CHECK_ARG(act == INK_ACT_NONE || act == INK_ACT_RELU);
  INK_CHECK_ARG(out_f16 == 0 || out_f16 == 1);
  const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
  const int64_t M = (int64_t)B * OH * OW;
  INK_CHECK_ARG(M <= INT32_MAX - 128 && (int64_t)9 * C <= INT32_MAX);
  InkGemm p = {};
  p.A = in_f16;
  p.W = wt_f16;
  p.bias = bias;
  p.residual = residual;
  p.C = out;
  p.M = (int32_t)M;
  p.N = N;
  p.K = 9 * C;
  p.lda = p.ldw = 9 * C;
  p.ldr = p.ldc = N;
  p.act = act;
  p.c_f16 = out_f16;
  const ConvGeom g = {H, W, C, OH, OW, stride};
  hipStream_t s = (hipStream_t)stream;
  if (C % 64 == 0) return relu_in ? launch_conv3x3<64, true>(p, g, s) : launch_conv3x3<64, false>(p, g, s);
  return relu_in ? launch_conv3x3<32, true>(p, g, s) : launch_conv3x3<32, false>(p, g, s);
}

static int g_variant = -1;  // ink_gemm_set_variant: -1 = the shape heuristic, else the forced tile family
// shape heuristic (tile sweeps on MI355X): the ping-pong 256x320 tile when N is a multiple of 320 and
// the launch is at least ~1.5 rounds of 256 CUs (SAM ViT-H: N = 1280 / 3840 / 5120, where batch 8 gives
// exact round counts and 10 % fewer staged bytes per flop than 256x256); else the 16-wave 256x256 tile whenever it
// fills the chip (>= ~200 tiles) and N does not waste a large part of a 256-wide tile; else the 128x128 tile.
extern "C" int ink_gemm_query_variant(int32_t M, int32_t N, int32_t K) {
  if (K % 64 != 0) return 32;      // 128x128x32 tile
  if (N % 320 == 0 && K >= 128 && (long)((M + 255) / 256) * (N / 320) >= 384) return 45;
  const long tiles256 = (long)((M + 255) / 256) * ((N + 255) / 256);
  const bool n_fits = (N % 256 == 0) || N >= 1024;
  return (tiles256 >= 200 && n_fits) ? 10 : 0;
}
extern "C" int ink_abi_version(void) { return INK_ABI_VERSION; }
extern "C" int ink_gemm_set_variant(int32_t v) {
  // test hook (process-wide, not thread-safe, not used by the product path): force one tile family of the heuristic
  INK_CHECK_ARG(v == -1 || v == 0 || v == 10 || v == 45);
  g_variant = v;
  return INK_OK;
}

extern "C" int ink_gemm_f16(const InkGemm* pp, void* stream) {
  INK_CHECK_ARG(pp != nullptr);
  const InkGemm& p = *pp;
  INK_CHECK_ARG(p.A && p.W && p.C);
  INK_CHECK_ARG(p.M > 0 && p.N > 0 && p.K > 0);
  INK_CHECK_ARG(p.K % 32 == 0 && p.N % 4 == 0);
  INK_CHECK_ARG(p.lda % 8 == 0 && p.ldw % 8 == 0 && p.lda >= p.K && p.ldw >= p.K);
  INK_CHECK_ARG(p.ldc % 4 == 0 && p.ldc >= p.N);
  INK_CHECK_ARG(!p.residual || (p.ldr % 4 == 0 && p.ldr >= p.N));
  INK_CHECK_ARG(ink_aligned<16>(p.A, p.W, p.C));
  INK_CHECK_ARG(p.act >= 0 && p.act <= 2);
  INK_CHECK_ARG(p.c_f16 == 0 || p.c_f16 == 1);
  hipStream_t s = (hipStream_t)stream;
  if (p.K % 64 != 0) return launch_gemm<128, 128, 32, 2, 2>(p, s);
  int v = g_variant;           // -1 (default): shape heuristic.  No environment variable reaches this function.
  if (v < 0) v = ink_gemm_query_variant(p.M, p.N, p.K);
  // 0 / 32: 128x128 tiles (K step 64 / 32) in row-major tile order; 10, 45: the large tiles in groups of 4 M-tiles
  switch (v) {
    case 10: return launch_gemm<256, 256, 64, 4, 4>(p, s, 4);   // 16 waves x (64x64), 2 x 64 KB stages
    case 45: return launch_gemm_pp(p, s, 4);                    // ping-pong 256x320, ring of 4 (144 KB)
    default: return launch_gemm<128, 128, 64, 2, 2>(p, s);     // variant 0
  }
}
