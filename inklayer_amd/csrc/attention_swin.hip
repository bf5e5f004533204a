// Swin window attention with the relative-position bias and the SW-MSA mask computed in the kernel, for gfx950:
//   O = softmax(scale q k^T + table[h][rel(q, k)] + (region[w % nW][q] != region[w % nW][k] ? -100 : 0)) v
// per (window, head), f16 rows of head_dim 32, f32 accumulation (WindowAttention.forward, swin_transformer.py:134-174,
// with the mask of BasicLayer.forward, :417-441).  It serves the windows ink_flash_attn's bias_mode 3 cannot take
// (more than 64 tokens: 12 x 12 = 144 for Swin-B/384) and takes its bias and mask COMPACT: the (2 ws - 1)^2 table of a
// head (2 KB at ws = 12) and one region id per token, instead of dense [n_heads, 144, 192] / [nW, 144, 192] f32 tables
// that would be more bytes per (window, head) than q, k, v and o together.
//
// Shape of the kernel (the ALLKV instance of attention.hip, specialised):
//   * one workgroup of ceil(ws^2 / 32) waves owns a (window, head) unit; wave w owns queries 32 w .. 32 w + 31, one
//     query per lane column.  All keys of the window are resident in LDS (K rows of 80 B, V rows of 64 B: 23 KB at
//     ws = 12; with the table, the key offsets and the region ids 26 KB per workgroup, so LDS never limits occupancy
//     below six workgroups per CU; 168 registers allow three waves per SIMD, two workgroups per CU).
//   * S^T = K Q^T and O^T = V^T P^T with mfma_f32_32x32x16_f16, as attention.hip: the lane holds all scores of ITS
//     query, so max and sum are in-lane plus one cross-half shuffle, and the S^T accumulator is the B operand of the
//     P V product without any lane movement (cdna_hip_programming.md section 3).  Every score of a query is in registers
//     at once (ceil(ws^2 / 32) accumulator tiles), so the softmax is ONE pass: no running maximum, no rescale.
//   * MFMA shape: 32x32x16 with a half-empty last tile, not 16x16x32.  144 = 4.5 x 32, so the fifth key tile and the
//     fifth query wave are half padding (10 % of the MFMA work; the P V step of the 16 padded keys is skipped
//     outright).  The MFMA pipe is not what bounds the kernel (20 MFMAs = 640 cycles per wave and unit against ~2800
//     cycles of HBM time per unit and CU; measured, it runs at about a quarter of the HBM floor, bound by the serial
//     per-unit chain at two workgroups per CU: DESIGN.md section 3), and the 32x32 form is the one whose
//     operand maps, accumulator-as-operand order and ds_read_b64_tr_b16 image the flash kernel already proves on this
//     chip; 16x16x32 would fit 144 = 9 x 16 exactly but needs a second set of maps for no time that shows.
//   * persistent: workgroup g walks units [g total / G, (g + 1) total / G) - consecutive heads of the same few
//     windows - and loads the K / V rows, the head's table and the window's region ids of unit i + 1 into registers
//     while it computes unit i; they go to LDS between two barriers at the top of the next unit.
//   * bias and mask: lane (query q) reads table[qbase(q) - koff(k)] from the head's table in LDS, qbase = (qy + ws - 1)
//     (2 ws - 1) + qx + ws - 1 and koff(k) = ky (2 ws - 1) + kx from a 4-keys-per-read LDS array written once; the region
//     ids of four keys are one LDS dword, compared bytewise against the query's.  An unshifted block (region NULL)
//     has no mask arithmetic in its code path.  The table is divided by scale on its way into LDS and the gathered
//     value (+ -100 / scale) is the INIT of the S^T accumulator, as in bias_mode 3: after the MFMAs a score costs one
//     max, one fma and one exp2, and the gather has nothing of the MFMA result to wait for.
// Stores are exact: query rows >= ws^2 of a wave are computed on clamped addresses and never stored.
#include "mfma_util.h"
#include "../../include/inklayer_hip.h"

namespace {

struct SwinAttn {
  const f16* Q; const f16* K; const f16* V; f16* O;
  int64_t ldq, ldk, ldv, ldo;
  int32_t n_units, n_heads, nW;
  float c, inv_scale, maskv;        // scale log2(e), 1 / scale, -100 / scale
  const float* table;               // [n_heads, (2 ws - 1)^2]
  const uint8_t* region;            // [nW, ws^2] or NULL
};

__device__ __forceinline__ f16x8 cvt8(const f32x16& s, int base) {
  f16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (f16)s[base + j];
  return r;
}

template <int WS>
__global__ __launch_bounds__(((WS * WS + 31) / 32) * 64) void swin_attn_kernel(SwinAttn p) {
  constexpr int NK = WS * WS;                 // tokens of a window: queries and keys
  constexpr int NSUB = (NK + 31) / 32;        // 32-key tiles = waves
  constexpr int NT = NSUB * 64;
  constexpr int KPAD = NSUB * 32;
  constexpr int KROW = 80;                    // 64 B of k + 16: odd chunk count -> conflict-free b128 reads
  constexpr int VROW = 64;                    // conflict-free tr_b16 reads
  constexpr int RW = 2 * WS - 1;
  constexpr int TAB = RW * RW;
  constexpr int KALL = (NK * 4 + NT - 1) / NT;
  constexpr int TIT = (TAB + NT - 1) / NT;
  constexpr float NEG = -1e30f;
  __shared__ __attribute__((aligned(16))) char sK[KPAD * KROW];
  __shared__ __attribute__((aligned(16))) char sV[KPAD * VROW];
  __shared__ __attribute__((aligned(16))) float sT[TAB + 3];
  __shared__ __attribute__((aligned(16))) int sKo[KPAD];       // byte offset of key k inside a query's table walk
  __shared__ __attribute__((aligned(16))) uint8_t sR[KPAD];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 31, hh = lane >> 5;
  const int q = wave * 32 + lq;
  const bool q_ok = q < NK;
  const int qc = q_ok ? q : NK - 1;
  const int qbase4 = ((qc / WS + WS - 1) * RW + qc % WS + WS - 1) * 4;

  int u = (int)((int64_t)blockIdx.x * p.n_units / gridDim.x);
  const int u_end = (int)((int64_t)(blockIdx.x + 1) * p.n_units / gridDim.x);
  if (u >= u_end) return;

  // written once: zero K / V rows of the padded keys (their scores are overwritten, their P is exactly 0, but 0 x NaN
  // is not), the key offsets, region id 0 everywhere (what an unshifted block keeps)
  for (int i = tid; i < (KPAD - NK) * 5; i += NT) *(f16x8*)(sK + NK * KROW + i * 16) = (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = tid; i < (KPAD - NK) * 4; i += NT) *(f16x8*)(sV + NK * VROW + i * 16) = (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = tid; i < KPAD; i += NT) {
    sKo[i] = i < NK ? ((i / WS) * RW + i % WS) * 4 : 0;
    sR[i] = 0;
  }

  f16x8 ka[KALL], va[KALL], qf[2];
  float tb[TIT];
  uint8_t rg = 0;
  auto load_unit = [&](int u_) {
    const int b_ = u_ / p.n_heads, h_ = u_ % p.n_heads;
#pragma unroll
    for (int it = 0; it < KALL; ++it) {
      const int ci = tid + it * NT;
      const int key = ci >> 2, cc = ci & 3;
      if (ci < NK * 4) {
        const int64_t r = (int64_t)b_ * NK + key;
        ka[it] = *(const f16x8*)(p.K + r * p.ldk + h_ * 32 + cc * 8);
        va[it] = *(const f16x8*)(p.V + r * p.ldv + h_ * 32 + cc * 8);
      }
    }
#pragma unroll
    for (int it = 0; it < TIT; ++it) {
      const int i = tid + it * NT;
      tb[it] = i < TAB ? p.table[(int64_t)h_ * TAB + i] : 0.f;
    }
    if (p.region && tid < NK) rg = p.region[(int64_t)(b_ % p.nW) * NK + tid];
  };
  auto load_q = [&](int u_) {
    const int b_ = u_ / p.n_heads, h_ = u_ % p.n_heads;
    const f16* Qrow = p.Q + ((int64_t)b_ * NK + qc) * p.ldq + h_ * 32;
    qf[0] = *(const f16x8*)(Qrow + 8 * hh);
    qf[1] = *(const f16x8*)(Qrow + 16 + 8 * hh);
  };
  load_unit(u);
  load_q(u);

  const bool masked = p.region != nullptr;
  const int voff = (4 * hh + ((lane & 15) >> 2)) * VROW + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;

  for (; u < u_end; ++u) {
    const int b = u / p.n_heads, h = u % p.n_heads;
    // the rows of this unit are in registers (issued one unit ago): hand them to LDS between two barriers (the first:
    // every wave has finished reading the previous unit), then issue the loads of the next unit at once
    __syncthreads();
#pragma unroll
    for (int it = 0; it < KALL; ++it) {
      const int ci = tid + it * NT;
      const int key = ci >> 2, cc = ci & 3;
      if (ci < NK * 4) {
        *(f16x8*)(sK + key * KROW + cc * 16) = ka[it];
        *(f16x8*)(sV + key * VROW + cc * 16) = va[it];
      }
    }
#pragma unroll
    for (int it = 0; it < TIT; ++it) {
      const int i = tid + it * NT;
      if (i < TAB) sT[i] = tb[it] * p.inv_scale;
    }
    if (masked && tid < NK) sR[tid] = rg;
    __syncthreads();
    if (u + 1 < u_end) load_unit(u + 1);

    // accumulator init = table[rel(q, k)] / scale (+ the mask, / scale): the bias enters through the MFMA's C operand,
    // as in bias_mode 3 of the flash kernel, and costs no VALU work after it; padded keys start (and, their K rows
    // being zero, stay) at NEG.  s[sub][r] is key 32 sub + (r & 3) + 8 (r >> 2) + 4 hh of this lane's query
    f32x16 s[NSUB];
    auto init_scores = [&](auto with_mask) {
      constexpr bool MASK = decltype(with_mask)::value;
      uint32_t rq4 = 0;
      if constexpr (MASK) rq4 = (uint32_t)sR[qc] * 0x01010101u;
#pragma unroll
      for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int k0 = sub * 32 + 8 * g + 4 * hh;
          if (sub * 32 + 8 * g >= NK) {                          // (compile time) four padded keys in both halves
#pragma unroll
            for (int j = 0; j < 4; ++j) s[sub][4 * g + j] = NEG;
          } else {
            const int4 ko = *(const int4*)(sKo + k0);
            uint32_t rr = 0;
            if constexpr (MASK) rr = *(const uint32_t*)(sR + k0) ^ rq4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int kj = j == 0 ? ko.x : j == 1 ? ko.y : j == 2 ? ko.z : ko.w;
              float x = *(const float*)((const char*)sT + (qbase4 - kj));
              if constexpr (MASK) {
                if ((rr >> (8 * j)) & 0xffu) x += p.maskv;
              }
              if (sub * 32 + 8 * g + 8 > NK && k0 + j >= NK) x = NEG;   // (first term: compile time)
              s[sub][4 * g + j] = x;
            }
          }
        }
    };
    if (masked) init_scores(std::true_type{}); else init_scores(std::false_type{});
    // S^T = K Q^T on top of it
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        const f16x8 kf = *(const f16x8*)(sK + (sub * 32 + lq) * KROW + st * 32 + hh * 16);
        s[sub] = mfma32(kf, qf[st], s[sub]);
      }
    float mx = NEG;
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
      for (int r = 0; r < 16; r += 2) mx = max3(mx, s[sub][r], s[sub][r + 1]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mc = -mx * p.c;
    float l = 0.f;
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = __builtin_amdgcn_exp2f(fmaf(s[sub][r], p.c, mc));
        s[sub][r] = e;
        l += e;
      }
    l += __shfl_xor(l, 32, 64);
    // O^T = V^T P^T: P rounded to f16, 16 keys per step; steps whose keys are all padding are skipped
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 2 * NSUB; ++ks) {
      if (16 * ks < NK) {
        const f16x8 pf = cvt8(s[ks >> 1], 8 * (ks & 1));
        const char* base = sV + voff + 16 * ks * VROW;
        const f16x4 a0 = tr_read(base);
        const f16x4 a1 = tr_read(base + 8 * VROW);
        const f16x8 vf = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
        o = mfma32(vf, pf, o);
      }
    }
    const float inv = 1.0f / l;
    if (q_ok) {
      f16* Orow = p.O + ((int64_t)b * NK + q) * p.ldo + h * 32;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f16x4 v = {(f16)(o[4 * g] * inv), (f16)(o[4 * g + 1] * inv), (f16)(o[4 * g + 2] * inv),
                         (f16)(o[4 * g + 3] * inv)};
        *(f16x4*)(Orow + 8 * g + 4 * hh) = v;
      }
    }
    if (u + 1 < u_end) load_q(u + 1);      // flies during the barriers / LDS hand-off of the next unit
  }
}

template <int WS>
void launch(const SwinAttn& p, int n_cus, hipStream_t s) {
  constexpr int NT = ((WS * WS + 31) / 32) * 64;
  const int grid = p.n_units < 2 * n_cus ? p.n_units : 2 * n_cus;
  hipLaunchKernelGGL((swin_attn_kernel<WS>), dim3(grid), dim3(NT), 0, s, p);
}

}  // namespace

extern "C" int ink_swin_attn(const void* Q, const void* K, const void* V, int64_t ldq, int64_t ldk, int64_t ldv, void* O,
                             int64_t ldo, int32_t n_windows, int32_t n_heads, int32_t ws, float scale,
                             const float* bias_table, const uint8_t* region, int32_t nW, void* stream) {
  INK_CHECK_ARG(Q && K && V && O && bias_table);
  INK_CHECK_ARG(ws == 7 || ws == 12);
  INK_CHECK_ARG(n_windows > 0 && n_heads > 0 && scale > 0.f && nW >= 0);
  INK_CHECK_ARG((int64_t)n_windows * n_heads < 0x7fffffffLL);
  INK_CHECK_ARG(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0);
  const int64_t C = (int64_t)n_heads * 32;
  INK_CHECK_ARG(ldq >= C && ldk >= C && ldv >= C && ldo >= C);
  INK_CHECK_ARG(ink_aligned<16>(Q, K, V) && ink_aligned<8>(O) && ink_aligned<4>(bias_table));
  INK_CHECK_ARG(!region || nW > 0);
  INK_CHECK_ARG(nW == 0 || n_windows % nW == 0);
  static const int n_cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    return n;
  }();
  SwinAttn p;
  p.Q = (const f16*)Q; p.K = (const f16*)K; p.V = (const f16*)V; p.O = (f16*)O;
  p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
  p.n_units = n_windows * n_heads; p.n_heads = n_heads; p.nW = nW > 0 ? nW : 1;
  p.c = scale * 1.44269504088896340736f; p.inv_scale = 1.0f / scale; p.maskv = -100.0f / scale;
  p.table = bias_table; p.region = region;
  hipStream_t s = (hipStream_t)stream;
  if (ws == 12) launch<12>(p, n_cus, s); else launch<7>(p, n_cus, s);
  return ink_launch_status();
}
