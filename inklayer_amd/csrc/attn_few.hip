// Attention with a handful of keys or a handful of queries: the detector's text attentions and the three attentions
// of the SAM two-way mask decoder.
#include "common.h"
#include "../../include/inklayer_hip.h"

namespace {

// 8 consecutive head-dim elements of an f16 or f32 row, as f32
__device__ __forceinline__ void load8(const f16* p, float* d) {
  const f16x8 v = *(const f16x8*)p;
#pragma unroll
  for (int j = 0; j < 8; ++j) d[j] = (float)v[j];
}
__device__ __forceinline__ void load8(const float* p, float* d) {
  const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) { d[j] = a[j]; d[4 + j] = b[j]; }
}
__device__ __forceinline__ void store8(f16* p, const float* d) {
  f16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (f16)d[j];
  *(f16x8*)p = v;
}
__device__ __forceinline__ void store8(float* p, const float* d) {
  *(f32x4*)p = (f32x4){d[0], d[1], d[2], d[3]};
  *(f32x4*)(p + 4) = (f32x4){d[4], d[5], d[6], d[7]};
}

// ---------------------------------------------------------------------------------------------
// Attention against a handful of keys (n_k <= 16): text self-attention (4x4, block-diagonal mask,
// transformer_vanilla.py:114-116) and decoder text cross-attention (900 x 4, transformer.py:893-900).
// One thread per (batch, query, head).
template <int HD, typename T>
__global__ __launch_bounds__(256) void attn_fewkeys_kernel(const T* __restrict__ Q, int64_t ldq,
                                                           const T* __restrict__ K, int64_t ldk,
                                                           const T* __restrict__ V, int64_t ldv, int B,
                                                           int n_q, int n_k, int n_heads, float scale,
                                                           const uint8_t* __restrict__ blocked,
                                                           const int32_t* __restrict__ q_rows,
                                                           const float* __restrict__ q_add,
                                                           T* __restrict__ O, int64_t ldo) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)B * n_q * n_heads) return;
  const int h = (int)(gid % n_heads);
  const int64_t bq = gid / n_heads;
  const int b = (int)(bq / n_q), q = (int)(bq % n_q);
  float qv[HD];
  const T* qp = Q + (q_rows ? (int64_t)q_rows[b] + q : bq) * ldq + h * HD;
#pragma unroll
  for (int i = 0; i < HD / 8; ++i) load8(qp + 8 * i, qv + 8 * i);
  if (q_add) {   // per-position constant of the query projection (the (x + pe) W = x W + pe W split, sam.py)
    const float* ap = q_add + ((int64_t)q * n_heads + h) * HD;
#pragma unroll
    for (int i = 0; i < HD; ++i) qv[i] += ap[i];
  }
  float sc[16];
  float mx = -3.0e38f;
  for (int t = 0; t < n_k; ++t) {
    const T* kp = K + ((int64_t)b * n_k + t) * ldk + h * HD;
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < HD / 8; ++i) {
      float kv[8];
      load8(kp + 8 * i, kv);
#pragma unroll
      for (int j = 0; j < 8; ++j) d = fmaf(qv[8 * i + j], kv[j], d);
    }
    d *= scale;
    if (blocked && blocked[q * n_k + t]) d = -3.0e38f;
    sc[t] = d;
    mx = fmaxf(mx, d);
  }
  float sum = 0.f;
  for (int t = 0; t < n_k; ++t) { sc[t] = sc[t] <= -1.0e38f ? 0.f : expf(sc[t] - mx); sum += sc[t]; }
  const float inv = 1.f / sum;
  float acc[HD];
#pragma unroll
  for (int i = 0; i < HD; ++i) acc[i] = 0.f;
  for (int t = 0; t < n_k; ++t) {
    const T* vp = V + ((int64_t)b * n_k + t) * ldv + h * HD;
    const float pw = sc[t] * inv;
#pragma unroll
    for (int i = 0; i < HD / 8; ++i) {
      float vv[8];
      load8(vp + 8 * i, vv);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[8 * i + j] = fmaf(pw, vv[j], acc[8 * i + j]);
    }
  }
  T* op = O + bq * ldo + h * HD;
#pragma unroll
  for (int i = 0; i < HD / 8; ++i) store8(op + 8 * i, acc + 8 * i);
}

// ---------------------------------------------------------------------------------------------
// The same contract for up to 256 keys (ink_attn_midkeys: the text attentions of a caption of 17..256 tokens), f16
// rows.  Plain VALU, not MFMA: the work is about 0.24 GFLOP per image and decoder layer.  One thread per (batch, query,
// head) as above, but the scores do not fit a register array, so the softmax is the online form over blocks of 8
// keys: 8 independent dot products, one rescale of the accumulator per block.  f32 math.  A fully blocked row (it
// cannot occur in the detector's shared-caption form: a token always sees itself) gives zeros, not NaN.
// ink_attn_midkeys_varlen adds a mask per batch entry (blocked_stride bytes apart; 0: one shared mask) and a key
// count per batch entry (k_len, clamped into 0..n_k here so that a bad device value cannot index out of range): the
// keys t >= k_len[b] do not exist for entry b - the loop ends there and their rows are never loaded.  The key rows
// stay at b n_k + t, so an entry's arithmetic is that of a uniform launch at n_k = k_len[b].
template <int HD>
__global__ __launch_bounds__(256) void attn_midkeys_kernel(const f16* __restrict__ Q, int64_t ldq,
                                                           const f16* __restrict__ K, int64_t ldk,
                                                           const f16* __restrict__ V, int64_t ldv, int B, int n_q,
                                                           int n_k, int n_heads, float scale,
                                                           const uint8_t* __restrict__ blocked,
                                                           int64_t blocked_stride,
                                                           const int32_t* __restrict__ k_len, f16* __restrict__ O,
                                                           int64_t ldo) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)B * n_q * n_heads) return;
  const int h = (int)(gid % n_heads);
  const int64_t bq = gid / n_heads;
  const int b = (int)(bq / n_q), q = (int)(bq % n_q);
  const int nk = k_len ? min(max(k_len[b], 0), n_k) : n_k;  // this entry's keys
  const uint8_t* brow = blocked ? blocked + b * blocked_stride + (int64_t)q * n_k : nullptr;
  float qv[HD];
  const f16* qp = Q + bq * ldq + h * HD;
#pragma unroll
  for (int i = 0; i < HD / 8; ++i) load8(qp + 8 * i, qv + 8 * i);
  float acc[HD];
#pragma unroll
  for (int i = 0; i < HD; ++i) acc[i] = 0.f;
  float m = -3.0e38f, l = 0.f;
  for (int t0 = 0; t0 < nk; t0 += 8) {
    float sc[8];
    float bm = -3.0e38f;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int t = t0 + u;
      float d = -3.0e38f;
      if (t < nk && !(brow && brow[t])) {
        const f16* kp = K + ((int64_t)b * n_k + t) * ldk + h * HD;
        d = 0.f;
#pragma unroll
        for (int i = 0; i < HD / 8; ++i) {
          float kv[8];
          load8(kp + 8 * i, kv);
#pragma unroll
          for (int j = 0; j < 8; ++j) d = fmaf(qv[8 * i + j], kv[j], d);
        }
        d *= scale;
      }
      sc[u] = d;
      bm = fmaxf(bm, d);
    }
    if (bm <= -1.0e38f) continue;                           // the whole block is blocked or past nk
    const float mn = fmaxf(m, bm);
    const float a = expf(m - mn);                           // first live block: exp(-3e38 - mn) = 0 on acc = 0
    l *= a;
#pragma unroll
    for (int i = 0; i < HD; ++i) acc[i] *= a;
    m = mn;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (sc[u] <= -1.0e38f) continue;
      const float pw = expf(sc[u] - m);
      l += pw;
      const f16* vp = V + ((int64_t)b * n_k + t0 + u) * ldv + h * HD;
#pragma unroll
      for (int i = 0; i < HD / 8; ++i) {
        float vv[8];
        load8(vp + 8 * i, vv);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[8 * i + j] = fmaf(pw, vv[j], acc[8 * i + j]);
      }
    }
  }
  const float inv = l > 0.f ? 1.f / l : 0.f;
#pragma unroll
  for (int i = 0; i < HD; ++i) acc[i] *= inv;
  f16* op = O + bq * ldo + h * HD;
#pragma unroll
  for (int i = 0; i < HD / 8; ++i) store8(op + 8 * i, acc + 8 * i);
}


// head_dim 16, f32 rows (the SAM decoder's image->token attention: 4096 queries x 7 keys per box, 8 heads): FOUR lanes
// per (query, head), 4 of the 16 dimensions each, so that every load and store instruction of a wave covers one
// contiguous KiB (a thread per (query, head) reads 64 B at a 64-B stride: every cache line is touched by four
// instructions); the four partial dot products meet through two shuffles.  Base-2 softmax (log2 e folded into the scale).
template <int NK>
__global__ __launch_bounds__(256) void attn_fewkeys16_f32_kernel(const float* __restrict__ Q, int64_t ldq,
                                                                 const float* __restrict__ K, int64_t ldk,
                                                                 const float* __restrict__ V, int64_t ldv, int B,
                                                                 int n_q, int n_heads, float scale,
                                                                 const int32_t* __restrict__ q_rows,
                                                                 const float* __restrict__ q_add,
                                                                 float* __restrict__ O, int64_t ldo) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)B * n_q * n_heads * 4) return;      // (whole 4-lane groups: the total is a multiple of 4)
  const int part = (int)(gid & 3);
  const int h = (int)((gid >> 2) % n_heads);
  const int64_t bq = (gid >> 2) / n_heads;
  const int b = (int)(bq / n_q), q = (int)(bq % n_q);
  const int col = h * 16 + 4 * part;
  f32x4 qv = *(const f32x4*)(Q + (q_rows ? (int64_t)q_rows[b] + q : bq) * ldq + col);
  if (q_add) qv += *(const f32x4*)(q_add + (int64_t)q * n_heads * 16 + col);
  qv *= scale * 1.44269504088896340736f;
  const float* kp = K + (int64_t)b * NK * ldk + col;
  const float* vp = V + (int64_t)b * NK * ldv + col;
  f32x4 kv[NK], vv[NK];
#pragma unroll
  for (int t = 0; t < NK; ++t) {
    kv[t] = *(const f32x4*)(kp + (int64_t)t * ldk);
    vv[t] = *(const f32x4*)(vp + (int64_t)t * ldv);
  }
  float sc[NK];
  float mx = -3.0e38f;
#pragma unroll
  for (int t = 0; t < NK; ++t) {
    float d = (qv[0] * kv[t][0] + qv[1] * kv[t][1]) + (qv[2] * kv[t][2] + qv[3] * kv[t][3]);
    // the four lanes of a (query, head) group are a DPP quad: xor 1 = quad_perm [1,0,3,2], xor 2 = [2,3,0,1] (no LDS trip)
    d += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, d), 0xB1, 0xF, 0xF, false));
    d += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, d), 0x4E, 0xF, 0xF, false));
    sc[t] = d;
    mx = fmaxf(mx, d);
  }
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < NK; ++t) { sc[t] = __builtin_amdgcn_exp2f(sc[t] - mx); sum += sc[t]; }
  const float inv = 1.f / sum;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < NK; ++t) acc += (sc[t] * inv) * vv[t];
  *(f32x4*)(O + bq * ldo + col) = acc;
}

// ---------------------------------------------------------------------------------------------
// Attention of a FEW queries (n_q <= 16) against many keys: SAM decoder token->image attention
// (7..16 tokens x 4096 image keys, 8 heads x 16; SA/modeling/transformer.py:163-168, 101-103), f32 rows, head_dim 16,
// n_heads % 4 == 0.  One workgroup serves (batch entry, 4 heads): a key row's 4-head slice is 256 contiguous bytes,
// 64-key K/V tiles are staged through LDS with 16-byte loads (each byte fetched once per workgroup), wave w owns queries
// QW w .. QW w + QW - 1, lane (kl = lane / 4, hl = lane % 4) streams keys kl, kl+16, ... of head hl with an online
// softmax, and the 16 key-lanes of a head are merged with in-wave shuffles.
//   QW = 2 (n_q <= 8, box prompts): the scaled queries live in registers.
//   QW = 4 (n_q 9..16, point prompts): they live in LDS and are read as broadcasts per tile - 64 query registers on top
//   of the 64 accumulators and the tile prefetch spill at two waves per SIMD.
// That is the only difference between the two instantiations: the per-query arithmetic (score order, one rescale per
// tile, merges, fold) is the same text, so a query gets the same bits from either.
template <int QW>
__global__ __launch_bounds__(512) void attn_fewq16_kernel(const float* __restrict__ Q, int64_t ldq,
                                                          const float* __restrict__ K, int64_t ldk,
                                                          const float* __restrict__ V, int64_t ldv, int n_q,
                                                          int n_k, int n_heads, float scale,
                                                          const int32_t* __restrict__ q_rows,
                                                          const int32_t* __restrict__ kv_rows,
                                                          const float* __restrict__ k_add,
                                                          float* __restrict__ O, int64_t ldo) {
  // KSPLIT groups of four waves share the key range (group g streams keys [g, g + 1) * n_k / KSPLIT through its own LDS
  // tiles; the partial softmax states meet in LDS at the end): the launch is only n_batch x n_heads / 4 workgroups - one
  // per CU for 128 boxes - and one wave per SIMD leaves every LDS and memory latency exposed (round 3: 268 us for
  // 4096 keys x 128 boxes with a single group, whatever the tile size or prefetch depth).
  constexpr int KSPLIT = 2, HD = 16, HB = 4, TK = 64;
  constexpr int ROWE = HB * HD;                      // floats of K (or V) per key and 4-head group
  constexpr int CH = 4, NCH = ROWE / CH;             // floats per 16-byte chunk, chunks per row
  constexpr int NU = TK * NCH / 256;                 // chunks per thread and operand
  constexpr bool Q_IN_LDS = QW > 2;
  extern __shared__ __attribute__((aligned(16))) char fewq_smem[];
  const int grp = threadIdx.x >> 8;                  // key-range group of this wave
  float* sk = (float*)fewq_smem + grp * 2 * TK * ROWE;
  float* sv = sk + TK * ROWE;
  const int hgroups = n_heads / HB;
  const int b = blockIdx.x / hgroups, h0 = (blockIdx.x % hgroups) * HB;
  const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
  const int per = ((n_k + KSPLIT - 1) / KSPLIT + TK - 1) / TK * TK;      // keys per group, whole tiles
  const int k_lo = grp * per, k_hi = min(n_k, k_lo + per);
  const int kl = lane >> 2, hl = lane & 3;
  const int64_t q0 = q_rows ? (int64_t)q_rows[b] : (int64_t)b * n_q;
  const int64_t k0 = kv_rows ? (int64_t)kv_rows[b] : (int64_t)b * n_k;
  // the wave's queries, scaled (scores in log2 units: exp2 below); slots past n_q read query 0 and are never stored
  float* sq = (float*)fewq_smem + KSPLIT * 2 * TK * ROWE;     // Q_IN_LDS: [4 QW queries][4 heads][16], written by group 0
  float qr[QW][HD];                                           // otherwise: every lane holds its head's slice
  if (!Q_IN_LDS || (grp == 0 && kl == 0)) {
    const float sc2 = scale * 1.44269504088896340736f;
#pragma unroll
    for (int j = 0; j < QW; ++j) {
      const int qi = QW * wave + j;
      const float* pq = Q + (q0 + (qi < n_q ? qi : 0)) * ldq + (h0 + hl) * HD;
      load8(pq, qr[j]);
      load8(pq + 8, qr[j] + 8);
#pragma unroll
      for (int e = 0; e < HD; ++e) qr[j][e] *= sc2;
      if constexpr (Q_IN_LDS) {                      // visible after the first tile's barrier
        store8(sq + (qi * HB + hl) * HD, qr[j]);
        store8(sq + (qi * HB + hl) * HD + 8, qr[j] + 8);
      }
    }
  }
  float m[QW], l[QW], acc[QW][HD];
#pragma unroll
  for (int j = 0; j < QW; ++j) {
    m[j] = -3.0e38f;
    l[j] = 0.f;
#pragma unroll
    for (int i = 0; i < HD; ++i) acc[j][i] = 0.f;
  }
  // staging: TK rows x NCH chunks of 16 B per operand; thread t moves chunks t, t + 256, ...  The NEXT tile's chunks are
  // loaded into registers before the current tile is computed (round 3: without that every one of the n_k / 64 tiles
  // exposed a full memory round trip - 268 us for 4096 keys, of which the arithmetic is ~100).
  f32x4 rk[NU], rv[NU];
  auto fetch = [&](int t0) {
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int c = tid + 256 * u, row = c / NCH, col = c % NCH;
      rk[u] = rv[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (t0 + row < k_hi) {
        rk[u] = *(const f32x4*)(K + (k0 + t0 + row) * ldk + h0 * HD + col * CH);
        rv[u] = *(const f32x4*)(V + (k0 + t0 + row) * ldv + h0 * HD + col * CH);
        // per-key constant of the key projection, [n_k, n_heads*HD] f32
        if (k_add) rk[u] += *(const f32x4*)(k_add + (int64_t)(t0 + row) * n_heads * HD + h0 * HD + col * CH);
      }
    }
  };
  fetch(k_lo);
  for (int t0 = k_lo; t0 < k_lo + per; t0 += TK) {       // every group runs the same number of tiles: shared barriers
    __syncthreads();                                   // previous tile consumed
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int c = tid + 256 * u, row = c / NCH, col = c % NCH;
      *(f32x4*)(sk + row * ROWE + col * CH) = rk[u];
      *(f32x4*)(sv + row * ROWE + col * CH) = rv[u];
    }
    __syncthreads();
    if (t0 + TK < k_hi) fetch(t0 + TK);                // in flight under this tile's arithmetic
    // scores of the lane's four keys of this tile (base-2 exponent units: log2(e) is folded into the query scale), ONE
    // rescale of the running sums per tile and query
    float d[QW][TK / 16];
#pragma unroll
    for (int kk = 0; kk < TK / 16; ++kk) {
      const int key = kk * 16 + kl;
      float kf[HD];
      load8(sk + key * ROWE + hl * HD, kf);
      load8(sk + key * ROWE + hl * HD + 8, kf + 8);
      const bool in = t0 + key < k_hi;
#pragma unroll
      for (int j = 0; j < QW; ++j) {
        float qf[HD];
        if constexpr (Q_IN_LDS) {
          load8(sq + ((QW * wave + j) * HB + hl) * HD, qf);
          load8(sq + ((QW * wave + j) * HB + hl) * HD + 8, qf + 8);
        } else {
#pragma unroll
          for (int e = 0; e < HD; ++e) qf[e] = qr[j][e];
        }
        float a0 = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          a0 = fmaf(qf[e], kf[e], a0);
          a0 = fmaf(qf[8 + e], kf[8 + e], a0);
        }
        d[j][kk] = in ? a0 : -3.0e38f;
      }
    }
    float n[QW];
#pragma unroll
    for (int j = 0; j < QW; ++j) {
      n[j] = m[j];
#pragma unroll
      for (int kk = 0; kk < TK / 16; ++kk) n[j] = fmaxf(n[j], d[j][kk]);
      const float sj = __builtin_amdgcn_exp2f(m[j] - n[j]);
      l[j] *= sj;
#pragma unroll
      for (int e = 0; e < HD; ++e) acc[j][e] *= sj;
      m[j] = n[j];
    }
#pragma unroll
    for (int kk = 0; kk < TK / 16; ++kk) {
      const int key = kk * 16 + kl;
      float vf[HD];
      load8(sv + key * ROWE + hl * HD, vf);
      load8(sv + key * ROWE + hl * HD + 8, vf + 8);
      const bool in = t0 + key < k_hi;
#pragma unroll
      for (int j = 0; j < QW; ++j) {
        const float pj = in ? __builtin_amdgcn_exp2f(d[j][kk] - n[j]) : 0.f;
        l[j] += pj;
#pragma unroll
        for (int e = 0; e < HD; ++e) acc[j][e] = fmaf(pj, vf[e], acc[j][e]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < QW; ++j) {
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) {               // the 16 key-lanes of this head: lane bits 2..5
      const float mo = __shfl_xor(m[j], o, 64), lo = __shfl_xor(l[j], o, 64);
      const float mn = fmaxf(m[j], mo);
      const float a = __builtin_amdgcn_exp2f(m[j] - mn), bsc = __builtin_amdgcn_exp2f(mo - mn);
      l[j] = l[j] * a + lo * bsc;
#pragma unroll
      for (int i = 0; i < HD; ++i) acc[j][i] = acc[j][i] * a + __shfl_xor(acc[j][i], o, 64) * bsc;
      m[j] = mn;
    }
  }
  // groups 1.. park their states (m, l, acc[16]) per (wave, query slot, head lane) in LDS; group 0 folds them in
  __syncthreads();                                     // the last tiles are consumed: the K/V tiles can be overwritten
  float* st = (float*)fewq_smem;
  if (grp > 0 && kl == 0) {
#pragma unroll
    for (int j = 0; j < QW; ++j) {
      float* ps = st + ((((grp - 1) * 4 + wave) * QW + j) * 4 + hl) * 18;
      ps[0] = m[j];
      ps[1] = l[j];
#pragma unroll
      for (int i = 0; i < HD; ++i) ps[2 + i] = acc[j][i];
    }
  }
  __syncthreads();
  if (grp > 0) return;
  if (kl == 0) {
#pragma unroll
    for (int g2 = 1; g2 < KSPLIT; ++g2)
#pragma unroll
      for (int j = 0; j < QW; ++j) {
        const float* ps = st + ((((g2 - 1) * 4 + wave) * QW + j) * 4 + hl) * 18;
        const float mo = ps[0], mn = fmaxf(m[j], mo);
        const float a = __builtin_amdgcn_exp2f(m[j] - mn), bsc = __builtin_amdgcn_exp2f(mo - mn);
        l[j] = l[j] * a + ps[1] * bsc;
#pragma unroll
        for (int i = 0; i < HD; ++i) acc[j][i] = acc[j][i] * a + ps[2 + i] * bsc;
        m[j] = mn;
      }
#pragma unroll
    for (int j = 0; j < QW; ++j) {
      const int qi = QW * wave + j;
      if (qi < n_q) {
        const float inv = 1.f / l[j];
#pragma unroll
        for (int i = 0; i < HD; ++i) acc[j][i] *= inv;
        float* op = O + ((int64_t)b * n_q + qi) * ldo + (h0 + hl) * HD;
        store8(op, acc[j]);
        store8(op + 8, acc[j] + 8);
      }
    }
  }
}

}  // namespace

extern "C" int ink_attn_fewkeys(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V,
                                int64_t ldv, int32_t B, int32_t n_q, int32_t n_k, int32_t n_heads,
                                int32_t head_dim, float scale, const uint8_t* blocked,
                                const int32_t* q_batch_rows, const float* q_add, int32_t io_f32, void* O,
                                int64_t ldo, void* stream) {
  INK_CHECK_ARG(Q && K && V && O && B > 0 && n_q > 0 && n_k > 0 && n_k <= 16 && n_heads > 0);
  INK_CHECK_ARG(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0);
  INK_CHECK_ARG(io_f32 == 0 || io_f32 == 1);
  // every kernel moves 16-byte vectors: with ld % 8 == 0 an aligned base keeps every row aligned
  INK_CHECK_ARG(ink_aligned<16>(Q, K, V, O, q_add));
  const int64_t total = (int64_t)B * n_q * n_heads;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
#define INK_FEWKEYS(HD, T)                                                                                     \
  hipLaunchKernelGGL((attn_fewkeys_kernel<HD, T>), grid, block, 0, s, (const T*)Q, ldq, (const T*)K, ldk,      \
                     (const T*)V, ldv, B, n_q, n_k, n_heads, scale, blocked, q_batch_rows, q_add, (T*)O, ldo)
  if (head_dim == 32 && !io_f32) INK_FEWKEYS(32, f16);
  else if (head_dim == 64 && !io_f32) INK_FEWKEYS(64, f16);
  else if (!io_f32) return INK_ERR_ARG;                    // f16 rows: the detector's head_dim 32 and 64 only
  else if (head_dim == 32) INK_FEWKEYS(32, float);
  else if (head_dim == 16 && !blocked && n_k >= 7) {        // SAM's 5 output tokens + 2..11 prompt tokens
    const dim3 g4((unsigned)((total * 4 + 255) / 256));
#define INK_FEWKEYS16(NK)                                                                                        \
  case NK:                                                                                                      \
    hipLaunchKernelGGL(attn_fewkeys16_f32_kernel<NK>, g4, block, 0, s, (const float*)Q, ldq, (const float*)K, ldk, \
                       (const float*)V, ldv, B, n_q, n_heads, scale, q_batch_rows, q_add, (float*)O, ldo);         \
    break
    switch (n_k) {
      INK_FEWKEYS16(7); INK_FEWKEYS16(8); INK_FEWKEYS16(9); INK_FEWKEYS16(10); INK_FEWKEYS16(11);
      INK_FEWKEYS16(12); INK_FEWKEYS16(13); INK_FEWKEYS16(14); INK_FEWKEYS16(15); INK_FEWKEYS16(16);
      default: return INK_ERR_ARG;                          // an n_k without an instantiation must not pass silently
    }
#undef INK_FEWKEYS16
  } else if (head_dim == 16) INK_FEWKEYS(16, float);
  else return INK_ERR_ARG;
#undef INK_FEWKEYS
  return ink_launch_status();
}

// both entry points of attn_midkeys_kernel: k_len == nullptr and blocked_stride == 0 is the uniform form
static int midkeys_launch(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                          int32_t B, int32_t n_q, int32_t n_k, int32_t n_heads, int32_t head_dim, float scale,
                          const uint8_t* blocked, int64_t blocked_stride, const int32_t* k_len, void* O, int64_t ldo,
                          void* stream) {
  INK_CHECK_ARG(Q && K && V && O && B > 0 && n_q > 0 && n_k > 0 && n_k <= 256 && n_heads > 0);
  INK_CHECK_ARG(head_dim == 32 || head_dim == 64);
  INK_CHECK_ARG(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0);
  INK_CHECK_ARG(ink_aligned<16>(Q, K, V, O));            // 16-byte vectors, as in ink_attn_fewkeys
  const int64_t total = (int64_t)B * n_q * n_heads;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
#define INK_MIDKEYS(HD)                                                                                            \
  hipLaunchKernelGGL(attn_midkeys_kernel<HD>, grid, block, 0, (hipStream_t)stream, (const f16*)Q, ldq,             \
                     (const f16*)K, ldk, (const f16*)V, ldv, B, n_q, n_k, n_heads, scale, blocked, blocked_stride, \
                     k_len, (f16*)O, ldo)
  if (head_dim == 32) INK_MIDKEYS(32); else INK_MIDKEYS(64);
#undef INK_MIDKEYS
  return ink_launch_status();
}

extern "C" int ink_attn_midkeys(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V,
                                int64_t ldv, int32_t B, int32_t n_q, int32_t n_k, int32_t n_heads,
                                int32_t head_dim, float scale, const uint8_t* blocked, void* O, int64_t ldo,
                                void* stream) {
  return midkeys_launch(Q, ldq, K, ldk, V, ldv, B, n_q, n_k, n_heads, head_dim, scale, blocked, 0, nullptr, O, ldo,
                        stream);
}

extern "C" int ink_attn_midkeys_varlen(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V,
                                       int64_t ldv, int32_t B, int32_t n_q, int32_t n_k, int32_t n_heads,
                                       int32_t head_dim, float scale, const uint8_t* blocked,
                                       int64_t blocked_batch_stride, const int32_t* k_len, void* O, int64_t ldo,
                                       void* stream) {
  INK_CHECK_ARG(blocked_batch_stride >= 0 && (blocked || blocked_batch_stride == 0) && ink_aligned<4>(k_len));
  return midkeys_launch(Q, ldq, K, ldk, V, ldv, B, n_q, n_k, n_heads, head_dim, scale, blocked, blocked_batch_stride,
                        k_len, O, ldo, stream);
}

extern "C" int ink_attn_fewq(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                             int32_t n_batch, int32_t n_q, int32_t n_k, int32_t n_heads, int32_t head_dim,
                             float scale, const int32_t* q_batch_rows, const int32_t* kv_batch_rows,
                             const float* k_add, void* O, int64_t ldo, void* stream) {
  INK_CHECK_ARG(Q && K && V && O && n_batch > 0 && n_q > 0 && n_q <= 16 && n_k > 0 && n_heads > 0);
  INK_CHECK_ARG(head_dim == 16 && n_heads % 4 == 0);
  INK_CHECK_ARG(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0);
  INK_CHECK_ARG(ink_aligned<16>(Q, K, V, O, k_add));   // 16-byte loads and stores
  // two key-range groups x (K, V) tiles of 64 keys x 4 heads x 16 f32; at 4 queries per wave also the scaled queries
  constexpr int lds2 = 2 * 2 * 64 * 64 * 4, lds4 = lds2 + 16 * 64 * 4;
  ink_dyn_lds<attn_fewq16_kernel<2>>(lds2);
  ink_dyn_lds<attn_fewq16_kernel<4>>(lds4);
  const bool wide = n_q > 8;                            // 9..16 queries: 4 per wave
  hipLaunchKernelGGL(wide ? attn_fewq16_kernel<4> : attn_fewq16_kernel<2>, dim3(n_batch * (n_heads / 4)), dim3(512),
                     wide ? lds4 : lds2, (hipStream_t)stream, (const float*)Q, ldq, (const float*)K, ldk,
                     (const float*)V, ldv, n_q, n_k, n_heads, scale, q_batch_rows, kv_batch_rows, k_add, (float*)O, ldo);
  return ink_launch_status();
}
