// BERT text encoder kernels (GD/.../bertwarper.py:31-166 around HF BertModel): the two steps of the caption encoder
// that no other kernel of the library serves.  Everything else of a BERT layer is ink_gemm_f16 on split-f16 operands,
// ink_layernorm_rows and ink_add_split_f16 (inklayer_amd/text_encoder.py).
//   ink_text_embed_ln   HF BertEmbeddings: word + position + token-type rows, LayerNorm, f32 and split-f16 outputs.
//   ink_attn_text_f32   HF BertSelfAttention with bertwarper's sub-sentence block mask for a batch of PACKED captions:
//                       f32 rows read in place from the fused qkv projection, head_dim 64, K and V staged through LDS.
#include "common.h"
#include "../../include/inklayer_hip.h"

namespace {

// one wave per token row, the row in registers (C <= 2048 -> <= 8 float4 per lane), as layernorm_rows_kernel.  The
// ids are clamped into their tables here: device data cannot index out of range (the wrapper refuses bad host ids).
template <int NV>
__global__ __launch_bounds__(256) void text_embed_ln_kernel(const int32_t* __restrict__ ids,
                                                            const int32_t* __restrict__ pos_ids, int R,
                                                            const float* __restrict__ word, int V,
                                                            const float* __restrict__ pos, int P,
                                                            const float* __restrict__ type_row,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps, int C,
                                                            float* __restrict__ out_f, f16* __restrict__ out_h) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int nv = C >> 2;
  const int id = min(max(ids[row], 0), V - 1), pid = min(max(pos_ids[row], 0), P - 1);
  const float* wr = word + (int64_t)id * C;
  const float* pr = pos + (int64_t)pid * C;
  f32x4 r[NV];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int v = lane + 64 * j;
    r[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (v < nv) r[j] = (*(const f32x4*)(wr + v * 4) + *(const f32x4*)(type_row + v * 4)) + *(const f32x4*)(pr + v * 4);
    s += (r[j][0] + r[j][1]) + (r[j][2] + r[j][3]);
  }
  const float mean = wave_sum(s) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int v = lane + 64 * j;
    if (v < nv) {
      const f32x4 d = r[j] - mean;
      q += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int v = lane + 64 * j;
    if (v < nv) {
      const f32x4 y = (r[j] - mean) * rstd * *(const f32x4*)(gamma + v * 4) + *(const f32x4*)(beta + v * 4);
      *(f32x4*)(out_f + (int64_t)row * C + v * 4) = y;
      split_store(out_h + (int64_t)row * 3 * C + v * 4, C, y);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Self-attention of packed captions on f32 rows, head_dim 64.  A workgroup owns (caption, head, 64 queries); FOUR
// lanes per query hold 16 of the 64 dimensions each (q, the tile's partial and the running accumulator: 48 registers),
// so a wave is 16 queries.  The head's K and V rows pass through LDS in tiles of 64 keys (16 KiB each), once per
// workgroup; every lane group of a wave reads the SAME key row at four distinct 64-byte segments, which the LDS
// broadcasts without a bank conflict.  Per tile: 64 scores in registers (a lane's 16 products run as four fma chains of four, two additions and two
// shuffles join the partial dot products, and x + y == y + x makes the four lanes agree bit for bit), the tile's maximum, the weights and the
// tile's own value sum, then ONE rescale-and-merge into the running state - the online softmax at tile granularity, so
// an output carries at most 64 + n_tiles roundings of its value sum.  A tile in which none of the workgroup's queries
// is allowed a key (the caption masks are block-diagonal) is skipped before it is staged.  Loop bounds, tile skips and
// addresses derive from the workgroup's OWN caption alone: caption b's results are those of a launch on it alone.
constexpr int TQ = 64, TK = 64, HD = 64;

__global__ __launch_bounds__(256) void attn_text_f32_kernel(const float* __restrict__ Q, int64_t ldq,
                                                            const float* __restrict__ K, int64_t ldk,
                                                            const float* __restrict__ V, int64_t ldv,
                                                            const int32_t* __restrict__ row_start, int R, int Tmax,
                                                            int n_heads, float scale,
                                                            const uint8_t* __restrict__ blocked, int64_t blocked_stride,
                                                            f16* __restrict__ out_h, int64_t ldo,
                                                            float* __restrict__ out_f, int64_t ldf) {
  __shared__ __attribute__((aligned(16))) float Ks[TK * HD];
  __shared__ __attribute__((aligned(16))) float Vs[TK * HD];
  const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * TQ;
  // this caption's rows, clamped so that bad device data cannot index out of range
  const int r0 = min(max(row_start[b], 0), R);
  const int n = min(min(max(row_start[b + 1] - r0, 0), Tmax), R - r0);
  if (q0 >= n) return;                                     // uniform: the whole workgroup
  const int tid = threadIdx.x, part = tid & 3, q = q0 + (tid >> 2);
  const bool live = q < n;
  const uint8_t* brow = blocked ? blocked + b * blocked_stride + (int64_t)q * Tmax : nullptr;

  float qv[16], acc[16];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x4 t = live ? *(const f32x4*)(Q + (int64_t)(r0 + q) * ldq + h * HD + part * 16 + 4 * i)
                         : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) qv[4 * i + e] = t[e], acc[4 * i + e] = 0.f;
  }
  float m = -3.0e38f, l = 0.f;

  for (int k0 = 0; k0 < n; k0 += TK) {
    // allowed-key bits of this query for the tile: each lane tests 16 keys, the four lanes of a query OR them
    uint32_t w0 = 0, w1 = 0;
    {
      uint32_t bits = 0;
      if (live) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int t = k0 + part * 16 + j;
          if (t < n && !(brow && brow[t])) bits |= 1u << j;
        }
      }
      bits <<= 16 * (part & 1);
      w0 = part < 2 ? bits : 0u;
      w1 = part < 2 ? 0u : bits;
      w0 |= __shfl_xor(w0, 1, 64); w0 |= __shfl_xor(w0, 2, 64);
      w1 |= __shfl_xor(w1, 1, 64); w1 |= __shfl_xor(w1, 2, 64);
    }
    if (!__syncthreads_or((w0 | w1) != 0u)) continue;     // nothing to see in this tile (also orders the LDS reuse)

    // stage K and V rows k0 .. k0 + 63 of head h; rows past the caption's end are zeros and never read from memory
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int kr = (tid >> 4) + 16 * i, c4 = (tid & 15) * 4;
      f32x4 kk = (f32x4){0.f, 0.f, 0.f, 0.f}, vv = kk;
      if (k0 + kr < n) {
        kk = *(const f32x4*)(K + (int64_t)(r0 + k0 + kr) * ldk + h * HD + c4);
        vv = *(const f32x4*)(V + (int64_t)(r0 + k0 + kr) * ldv + h * HD + c4);
      }
      *(f32x4*)(Ks + kr * HD + c4) = kk;
      *(f32x4*)(Vs + kr * HD + c4) = vv;
    }
    __syncthreads();

    float sc[TK];
    float tm = -3.0e38f;
#pragma unroll
    for (int u = 0; u < TK; ++u) {
      f32x4 d4 = (f32x4){0.f, 0.f, 0.f, 0.f};              // four chains of four: eight roundings deep with the joins
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f32x4 kk = *(const f32x4*)(Ks + u * HD + part * 16 + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) d4[e] = fmaf(qv[4 * i + e], kk[e], d4[e]);
      }
      float d = (d4[0] + d4[1]) + (d4[2] + d4[3]);
      d += __shfl_xor(d, 1, 64);
      d += __shfl_xor(d, 2, 64);
      const bool ok = (((u < 32 ? w0 : w1) >> (u & 31)) & 1u) != 0u;
      sc[u] = ok ? d * scale : -3.0e38f;
      tm = fmaxf(tm, sc[u]);
    }
    if (tm > -1.0e38f) {                                   // this query sees a key of the tile
      const float mn = fmaxf(m, tm);
      float lt = 0.f, at[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) at[i] = 0.f;
#pragma unroll
      for (int u = 0; u < TK; ++u) {
        if (sc[u] > -1.0e38f) {                            // a blocked key's value row reaches no output
          const float pw = expf(sc[u] - mn);
          lt += pw;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const f32x4 vv = *(const f32x4*)(Vs + u * HD + part * 16 + 4 * i);
#pragma unroll
            for (int e = 0; e < 4; ++e) at[4 * i + e] = fmaf(pw, vv[e], at[4 * i + e]);
          }
        }
      }
      const float a = expf(m - mn);                        // first live tile: exp(-3e38 - mn) = 0 on acc = 0
      l = fmaf(l, a, lt);
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = fmaf(acc[i], a, at[i]);
      m = mn;
    }
  }
  if (!live) return;
  const float inv = l > 0.f ? 1.f / l : 0.f;             // no allowed key: zeros
  const int C = n_heads * HD;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x4 y = (f32x4){acc[4 * i] * inv, acc[4 * i + 1] * inv, acc[4 * i + 2] * inv, acc[4 * i + 3] * inv};
    const int c = h * HD + part * 16 + 4 * i;
    split_store(out_h + (int64_t)(r0 + q) * ldo + c, C, y);
    if (out_f) *(f32x4*)(out_f + (int64_t)(r0 + q) * ldf + c) = y;
  }
}

}  // namespace

extern "C" int ink_text_embed_ln(const int32_t* ids, const int32_t* pos_ids, int32_t R, const float* word, int32_t V,
                                 const float* pos, int32_t P, const float* type_row, const float* gamma,
                                 const float* beta, float eps, int32_t C, float* out_f32, void* out_split_f16,
                                 void* stream) {
  INK_CHECK_ARG(ids && pos_ids && word && pos && type_row && gamma && beta && out_f32 && out_split_f16);
  INK_CHECK_ARG(R > 0 && V > 0 && P > 0 && C > 0 && C % 4 == 0 && C <= 2048);
  INK_CHECK_ARG(ink_aligned<4>(ids, pos_ids));
  INK_CHECK_ARG(ink_aligned<16>(word, pos, type_row, gamma, beta, out_f32) && ink_aligned<16>(out_split_f16));
  const dim3 grid((R + 3) / 4), block(256);
  hipStream_t s = (hipStream_t)stream;
  const int nv = (C / 4 + 63) / 64;
#define INK_EMB(NV)                                                                                          \
  hipLaunchKernelGGL(text_embed_ln_kernel<NV>, grid, block, 0, s, ids, pos_ids, R, word, V, pos, P, type_row, \
                     gamma, beta, eps, C, out_f32, (f16*)out_split_f16)
  switch (nv) {
    case 1: INK_EMB(1); break;
    case 2: INK_EMB(2); break;
    case 3: INK_EMB(3); break;
    case 4: INK_EMB(4); break;
    default: INK_EMB(8); break;
  }
#undef INK_EMB
  return ink_launch_status();
}

extern "C" int ink_attn_text_f32(const float* Q, int64_t ldq, const float* K, int64_t ldk, const float* V, int64_t ldv,
                                 const int32_t* row_start, int32_t B, int32_t R, int32_t Tmax, int32_t n_heads,
                                 int32_t head_dim, float scale, const uint8_t* blocked, int64_t blocked_batch_stride,
                                 void* out_split_f16, int64_t ldo, float* out_f32, int64_t ldf, void* stream) {
  INK_CHECK_ARG(Q && K && V && row_start && out_split_f16);
  INK_CHECK_ARG(head_dim == HD && n_heads >= 1 && n_heads <= 65535);
  INK_CHECK_ARG(B >= 1 && B <= 65535 && R >= 1 && Tmax >= 1 && Tmax <= 256);
  const int64_t C = (int64_t)n_heads * HD;
  INK_CHECK_ARG(ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldq >= C && ldk >= C && ldv >= C);
  INK_CHECK_ARG(ldo % 8 == 0 && ldo >= 3 * C);
  INK_CHECK_ARG(!out_f32 || (ldf % 4 == 0 && ldf >= C));
  INK_CHECK_ARG(blocked_batch_stride >= 0 && (blocked || blocked_batch_stride == 0));
  INK_CHECK_ARG(ink_aligned<16>(Q, K, V, out_f32) && ink_aligned<16>(out_split_f16) && ink_aligned<4>(row_start));
  const dim3 grid((Tmax + TQ - 1) / TQ, n_heads, B), block(256);
  hipLaunchKernelGGL(attn_text_f32_kernel, grid, block, 0, (hipStream_t)stream, Q, ldq, K, ldk, V, ldv, row_start, R,
                     Tmax, n_heads, scale, blocked, blocked_batch_stride, (f16*)out_split_f16, ldo, out_f32,
                     ldf);
  return ink_launch_status();
}
