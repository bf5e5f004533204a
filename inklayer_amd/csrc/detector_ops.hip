// Small GroundingDINO-side kernels (HBM / latency bound): Swin patch gather, patch-merge LayerNorm,
// GroupNorm, top-k query selection, sine position embedding of boxes, iterative box refinement.  (The text attentions
// against a handful of keys are in attn_few.hip, the image<->text fusion attention in fusion_fold.hip / biattn_wide.hip.)
#include "common.h"
#include "../../include/inklayer_hip.h"

namespace {

// ---------------------------------------------------------------------------------------------
// load_image normalisation + 4x4/s4 PatchEmbed gather: u8 HWC -> f16 [tokens, 64]
// (48 real columns c*16 + ky*4 + kx, 16 zero columns so that K % 32 == 0)
__global__ __launch_bounds__(256) void swin_patchify_kernel(const uint8_t* __restrict__ img, int h, int w,
                                                            int gh, int gw, f32x4 mean, f32x4 stdv,
                                                            f16* __restrict__ out) {
  const int tok = blockIdx.x * 256 + threadIdx.x;
  if (tok >= gh * gw) return;
  const int ty = tok / gw, tx = tok % gw;
  f16 v[64];
#pragma unroll
  for (int i = 48; i < 64; ++i) v[i] = (f16)0;
#pragma unroll
  for (int ky = 0; ky < 4; ++ky) {
    const int y = ty * 4 + ky;
#pragma unroll
    for (int kx = 0; kx < 4; ++kx) {
      const int x = tx * 4 + kx;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float f = 0.f;  // PatchEmbed pads the NORMALISED image with zeros (swin_transformer.py:483-487)
        if (y < h && x < w) f = ((float)img[((int64_t)y * w + x) * 3 + c] / 255.0f - mean[c]) / stdv[c];
        v[c * 16 + ky * 4 + kx] = (f16)f;
      }
    }
  }
  f16x8* o = (f16x8*)(out + (int64_t)tok * 64);
#pragma unroll
  for (int i = 0; i < 8; ++i)
    o[i] = (f16x8){v[8 * i], v[8 * i + 1], v[8 * i + 2], v[8 * i + 3], v[8 * i + 4], v[8 * i + 5], v[8 * i + 6], v[8 * i + 7]};
}

// ---------------------------------------------------------------------------------------------
// PatchMerging: out[r] = LN(concat(x[g[r][0]], x[g[r][1]], x[g[r][2]], x[g[r][3]])) in f16; -1 = zero row.
// One wave per output row; 4C <= 4096.
template <int NV>
__global__ __launch_bounds__(256) void ln_merge4_kernel(const float* __restrict__ x, int64_t ldx,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps,
                                                        const int32_t* __restrict__ g4, int rows, int C,
                                                        f16* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int cv = C >> 2, nv = cv * 4;
  f32x4 r[NV];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int v = lane + 64 * j;
    r[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (v < nv) {
      const int src = g4[row * 4 + v / cv];
      if (src >= 0) r[j] = *(const f32x4*)(x + (int64_t)src * ldx + (v % cv) * 4);
    }
    s += (r[j][0] + r[j][1]) + (r[j][2] + r[j][3]);
  }
  const float n = (float)(4 * C);
  const float mean = wave_sum(s) / n;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    if (lane + 64 * j < nv) {
      const f32x4 d = r[j] - mean;
      q += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / n + eps);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int v = lane + 64 * j;
    if (v < nv) {
      f32x4 y = (r[j] - mean) * rstd * *(const f32x4*)(gamma + v * 4) + *(const f32x4*)(beta + v * 4);
      *(f16x4*)(out + (int64_t)row * 4 * C + v * 4) = (f16x4){(f16)y[0], (f16)y[1], (f16)y[2], (f16)y[3]};
    }
  }
}

// ---------------------------------------------------------------------------------------------
// GroupNorm(G, C) on NHWC tokens [B, T, C]: stats over (T x C/G) per (b, group).
__global__ __launch_bounds__(256) void groupnorm_stats_kernel(const float* __restrict__ x, int T, int C,
                                                              int G, float eps, float* __restrict__ stats) {
  const int b = blockIdx.x / G, g = blockIdx.x % G;
  const int cg = C / G;                     // 8 for GroupNorm(32, 256)
  const float* xb = x + (int64_t)b * T * C + g * cg;
  __shared__ float red[4];
  auto block_sum = [&](float v) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
  };
  float s = 0.f;
  for (int t = threadIdx.x; t < T; t += 256)
    for (int c = 0; c < cg; c += 4) {
      const f32x4 v = *(const f32x4*)(xb + (int64_t)t * C + c);
      s += (v[0] + v[1]) + (v[2] + v[3]);
    }
  const float n = (float)T * cg;
  const float mean = block_sum(s) / n;
  float q = 0.f;
  for (int t = threadIdx.x; t < T; t += 256)
    for (int c = 0; c < cg; c += 4) {
      const f32x4 d = *(const f32x4*)(xb + (int64_t)t * C + c) - mean;
      q += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
    }
  const float var = block_sum(q) / n;
  if (threadIdx.x == 0) {
    stats[blockIdx.x * 2] = mean;
    stats[blockIdx.x * 2 + 1] = 1.0f / sqrtf(var + eps);
  }
}
__global__ __launch_bounds__(256) void groupnorm_apply_kernel(const float* __restrict__ x, int T, int C,
                                                              int G, const float* __restrict__ stats,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta,
                                                              float* __restrict__ out, int64_t out_bstride,
                                                              int B) {
  const int cv = C / 4;
  const int64_t total = (int64_t)B * T * cv;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c4 = (int)(i % cv);
    const int64_t bt = i / cv;
    const int b = (int)(bt / T), t = (int)(bt % T);
    const int g = (c4 * 4) / (C / G);
    const float mean = stats[(b * G + g) * 2], rstd = stats[(b * G + g) * 2 + 1];
    const f32x4 v = (*(const f32x4*)(x + bt * C + c4 * 4) - mean) * rstd * *(const f32x4*)(gamma + c4 * 4) +
                    *(const f32x4*)(beta + c4 * 4);
    *(f32x4*)(out + (int64_t)b * out_bstride + (int64_t)t * C + c4 * 4) = v;
  }
}

// ---------------------------------------------------------------------------------------------
// f32 rows -> f16 with a row gather (-1 -> zeros): masked_fill of invalid proposals
// (utils.py:111-113) and the top-k gathers (transformer.py:302-316).
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ x, int64_t ldx,
                                                          const int32_t* __restrict__ idx,
                                                          int64_t idx_bstride, int64_t x_bstride_rows,
                                                          int rows_per_b, int B, int C,
                                                          f16* __restrict__ out_h, float* __restrict__ out_f) {
  const int cv = C / 4;
  const int64_t total = (int64_t)B * rows_per_b * cv;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c4 = (int)(i % cv);
    const int64_t r = i / cv;
    const int b = (int)(r / rows_per_b), rr = (int)(r % rows_per_b);
    const int src = idx[(int64_t)b * idx_bstride + rr];
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (src >= 0) v = *(const f32x4*)(x + ((int64_t)b * x_bstride_rows + src) * ldx + c4 * 4);
    if (out_h) *(f16x4*)(out_h + r * C + c4 * 4) = (f16x4){(f16)v[0], (f16)v[1], (f16)v[2], (f16)v[3]};
    if (out_f) *(f32x4*)(out_f + r * C + c4 * 4) = v;
  }
}

// ---------------------------------------------------------------------------------------------
// Two-stage query selection: key[s] = max_t logits[b,s,t]; indices of the K largest, in descending
// order, ties -> lower index (torch.topk leaves tie order unspecified).  One 1024-thread workgroup
// per image, bitonic sort of 64-bit (ordered-value, index) keys in LDS (S <= 16384 -> 128 KiB).
__device__ __forceinline__ void bitonic_sort_lds(unsigned long long* keys, int NP) {
  for (int size = 2; size <= NP; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = threadIdx.x; i < NP / 2; i += 1024) {
        const int lo = 2 * i - (i & (stride - 1));         // index with the `stride` bit clear
        const int hi = lo + stride;
        const bool up = (lo & size) == 0;
        const unsigned long long a = keys[lo], c = keys[hi];
        if ((a > c) == up) { keys[lo] = c; keys[hi] = a; }
      }
      __syncthreads();
    }
  }
}
__device__ __forceinline__ void emit_topk(const unsigned long long* keys, int K, int b, int32_t* out_idx,
                                          float* out_val) {
  for (int i = threadIdx.x; i < K; i += 1024) {
    const unsigned long long k = keys[i];
    out_idx[(int64_t)b * K + i] = (int)(k & 0xffffffffu);
    if (out_val) {
      unsigned u = ~(unsigned)(k >> 32);
      u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
      out_val[(int64_t)b * K + i] = __uint_as_float(u);
    }
  }
}
// pass 1: grid (B, nchunk); each workgroup sorts one chunk of <= 16384 tokens and keeps its K best keys
// (nchunk == 1: writes the final result directly)
__global__ __launch_bounds__(1024) void topk_kernel(const float* __restrict__ logits, int S, int T, int K,
                                                    int chunk, int NP, unsigned long long* __restrict__ cand,
                                                    int32_t* __restrict__ out_idx, float* __restrict__ out_val) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* keys = (unsigned long long*)smem;
  const int b = blockIdx.x, c = blockIdx.y, nchunk = gridDim.y;
  const float* lp = logits + (int64_t)b * S * T;
  const int s0 = c * chunk, s1 = min(S, s0 + chunk);
  for (int i = threadIdx.x; i < NP; i += 1024) {
    unsigned long long k = ~0ull;
    const int sidx = s0 + i;
    if (sidx < s1) {
      float v = lp[(int64_t)sidx * T];
      for (int t = 1; t < T; ++t) v = fmaxf(v, lp[(int64_t)sidx * T + t]);
      unsigned u = __float_as_uint(v);
      u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);     // monotone float -> uint
      k = ((unsigned long long)(~u) << 32) | (unsigned)sidx;  // ascending key == descending value, then index
    }
    keys[i] = k;
  }
  __syncthreads();
  bitonic_sort_lds(keys, NP);
  if (nchunk == 1) {
    emit_topk(keys, K, b, out_idx, out_val);
  } else {
    for (int i = threadIdx.x; i < K; i += 1024) cand[((int64_t)b * nchunk + c) * K + i] = keys[i];
  }
}
// pass 2: merge the nchunk * K candidates of one image
__global__ __launch_bounds__(1024) void topk_merge_kernel(const unsigned long long* __restrict__ cand, int n,
                                                          int K, int NP, int32_t* __restrict__ out_idx,
                                                          float* __restrict__ out_val) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* keys = (unsigned long long*)smem;
  const int b = blockIdx.x;
  for (int i = threadIdx.x; i < NP; i += 1024) keys[i] = i < n ? cand[(int64_t)b * n + i] : ~0ull;
  __syncthreads();
  bitonic_sort_lds(keys, NP);
  emit_topk(keys, K, b, out_idx, out_val);
}

// ---------------------------------------------------------------------------------------------
// gen_sineembed_for_position for 4-d boxes (utils.py:204-230): ref [N,4] (cx,cy,w,h) -> f16 [N,512]
// ordered (y, x, w, h) x 128, element i = sin / cos (i even / odd) of 2*pi*v / dim_t[i].
__global__ __launch_bounds__(256) void sine_embed4_kernel(const float* __restrict__ ref,
                                                          const float* __restrict__ dim_t, int N,
                                                          f16* __restrict__ out) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)N * 512) return;
  const int n = (int)(gid >> 9), c = (int)(gid & 511);
  const int j = c >> 7, i = c & 127;
  const int src = j == 0 ? 1 : (j == 1 ? 0 : j);
  const float v = ref[n * 4 + src] * 6.283185307179586f / dim_t[i];
  out[gid] = (f16)((i & 1) ? cosf(v) : sinf(v));
}

// new_ref = sigmoid(delta + inverse_sigmoid(ref))  (transformer.py:716-722, misc.py:704-708)
__global__ __launch_bounds__(256) void box_refine_kernel(const float* __restrict__ delta, int64_t ldd,
                                                         const float* __restrict__ ref, int N,
                                                         int ref_is_logit, float* __restrict__ out) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= N * 4) return;
  const int n = gid >> 2, c = gid & 3;
  float x = ref[gid];
  float lg = x;
  if (!ref_is_logit) {
    x = fminf(fmaxf(x, 0.f), 1.f);
    const float x1 = fmaxf(x, 1e-3f), x2 = fmaxf(1.f - x, 1e-3f);
    lg = logf(x1 / x2);
  }
  const float z = delta[(int64_t)n * ldd + c] + lg;
  out[gid] = 1.f / (1.f + expf(-z));
}

}  // namespace

extern "C" int ink_swin_patchify(const void* image_u8, int32_t h, int32_t w, const float* mean3,
                                 const float* std3, void* out_f16, void* stream) {
  INK_CHECK_ARG(image_u8 && mean3 && std3 && out_f16 && h > 0 && w > 0);
  const int gh = (h + 3) / 4, gw = (w + 3) / 4;
  const f32x4 m = {mean3[0], mean3[1], mean3[2], 0.f}, sd = {std3[0], std3[1], std3[2], 1.f};
  hipLaunchKernelGGL(swin_patchify_kernel, dim3((gh * gw + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)image_u8, h, w, gh, gw, m, sd, (f16*)out_f16);
  return ink_launch_status();
}

extern "C" int ink_layernorm_merge4(const float* x, int64_t ldx, const float* gamma, const float* beta,
                                    float eps, const int32_t* gather4, int32_t rows, int32_t C,
                                    void* out_f16, void* stream) {
  INK_CHECK_ARG(x && gamma && beta && gather4 && out_f16 && rows > 0 && C > 0 && C % 4 == 0 && C <= 1024);
  INK_CHECK_ARG(ldx % 4 == 0 && ldx >= C);
  const dim3 grid((rows + 3) / 4), block(256);
  hipStream_t s = (hipStream_t)stream;
  const int nv = (C + 63) / 64;  // float4 per lane over 4C values
#define INK_M4(NV) hipLaunchKernelGGL(ln_merge4_kernel<NV>, grid, block, 0, s, x, ldx, gamma, beta, eps, gather4, rows, C, (f16*)out_f16)
  if (nv <= 2) { INK_M4(2); } else if (nv <= 3) { INK_M4(3); } else if (nv <= 6) { INK_M4(6); } else if (nv <= 12) { INK_M4(12); } else { INK_M4(16); }
#undef INK_M4
  return ink_launch_status();
}

extern "C" int ink_groupnorm_nhwc(const float* x, int32_t B, int32_t T, int32_t C, int32_t G,
                                  const float* gamma, const float* beta, float eps, float* stats_ws,
                                  float* out, int64_t out_batch_stride, void* stream) {
  INK_CHECK_ARG(x && gamma && beta && stats_ws && out && B > 0 && T > 0 && G > 0 && C % G == 0 && (C / G) % 4 == 0);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(groupnorm_stats_kernel, dim3(B * G), dim3(256), 0, s, x, T, C, G, eps, stats_ws);
  const int64_t total = (int64_t)B * T * C / 4;
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(groupnorm_apply_kernel, dim3(blocks), dim3(256), 0, s, x, T, C, G, stats_ws, gamma, beta,
                     out, out_batch_stride, B);
  return ink_launch_status();
}

extern "C" int ink_gather_rows(const float* x, int64_t ldx, int64_t x_batch_rows, const int32_t* idx,
                               int64_t idx_batch_stride, int32_t rows_per_batch, int32_t B, int32_t C,
                               void* out_f16, float* out_f32, void* stream) {
  INK_CHECK_ARG(x && idx && (out_f16 || out_f32) && rows_per_batch > 0 && B > 0 && C > 0 && C % 4 == 0 && ldx % 4 == 0);
  const int64_t total = (int64_t)B * rows_per_batch * C / 4;
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(gather_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, ldx, idx,
                     idx_batch_stride, x_batch_rows, rows_per_batch, B, C, (f16*)out_f16, out_f32);
  return ink_launch_status();
}

extern "C" int ink_topk_rowmax(const float* logits, int32_t B, int32_t S, int32_t T, int32_t K,
                               int32_t* out_idx, float* out_val, void* cand_ws, void* stream) {
  constexpr int CHUNK = 16384;
  INK_CHECK_ARG(logits && out_idx && B > 0 && S > 0 && T > 0 && K > 0 && K <= S);
  const int nchunk = (S + CHUNK - 1) / CHUNK;
  INK_CHECK_ARG(nchunk == 1 || (cand_ws && K <= CHUNK / 2 && S - (nchunk - 1) * CHUNK >= 0 && nchunk * K <= 16384));
  INK_CHECK_ARG(nchunk == 1 || S / nchunk >= K);   // every chunk must hold at least K tokens
  ink_dyn_lds<topk_kernel>(CHUNK * 8);
  ink_dyn_lds<topk_merge_kernel>(CHUNK * 8);
  hipStream_t s = (hipStream_t)stream;
  // equal chunks so that each one has >= K tokens
  const int chunk = (S + nchunk - 1) / nchunk;
  int NP = 2;
  while (NP < chunk) NP <<= 1;
  hipLaunchKernelGGL(topk_kernel, dim3(B, nchunk), dim3(1024), NP * 8, s, logits, S, T, K, chunk, NP,
                     (unsigned long long*)cand_ws, out_idx, out_val);
  if (nchunk > 1) {
    const int n = nchunk * K;
    int NP2 = 2;
    while (NP2 < n) NP2 <<= 1;
    hipLaunchKernelGGL(topk_merge_kernel, dim3(B), dim3(1024), NP2 * 8, s, (const unsigned long long*)cand_ws, n, K,
                       NP2, out_idx, out_val);
  }
  return ink_launch_status();
}

extern "C" int ink_sine_embed4(const float* ref, const float* dim_t, int32_t N, void* out_f16, void* stream) {
  INK_CHECK_ARG(ref && dim_t && out_f16 && N > 0);
  const int64_t total = (int64_t)N * 512;
  hipLaunchKernelGGL(sine_embed4_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, ref, dim_t, N, (f16*)out_f16);
  return ink_launch_status();
}

extern "C" int ink_box_refine(const float* delta, int64_t ldd, const float* ref, int32_t N,
                              int32_t ref_is_logit, float* out, void* stream) {
  INK_CHECK_ARG(delta && ref && out && N > 0 && ldd >= 4);
  hipLaunchKernelGGL(box_refine_kernel, dim3((N * 4 + 255) / 256), dim3(256), 0, (hipStream_t)stream, delta,
                     ldd, ref, N, ref_is_logit, out);
  return ink_launch_status();
}
