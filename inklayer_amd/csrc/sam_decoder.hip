// SAM prompt-encoder / mask-decoder tail kernels (small, HBM/latency bound).
#include "common.h"
#include "sam_postprocess.h"
#include "../../include/inklayer_hip.h"

namespace {

// Feature f of PositionEmbeddingRandom._pe_encoding at a point (x, y) in [0, 1]^2: sin / cos(2*pi*((2c-1) @ G[:, f]))
__device__ __forceinline__ void pe_feature(float x, float y, const float* __restrict__ G, int F, int f, float& sv,
                                           float& cv) {
  const float cx = 2.f * x - 1.f, cy = 2.f * y - 1.f;
  float v = cx * G[f] + cy * G[F + f];
  v = 6.283185307179586f * v;
  sv = sinf(v);
  cv = cosf(v);
}

// PositionEmbeddingRandom._pe_encoding: out = [sin(2*pi*((2c-1) @ G)), cos(..)]
__global__ __launch_bounds__(256) void pe_encode_kernel(const float* __restrict__ coords,
                                                        const float* __restrict__ G, int N, int F,
                                                        const float* __restrict__ add, int n_add,
                                                        float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N * F) return;
  const int n = i / F, f = i % F;
  float sv, cv;
  pe_feature(coords[2 * n], coords[2 * n + 1], G, F, f, sv, cv);
  if (add) {
    const float* ar = add + (int64_t)(n % n_add) * 2 * F;
    sv += ar[f];
    cv += ar[F + f];
  }
  out[(int64_t)n * 2 * F + f] = sv;
  out[(int64_t)n * 2 * F + F + f] = cv;
}

// The whole token block of P prompts, [P, NT, 2F] with NT = 5 + n_pts + pad + 2 * (boxes != null): the 5 output tokens
// (iou + 4 mask tokens, copied), then PromptEncoder._embed_points and _embed_boxes (SA/modeling/prompt_encoder.py:73-100,
// 128-166).  Points and boxes are in the resized-input frame; the +0.5 pixel-centre shift and the division by the input
// size happen here in f32, as the reference does them.  The pad point (0, 0) is appended after the shift, unshifted.
// Label -1: not_a_point_embed in place of the positional encoding; 0 / 1: PE + point_embeddings[label]; any other
// label: the PE alone.  pemb = point_embeddings[0..3] ([4, 2F]: negative, positive, box corner 0, box corner 1).
__global__ __launch_bounds__(256) void prompt_tokens_kernel(const float* __restrict__ points,
                                                            const int32_t* __restrict__ labels, int n_pts, int pad,
                                                            const float* __restrict__ boxes, const float* __restrict__ G,
                                                            int F, const float* __restrict__ pemb,
                                                            const float* __restrict__ nap,
                                                            const float* __restrict__ out_tok, float size, int P, int NT,
                                                            float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)P * NT * F) return;
  const int f = (int)(i % F), t = (int)((i / F) % NT);
  const int64_t p = i / ((int64_t)F * NT);
  float* o = out + (p * NT + t) * 2 * F;
  if (t < 5) {
    o[f] = out_tok[t * 2 * F + f];
    o[F + f] = out_tok[t * 2 * F + F + f];
    return;
  }
  const int s = t - 5;
  float x, y;
  const float* add;
  if (s < n_pts + pad) {
    int lab = -1;
    x = y = 0.f;
    if (s < n_pts) {
      lab = labels[p * n_pts + s];
      x = (points[(p * n_pts + s) * 2] + 0.5f) / size;
      y = (points[(p * n_pts + s) * 2 + 1] + 0.5f) / size;
    }
    if (lab == -1) {                 // point_embedding[labels == -1] = 0; += not_a_point_embed
      o[f] = 0.f + nap[f];
      o[F + f] = 0.f + nap[F + f];
      return;
    }
    add = (lab == 0 || lab == 1) ? pemb + lab * 2 * F : nullptr;
  } else {
    const int c = s - n_pts - pad;   // box corner 0 / 1
    x = (boxes[p * 4 + 2 * c] + 0.5f) / size;
    y = (boxes[p * 4 + 2 * c + 1] + 0.5f) / size;
    add = pemb + (2 + c) * 2 * F;
  }
  float sv, cv;
  pe_feature(x, y, G, F, f, sv, cv);
  if (add) {
    sv += add[f];
    cv += add[F + f];
  }
  o[f] = sv;
  o[F + f] = cv;
}

// PromptEncoder.mask_downscaling (prompt_encoder.py:50-59) + the image embedding it is added to (mask_decoder.py:123-126),
// for E = 256 and mask_in_chans = 16: keys[p*g*g + tok] = emb[emb_rows[p] + tok] + Conv1x1(GELU(LN2d(Conv2x2(GELU(LN2d(
// Conv2x2(mask[p])))))))[tok].  Output token (y, x) depends on the 4x4 input patch at (4y, 4x) only.  One workgroup per
// (prompt, token row y): lanes 0..g-1 run the two tiny convolutions of one token each in registers (f32) and park the 16
// channels in LDS; then every wave writes whole 1-KiB output rows (lane = 4 channels of the 16 -> 256 projection, whose
// weights stay in registers).  Optionally the split-f16 GEMM operand of the keys ([hi | lo*64 | hi/64], ink_add_split_f16)
// is written in the same pass.
// prm (f32): conv1 w [4][2][2], b [4], ln1 w [4], b [4], conv2 w [16][4][2][2], b [16], ln2 w [16], b [16],
//            conv3 w [256][16], b [256]
constexpr int ME = 256, MC = 16, MC1 = MC / 4;
constexpr int MP_W1 = 0, MP_B1 = 16, MP_G1 = 20, MP_BE1 = 24, MP_W2 = 28, MP_B2 = 284, MP_G2 = 300, MP_BE2 = 316,
              MP_W3 = 332, MP_B3 = 332 + ME * MC, MP_TOTAL = MP_B3 + ME;

__global__ __launch_bounds__(256) void mask_embed_kernel(const float* __restrict__ mask, const float* __restrict__ emb,
                                                         const int32_t* __restrict__ emb_rows,
                                                         const float* __restrict__ prm, float eps, int g,
                                                         float* __restrict__ keys, f16* __restrict__ split) {
  __shared__ float s_h[64 * MC];
  const int p = blockIdx.x / g, y = blockIdx.x % g, tid = threadIdx.x;
  const int S = 4 * g;                                   // mask side
  if (tid < g) {
    const int x = tid;
    const float* mp = mask + ((int64_t)p * S + 4 * y) * S + 4 * x;
    f32x4 m[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) m[r] = *(const f32x4*)(mp + (int64_t)r * S);
    float h1[MC1][2][2];                                 // conv1 -> LayerNorm2d(4) -> GELU at the 2x2 positions
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float c[MC1], mu = 0.f;
#pragma unroll
        for (int ch = 0; ch < MC1; ++ch) {
          const float* w = prm + MP_W1 + ch * 4;
          float a = prm[MP_B1 + ch];
          a = fmaf(w[0], m[2 * i][2 * j], a);
          a = fmaf(w[1], m[2 * i][2 * j + 1], a);
          a = fmaf(w[2], m[2 * i + 1][2 * j], a);
          a = fmaf(w[3], m[2 * i + 1][2 * j + 1], a);
          c[ch] = a;
          mu += a;
        }
        mu *= 1.f / MC1;
        float var = 0.f;
#pragma unroll
        for (int ch = 0; ch < MC1; ++ch) var += (c[ch] - mu) * (c[ch] - mu);
        const float rs = 1.f / sqrtf(var * (1.f / MC1) + eps);
#pragma unroll
        for (int ch = 0; ch < MC1; ++ch)
          h1[ch][i][j] = gelu_erf(prm[MP_G1 + ch] * ((c[ch] - mu) * rs) + prm[MP_BE1 + ch]);
      }
    float c2[MC], mu = 0.f;                              // conv2 -> LayerNorm2d(16) -> GELU
#pragma unroll
    for (int o = 0; o < MC; ++o) {
      const float* w = prm + MP_W2 + o * MC1 * 4;
      float a = prm[MP_B2 + o];
#pragma unroll
      for (int ch = 0; ch < MC1; ++ch)
#pragma unroll
        for (int k = 0; k < 4; ++k) a = fmaf(w[ch * 4 + k], h1[ch][k >> 1][k & 1], a);
      c2[o] = a;
      mu += a;
    }
    mu *= 1.f / MC;
    float var = 0.f;
#pragma unroll
    for (int o = 0; o < MC; ++o) var += (c2[o] - mu) * (c2[o] - mu);
    const float rs = 1.f / sqrtf(var * (1.f / MC) + eps);
#pragma unroll
    for (int o = 0; o < MC; ++o) s_h[x * MC + o] = gelu_erf(prm[MP_G2 + o] * ((c2[o] - mu) * rs) + prm[MP_BE2 + o]);
  }
  __syncthreads();
  // conv3 (1x1, 16 -> 256) + the image embedding: lane = channels 4 c4 .. 4 c4 + 3, wave w = tokens w, w + 4, ...
  const int c4 = tid & 63, w = tid >> 6;
  float w3[4][MC], b3[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    b3[e] = prm[MP_B3 + 4 * c4 + e];
#pragma unroll
    for (int o = 0; o < MC; ++o) w3[e][o] = prm[MP_W3 + (4 * c4 + e) * MC + o];
  }
  for (int x = w; x < g; x += 4) {
    const float* h = s_h + x * MC;
    f32x4 d;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float a = b3[e];
#pragma unroll
      for (int o = 0; o < MC; ++o) a = fmaf(w3[e][o], h[o], a);
      d[e] = a;
    }
    const int tok = y * g + x;
    const f32x4 v = *(const f32x4*)(emb + ((int64_t)emb_rows[p] + tok) * ME + 4 * c4) + d;
    const int64_t row = (int64_t)p * g * g + tok;
    *(f32x4*)(keys + row * ME + 4 * c4) = v;
    if (split) {
      f16 hi[4], lo[4], hs[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) split_f16(v[e], hi[e], lo[e], hs[e]);
      f16* sp = split + row * 3 * ME + 4 * c4;
      *(f16x4*)sp = (f16x4){hi[0], hi[1], hi[2], hi[3]};
      *(f16x4*)(sp + ME) = (f16x4){lo[0], lo[1], lo[2], lo[3]};
      *(f16x4*)(sp + 2 * ME) = (f16x4){hs[0], hs[1], hs[2], hs[3]};
    }
  }
}

// masks[n, 4y+2dy1+dy2, 4x+2dx1+dx2] = hyper[n,:] . up[((n*g*g + y*g + x)*4 + s1)*4 + s2, :]
template <int C>
__global__ __launch_bounds__(256) void mask_logits_kernel(const float* __restrict__ up,
                                                          const float* __restrict__ hyper, int n,
                                                          int g, float* __restrict__ out) {
  const int64_t total = (int64_t)n * g * g * 16;
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= total) return;
  const int s2 = (int)(r & 3), s1 = (int)((r >> 2) & 3);
  const int64_t tok = r >> 4;
  const int x = (int)(tok % g), y = (int)((tok / g) % g);
  const int b = (int)(tok / ((int64_t)g * g));
  const float* u = up + r * C;
  const float* h = hyper + (int64_t)b * C;
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < C; c += 4) {
    const f32x4 uv = *(const f32x4*)(u + c);
    const f32x4 hv = *(const f32x4*)(h + c);
    acc = fmaf(hv[0], uv[0], acc);
    acc = fmaf(hv[1], uv[1], acc);
    acc = fmaf(hv[2], uv[2], acc);
    acc = fmaf(hv[3], uv[3], acc);
  }
  const int Y = 4 * y + 2 * (s1 >> 1) + (s2 >> 1), X = 4 * x + 2 * (s1 & 1) + (s2 & 1);
  out[((int64_t)b * 4 * g + Y) * 4 * g + X] = acc;
}

// Sam.postprocess_masks + threshold, fused: low [n, S, S] -> (virtual) [L, L] -> crop
// [in_h, in_w] -> [out_h, out_w] -> (> thr) as uint8.  Nothing but the bool mask is written.
// The per-pixel arithmetic is post_pixel / post_cols + post_row of sam_postprocess.h.
__global__ __launch_bounds__(256) void postprocess_kernel(const float* __restrict__ low, int n, int S,
                                                          int L, int in_h, int in_w, int out_h,
                                                          int out_w, float thr,
                                                          uint8_t* __restrict__ out,
                                                          float* __restrict__ out_logits) {
  const int64_t total = (int64_t)n * out_h * out_w;
  const PostScales sc = post_scales(S, L, in_h, in_w, out_h, out_w);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int X = (int)(i % out_w), Y = (int)((i / out_w) % out_h);
    const int b = (int)(i / ((int64_t)out_w * out_h));
    const float v = post_pixel(low + (int64_t)b * S * S, S, sc, in_h, in_w, Y, X);
    if (out) out[i] = v > thr ? 1 : 0;
    if (out_logits) out_logits[i] = v;
  }
}

// Same arithmetic, four consecutive output pixels of one row per thread, workgroups walking ROWS: the mask goes out
// as one packed 4-byte store per lane instead of four one-byte stores (the one-pixel form is bound by store
// INSTRUCTIONS: 2.1 M of them for 128 masks of 1024^2, 710 us), and everything that depends on the column only -
// the second-stage source columns and weights and, for each of them, the first-stage columns and weights - is
// computed once per thread instead of once per pixel (the index/weight arithmetic was ~half of the instructions).
// The body states post_cols + post_row of sam_postprocess.h in place: written through those functions the kernel
// allocates 168 instead of 126 VGPRs (one wave per SIMD less), so the text stays here and amg.hip's kernels, which call
// the functions, are held to these floats bit for bit by tests/test_amg_gpu.py.
__global__ __launch_bounds__(256) void postprocess_rows_kernel(const float* __restrict__ low, int n, int S, int L,
                                                               int in_h, int in_w, int out_h, int out_w, float thr,
                                                               uint8_t* __restrict__ out,
                                                               float* __restrict__ out_logits) {
  constexpr int PX = 4;
  const float sA = (float)S / (float)L;
  const float sBh = (float)in_h / (float)out_h, sBw = (float)in_w / (float)out_w;
  const int wq = out_w / PX;                         // out_w % 4 == 0 (checked by the launcher)
  for (int xq = threadIdx.x; xq < wq; xq += 256) {
    float lx[PX], lc[PX][2];
    int c0[PX][2], c1[PX][2];
#pragma unroll
    for (int px = 0; px < PX; ++px) {
      int x0, x1;
      bil(xq * PX + px, sBw, in_w, x0, x1, lx[px]);
      bil(x0, sA, S, c0[px][0], c1[px][0], lc[px][0]);
      bil(x1, sA, S, c0[px][1], c1[px][1], lc[px][1]);
    }
    for (int row = blockIdx.x; row < n * out_h; row += gridDim.x) {
      const int b = row / out_h, Y = row - b * out_h;
      const float* lp = low + (int64_t)b * S * S;
      int y0, y1;
      float ly;
      bil(Y, sBh, in_h, y0, y1, ly);
      int a0[2], a1[2];
      float la[2];
      bil(y0, sA, S, a0[0], a1[0], la[0]);
      bil(y1, sA, S, a0[1], a1[1], la[1]);
      const float* r00 = lp + a0[0] * S;
      const float* r01 = lp + a1[0] * S;
      const float* r10 = lp + a0[1] * S;
      const float* r11 = lp + a1[1] * S;
      float vals[PX];
#pragma unroll
      for (int px = 0; px < PX; ++px) {
        auto stageA = [&](const float* ra, const float* rb, float lav, int k) {
          const float v00 = ra[c0[px][k]], v01 = ra[c1[px][k]];
          const float v10 = rb[c0[px][k]], v11 = rb[c1[px][k]];
          return (1.f - lav) * ((1.f - lc[px][k]) * v00 + lc[px][k] * v01) + lav * ((1.f - lc[px][k]) * v10 + lc[px][k] * v11);
        };
        const float v00 = stageA(r00, r01, la[0], 0), v01 = stageA(r00, r01, la[0], 1);
        const float v10 = stageA(r10, r11, la[1], 0), v11 = stageA(r10, r11, la[1], 1);
        vals[px] = (1.f - ly) * ((1.f - lx[px]) * v00 + lx[px] * v01) + ly * ((1.f - lx[px]) * v10 + lx[px] * v11);
      }
      const int64_t o = (int64_t)row * out_w + (int64_t)xq * PX;
      if (out)
        *(uint32_t*)(out + o) = (uint32_t)(vals[0] > thr) | ((uint32_t)(vals[1] > thr) << 8) |
                                ((uint32_t)(vals[2] > thr) << 16) | ((uint32_t)(vals[3] > thr) << 24);
      if (out_logits) *(f32x4*)(out_logits + o) = (f32x4){vals[0], vals[1], vals[2], vals[3]};
    }
  }
}

}  // namespace

extern "C" int ink_sam_pe_encode(const float* coords01, const float* gauss, int32_t N, int32_t F,
                                 const float* add, int32_t n_add, float* out, void* stream) {
  INK_CHECK_ARG(coords01 && gauss && out && N > 0 && F > 0 && (!add || n_add > 0));
  hipLaunchKernelGGL(pe_encode_kernel, dim3((N * F + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     coords01, gauss, N, F, add, n_add, out);
  return ink_launch_status();
}

extern "C" int ink_sam_mask_logits(const float* up, const float* hyper, int32_t n, int32_t g,
                                   int32_t C, float* out, void* stream) {
  INK_CHECK_ARG(up && hyper && out && n > 0 && g > 0);
  const int64_t total = (int64_t)n * g * g * 16;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  if (C == 32) {
    hipLaunchKernelGGL(mask_logits_kernel<32>, grid, block, 0, (hipStream_t)stream, up, hyper, n, g, out);
  } else if (C == 8) {
    hipLaunchKernelGGL(mask_logits_kernel<8>, grid, block, 0, (hipStream_t)stream, up, hyper, n, g, out);
  } else {
    return INK_ERR_ARG;
  }
  return ink_launch_status();
}

extern "C" int ink_sam_postprocess(const float* low, int32_t n, int32_t S, int32_t L, int32_t in_h,
                                   int32_t in_w, int32_t out_h, int32_t out_w, float thr,
                                   void* out_u8, float* out_logits, void* stream) {
  INK_CHECK_ARG(low && (out_u8 || out_logits) && n > 0 && S > 0 && L >= S);
  INK_CHECK_ARG(in_h > 0 && in_w > 0 && in_h <= L && in_w <= L && out_h > 0 && out_w > 0);
  const int64_t total = (int64_t)n * out_h * out_w;
  if (out_w % 4 == 0 && (int64_t)n * out_h < (int64_t)1 << 30 && ink_aligned<4>(out_u8) &&
      ink_aligned<16>(out_logits)) {
    const int64_t rows = (int64_t)n * out_h;
    const int blocks = (int)(rows < 8192 ? rows : 8192);
    hipLaunchKernelGGL(postprocess_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, low, n, S, L, in_h,
                       in_w, out_h, out_w, thr, (uint8_t*)out_u8, out_logits);
    return ink_launch_status();
  }
  const int blocks = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
  hipLaunchKernelGGL(postprocess_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, low, n, S,
                     L, in_h, in_w, out_h, out_w, thr, (uint8_t*)out_u8, out_logits);
  return ink_launch_status();
}

extern "C" int ink_sam_prompt_tokens(const float* points, const int32_t* labels, int32_t n_pts, int32_t pad,
                                     const float* boxes, const float* gauss, int32_t F, const float* point_emb,
                                     const float* not_a_point, const float* out_tok, float input_size, int32_t P,
                                     float* out, void* stream) {
  INK_CHECK_ARG(gauss && point_emb && not_a_point && out_tok && out && P > 0 && F > 0 && input_size > 0.f);
  INK_CHECK_ARG(n_pts >= 0 && (n_pts == 0 || (points && labels)) && (pad == 0 || pad == 1));
  const int NT = 5 + n_pts + pad + (boxes ? 2 : 0);
  INK_CHECK_ARG(NT <= 16);
  const int64_t total = (int64_t)P * NT * F;
  hipLaunchKernelGGL(prompt_tokens_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     points, labels, n_pts, pad, boxes, gauss, F, point_emb, not_a_point, out_tok, input_size, P, NT, out);
  return ink_launch_status();
}

extern "C" int ink_sam_mask_embed(const float* mask, const float* emb, const int32_t* emb_rows, const float* params,
                                  int32_t n_params, float eps, int32_t P, int32_t g, float* keys, void* split_f16,
                                  void* stream) {
  INK_CHECK_ARG(mask && emb && emb_rows && params && keys && P > 0 && g > 0 && g <= 64 && n_params == MP_TOTAL);
  INK_CHECK_ARG(ink_aligned<16>(mask, emb, keys) && ink_aligned<8>(split_f16));
  hipLaunchKernelGGL(mask_embed_kernel, dim3((unsigned)(P * g)), dim3(256), 0, (hipStream_t)stream, mask, emb, emb_rows,
                     params, eps, g, keys, (f16*)split_f16);
  return ink_launch_status();
}
