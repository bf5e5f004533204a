// Closed-set post-processing of the detector (PostProcessCocoGrounding.forward, GD/demo/test_ap_on_coco.py:99-137, and
// the given-phrase mode of GD/demo/inference_on_a_image.py:117-142), on resident logits and boxes:
//   ink_class_scores   prob[b, q, c] = sum_t sigmoid(logits[b, q, t]) * positive_map[c, t]
//   ink_select_boxes   the boxes, labels and queries of the (query, class) indices ink_topk_rowmax selected
// Both are small next to the forward (B * nq * C * T <= 8 * 900 * 255 * 256 multiply-adds); what matters is that every
// load and store is coalesced, that no score leaves the device before the selection, and that a score is the same bits
// whatever else is in the batch.
#include "common.h"

namespace {

constexpr int CS_QB = 8;        // queries per workgroup: the positive map is re-read once per CS_QB queries
constexpr int CS_TMAX = 256;    // max_text_len of the reference (GD/config: max_text_len = 256)
constexpr int CS_CT = 64;       // classes per output tile

// Grid (ceil(nq / CS_QB), B), 256 threads = 4 waves.  The sigmoids of the workgroup's CS_QB rows are staged in LDS once
// (columns t >= T as 0).  Then a WAVE takes a class: lane l holds pm[c, l], pm[c, l + 64], pm[c, l + 128], pm[c, l + 192]
// (one coalesced read of the row per workgroup), forms its four terms upwards in t and the wave adds the 64 partials by
// the xor butterfly.  That order depends on t alone - not on T, C, B or the launch - so a column that contributes 0
// (a -inf logit, a zero map entry, t >= T) leaves the bits of the sum as they were: x + 0 == x.
// sigmoid(x) = 1 / (1 + exp(-x)) as torch's: -inf -> 1 / inf = 0 exactly, +inf -> 1 / 1 = 1 exactly, and no finite x
// leaves [0, 1], so no product is 0 * inf and no NaN can form from a NaN-free input.
__global__ __launch_bounds__(256) void class_scores_kernel(const float* __restrict__ logits, int64_t ld_row,
                                                           const float* __restrict__ pm, int64_t pm_image_stride,
                                                           const int32_t* __restrict__ n_cls, int nq, int T, int C,
                                                           float* __restrict__ out) {
  __shared__ float sig[CS_QB][CS_TMAX];
  __shared__ float res[CS_QB][CS_CT];
  const int b = blockIdx.y, q0 = blockIdx.x * CS_QB;
  const int nrow = min(CS_QB, nq - q0);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* lp = logits + ((int64_t)b * nq + q0) * ld_row;
  for (int i = tid; i < CS_QB * CS_TMAX; i += 256) {
    const int r = i >> 8, t = i & (CS_TMAX - 1);
    float s = 0.f;
    if (r < nrow && t < T) s = 1.f / (1.f + expf(-lp[(int64_t)r * ld_row + t]));
    sig[r][t] = s;
  }
  int ncls = C;
  if (n_cls) ncls = max(0, min(C, n_cls[b]));
  const float* pmb = pm + (int64_t)b * pm_image_stride;
  float* ob = out + ((int64_t)b * nq + q0) * C;
  __syncthreads();
  for (int c0 = 0; c0 < C; c0 += CS_CT) {
    const int nc = min(CS_CT, C - c0);
    for (int ci = wave; ci < nc; ci += 4) {
      const int c = c0 + ci;
      if (c >= ncls) continue;                     // wave-uniform: written as -1 below
      float p[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int t = lane + 64 * j;
        p[j] = t < T ? pmb[(int64_t)c * T + t] : 0.f;
      }
      const bool any = (p[0] != 0.f) | (p[1] != 0.f) | (p[2] != 0.f) | (p[3] != 0.f);
      if (__ballot(any) == 0ull) {                 // a class without a token: exactly 0
        if (lane < CS_QB) res[lane][ci] = 0.f;
        continue;
      }
#pragma unroll
      for (int r = 0; r < CS_QB; ++r) {
        float acc = sig[r][lane] * p[0];
        acc += sig[r][lane + 64] * p[1];
        acc += sig[r][lane + 128] * p[2];
        acc += sig[r][lane + 192] * p[3];
        acc = wave_sum(acc);
        if (lane == r) res[r][ci] = acc;
      }
    }
    __syncthreads();
    for (int i = tid; i < CS_QB * CS_CT; i += 256) {
      const int r = i >> 6, ci = i & (CS_CT - 1);
      if (r < nrow && ci < nc) ob[(int64_t)r * C + c0 + ci] = (c0 + ci) < ncls ? res[r][ci] : -1.0f;
    }
    __syncthreads();
  }
}

// One thread per selected (image, k).  An index outside [0, nq * Cmax) - nothing ink_topk_rowmax writes - reads no box:
// its box is zeros and its label and query are -1.
__global__ __launch_bounds__(256) void select_boxes_kernel(const int32_t* __restrict__ idx, const float* __restrict__ boxes,
                                                           const float* __restrict__ scale, int B, int K, int nq, int Cmax,
                                                           float* __restrict__ out_boxes, int32_t* __restrict__ labels,
                                                           int32_t* __restrict__ query) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= B * K) return;
  const int b = gid / K;
  const int i = idx[gid];
  int q = -1, lab = -1;
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  if (i >= 0 && i / Cmax < nq) {
    q = i / Cmax;
    lab = i - q * Cmax;
    const f32x4 bx = *(const f32x4*)(boxes + ((int64_t)b * nq + q) * 4);       // cx, cy, w, h
    const float W = scale[b * 2], H = scale[b * 2 + 1];
    const float hw = 0.5f * bx[2], hh = 0.5f * bx[3];
    o = (f32x4){(bx[0] - hw) * W, (bx[1] - hh) * H, (bx[0] + hw) * W, (bx[1] + hh) * H};
  }
  *(f32x4*)(out_boxes + (int64_t)gid * 4) = o;
  labels[gid] = lab;
  query[gid] = q;
}

}  // namespace

extern "C" int ink_class_scores(const float* logits, int64_t ld_row, const float* pos_map, int64_t pm_image_stride,
                                const int32_t* n_cls, int32_t B, int32_t nq, int32_t T, int32_t C, float* out,
                                void* stream) {
  INK_CHECK_ARG(logits && pos_map && out && B >= 1 && B <= 65535 && nq >= 1 && T >= 1 && T <= CS_TMAX && C >= 1);
  INK_CHECK_ARG(ld_row >= T && (pm_image_stride == 0 || pm_image_stride >= (int64_t)C * T));
  INK_CHECK_ARG((int64_t)nq * C <= INT32_MAX);             // a (query, class) index is an int32
  INK_CHECK_ARG(ink_aligned<4>(logits, pos_map, out) && ink_aligned<4>(n_cls));
  hipLaunchKernelGGL(class_scores_kernel, dim3((nq + CS_QB - 1) / CS_QB, B), dim3(256), 0, (hipStream_t)stream, logits,
                     ld_row, pos_map, pm_image_stride, n_cls, nq, T, C, out);
  return ink_launch_status();
}

extern "C" int ink_select_boxes(const int32_t* idx, const float* boxes, const float* scale_wh, int32_t B, int32_t K,
                                int32_t nq, int32_t Cmax, float* out_boxes, int32_t* labels, int32_t* query,
                                void* stream) {
  INK_CHECK_ARG(idx && boxes && scale_wh && out_boxes && labels && query && B >= 1 && K >= 1 && nq >= 1 && Cmax >= 1);
  INK_CHECK_ARG((int64_t)nq * Cmax <= INT32_MAX && (int64_t)B * K <= (1 << 30));
  INK_CHECK_ARG(ink_aligned<16>(boxes, out_boxes) && ink_aligned<4>(idx, labels, query) && ink_aligned<4>(scale_wh));
  hipLaunchKernelGGL(select_boxes_kernel, dim3((B * K + 255) / 256), dim3(256), 0, (hipStream_t)stream, idx, boxes,
                     scale_wh, B, K, nq, Cmax, out_boxes, labels, query);
  return ink_launch_status();
}
