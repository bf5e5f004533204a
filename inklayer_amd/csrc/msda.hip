// Multi-scale deformable attention for gfx950 — replaces the reference's only native extension,
// groundingdino._C (GD/models/GroundingDINO/csrc/vision.cpp:54-55: ms_deform_attn_forward / _backward;
// forward kernel ms_deform_im2col_cuda.cuh:237-299, host ms_deform_attn_cuda.cu:21-81).
//
// The reference launches one thread per output ELEMENT (b,q,head,channel) and re-derives the 16
// sample positions per channel.  Here 4 lanes share one (query, head): each lane owns 8 of the 32
// channels (one 16-B f16 / two 16-B f32 gathers per corner), the sample geometry is computed once
// per 4-lane group, and a wave64 covers 2 queries x 8 heads.  Everything is a gather from an
// L2/Infinity-Cache resident value map (13294 x 256 f16 = 6.8 MB per image), so the kernel is
// bound by gather issue + L2 latency, not HBM: high occupancy (few VGPRs), no LDS.
//
// Entry points:
//   ink_ms_deform_attn_forward      — the reference's argument list with HOST shape tables (f32 value,
//                                     C == 32, L <= 8) for operator-level parity;
//   ink_ms_deform_attn_forward_dev  — the same op with the reference's DEVICE int64 shape tables, f32 or
//   ink_ms_deform_attn_backward_dev   f64, any C and L, and its gradient (grad_value by float atomics:
//                                     not bitwise reproducible run to run, as the reference's is not);
//   ink_msda_fused                  — what the pipeline uses: f16 value map, raw sampling_offsets /
//                                     attention_weights projections (one f32 GEMM output [.., 384]),
//                                     reference points; softmax over the 16 (level,point) logits and the
//                                     location arithmetic of ms_deform_attn.py:296-322 are done in-kernel
//                                     and the result is written in f16 for the output_proj GEMM.
// The first two share one kernel template (msda_fwd_kernel): at f32 they give the same bits.
#include "common.h"
#include "../../include/inklayer_hip.h"

namespace {

constexpr int MAXL = 8;

struct LevelInfo {
  int H[MAXL], W[MAXL], start[MAXL];
};

// Level tables of the reference-ABI forms.  HostLevels: validated on the host (positive sizes, contiguous starts,
// sum h*w == S) and passed by value.  DevLevels: the int64 device tables the reference takes, read in the kernel
// (wave-uniform addresses: scalar loads).  The host cannot check those without a synchronisation, so a level whose
// rows would leave [0, S) is skipped: an inconsistent table gives wrong numbers, never an out-of-bounds access.  A
// level that passes bounds every corner row it samples to [start, start + H*W) within [0, S).
struct HostLevels {
  LevelInfo li;
  __device__ __forceinline__ bool get(int l, int, int& H, int& W, int64_t& start) const {
    H = li.H[l];
    W = li.W[l];
    start = li.start[l];
    return true;
  }
};

struct DevLevels {
  const int64_t* shapes;   // [L, 2] (h, w)
  const int64_t* starts;   // [L]
  __device__ __forceinline__ bool get(int l, int S, int& H, int& W, int64_t& start) const {
    const int64_t h = shapes[2 * l], w = shapes[2 * l + 1], s = starts[l];
    const bool ok = h > 0 && w > 0 && h <= S && w <= S && s >= 0 && s <= S && s + h * w <= S;
    H = ok ? (int)h : 0;
    W = ok ? (int)w : 0;
    start = ok ? s : 0;
    return ok;
  }
};

// NV consecutive elements: 16-B loads / stores when NV * sizeof(T) is a multiple of 16 (the caller checks alignment)
template <typename T, int NV>
__device__ __forceinline__ void loadv(const T* p, T (&v)[NV]) {
  if constexpr (NV * sizeof(T) % 16 == 0) {
#pragma unroll
    for (int i = 0; i < (int)(NV * sizeof(T) / 16); ++i) {
      const f32x4 a = *(const f32x4*)((const char*)p + 16 * i);
      __builtin_memcpy((char*)v + 16 * i, &a, 16);
    }
  } else {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = p[i];
  }
}
template <typename T, int NV>
__device__ __forceinline__ void storev(T* p, const T (&v)[NV]) {
  if constexpr (NV * sizeof(T) % 16 == 0) {
#pragma unroll
    for (int i = 0; i < (int)(NV * sizeof(T) / 16); ++i) {
      f32x4 a;
      __builtin_memcpy(&a, (const char*)v + 16 * i, 16);
      *(f32x4*)((char*)p + 16 * i) = a;
    }
  } else {
#pragma unroll
    for (int i = 0; i < NV; ++i) p[i] = v[i];
  }
}

// bilinear sample of NV channels with zero padding (ms_deform_attn_im2col_bilinear, :33-84).  The per-channel
// arithmetic does not depend on NV: every vector width gives the same bits.
template <typename T, int NV>
__device__ __forceinline__ void sample_acc(const T* __restrict__ vbase, int64_t row_stride, int H, int W,
                                           T h_im, T w_im, T aw, T (&acc)[NV]) {
  if (!(h_im > (T)-1 && w_im > (T)-1 && h_im < (T)H && w_im < (T)W)) return;
  const int h0 = (int)floor(h_im), w0 = (int)floor(w_im);
  const T lh = h_im - (T)h0, lw = w_im - (T)w0;
  const T hh = (T)1 - lh, hw = (T)1 - lw;
  const T w00 = hh * hw * aw, w01 = hh * lw * aw, w10 = lh * hw * aw, w11 = lh * lw * aw;
  T v[NV];
  if (h0 >= 0 && w0 >= 0) {
    loadv<T, NV>(vbase + ((int64_t)h0 * W + w0) * row_stride, v);
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = fma(w00, v[i], acc[i]);
  }
  if (h0 >= 0 && w0 + 1 <= W - 1) {
    loadv<T, NV>(vbase + ((int64_t)h0 * W + w0 + 1) * row_stride, v);
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = fma(w01, v[i], acc[i]);
  }
  if (h0 + 1 <= H - 1 && w0 >= 0) {
    loadv<T, NV>(vbase + ((int64_t)(h0 + 1) * W + w0) * row_stride, v);
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = fma(w10, v[i], acc[i]);
  }
  if (h0 + 1 <= H - 1 && w0 + 1 <= W - 1) {
    loadv<T, NV>(vbase + ((int64_t)(h0 + 1) * W + w0 + 1) * row_stride, v);
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = fma(w11, v[i], acc[i]);
  }
}

// One sample for the fused kernel, branch-free: every corner is loaded from a clamped (always valid) address and an
// out-of-range corner / sample gets weight 0, so that the four gathers of the sample are in flight together (the
// conditional form above waits for each corner's load inside its own branch).  fma(0, v, acc) == acc for the finite f16
// values of the map and the accumulation order is unchanged.  (Two samples / all 16 gathers of a level in flight were tried:
// 16 / 48 more registers cost occupancy - 245 -> 394 / 370 us.)
__device__ __forceinline__ void sample_acc_bf(const f16* __restrict__ vbase, int64_t row_stride, int H, int W, float h_im,
                                              float w_im, float aw, float (&acc)[8]) {
  const bool in = h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W;
  const float hf = floorf(h_im), wf = floorf(w_im);
  const int h0 = in ? (int)hf : 0, w0 = in ? (int)wf : 0;
  const float lh = h_im - hf, lw = w_im - wf;
  const float hh = 1.f - lh, hw = 1.f - lw;
  const bool t = h0 >= 0, b = h0 + 1 <= H - 1, l = w0 >= 0, r = w0 + 1 <= W - 1;
  const float w00 = (in && t && l) ? hh * hw * aw : 0.f, w01 = (in && t && r) ? hh * lw * aw : 0.f;
  const float w10 = (in && b && l) ? lh * hw * aw : 0.f, w11 = (in && b && r) ? lh * lw * aw : 0.f;
  const int ht = max(h0, 0), hb = min(h0 + 1, H - 1), wl = max(w0, 0), wr = min(w0 + 1, W - 1);
  const f16x8 v00 = *(const f16x8*)(vbase + ((int64_t)ht * W + wl) * row_stride);
  const f16x8 v01 = *(const f16x8*)(vbase + ((int64_t)ht * W + wr) * row_stride);
  const f16x8 v10 = *(const f16x8*)(vbase + ((int64_t)hb * W + wl) * row_stride);
  const f16x8 v11 = *(const f16x8*)(vbase + ((int64_t)hb * W + wr) * row_stride);
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = fmaf(w00, (float)v00[i], acc[i]);
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = fmaf(w01, (float)v01[i], acc[i]);
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = fmaf(w10, (float)v10[i], acc[i]);
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = fmaf(w11, (float)v11[i], acc[i]);
}

// ---- reference-ABI forward: explicit locations + weights, f32 or f64 value, any C, any L.
// NV channels per lane (16-B gathers when C % NV == 0 and the buffers are 16-B aligned, NV = 1 otherwise), C / NV
// lanes per (b, q, m); the sample geometry is recomputed by each lane of the group.
template <typename T, int NV, typename Levels>
__global__ __launch_bounds__(256) void msda_fwd_kernel(const T* __restrict__ value, const T* __restrict__ loc,
                                                       const T* __restrict__ aw, Levels lv, int B, int S, int M,
                                                       int C, int Q, int L, int P, T* __restrict__ out) {
  const int nsl = C / NV;
  const int gid = xcd_remap(blockIdx.x, gridDim.x) * 256 + threadIdx.x;   // B*Q*M*nsl < 2^31: checked on the host
  const int qm = gid / nsl, sl = gid - qm * nsl;                          // (b, q, m) flat, channel slice
  if (qm >= B * Q * M) return;
  const int m = qm % M, b = qm / M / Q;
  T acc[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) acc[i] = 0;
  const T* lp = loc + (int64_t)qm * L * P * 2;
  const T* wp = aw + (int64_t)qm * L * P;
  const int64_t rs = (int64_t)M * C;
  for (int l = 0; l < L; ++l) {
    int H, W;
    int64_t start;
    if (!lv.get(l, S, H, W, start)) continue;
    const T* vb = value + ((int64_t)b * S + start) * rs + m * C + sl * NV;
    for (int p = 0; p < P; ++p) {
      const T lx = lp[(l * P + p) * 2], ly = lp[(l * P + p) * 2 + 1];
      sample_acc<T, NV>(vb, rs, H, W, ly * (T)H - (T)0.5, lx * (T)W - (T)0.5, wp[l * P + p], acc);
    }
  }
  storev<T, NV>(out + (int64_t)qm * C + sl * NV, acc);
}

template <int G, typename T>
__device__ __forceinline__ T group_sum(T v) {   // over aligned groups of G lanes
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- reference-ABI backward.  Per sample (b,q,m,l,p) with g = grad_output[b,q,m,:], corner rows v_ij, corner
// weights w_ij (zero for a corner outside the map) and sample_c = sum_ij w_ij v_ij,c:
//   grad_attn_weight = sum_c g_c sample_c
//   grad_loc.x = W * aw * sum_c g_c ((v01 - v00)(1 - lh) + (v11 - v10) lh)      (d w_im / d x = W)
//   grad_loc.y = H * aw * sum_c g_c ((v10 - v00)(1 - lw) + (v11 - v01) lw)      (d h_im / d y = H)
//   grad_value[corner ij] += w_ij * aw * g                                       (in-range corners only)
// One lane per channel: a group of G lanes (G = C rounded up to a power of two, at most 64) per (b, q, m), K
// channels per lane at stride G, so each atomic wave-instruction adds whole contiguous row segments (at C = 32 f32:
// two 128-B rows per wave).  g stays in registers across the L*P samples (when C <= G*K); the two sample sums are
// reduced across the group with shuffles and stored by its first lane: a sample belongs to exactly one group, so
// grad_loc / grad_attn_weight need no atomics.  A corner outside the map issues no atomic.  grad_value is zeroed on
// the stream by the entry point.  Float atomics sum in arrival order: grad_value is not bitwise reproducible.
template <typename T, int G, int K>
__global__ __launch_bounds__(256) void msda_bwd_kernel(const T* __restrict__ value, DevLevels lv,
                                                       const T* __restrict__ loc, const T* __restrict__ aw,
                                                       const T* __restrict__ gout, int B, int S, int M, int C,
                                                       int Q, int L, int P, T* __restrict__ gval,
                                                       T* __restrict__ gloc, T* __restrict__ gaw) {
  const int gid = xcd_remap(blockIdx.x, gridDim.x) * 256 + threadIdx.x;   // B*Q*M*G < 2^31: checked on the host
  const int qm = gid / G, lane = gid & (G - 1);
  if (qm >= B * Q * M) return;    // whole groups: G divides 256
  const int m = qm % M, b = qm / M / Q;
  const int64_t rs = (int64_t)M * C;
  const T* gp = gout + (int64_t)qm * C;
  const int nch = (C + G * K - 1) / (G * K);
  T g[K];
#pragma unroll
  for (int k = 0; k < K; ++k) g[k] = lane + G * k < C ? gp[lane + G * k] : (T)0;
  for (int l = 0; l < L; ++l) {
    int H, W;
    int64_t start;
    const bool lvl = lv.get(l, S, H, W, start);
    const int64_t vrow = ((int64_t)b * S + start) * rs + m * C;     // element offset of the level's first row
    for (int p = 0; p < P; ++p) {
      const int64_t i = ((int64_t)qm * L + l) * P + p;
      const T x = loc[2 * i], y = loc[2 * i + 1], a = aw[i];
      const T h_im = y * (T)H - (T)0.5, w_im = x * (T)W - (T)0.5;
      T sa = 0, sx = 0, sy = 0;
      if (lvl && h_im > (T)-1 && w_im > (T)-1 && h_im < (T)H && w_im < (T)W) {
        const int h0 = (int)floor(h_im), w0 = (int)floor(w_im);
        const T lh = h_im - (T)h0, lw = w_im - (T)w0;
        const T hh = (T)1 - lh, hw = (T)1 - lw;
        const T w00 = hh * hw, w01 = hh * lw, w10 = lh * hw, w11 = lh * lw;
        const bool t = h0 >= 0, bt = h0 + 1 <= H - 1, lf = w0 >= 0, rt = w0 + 1 <= W - 1;
        const bool k00 = t && lf, k01 = t && rt, k10 = bt && lf, k11 = bt && rt;
        const int64_t o00 = vrow + ((int64_t)h0 * W + w0) * rs, o01 = o00 + rs;
        const int64_t o10 = o00 + (int64_t)W * rs, o11 = o10 + rs;
        for (int ch = 0; ch < nch; ++ch) {
#pragma unroll
          for (int k = 0; k < K; ++k) {
            const int c = ch * G * K + lane + G * k;
            if (c >= C) continue;
            const T gc = nch == 1 ? g[k] : gp[c];
            const T v00 = k00 ? value[o00 + c] : (T)0, v01 = k01 ? value[o01 + c] : (T)0;
            const T v10 = k10 ? value[o10 + c] : (T)0, v11 = k11 ? value[o11 + c] : (T)0;
            sa += gc * (w00 * v00 + w01 * v01 + w10 * v10 + w11 * v11);
            sx += gc * (hh * (v01 - v00) + lh * (v11 - v10));
            sy += gc * (hw * (v10 - v00) + lw * (v11 - v01));
            const T ag = a * gc;
            if (k00) atomicAdd(gval + o00 + c, w00 * ag);
            if (k01) atomicAdd(gval + o01 + c, w01 * ag);
            if (k10) atomicAdd(gval + o10 + c, w10 * ag);
            if (k11) atomicAdd(gval + o11 + c, w11 * ag);
          }
        }
      }
      sa = group_sum<G>(sa);
      sx = group_sum<G>(sx);
      sy = group_sum<G>(sy);
      if (lane == 0) {
        gaw[i] = sa;
        gloc[2 * i] = (T)W * a * sx;
        gloc[2 * i + 1] = (T)H * a * sy;
      }
    }
  }
}

// ---- fused form: L == 4, P == 4, M == 8, C == 32 (GroundingDINO_SwinT_OGC.py)
template <int REFD>
__global__ __launch_bounds__(256) void msda_fused_kernel(const f16* __restrict__ value,
                                                         const float* __restrict__ proj, int64_t ldp,
                                                         const float* __restrict__ ref,
                                                         int64_t ref_q_stride, int64_t ref_b_stride,
                                                         LevelInfo li, int B, int S, int Q,
                                                         f16* __restrict__ out) {
  constexpr int M = 8, L = 4, P = 4, C = 32;
  // XCD-contiguous work order: workgroups are dealt round-robin to the 8 XCDs, so without the remap every XCD's
  // 4 MiB L2 would gather from the value maps of ALL images (6.8 MB each); with it XCD x works on one contiguous
  // eighth of the (image, query) space - one image's map at batch 8 - and consecutive queries sample nearby rows
  const int64_t gid = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
  const int c8 = (int)(gid & 3);
  const int64_t qm = gid >> 2;
  if (qm >= (int64_t)B * Q * M) return;
  const int m = (int)(qm % M);
  const int64_t bq = qm / M;
  const int b = (int)(bq / Q), q = (int)(bq % Q);
  const float* pr = proj + bq * ldp;
  // sampling_offsets: cols [0, 256) as (m, l, p, xy); attention logits: cols [256, 384) as (m, l, p)
  float off[L * P * 2], lg[L * P];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const f32x4 v = *(const f32x4*)(pr + m * 32 + 4 * i);
    off[4 * i] = v[0]; off[4 * i + 1] = v[1]; off[4 * i + 2] = v[2]; off[4 * i + 3] = v[3];
  }
  float mx = -3.0e38f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x4 v = *(const f32x4*)(pr + 256 + m * 16 + 4 * i);
#pragma unroll
    for (int j = 0; j < 4; ++j) { lg[4 * i + j] = v[j]; mx = fmaxf(mx, v[j]); }
  }
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) { lg[i] = expf(lg[i] - mx); sum += lg[i]; }
  const float inv = 1.f / sum;
  const float* rp = ref + (int64_t)b * ref_b_stride + (int64_t)q * ref_q_stride;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int64_t rs = (int64_t)M * C;
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const int H = li.H[l], W = li.W[l];
    const f16* vb = value + ((int64_t)b * S + li.start[l]) * rs + m * C + c8 * 8;
    // reference points are per level in the 2-d (encoder) form, shared across levels in the 4-d form
    float rx, ry, rw = 0.f, rh = 0.f;
    if (REFD == 2) {
      rx = rp[0]; ry = rp[1];
    } else {
      rx = rp[0]; ry = rp[1]; rw = rp[2]; rh = rp[3];
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const float ox = off[(l * P + p) * 2], oy = off[(l * P + p) * 2 + 1];
      float lx, ly;
      if (REFD == 2) {       // ref + off / (W_l, H_l)              (ms_deform_attn.py:309-314)
        lx = rx + ox / (float)W;
        ly = ry + oy / (float)H;
      } else {               // ref_xy + off / P * ref_wh * 0.5     (ms_deform_attn.py:315-322)
        lx = rx + ox / (float)P * rw * 0.5f;
        ly = ry + oy / (float)P * rh * 0.5f;
      }
      sample_acc_bf(vb, rs, H, W, ly * H - 0.5f, lx * W - 0.5f, lg[l * P + p] * inv, acc);
    }
  }
  f16x8 o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = (f16)acc[i];
  *(f16x8*)(out + qm * C + c8 * 8) = o;
}

template <typename T, int NV, typename Levels>
int launch_fwd(const void* value, const void* loc, const void* aw, Levels lv, int B, int S, int M, int C, int Q,
               int L, int P, void* out, hipStream_t s) {
  const int64_t threads = (int64_t)B * Q * M * (C / NV);
  hipLaunchKernelGGL((msda_fwd_kernel<T, NV, Levels>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s,
                     (const T*)value, (const T*)loc, (const T*)aw, lv, B, S, M, C, Q, L, P, (T*)out);
  return ink_launch_status();
}

// widest gather that C and the alignment of value / out allow: NVMAX (32 B per lane), NVMAX / 2 (16 B), 1
template <typename T, int NVMAX, typename Levels>
int dispatch_fwd(const void* value, const void* loc, const void* aw, Levels lv, int B, int S, int M, int C, int Q,
                 int L, int P, void* out, hipStream_t s) {
  const bool aligned = ink_aligned<16>(value, out);
  if (aligned && C % NVMAX == 0) return launch_fwd<T, NVMAX>(value, loc, aw, lv, B, S, M, C, Q, L, P, out, s);
  if (aligned && C % (NVMAX / 2) == 0) return launch_fwd<T, NVMAX / 2>(value, loc, aw, lv, B, S, M, C, Q, L, P, out, s);
  return launch_fwd<T, 1>(value, loc, aw, lv, B, S, M, C, Q, L, P, out, s);
}

template <typename T, int G, int K>
int launch_bwd(const void* value, DevLevels lv, const void* loc, const void* aw, const void* gout, int B, int S,
               int M, int C, int Q, int L, int P, void* gval, void* gloc, void* gaw, hipStream_t s) {
  const int64_t threads = (int64_t)B * Q * M * G;
  hipLaunchKernelGGL((msda_bwd_kernel<T, G, K>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s,
                     (const T*)value, lv, (const T*)loc, (const T*)aw, (const T*)gout, B, S, M, C, Q, L, P, (T*)gval,
                     (T*)gloc, (T*)gaw);
  return ink_launch_status();
}

template <typename T>
int dispatch_bwd(const void* value, DevLevels lv, const void* loc, const void* aw, const void* gout, int B, int S,
                 int M, int C, int Q, int L, int P, void* gval, void* gloc, void* gaw, hipStream_t s) {
  if (hipMemsetAsync(gval, 0, (size_t)B * S * M * C * sizeof(T), s) != hipSuccess) return INK_ERR_LAUNCH;
#define INK_MSDA_BWD(G, K) launch_bwd<T, G, K>(value, lv, loc, aw, gout, B, S, M, C, Q, L, P, gval, gloc, gaw, s)
  if (C > 64) return INK_MSDA_BWD(64, 4);
  if (C > 32) return INK_MSDA_BWD(64, 1);
  if (C > 16) return INK_MSDA_BWD(32, 1);
  if (C > 8) return INK_MSDA_BWD(16, 1);
  if (C > 4) return INK_MSDA_BWD(8, 1);
  if (C > 2) return INK_MSDA_BWD(4, 1);
  if (C > 1) return INK_MSDA_BWD(2, 1);
  return INK_MSDA_BWD(1, 1);
#undef INK_MSDA_BWD
}

// lanes per (b, q, m) of the backward: C rounded up to a power of two, at most 64
int bwd_group(int C) {
  int g = 1;
  while (g < C && g < 64) g <<= 1;
  return g;
}

}  // namespace

extern "C" int ink_ms_deform_attn_forward(const float* value, const int64_t* spatial_shapes_host,
                                          const int64_t* level_start_index_host,
                                          const float* sampling_loc, const float* attn_weight,
                                          int32_t B, int32_t S, int32_t M, int32_t C, int32_t Q,
                                          int32_t L, int32_t P, int32_t im2col_step, float* out,
                                          void* stream) {
  INK_CHECK_ARG(value && spatial_shapes_host && level_start_index_host && sampling_loc && attn_weight && out);
  INK_CHECK_ARG(B > 0 && S > 0 && M > 0 && Q > 0 && L > 0 && L <= MAXL && P > 0 && C == 32);
  INK_CHECK_ARG((int64_t)B * Q * M * C <= INT32_MAX - 255);
  // the reference requires batch % min(batch, im2col_step) == 0 (ms_deform_attn_cuda.cu:51-53)
  const int step = B < im2col_step ? B : im2col_step;
  INK_CHECK_ARG(im2col_step > 0 && B % step == 0);
  HostLevels lv;
  int64_t total = 0;
  for (int l = 0; l < L; ++l) {
    lv.li.H[l] = (int)spatial_shapes_host[2 * l];
    lv.li.W[l] = (int)spatial_shapes_host[2 * l + 1];
    lv.li.start[l] = (int)level_start_index_host[l];
    INK_CHECK_ARG(lv.li.H[l] > 0 && lv.li.W[l] > 0 && lv.li.start[l] == total);
    total += (int64_t)lv.li.H[l] * lv.li.W[l];
  }
  INK_CHECK_ARG(total == S);
  return dispatch_fwd<float, 8>(value, sampling_loc, attn_weight, lv, B, S, M, C, Q, L, P, out, (hipStream_t)stream);
}

// shared argument checks of the device-table forms; nothing is read through the pointers
static bool msda_dev_args_ok(int32_t dtype, int32_t B, int32_t S, int32_t M, int32_t C, int32_t Q, int32_t L,
                             int32_t P, int32_t im2col_step) {
  if (dtype != 0 && dtype != 1) return false;
  if (!(B > 0 && S > 0 && M > 0 && C > 0 && Q > 0 && L > 0 && P > 0 && im2col_step > 0)) return false;
  const int step = B < im2col_step ? B : im2col_step;
  if (B % step != 0) return false;     // as the reference (ms_deform_attn_cuda.cu:51-53)
  const int64_t lanes = (int64_t)B * Q * M * (C > bwd_group(C) ? C : bwd_group(C));
  return lanes <= INT32_MAX - 255;     // every lane index of both kernels fits an int
}

extern "C" int ink_ms_deform_attn_forward_dev(const void* value, const int64_t* spatial_shapes,
                                              const int64_t* level_start_index, const void* sampling_loc,
                                              const void* attn_weight, int32_t dtype, int32_t B, int32_t S,
                                              int32_t M, int32_t C, int32_t Q, int32_t L, int32_t P,
                                              int32_t im2col_step, void* out, void* stream) {
  INK_CHECK_ARG(value && spatial_shapes && level_start_index && sampling_loc && attn_weight && out);
  INK_CHECK_ARG(msda_dev_args_ok(dtype, B, S, M, C, Q, L, P, im2col_step));
  const DevLevels lv{spatial_shapes, level_start_index};
  hipStream_t s = (hipStream_t)stream;
  if (dtype == 0) return dispatch_fwd<float, 8>(value, sampling_loc, attn_weight, lv, B, S, M, C, Q, L, P, out, s);
  return dispatch_fwd<double, 4>(value, sampling_loc, attn_weight, lv, B, S, M, C, Q, L, P, out, s);
}

extern "C" int ink_ms_deform_attn_backward_dev(const void* value, const int64_t* spatial_shapes,
                                               const int64_t* level_start_index, const void* sampling_loc,
                                               const void* attn_weight, const void* grad_output, int32_t dtype,
                                               int32_t B, int32_t S, int32_t M, int32_t C, int32_t Q, int32_t L,
                                               int32_t P, int32_t im2col_step, void* grad_value,
                                               void* grad_sampling_loc, void* grad_attn_weight, void* stream) {
  INK_CHECK_ARG(value && spatial_shapes && level_start_index && sampling_loc && attn_weight && grad_output);
  INK_CHECK_ARG(grad_value && grad_sampling_loc && grad_attn_weight);
  INK_CHECK_ARG(msda_dev_args_ok(dtype, B, S, M, C, Q, L, P, im2col_step));
  const DevLevels lv{spatial_shapes, level_start_index};
  hipStream_t s = (hipStream_t)stream;
  if (dtype == 0)
    return dispatch_bwd<float>(value, lv, sampling_loc, attn_weight, grad_output, B, S, M, C, Q, L, P, grad_value,
                               grad_sampling_loc, grad_attn_weight, s);
  return dispatch_bwd<double>(value, lv, sampling_loc, attn_weight, grad_output, B, S, M, C, Q, L, P, grad_value,
                              grad_sampling_loc, grad_attn_weight, s);
}

extern "C" int ink_msda_fused(const void* value_f16, const float* proj, int64_t ldp, const float* ref,
                              int32_t ref_dim, int64_t ref_q_stride, int64_t ref_b_stride,
                              const int32_t* shapes_host, int32_t B, int32_t S, int32_t Q,
                              void* out_f16, void* stream) {
  INK_CHECK_ARG(value_f16 && proj && ref && shapes_host && out_f16);
  INK_CHECK_ARG(B > 0 && S > 0 && Q > 0 && ldp >= 384 && ldp % 4 == 0 && (ref_dim == 2 || ref_dim == 4));
  LevelInfo li;
  int total = 0;
  for (int l = 0; l < 4; ++l) {
    li.H[l] = shapes_host[2 * l];
    li.W[l] = shapes_host[2 * l + 1];
    li.start[l] = total;
    INK_CHECK_ARG(li.H[l] > 0 && li.W[l] > 0);
    total += li.H[l] * li.W[l];
  }
  INK_CHECK_ARG(total == S);
  const int64_t threads = (int64_t)B * Q * 8 * 4;
  const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (ref_dim == 2) {
    hipLaunchKernelGGL(msda_fused_kernel<2>, grid, block, 0, s, (const f16*)value_f16, proj, ldp, ref,
                       ref_q_stride, ref_b_stride, li, B, S, Q, (f16*)out_f16);
  } else {
    hipLaunchKernelGGL(msda_fused_kernel<4>, grid, block, 0, s, (const f16*)value_f16, proj, ldp, ref,
                       ref_q_stride, ref_b_stride, li, B, S, Q, (f16*)out_f16);
  }
  return ink_launch_status();
}
