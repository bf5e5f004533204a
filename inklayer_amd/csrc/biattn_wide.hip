// BiMultiHeadAttention core (fuse_modules.py:168-240), both directions, for captions of 1 to 256 tokens:
// ink_biattn_wide, the fusion layer's general kernel (fusion_fold.hip is the specialisation for T <= 4).
//
//   QV f16 [B*S, 2E] = [v_proj(v) | values_v_proj(v)],  KL f16 [B*T, 2E] = [l_proj(l) | values_l_proj(l)],
//   E = 1024 = 4 heads x 256, score[s,h,t] = scale * q[s,h,:] . k[t,h,:],
//   out_v[s,h,:] = sum_t softmax_t(score)[t] * values_l[t,h,:]      (image side, softmax over the T text tokens)
//   out_l[t,h,:] = sum_s softmax_s(score)[s] * values_v[s,h,:]      (text side, softmax over the S image tokens)
// The global max subtraction / +-50000 clamps of the reference are no-ops for a softmax unless
// |score| > 5e4 (never for sane weights) and are not reproduced.
//
// All three products run on the 32x32x16 f16 MFMA with f32 accumulation (mfma_util.h), 8 waves per workgroup, an
// ordinary multi-wave kernel (no waves_per_eu, no register-file ownership).  T is padded to Tp = 32 ceil(T / 32)
// inside the kernels: a pad column's score is -inf (weight exactly 0 on the image side, never read on the text side).
//
// THE SCORE TILE IS RECOMPUTED, NOT SHARED.  No score matrix reaches HBM; the text side is a split over S chunks:
//   wide_prep      values_l of each head transposed to VLt [B,4,256,Tp] f16 (pad columns zero), so that the B operand
//                  of P.VL is 16 contiguous bytes per lane.
//   wide_image     grid (ceil(S/128), 4, B): per 32-row tile Q.K^T (wave w: text columns 32w..32w+31; A and B
//                  fragments are 16-byte global loads, both row-major), scores through an f32 LDS tile, row softmax,
//                  P.VL with wave w owning value dims 32w..32w+31.  It also leaves the column max of its 128 rows.
//   wide_text      grid (ceil(S/1024), 4, B): the chunk's column max m_c is the max of its eight 128-row maxima; per
//                  32-row tile the scores are computed AGAIN by the same code (bitwise the same numbers, so
//                  exp(score - m_c) <= 1), and the accumulator tile - text column on the lane, image rows in the 16
//                  registers - is itself the A operand of P^T.VV (no LDS, no lane movement: registers 8k..8k+7 are
//                  the fragment of k-step k, whose k order is the accumulator's row order; the values_v tile is laid
//                  out in LDS in that same order).  Wave w keeps the [32, 256] f32 partial of its text columns.
//                  Each chunk produces m_c, a sum-exp and an unnormalised [Tp, 256] partial per head.
//   wide_merge     combines the chunks: out_l = sum_c partial_c e^(m_c - M) / sum_c sumexp_c e^(m_c - M), M = max m_c.
// Weights enter the value MFMAs as f16(w * 2^14) with w = exp(score - max) <= 1 and the normaliser is the sum of those
// SAME rounded numbers, so the weights of an output are an exact convex combination and only weights below 2^-28 of
// the largest fall below f16's smallest normal.  ink_biattn_wide_varlen gives every image its own token count (a
// device array t_len; KL / out_l rows at stride Tmax): the kernels are the same text, see image_tokens.  No atomics: every output element has one writer and a fixed
// summation order, so the results of image b are bitwise independent of B and identical run to run.
//
// Workspace (ink_biattn_wide_workspace, in floats), Tp as above, NG = ceil(S/128), NC = ceil(S/1024):
//   B*4*256*Tp/2 (VLt) + B*4*NG*Tp (group column max) + B*4*NC*Tp*2 (m_c, sum-exp) + B*4*NC*Tp*256 (partials)
// = 13.9 MB per image at S = 13294, T = 256 (the score strip it replaces would be 54 MB).
// Traffic floor: QV is read TWICE (q by both passes: 2 x S x 2 KB; values_v once: S x 2 KB) plus out_v (S x 2 KB).
#include "mfma_util.h"
#include "../../include/inklayer_hip.h"

namespace {

constexpr int BW_E = 1024, BW_H = 4, BW_HD = 256, BW_LD = 2 * BW_E;
constexpr int BW_TILE = 32;            // image rows per MFMA tile
constexpr int BW_GROUP = 128;          // rows per image-side workgroup (4 tiles)
constexpr int BW_CHUNK = 1024;         // rows per text-side workgroup (8 groups)
constexpr int BW_THREADS = 512;        // 8 waves: one per 32 text columns (scores) / 32 value dims (image side)
constexpr float BW_PSCALE = 16384.0f;  // 2^14: weights <= 1 enter the MFMA as f16(w * 2^14) <= 16384 < 65504

// accumulator register i of lane half hh holds row (i & 3) + 8 (i >> 2) + 4 hh of the 32x32 tile; the column is lane & 31
__device__ __forceinline__ int acc_row(int i, int hh) { return (i & 3) + 8 * (i >> 2) + 4 * hh; }

// Scaled scores of image rows s0..s0+31 against text columns 32 ct..32 ct+31 of one head: row on the registers, column
// on the lane.  Qh / Kh point at the head's 256 q / k columns of the image's first row; rows past S and columns past T
// are loaded from the last valid row (never out of bounds) and a pad COLUMN comes back as -inf.
__device__ __forceinline__ f32x16 score_tile(const f16* __restrict__ Qh, const f16* __restrict__ Kh, int S, int T,
                                             int s0, int ct, float scale, int lane) {
  const int r = lane & 31, hh = lane >> 5;
  const int srow = min(s0 + r, S - 1), t = ct * 32 + r, trow = min(t, T - 1);
  const f16* qp = Qh + (int64_t)srow * BW_LD + 8 * hh;
  const f16* kp = Kh + (int64_t)trow * BW_LD + 8 * hh;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
  for (int ks = 0; ks < BW_HD / 16; ++ks)
    acc = mfma32(*(const f16x8*)(qp + 16 * ks), *(const f16x8*)(kp + 16 * ks), acc);
  const bool pad = t >= T;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = pad ? -INFINITY : acc[i] * scale;
  return acc;
}

// The token count of image b.  t_len == nullptr: every image has the launch's T (ink_biattn_wide).  Otherwise
// (ink_biattn_wide_varlen) T is the row stride Tmax of KL / out_l and image b has t_len[b] tokens, clamped into 1..T
// here so that a bad device value cannot index out of range.  Every kernel below derives its own padded count
// Tpb = 32 ceil(Tb / 32) from it - an image's arithmetic is that of a uniform launch at T = Tb - while the workspace
// strides stay at the launch-wide Tp.
__device__ __forceinline__ int image_tokens(const int32_t* __restrict__ t_len, int b, int T) {
  return t_len ? min(max(t_len[b], 1), T) : T;
}

// values_l of every head, transposed and padded: VLt[b][h][d][t] = KL[b*T + t][E + 256 h + d], zero for t >= Tb (a pad
// row of KL is never read)
__global__ __launch_bounds__(256) void wide_prep_kernel(const f16* __restrict__ KL, int T, int Tp, int64_t total,
                                                        const int32_t* __restrict__ t_len, f16* __restrict__ VLt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int t = (int)(i % Tp);
  const int64_t r = i / Tp;                                 // (b * 4 + h) * 256 + d
  const int d = (int)(r % BW_HD), h = (int)((r / BW_HD) % BW_H);
  const int64_t b = r / (BW_HD * BW_H);
  VLt[i] = t < image_tokens(t_len, (int)b, T) ? KL[(b * T + t) * BW_LD + BW_E + h * BW_HD + d] : (f16)0.f;
}

constexpr int BW_SS = 256 + 4;         // f32 row stride of the score tile (floats)
constexpr int BW_ES = 256 + 8;         // f16 row stride of the weight tile (halves; rows stay 16-byte aligned)

__global__ __launch_bounds__(BW_THREADS) void wide_image_kernel(const f16* __restrict__ QV, const f16* __restrict__ KL,
                                                                const f16* __restrict__ VLt, int S, int T, int Tp,
                                                                const int32_t* __restrict__ t_len, float scale,
                                                                float* __restrict__ gmax,
                                                                f16* __restrict__ out_v) {
  __shared__ __attribute__((aligned(16))) float ssc[BW_TILE * BW_SS];
  __shared__ __attribute__((aligned(16))) f16 e16[BW_TILE * BW_ES];
  __shared__ float inv[BW_TILE];
  const int g = blockIdx.x, h = blockIdx.y, b = blockIdx.z, NG = gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int Tb = image_tokens(t_len, b, T), Tpb = (Tb + 31) / 32 * 32, NT = Tpb / 32;
  const f16* Qh = QV + (int64_t)b * S * BW_LD + h * BW_HD;
  const f16* Kh = KL + (int64_t)b * T * BW_LD + h * BW_HD;
  const f16* vl = VLt + (((int64_t)b * BW_H + h) * BW_HD + w * 32 + r) * Tp + 8 * hh;
  float cm = -INFINITY;                                     // thread tid < Tpb: running max of text column tid
  for (int tile = 0; tile < BW_GROUP / BW_TILE; ++tile) {
    const int s0 = g * BW_GROUP + tile * BW_TILE;
    if (s0 >= S) break;                                     // uniform over the workgroup
    const int nrow = min(BW_TILE, S - s0);
    if (w < NT) {
      const f32x16 sc = score_tile(Qh, Kh, S, Tb, s0, w, scale, lane);
#pragma unroll
      for (int i = 0; i < 16; ++i) ssc[acc_row(i, hh) * BW_SS + w * 32 + r] = sc[i];
    }
    __syncthreads();
    if (tid < Tpb)
      for (int row = 0; row < nrow; ++row) cm = fmaxf(cm, ssc[row * BW_SS + tid]);
    {   // row softmax: 16 consecutive lanes per row
      const int row = tid >> 4, sub = tid & 15;
      float m = -INFINITY;
      for (int c = sub; c < Tpb; c += 16) m = fmaxf(m, ssc[row * BW_SS + c]);
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
      float sum = 0.f;
      for (int c = sub; c < Tpb; c += 16) {
        const f16 e = (f16)(expf(ssc[row * BW_SS + c] - m) * BW_PSCALE);   // pad column: exp(-inf) = 0
        e16[row * BW_ES + c] = e;
        sum += (float)e;
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
      if (sub == 0) inv[row] = 1.f / sum;
    }
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int ks = 0; ks < Tpb / 16; ++ks)
      acc = mfma32(*(const f16x8*)(e16 + r * BW_ES + 16 * ks + 8 * hh), *(const f16x8*)(vl + 16 * ks), acc);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = acc_row(i, hh);
      if (row < nrow) out_v[((int64_t)b * S + s0 + row) * BW_E + h * BW_HD + w * 32 + r] = (f16)(acc[i] * inv[row]);
    }
    // the next tile's ssc writes wait behind the barrier above (every softmax read is done), its e16 / inv writes
    // behind its own first barrier (every MFMA read and store of this tile is done)
  }
  if (tid < Tpb) gmax[(((int64_t)b * BW_H + h) * NG + g) * Tp + tid] = cm;
}

constexpr int BW_VS = 40;              // f16 row stride of the transposed values_v tile (halves; 80 B, 16-byte aligned)

__global__ __launch_bounds__(BW_THREADS) void wide_text_kernel(const f16* __restrict__ QV, const f16* __restrict__ KL,
                                                               const float* __restrict__ gmax, int S, int T, int Tp,
                                                               const int32_t* __restrict__ t_len, int NG,
                                                               float scale, float* __restrict__ tstat,
                                                               float* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) f16 vvt[BW_HD * BW_VS];   // [value dim][image row, in accumulator k order]
  __shared__ float cmx[256];
  const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z, NC = gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int Tb = image_tokens(t_len, b, T), Tpb = (Tb + 31) / 32 * 32, NT = Tpb / 32;
  const f16* Qh = QV + (int64_t)b * S * BW_LD + h * BW_HD;
  const f16* Kh = KL + (int64_t)b * T * BW_LD + h * BW_HD;
  const f16* VVh = QV + (int64_t)b * S * BW_LD + BW_E + h * BW_HD;
  const int s_begin = c * BW_CHUNK, s_end = min(S, s_begin + BW_CHUNK);
  if (tid < Tpb) {
    const int g0 = c * (BW_CHUNK / BW_GROUP), g1 = min(NG, g0 + BW_CHUNK / BW_GROUP);
    float m = -INFINITY;
    for (int g = g0; g < g1; ++g) m = fmaxf(m, gmax[(((int64_t)b * BW_H + h) * NG + g) * Tp + tid]);
    cmx[tid] = m;
  }
  __syncthreads();
  const int t = w * 32 + r;                                 // this lane's text column (w < NT)
  const bool live = w < NT && t < Tb;
  const float mycm = live ? cmx[t] : 0.f;
  f32x16 acc[8];
#pragma unroll
  for (int dt = 0; dt < 8; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[dt][i] = 0.f;
  float lsum = 0.f;
  for (int s0 = s_begin; s0 < s_end; s0 += BW_TILE) {
    __syncthreads();                                        // the previous tile's fragment reads are done
    for (int idx = tid; idx < BW_TILE * (BW_HD / 8); idx += BW_THREADS) {
      const int row = idx & 31, dg = idx >> 5;
      f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};                   // rows past S weigh nothing AND read nothing
      if (s0 + row < S) v = *(const f16x8*)(VVh + (int64_t)(s0 + row) * BW_LD + dg * 8);
      // row = 16 ks + 8 (j >> 2) + 4 hh + (j & 3)  ->  position 16 ks + 8 hh + j: element j of lane half hh, k-step ks
      const int pos = (row & 16) + 8 * ((row >> 2) & 1) + 4 * ((row >> 3) & 1) + (row & 3);
#pragma unroll
      for (int i = 0; i < 8; ++i) vvt[(dg * 8 + i) * BW_VS + pos] = v[i];
    }
    __syncthreads();
    if (w < NT) {
      const f32x16 sc = score_tile(Qh, Kh, S, Tb, s0, w, scale, lane);
      f16x8 p[2];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const bool on = live && s0 + acc_row(i, hh) < S;
        const f16 e = (f16)(on ? expf(sc[i] - mycm) * BW_PSCALE : 0.f);
        p[i >> 3][i & 7] = e;
        lsum += (float)e;
      }
#pragma unroll
      for (int dt = 0; dt < 8; ++dt)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          acc[dt] = mfma32(p[ks], *(const f16x8*)(vvt + (dt * 32 + r) * BW_VS + 16 * ks + 8 * hh), acc[dt]);
    }
  }
  if (w < NT) {
    const int64_t base = (((int64_t)b * BW_H + h) * NC + c) * Tp;
    lsum += __shfl_xor(lsum, 32, 64);                       // the two lane halves hold the column's other rows
    if (hh == 0) {
      tstat[(base + t) * 2] = live ? cmx[t] : -INFINITY;
      tstat[(base + t) * 2 + 1] = lsum * (1.0f / BW_PSCALE);
    }
#pragma unroll
    for (int dt = 0; dt < 8; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i)
        partial[(base + w * 32 + acc_row(i, hh)) * BW_HD + dt * 32 + r] = acc[dt][i] * (1.0f / BW_PSCALE);
  }
}

// out_l[b*T + t, 256 h + d] from the chunks' (m_c, sum-exp, partial): grid (T, 4, B), thread = value dim d; the rows
// t >= Tb of an image with fewer tokens than the launch's T are written as zeros
__global__ __launch_bounds__(BW_HD) void wide_merge_kernel(const float* __restrict__ tstat,
                                                           const float* __restrict__ partial, int T, int Tp, int NC,
                                                           const int32_t* __restrict__ t_len, f16* __restrict__ out_l) {
  const int t = blockIdx.x, h = blockIdx.y, b = blockIdx.z, d = threadIdx.x;
  if (t >= image_tokens(t_len, b, T)) {                     // uniform over the workgroup
    out_l[((int64_t)b * T + t) * BW_E + h * BW_HD + d] = (f16)0.f;
    return;
  }
  const int64_t base = ((int64_t)b * BW_H + h) * NC;
  float M = -INFINITY;
  for (int c = 0; c < NC; ++c) M = fmaxf(M, tstat[((base + c) * Tp + t) * 2]);
  float num = 0.f, den = 0.f;
  for (int c = 0; c < NC; ++c) {
    const float f = expf(tstat[((base + c) * Tp + t) * 2] - M);
    den += tstat[((base + c) * Tp + t) * 2 + 1] * f;
    num += partial[((base + c) * Tp + t) * BW_HD + d] * f;
  }
  out_l[((int64_t)b * T + t) * BW_E + h * BW_HD + d] = (f16)(num / den);
}

struct WideWs { int64_t vlt, gmax, tstat, partial, total; int Tp, NG, NC; };   // offsets in floats

static inline WideWs wide_ws(int B, int S, int T) {
  WideWs o;
  o.Tp = (T + 31) / 32 * 32;
  o.NG = (S + BW_GROUP - 1) / BW_GROUP;
  o.NC = (S + BW_CHUNK - 1) / BW_CHUNK;
  const int64_t bh = (int64_t)B * BW_H;
  o.vlt = 0;
  o.gmax = o.vlt + bh * BW_HD * o.Tp / 2;
  o.tstat = o.gmax + bh * o.NG * o.Tp;
  o.partial = o.tstat + bh * o.NC * o.Tp * 2;
  o.total = o.partial + bh * o.NC * o.Tp * BW_HD;
  return o;
}

}  // namespace

extern "C" int ink_biattn_wide_workspace(int32_t B, int32_t S, int32_t T, int64_t* out_floats) {
  INK_CHECK_ARG(out_floats && B > 0 && B <= 65535 && S > 0 && S <= 32768 && T >= 1 && T <= 256);
  *out_floats = wide_ws(B, S, T).total;
  return INK_OK;
}

// the four launches of both entry points: t_len == nullptr is the uniform form
static int wide_launch(const void* QV_f16, const void* KL_f16, int32_t B, int32_t S, int32_t T, const int32_t* t_len,
                       float scale, float* ws, void* out_v_f16, void* out_l_f16, void* stream) {
  const WideWs o = wide_ws(B, S, T);
  hipStream_t s = (hipStream_t)stream;
  f16* vlt = (f16*)(ws + o.vlt);
  const int64_t nprep = (int64_t)B * BW_H * BW_HD * o.Tp;
  hipLaunchKernelGGL(wide_prep_kernel, dim3((unsigned)((nprep + 255) / 256)), dim3(256), 0, s, (const f16*)KL_f16, T,
                     o.Tp, nprep, t_len, vlt);
  hipLaunchKernelGGL(wide_image_kernel, dim3(o.NG, BW_H, B), dim3(BW_THREADS), 0, s, (const f16*)QV_f16,
                     (const f16*)KL_f16, (const f16*)vlt, S, T, o.Tp, t_len, scale, ws + o.gmax, (f16*)out_v_f16);
  hipLaunchKernelGGL(wide_text_kernel, dim3(o.NC, BW_H, B), dim3(BW_THREADS), 0, s, (const f16*)QV_f16,
                     (const f16*)KL_f16, (const float*)(ws + o.gmax), S, T, o.Tp, t_len, o.NG, scale, ws + o.tstat,
                     ws + o.partial);
  hipLaunchKernelGGL(wide_merge_kernel, dim3(T, BW_H, B), dim3(BW_HD), 0, s, (const float*)(ws + o.tstat),
                     (const float*)(ws + o.partial), T, o.Tp, o.NC, t_len, (f16*)out_l_f16);
  return ink_launch_status();
}

extern "C" int ink_biattn_wide(const void* QV_f16, const void* KL_f16, int32_t B, int32_t S, int32_t T, int32_t E,
                               float scale, float* ws, void* out_v_f16, void* out_l_f16, void* stream) {
  INK_CHECK_ARG(QV_f16 && KL_f16 && ws && out_v_f16 && out_l_f16);
  INK_CHECK_ARG(B > 0 && B <= 65535 && S > 0 && S <= 32768 && T >= 1 && T <= 256 && E == BW_E);
  INK_CHECK_ARG(ink_aligned<16>(QV_f16, KL_f16, ws, out_v_f16, out_l_f16));   // 16-byte fragment loads
  return wide_launch(QV_f16, KL_f16, B, S, T, nullptr, scale, ws, out_v_f16, out_l_f16, stream);
}

extern "C" int ink_biattn_wide_varlen(const void* QV_f16, const void* KL_f16, int32_t B, int32_t S, int32_t Tmax,
                                      const int32_t* t_len, int32_t E, float scale, float* ws, void* out_v_f16,
                                      void* out_l_f16, void* stream) {
  INK_CHECK_ARG(QV_f16 && KL_f16 && t_len && ws && out_v_f16 && out_l_f16);
  INK_CHECK_ARG(B > 0 && B <= 65535 && S > 0 && S <= 32768 && Tmax >= 1 && Tmax <= 256 && E == BW_E);
  INK_CHECK_ARG(ink_aligned<16>(QV_f16, KL_f16, ws, out_v_f16, out_l_f16) && ink_aligned<4>(t_len));
  return wide_launch(QV_f16, KL_f16, B, S, Tmax, t_len, scale, ws, out_v_f16, out_l_f16, stream);
}
