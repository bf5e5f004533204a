// SamAutomaticMaskGenerator's tail (SA/automatic_mask_generator.py:266-321, SA/utils/amg.py) on low-res logits:
//   * amg_stats_kernel: ONE pass from the 256 x 256 logits of a mask to its stability counts, area, box and the
//     thresholded mask as a COLUMN-MAJOR bit plane in the original-image frame - the full-resolution f32 logits the
//     reference materialises (return_logits=True) never exist;
//   * rle_kernel: the reference's uncompressed RLE (column-major runs) from those planes;
//   * nms_*: torchvision box NMS for one category;
//   * rsr_*: remove_small_regions (holes / islands below an area) on the planes, over bitplane.h's components.
// COLUMN-MAJOR BIT PLANE of an H x W image: Hp = ceil(H / 64) uint64 words per column, bit b of word w of column x =
// pixel (64 w + b, x), bits of rows >= H are 0; m planes are [m, W, Hp].  It is bitplane.h's layout of the transposed
// image, which is the order mask_to_rle_pytorch walks (permute(0, 2, 1).flatten(1)).
#include "common.h"
#include "bitplane.h"
#include "sam_postprocess.h"
#include "../../include/inklayer_hip.h"

namespace {

constexpr int AMG_T = 8;          // table ints per mask: hi, lo, area, x_min, y_min, x_max, y_max, 0

// PX = POST_PX: the rows form of the arithmetic (post_cols + post_row), PX = 1: the one-pixel form (post_pixel) - the
// launcher picks as ink_sam_postprocess does, so the floats are that entry's.  Workgroup = (band of 64 frame rows,
// mask); a thread owns PX columns, walks the band's rows and collects each column's 64 mask bits in a register pair:
// the plane words need no ballot, no LDS and no atomics (one owner per word).  Counts / box: per-thread registers ->
// wave shuffles -> LDS -> one integer atomic per workgroup and quantity (order-independent: deterministic).  While the
// kernel runs the table holds crop_w - x_min and crop_h - y_min (so that all-zero = empty and every box update is an
// atomicMax); amg_finish_kernel turns them into the minima.
template <int PX>
__global__ __launch_bounds__(256) void amg_stats_kernel(const float* __restrict__ low, int n, const int32_t* __restrict__ idx,
                                                        const int32_t* __restrict__ m_dev, int S, int L, int in_h,
                                                        int in_w, int ch, int cw, float thr, float thr_hi, float thr_lo,
                                                        int x0, int y0, int OW, int Hp, int band0,
                                                        int32_t* __restrict__ table, u64* __restrict__ planes,
                                                        float* __restrict__ out_logits) {
  __shared__ int s_red[4][7];
  const int b = blockIdx.y;
  if (m_dev && b >= *m_dev) return;
  const int src = idx ? idx[b] : b;
  if (src < 0 || src >= n) return;
  const float* lp = low + (int64_t)src * S * S;
  const PostScales sc = post_scales(S, L, in_h, in_w, ch, cw);
  const int band = band0 + blockIdx.x;
  const int Ya = band * 64 - y0 > 0 ? band * 64 - y0 : 0;                 // crop rows of this band: [Ya, Yb)
  const int Yb = band * 64 + 64 - y0 < ch ? band * 64 + 64 - y0 : ch;
  int n_hi = 0, n_lo = 0, n_on = 0, bx0 = 0, by0 = 0, bx1 = 0, by1 = 0;   // bx0 = cw - x_min, by0 = ch - y_min
  for (int xq = threadIdx.x; xq * PX < cw; xq += 256) {
    PostCols cols;
    if constexpr (PX == POST_PX) post_cols(xq, S, sc, in_w, cols);
    u64 word[PX];
#pragma unroll
    for (int px = 0; px < PX; ++px) word[px] = 0ull;
    for (int Y = Ya; Y < Yb; ++Y) {
      float vals[PX];
      if constexpr (PX == POST_PX) {
        post_row(lp, S, sc, in_h, Y, cols, vals);
      } else {
        vals[0] = post_pixel(lp, S, sc, in_h, in_w, Y, xq);
      }
      const int r = y0 + Y - band * 64;
      bool any = false;
#pragma unroll
      for (int px = 0; px < PX; ++px) {
        const float v = vals[px];
        const bool on = v > thr;
        n_hi += v > thr_hi ? 1 : 0;
        n_lo += v > thr_lo ? 1 : 0;
        n_on += on ? 1 : 0;
        word[px] |= (u64)(on ? 1 : 0) << r;
        any |= on;
      }
      if (any) {
        by0 = by0 > ch - Y ? by0 : ch - Y;
        by1 = by1 > Y ? by1 : Y;
      }
      if (out_logits) {
        float* o = out_logits + ((int64_t)b * ch + Y) * cw + (int64_t)xq * PX;
        if constexpr (PX == POST_PX) {
          *(f32x4*)o = (f32x4){vals[0], vals[1], vals[2], vals[3]};
        } else {
          *o = vals[0];
        }
      }
    }
#pragma unroll
    for (int px = 0; px < PX; ++px) {
      const int X = xq * PX + px;
      if (word[px]) {
        bx0 = bx0 > cw - X ? bx0 : cw - X;
        bx1 = bx1 > X ? bx1 : X;
      }
      planes[((int64_t)b * OW + x0 + X) * Hp + band] = word[px];
    }
  }
  int red[7] = {n_hi, n_lo, n_on, bx0, by0, bx1, by1};
#pragma unroll
  for (int q = 0; q < 7; ++q)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int t = __shfl_xor(red[q], o, 64);
      red[q] = q < 3 ? red[q] + t : (red[q] > t ? red[q] : t);
    }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int q = 0; q < 7; ++q) s_red[wave][q] = red[q];
  __syncthreads();
  if (threadIdx.x < 7) {
    const int q = threadIdx.x;
    int v = s_red[0][q];
    for (int w = 1; w < 4; ++w) v = q < 3 ? v + s_red[w][q] : (v > s_red[w][q] ? v : s_red[w][q]);
    int32_t* t = table + (int64_t)b * AMG_T + q;
    if (q < 3) {
      if (v) atomicAdd(t, v);
    } else if (s_red[0][2] + s_red[1][2] + s_red[2][2] + s_red[3][2] > 0) {
      atomicMax(t, v);
    }
  }
}

// batched_mask_to_box's convention: inclusive maxima, [0, 0, 0, 0] for an empty mask (the table is already all zero then)
__global__ __launch_bounds__(256) void amg_finish_kernel(int32_t* __restrict__ table, int m, const int32_t* __restrict__ m_dev,
                                                         int ch, int cw) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= m || (m_dev && b >= *m_dev)) return;
  int32_t* t = table + (int64_t)b * AMG_T;
  if (t[2] > 0) {
    t[3] = cw - t[3];
    t[4] = ch - t[4];
  }
}

// mask_to_rle_pytorch (SA/utils/amg.py:107-135) on column-major planes.  In the flattened column-major order p = x H + y
// a CHANGE is a position whose bit differs from its predecessor's (the predecessor of p = 0 counts as 0, which makes the
// first count the length of the leading zero run, 0 when the mask starts with a one); counts = differences of
// consecutive change positions, then H W - the last one.  Changes of a word = w ^ (w << 1 | previous bit): popcount
// sizes, ctz walks.  One workgroup per plane, a contiguous chunk of words per thread; the exclusive scan over the 256
// chunks carries (number of changes, last change position).  WRITE = false: nruns[k] only.
template <bool WRITE>
__global__ __launch_bounds__(256) void rle_kernel(const u64* __restrict__ planes, const int32_t* __restrict__ sel, int H,
                                                  int W, int Hp, int32_t* __restrict__ nruns,
                                                  const int32_t* __restrict__ offsets, int32_t* __restrict__ counts) {
  __shared__ int s_cnt[256], s_last[256];
  const int k = blockIdx.x, tid = threadIdx.x;
  const u64* pl = planes + (int64_t)(sel ? sel[k] : k) * W * Hp;
  const int T = W * Hp, chunk = (T + 255) / 256;
  const int i0 = tid * chunk < T ? tid * chunk : T, i1 = i0 + chunk < T ? i0 + chunk : T;
  const int last_bit = (H - 1) & 63;
  auto changes = [&](int i, int& base) {
    const int col = i / Hp, w = i - col * Hp;
    const u64 x = pl[i];
    const u64 prev = i == 0 ? 0ull : (w > 0 ? pl[i - 1] >> 63 : (pl[i - 1] >> last_bit) & 1ull);
    base = col * H + w * 64;
    return (x ^ ((x << 1) | prev)) & bp_tail_mask(w, H);
  };
  int cnt = 0, last = -1;
  for (int i = i0; i < i1; ++i) {
    int base;
    const u64 c = changes(i, base);
    if (c) {
      cnt += __builtin_popcountll(c);
      last = base + 63 - __builtin_clzll(c);
    }
  }
  s_cnt[tid] = cnt;
  s_last[tid] = last;
  __syncthreads();
  int before = 0, prev_pos = -1, total = 0, total_last = -1;
  for (int t = 0; t < 256; ++t) {
    const int c = s_cnt[t], l = s_last[t];
    if (t < tid) {
      before += c;
      prev_pos = l > prev_pos ? l : prev_pos;
    }
    total += c;
    total_last = l > total_last ? l : total_last;
  }
  if (!WRITE) {
    if (tid == 0) nruns[k] = total + 1;
    return;
  }
  int32_t* out = counts + offsets[k];
  int o = before, pp = prev_pos < 0 ? 0 : prev_pos;
  for (int i = i0; i < i1; ++i) {
    int base;
    u64 c = changes(i, base);
    while (c) {
      const int p = base + __builtin_ctzll(c);
      c &= c - 1;
      out[o++] = p - pp;
      pp = p;
    }
  }
  if (tid == 0) out[total] = H * W - (total_last < 0 ? 0 : total_last);
}

// ------------------------------------------------------------------------------------------------------------------
// box NMS (torchvision.ops.nms for one category = batched_nms with idxs == 0, SA/automatic_mask_generator.py:251-257)
constexpr int NMS_MAX = 4096;                 // 64 words of 64 boxes: the sweep keeps one word per lane of ONE wave

// rank of box i in descending score order, ties to the lower index; order[rank] = i, sorted[rank] = box i
__global__ __launch_bounds__(256) void nms_rank_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                       int n, int32_t* __restrict__ order, f32x4* __restrict__ sorted) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float s = scores[i];
  int rank = 0;
  for (int j = 0; j < n; ++j) {
    const float t = scores[j];
    rank += (t > s || (t == s && j < i)) ? 1 : 0;
  }
  order[rank] = i;
  sorted[rank] = (f32x4){boxes[4 * i], boxes[4 * i + 1], boxes[4 * i + 2], boxes[4 * i + 3]};
}

// sup[i, w] bit b: sorted box j = 64 w + b comes after i and iou(i, j) > thr.  f32 throughout, in torchvision's order of
// operations: inter = max(0, w) * max(0, h), iou = inter / (a_i + a_j - inter).
__global__ __launch_bounds__(64) void nms_matrix_kernel(const f32x4* __restrict__ sorted, int n, int nw, float thr,
                                                        u64* __restrict__ sup) {
  __shared__ f32x4 s_col[64];
  const int cb = blockIdx.x, rb = blockIdx.y, lane = threadIdx.x;
  const int i = rb * 64 + lane;
  if (cb * 64 + lane < n) s_col[lane] = sorted[cb * 64 + lane];
  __syncthreads();
  if (i >= n) return;
  u64 bits = 0ull;
  if (cb >= rb) {
    const f32x4 a = sorted[i];
    const float aa = (a[2] - a[0]) * (a[3] - a[1]);
    const int jn = n - cb * 64 < 64 ? n - cb * 64 : 64;
    for (int jj = 0; jj < jn; ++jj) {
      if (cb * 64 + jj <= i) continue;
      const f32x4 c = s_col[jj];
      const float ca = (c[2] - c[0]) * (c[3] - c[1]);
      const float xx1 = a[0] > c[0] ? a[0] : c[0], yy1 = a[1] > c[1] ? a[1] : c[1];
      const float xx2 = a[2] < c[2] ? a[2] : c[2], yy2 = a[3] < c[3] ? a[3] : c[3];
      const float w = xx2 - xx1 > 0.f ? xx2 - xx1 : 0.f, h = yy2 - yy1 > 0.f ? yy2 - yy1 : 0.f;
      const float inter = w * h;
      const float iou = inter / (aa + ca - inter);
      if (iou > thr) bits |= 1ull << jj;
    }
  }
  sup[(int64_t)i * nw + cb] = bits;
}

// The greedy sweep, one wave: lane l holds word l of the removed set.  Per block of 64 sorted boxes: the block's own
// (diagonal) words sit one per lane, so the 64 serial decisions are lane reads, no memory; then every lane ORs the rows
// of the block's kept boxes into its word (independent loads).  keep = original indices in descending score order.
__global__ __launch_bounds__(64) void nms_sweep_kernel(const u64* __restrict__ sup, const int32_t* __restrict__ order,
                                                       int n, int nw, int32_t* __restrict__ keep,
                                                       int32_t* __restrict__ n_keep) {
  const int lane = threadIdx.x;
  u64 removed = 0ull;
  int base = 0;
  for (int b = 0; b < nw; ++b) {
    const int i = b * 64 + lane;
    const u64 diag = i < n ? sup[(int64_t)i * nw + b] : 0ull;
    u64 cur = __shfl(removed, b, 64);
    const int rn = n - b * 64 < 64 ? n - b * 64 : 64;
    u64 keepw = 0ull;
    for (int r = 0; r < rn; ++r) {
      const u64 d = __shfl(diag, r, 64);
      if (!((cur >> r) & 1ull)) {
        keepw |= 1ull << r;
        cur |= d;
      }
    }
    if (lane > b && lane < nw) {
      u64 kk = keepw;
      while (kk) {
        const int r = __builtin_ctzll(kk);
        kk &= kk - 1;
        removed |= sup[(int64_t)(b * 64 + r) * nw + lane];
      }
    }
    if ((keepw >> lane) & 1ull) keep[base + __builtin_popcountll(keepw & ((1ull << lane) - 1ull))] = order[i];
    base += __builtin_popcountll(keepw);
  }
  if (lane == 0) *n_keep = base;
}


// ------------------------------------------------------------------------------------------------------------------
// remove_small_regions (SA/utils/amg.py:267-291) on column-major planes.  Connected components do not change under a
// transpose, so bitplane.h's run-based components run on the plane as it is: a "row" of theirs is a column x of the
// image (W rows of H pixels, Hp words each).  Only the tie rule of "keep the largest" needs the image's orientation:
// cv2 numbers components in raster order of their first pixel, i.e. by the smallest (y, x); a run [s, e] of plane row x
// starts at image pixel (s, x), so a component's first pixel is the minimum of s << 14 | x over its runs.
// Per plane: changed = a component smaller than min_area exists (the reference's flag), info[1] = a component of
// at least min_area exists, info[2..3] = max over components of area << 32 | (0x0fffffff - first-pixel key) as one
// uint64: the largest area, the earliest first pixel among equals.
constexpr int RSR_KEY = 0x0fffffff;

// area and first-pixel key per root (atomics over runs; parents are only read)
__global__ __launch_bounds__(256) void rsr_stats_kernel(int R, int RM, int* __restrict__ ws_all, int64_t ws_stride) {
  const int lane = threadIdx.x & 63;
  const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (y >= R) return;
  const CcWs ws = cc_ws(ws_all, ws_stride, blockIdx.y, R, RM);
  const int n = ws.nruns[y];
  for (int i = lane; i < n; i += 64) {
    const int id = y * RM + i;
    const int root = cc_find(ws.parent, id);
    const int r = ws.run[id];
    const int s = r & 0xffff, e = (r >> 16) & 0xffff;
    atomicAdd(&ws.area[root], e - s + 1);
    atomicMax(&ws.ymax[root], RSR_KEY - ((s << 14) | y));
  }
}

__global__ __launch_bounds__(256) void rsr_best_kernel(int R, int RM, int min_area, int* __restrict__ ws_all,
                                                       int64_t ws_stride, int* __restrict__ info_all,
                                                       int* __restrict__ changed) {
  const int lane = threadIdx.x & 63;
  const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (y >= R) return;
  const CcWs ws = cc_ws(ws_all, ws_stride, blockIdx.y, R, RM);
  int* info = info_all + 4 * blockIdx.y;
  const int n = ws.nruns[y];
  for (int i = lane; i < n; i += 64) {
    const int id = y * RM + i;
    if (ws.parent[id] != id) continue;
    const int a = ws.area[id];
    atomicOr(a < min_area ? &changed[blockIdx.y] : &info[1], 1);
    atomicMax((u64*)(info + 2), ((u64)a << 32) | (u64)(unsigned)ws.ymax[id]);
  }
}

// holes != 0 (the plane is the complement): mark the small components, which get filled; else mark what stays: the
// components of at least min_area or, when there is none, the one info[2..3] names.  The verdict goes into bit 31 of
// the run word, where cc_paint_kernel looks for it.
__global__ __launch_bounds__(256) void rsr_decide_kernel(int R, int RM, int min_area, int holes, int* __restrict__ ws_all,
                                                         int64_t ws_stride, const int* __restrict__ info_all) {
  const int lane = threadIdx.x & 63;
  const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (y >= R) return;
  const CcWs ws = cc_ws(ws_all, ws_stride, blockIdx.y, R, RM);
  const int* info = info_all + 4 * blockIdx.y;
  const bool any_big = info[1] != 0;
  const u64 best = *(const u64*)(info + 2);
  const int n = ws.nruns[y];
  for (int i = lane; i < n; i += 64) {
    const int id = y * RM + i;
    const int root = cc_find(ws.parent, id);
    const int a = ws.area[root];
    const bool small = a < min_area;
    const bool mark = holes ? small : (!small || (!any_big && (((u64)a << 32) | (u64)(unsigned)ws.ymax[root]) == best));
    if (mark) ws.run[id] |= (int)0x80000000;
  }
}

// workspace (int32): [0] run-table overflow flag (cannot be set: RM is the true bound), [4 .. 4 + 4 k) info, then the
// components workspace of k planes
static inline int rsr_rm(int H) { return (H + 1) / 2; }

}  // namespace

extern "C" int ink_sam_amg_stats(const float* low, int32_t n, const int32_t* index, int32_t m, const int32_t* m_dev,
                                 int32_t S, int32_t L, int32_t in_h, int32_t in_w, int32_t crop_h, int32_t crop_w,
                                 double thr, double offset, int32_t x0, int32_t y0, int32_t orig_h, int32_t orig_w,
                                 int32_t* table, void* planes_u64, float* out_logits, void* stream) {
  INK_CHECK_ARG(low && table && planes_u64 && n > 0 && m > 0 && (index || m <= n) && S > 0 && L >= S);
  INK_CHECK_ARG(in_h > 0 && in_w > 0 && in_h <= L && in_w <= L && crop_h > 0 && crop_w > 0);
  INK_CHECK_ARG(x0 >= 0 && y0 >= 0 && orig_h <= 16383 && orig_w <= 16383 && x0 + crop_w <= orig_w && y0 + crop_h <= orig_h);
  INK_CHECK_ARG((int64_t)m * crop_h < (int64_t)1 << 30 && ink_aligned<8>(planes_u64) && m <= 65535);
  const bool rows = crop_w % POST_PX == 0;               // ink_sam_postprocess's choice for the same crop size
  INK_CHECK_ARG(!rows || ink_aligned<16>(out_logits));
  hipStream_t s = (hipStream_t)stream;
  const int Hp = (orig_h + 63) / 64, band0 = y0 / 64, nb = (y0 + crop_h - 1) / 64 - band0 + 1;
  if (hipMemsetAsync(table, 0, (size_t)m * AMG_T * sizeof(int32_t), s) != hipSuccess) return INK_ERR_LAUNCH;
  if (x0 != 0 || y0 != 0 || crop_w != orig_w || crop_h != orig_h)      // uncrop_masks: zeros outside the crop
    if (hipMemsetAsync(planes_u64, 0, (size_t)m * orig_w * Hp * sizeof(u64), s) != hipSuccess) return INK_ERR_LAUNCH;
  // the three cut-offs as torch makes them from Python floats: the sum in double, then one rounding to f32
  const float thr_f = (float)thr, thr_hi = (float)(thr + offset), thr_lo = (float)(thr - offset);
  if (rows) {
    hipLaunchKernelGGL(amg_stats_kernel<POST_PX>, dim3(nb, m), dim3(256), 0, s, low, n, index, m_dev, S, L, in_h, in_w,
                       crop_h, crop_w, thr_f, thr_hi, thr_lo, x0, y0, orig_w, Hp, band0, table, (u64*)planes_u64, out_logits);
  } else {
    hipLaunchKernelGGL(amg_stats_kernel<1>, dim3(nb, m), dim3(256), 0, s, low, n, index, m_dev, S, L, in_h, in_w,
                       crop_h, crop_w, thr_f, thr_hi, thr_lo, x0, y0, orig_w, Hp, band0, table, (u64*)planes_u64, out_logits);
  }
  hipLaunchKernelGGL(amg_finish_kernel, dim3((m + 255) / 256), dim3(256), 0, s, table, m, m_dev, crop_h, crop_w);
  return ink_launch_status();
}

static int rle_check(const void* planes, int32_t k, int32_t H, int32_t W) {
  INK_CHECK_ARG(planes && ink_aligned<8>(planes) && k > 0 && H > 0 && W > 0 && H <= 16383 && W <= 16383);
  return INK_OK;
}

extern "C" int ink_mask_rle_counts(const void* planes_u64, const int32_t* select, int32_t k, int32_t H, int32_t W,
                                   int32_t* n_counts, void* stream) {
  if (rle_check(planes_u64, k, H, W) != INK_OK || !n_counts) return INK_ERR_ARG;
  hipLaunchKernelGGL(rle_kernel<false>, dim3(k), dim3(256), 0, (hipStream_t)stream, (const u64*)planes_u64, select, H, W,
                     (H + 63) / 64, n_counts, (const int32_t*)nullptr, (int32_t*)nullptr);
  return ink_launch_status();
}

extern "C" int ink_mask_rle_write(const void* planes_u64, const int32_t* select, int32_t k, int32_t H, int32_t W,
                                  const int32_t* offsets, int32_t* counts, void* stream) {
  if (rle_check(planes_u64, k, H, W) != INK_OK || !offsets || !counts) return INK_ERR_ARG;
  hipLaunchKernelGGL(rle_kernel<true>, dim3(k), dim3(256), 0, (hipStream_t)stream, (const u64*)planes_u64, select, H, W,
                     (H + 63) / 64, (int32_t*)nullptr, offsets, counts);
  return ink_launch_status();
}

extern "C" int ink_box_nms(const float* boxes, const float* scores, int32_t n, float iou_threshold, void* workspace_u64,
                           int32_t* keep, int32_t* n_keep, void* stream) {
  INK_CHECK_ARG(n_keep && n >= 0 && n <= NMS_MAX);
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return hipMemsetAsync(n_keep, 0, sizeof(int32_t), s) == hipSuccess ? INK_OK : INK_ERR_LAUNCH;
  INK_CHECK_ARG(boxes && scores && keep && workspace_u64 && ink_aligned<16>(workspace_u64));
  const int nw = (n + 63) / 64;
  f32x4* sorted = (f32x4*)workspace_u64;                            // 2 n words
  u64* sup = (u64*)workspace_u64 + 2 * (int64_t)n;                  // n nw words
  int32_t* order = (int32_t*)(sup + (int64_t)n * nw);               // n / 2 words
  hipLaunchKernelGGL(nms_rank_kernel, dim3((n + 255) / 256), dim3(256), 0, s, boxes, scores, n, order, sorted);
  hipLaunchKernelGGL(nms_matrix_kernel, dim3(nw, nw), dim3(64), 0, s, (const f32x4*)sorted, n, nw, iou_threshold, sup);
  hipLaunchKernelGGL(nms_sweep_kernel, dim3(1), dim3(64), 0, s, (const u64*)sup, (const int32_t*)order, n, nw, keep, n_keep);
  return ink_launch_status();
}

extern "C" int ink_mask_small_regions_workspace_ints(int32_t k, int32_t H, int32_t W, int64_t* out_ints) {
  INK_CHECK_ARG(out_ints && k > 0 && H > 0 && W > 0 && H <= 16383 && W <= 16383);
  *out_ints = 4 + 4 * (int64_t)k + (int64_t)k * cc_ws_ints_per_plane(W, rsr_rm(H));
  return INK_OK;
}

extern "C" int ink_mask_small_regions(const void* planes_u64, int32_t k, int32_t H, int32_t W, int32_t min_area,
                                      int32_t holes, void* tmp_planes_u64, int32_t* workspace, void* out_planes_u64,
                                      int32_t* changed, void* stream) {
  INK_CHECK_ARG(planes_u64 && tmp_planes_u64 && workspace && out_planes_u64 && changed && k > 0 && k <= 65535);
  INK_CHECK_ARG(H > 0 && W > 0 && H <= 16383 && W <= 16383 && min_area >= 0);
  INK_CHECK_ARG(ink_aligned<8>(planes_u64, tmp_planes_u64, out_planes_u64, workspace));
  hipStream_t s = (hipStream_t)stream;
  const int Hp = (H + 63) / 64, R = W, RM = rsr_rm(H);
  const int64_t plane = (int64_t)W * Hp, stride = cc_ws_ints_per_plane(R, RM);
  INK_CHECK_ARG((size_t)4 * Hp * sizeof(u64) <= 64 * 1024);
  int* info = workspace + 4;
  int* ws = workspace + 4 + 4 * (int64_t)k;
  if (hipMemsetAsync(workspace, 0, (size_t)(4 + 4 * (int64_t)k) * sizeof(int32_t), s) != hipSuccess) return INK_ERR_LAUNCH;
  if (hipMemsetAsync(changed, 0, (size_t)k * sizeof(int32_t), s) != hipSuccess) return INK_ERR_LAUNCH;
  const u64* src = (const u64*)planes_u64;
  const dim3 rows((R + 3) / 4, k);
  if (holes) {
    bp_logic(BP_NOT, src, nullptr, nullptr, (u64*)tmp_planes_u64, k, R, H, s);
    src = (const u64*)tmp_planes_u64;
  }
  cc_label(src, plane, k, R, H, Hp, RM, 1, ws, workspace, s);
  hipLaunchKernelGGL(rsr_stats_kernel, rows, dim3(256), 0, s, R, RM, ws, stride);
  hipLaunchKernelGGL(rsr_best_kernel, rows, dim3(256), 0, s, R, RM, min_area, ws, stride, info, changed);
  hipLaunchKernelGGL(rsr_decide_kernel, rows, dim3(256), 0, s, R, RM, min_area, holes, ws, stride, (const int*)info);
  // paint the marked runs: the filled holes into tmp (then out = mask | holes), the kept islands straight into out
  u64* painted = holes ? (u64*)tmp_planes_u64 : (u64*)out_planes_u64;
  cc_paint(k, R, H, Hp, RM, ws, nullptr, painted, plane, s);
  if (holes)
    bp_logic(BP_OR, (const u64*)planes_u64, (const u64*)tmp_planes_u64, nullptr, (u64*)out_planes_u64, k, R, H, s);
  return ink_launch_status();
}
