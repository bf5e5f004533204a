// Layer assembly: everything of the reference's inpainting stage around the diffusion model - the
// background mask of an object (get_mask), the per-layer sketch layer / edit mask / debug image, the composite and the
// RGBA layers.  Integer work on bit planes (bitplane.h), batched over the n objects of a sketch; bit-exact against
// tests/layers_ref.py, which the reference's committed outputs pin.
//   reference: InkLayer/inpainting/fill_object_bg_mask.py:4-47   (hole filling by contour hierarchy)
//              InkLayer/inpainting/fill_object_bg_mask.py:50-114 (get_mask: Otsu, ellipse dilation, border band, flood
//              fill, largest contour, 5x5 chamfer distance, shrink, hole filling)
//              InkLayer/inpainting/fill_object_bg_mask.py:117-185 (RGBA layer)
//              InkLayer/inpainting/util.py:22-106, 109-133, 137-159, 198-204, 242-260 (assembly, composite, bbox rules)
#include "bitplane.h"
#include "../../include/inklayer_hip.h"

namespace {

static inline BpShape bp_shape_ellipse5() { return BpShape{2, {0, 2, 2, 2, 0, -1, -1}}; }   // cv2 5x5 MORPH_ELLIPSE

// ------------------------------------------------------------------------------------------------------------------
// grey level histogram -> Otsu threshold -> bit plane
__global__ __launch_bounds__(256) void lay_hist_kernel(const uint8_t* __restrict__ gray, int64_t npix, int invert,
                                                       int* __restrict__ hist) {
  __shared__ int h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint8_t* g = gray + (int64_t)blockIdx.y * npix;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
    const int v = g[i];
    atomicAdd(&h[invert ? 255 - v : v], 1);
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&hist[blockIdx.y * 256 + threadIdx.x], h[threadIdx.x]);
}

// Otsu's threshold from the 256 counts in float64, evaluated in cv2's order (getThreshVal_Otsu_8u); the first maximum
// wins (strict >).  One thread per image: 256 dependent steps.
__global__ void lay_otsu_kernel(const int* __restrict__ hist, int n, int* __restrict__ thresh) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int* h = hist + p * 256;
  double total = 0.0, mu = 0.0;
  for (int i = 0; i < 256; ++i) {
    total += (double)h[i];
    mu += (double)i * (double)h[i];
  }
  const double scale = 1.0 / total;
  mu *= scale;
  double mu1 = 0.0, q1 = 0.0, best = 0.0;
  int best_t = 0;
  const double eps = 1.1920928955078125e-07;               // FLT_EPSILON
  for (int i = 0; i < 256; ++i) {
    const double pi = (double)h[i] * scale;
    mu1 *= q1;
    q1 += pi;
    const double q2 = 1.0 - q1;
    if (fmin(q1, q2) < eps || fmax(q1, q2) > 1.0 - eps) continue;
    mu1 = (mu1 + (double)i * pi) / q1;
    const double mu2 = (mu - q1 * mu1) / q2;
    const double sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2);
    if (sigma > best) {
      best = sigma;
      best_t = i;
    }
  }
  thresh[p] = best_t;
}

__global__ __launch_bounds__(256) void lay_pack_kernel(const uint8_t* __restrict__ gray, int H, int W, int Wp, int invert,
                                                       const int* __restrict__ thresh, u64* __restrict__ planes) {
  const int word = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (word >= H * Wp) return;
  const int y = word / Wp, w = word - y * Wp, x = w * 64 + lane;
  int v = x < W ? (int)gray[((int64_t)blockIdx.y * H + y) * W + x] : 0;
  if (invert) v = 255 - v;
  const u64 m = __ballot(x < W && v > thresh[blockIdx.y]);
  if (lane == 0) planes[(int64_t)blockIdx.y * H * Wp + word] = m;
}

// flags[plane] = 1 iff the plane has a pixel within `band` rows / columns of an image edge
__global__ __launch_bounds__(256) void lay_band_kernel(const u64* __restrict__ planes, int H, int W, int Wp, int band,
                                                       int* __restrict__ flags) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= H * Wp) return;
  const int y = idx / Wp, w = idx - y * Wp;
  u64 v = planes[(int64_t)blockIdx.y * H * Wp + idx];
  if (y >= band && y < H - band) {                          // inner rows: only the left / right columns count
    u64 m = 0ull;
    for (int b = 0; b < 64; ++b) {
      const int x = w * 64 + b;
      if (x < W && (x < band || x >= W - band)) m |= 1ull << b;
    }
    v &= m;
  }
  if (v) atomicOr(&flags[blockIdx.y], 1);
}

// ------------------------------------------------------------------------------------------------------------------
// Components with the contour statistics of this stage.  Workspace (int32): header LAY_HDR | n blocks of bitplane.h's
// component workspace | n x [H * RM] Euler sums.  Header: [0] run overflow, [1] number of undecided holes, [2 ..] their
// records (plane, xmin, xmax, ymin, ymax, twice the area found, y and x of the hole's first pixel), [1024 + 2 plane] the
// 64-bit maximum of LARGEST.
#define LAY_HDR 2048
#define LAY_AMB_CAP 64
#define LAY_BEST 1024
enum { LAY_FLOOD = 0, LAY_FILL_ALL = 1, LAY_FILL_RULE = 2, LAY_LARGEST = 3 };
static inline int lay_rm(int W) { return W / 2 + 1; }        // a row of W pixels has at most ceil(W / 2) runs

__device__ __forceinline__ u64 lay_bits(const u64* row, int Wp, int x0) {   // pixels x0 .. x0 + 63 of a row (0 outside)
  if (!row) return 0ull;
  const int w = x0 >> 6, sh = x0 & 63;
  const u64 lo = (w >= 0 && w < Wp) ? row[w] : 0ull;
  const u64 hi = (w + 1 >= 0 && w + 1 < Wp) ? row[w + 1] : 0ull;
  return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}

// Per component (root): bounding box, TWICE the contour area and, for holes, the Euler sum.
// The contour area (polygon through the pixel centres of the followed border) in closed form over the 2x2 cells of
// pixel centres: for an 8-connected component without enclosed background a cell counts 1 when all four corners
// belong to it and 1/2 when three do (the border cuts such a cell diagonally); for a hole (a 4-connected background
// component, whose border runs on the foreground pixels AROUND it) a cell counts 1 when two or more corners belong
// to the hole and 1/2 when one does, and a cell whose only two hole corners are diagonal counts 1/2 for each.  Every
// cell is charged to the run holding its top pixels, or to the run of its bottom pixels when the top ones are clear
// (diagonal cells: each pixel charges its own half).  Euler sum of a 4-connected component = runs - vertical run
// contacts = 1 - (number of foreground islands inside it).
__global__ __launch_bounds__(256) void lay_stats_kernel(const u64* __restrict__ planes, int64_t plane_stride, int H,
                                                        int W, int Wp, int RM, int hole, int* __restrict__ ws_all,
                                                        int64_t ws_stride, int* __restrict__ euler_all) {
  const int lane = threadIdx.x & 63;
  const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (y >= H) return;
  const CcWs ws = cc_ws(ws_all, ws_stride, blockIdx.y, H, RM);
  int* euler = euler_all + (int64_t)blockIdx.y * H * RM;
  const u64* A = planes + (int64_t)blockIdx.y * plane_stride + (int64_t)y * Wp;
  const u64* B = y + 1 < H ? A + Wp : nullptr;
  const u64* Z = y > 0 ? A - Wp : nullptr;
  const int n = ws.nruns[y], nb = y > 0 ? ws.nruns[y - 1] : 0;
  const int* rb = ws.run + (int64_t)(y - 1) * RM;
  for (int i = lane; i < n; i += 64) {
    const int id = y * RM + i;
    const int root = cc_find(ws.parent, id);
    const int r = ws.run[id];
    const int s = r & 0xffff, e = (r >> 16) & 0xffff;
    atomicMin(&ws.xmin[root], s);
    atomicMax(&ws.xmax[root], e);
    atomicMin(&ws.ymin[root], y);
    atomicMax(&ws.ymax[root], y);
    int a2 = 0;
    for (int x0 = s - 1; x0 <= e; x0 += 64) {                // cells with the columns (x, x + 1), x = s - 1 .. e
      const int cnt = e - x0 + 1;
      const u64 valid = cnt >= 64 ? ~0ull : ((1ull << cnt) - 1ull);
      const u64 a0 = lay_bits(A, Wp, x0), a1 = lay_bits(A, Wp, x0 + 1);
      const u64 b0 = lay_bits(B, Wp, x0), b1 = lay_bits(B, Wp, x0 + 1);
      const u64 t_both = a0 & a1, t_x = a0 ^ a1, b_any = b0 | b1, b_both = b0 & b1, b_x = b0 ^ b1;
      if (hole) {
        const u64 z0 = lay_bits(Z, Wp, x0), z1 = lay_bits(Z, Wp, x0 + 1);
        const u64 diag = (a0 & b1 & ~a1 & ~b0) | (a1 & b0 & ~a0 & ~b1);
        const u64 one = (diag | (t_x & ~b_any)) & valid;      // the top pixels are never both clear here
        a2 += __builtin_popcountll(one) + 2 * __builtin_popcountll(valid & ~one);
        const u64 zn = ~(z0 | z1);
        const u64 diag_up = (a0 & z1 & ~a1 & ~z0) | (a1 & z0 & ~a0 & ~z1);
        a2 += __builtin_popcountll((zn & t_x) & valid) + 2 * __builtin_popcountll((zn & t_both) & valid) +
              __builtin_popcountll(diag_up & valid);
      } else {
        a2 += 2 * __builtin_popcountll(t_both & b_both & valid) +
              __builtin_popcountll(((t_both & b_x) | (b_both & t_x)) & valid);
      }
    }
    if (a2) atomicAdd(&ws.area[root], a2);
    if (hole) {
      int lo = 0, hi = nb;                                   // runs of the row above that share a column with [s, e]
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (((rb[mid] >> 16) & 0xffff) < s) lo = mid + 1; else hi = mid;
      }
      int contacts = 0;
      for (int j = lo; j < nb && (rb[j] & 0xffff) <= e; ++j) ++contacts;
      if (contacts != 1) atomicAdd(&euler[root], 1 - contacts);
    }
  }
}

// LARGEST: (twice the area << 32 | root id) maximum per plane; equal areas: the component found last in raster order
__global__ __launch_bounds__(256) void lay_best_kernel(int H, int RM, int* __restrict__ ws_all, int64_t ws_stride,
                                                       u64* __restrict__ best) {
  const int lane = threadIdx.x & 63;
  const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (y >= H) return;
  const CcWs ws = cc_ws(ws_all, ws_stride, blockIdx.y, H, RM);
  const int n = ws.nruns[y];
  for (int i = lane; i < n; i += 64) {
    const int id = y * RM + i;
    if (ws.parent[id] == id) atomicMax(&best[blockIdx.y], ((u64)(unsigned)ws.area[id] << 32) | (unsigned)id);
  }
}

__global__ __launch_bounds__(256) void lay_decide_kernel(int H, int W, int RM, int mode, int* __restrict__ ws_all,
                                                         int64_t ws_stride, const int* __restrict__ euler_all,
                                                         const u64* __restrict__ best, int* __restrict__ hdr) {
  const int lane = threadIdx.x & 63;
  const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (y >= H) return;
  const CcWs ws = cc_ws(ws_all, ws_stride, blockIdx.y, H, RM);
  const int* euler = euler_all + (int64_t)blockIdx.y * H * RM;
  const int n = ws.nruns[y];
  int corner = -1;
  if (mode == LAY_FLOOD && ws.nruns[0] > 0 && (ws.run[0] & 0xffff) == 0) corner = cc_find(ws.parent, 0);
  for (int i = lane; i < n; i += 64) {
    const int id = y * RM + i;
    const int root = cc_find(ws.parent, id);
    const int x0 = ws.xmin[root], x1 = ws.xmax[root], y0 = ws.ymin[root], y1 = ws.ymax[root];
    const bool inner = x0 > 0 && y0 > 0 && x1 < W - 1 && y1 < H - 1;
    bool keep;
    if (mode == LAY_FLOOD) keep = root == corner;
    else if (mode == LAY_FILL_ALL) keep = inner;
    else if (mode == LAY_LARGEST) keep = (unsigned)root == (unsigned)(best[blockIdx.y] & 0xffffffffull);
    else {                                                  // fill_object_bg_mask.py:41-45, rect = hole box grown by one
      const bool off_edge = inner && x0 > 1 && y0 > 1 && x1 < W - 2 && y1 < H - 2;
      const int a2 = ws.area[root];
      keep = off_edge && a2 >= 100;
      // a hole with foreground islands encloses more than its own cells: undecided while the box still allows 50
      if (off_edge && !keep && euler[root] < 1 && 2 * (x1 - x0 + 2) * (y1 - y0 + 2) >= 100 && id == root) {
        const int k = atomicAdd(&hdr[1], 1);
        if (k < LAY_AMB_CAP) {
          int* rec = hdr + 2 + 8 * k;
          rec[0] = blockIdx.y; rec[1] = x0; rec[2] = x1; rec[3] = y0; rec[4] = y1; rec[5] = a2;
          rec[6] = y; rec[7] = ws.run[id] & 0xffff;
        }
      }
    }
    if (keep) ws.run[id] |= (int)0x80000000;
  }
}

// components of `src` (np planes) -> the kept ones painted into `dst`
static int lay_cc(const u64* src, u64* dst, int np, int H, int W, int Wp, int conn8, int mode, int hole, int* wsbuf,
                  hipStream_t s) {
  const int RM = lay_rm(W);
  const int64_t stride = cc_ws_ints_per_plane(H, RM), ps = (int64_t)H * Wp;
  int* ws = wsbuf + LAY_HDR;
  int* euler = ws + (int64_t)np * stride;
  u64* best = (u64*)(wsbuf + LAY_BEST);
  if (hipMemsetAsync(euler, 0, (size_t)np * H * RM * sizeof(int), s) != hipSuccess) return INK_ERR_LAUNCH;
  if (hipMemsetAsync(best, 0, (size_t)np * sizeof(u64), s) != hipSuccess) return INK_ERR_LAUNCH;
  const dim3 rows((H + 3) / 4, np);
  cc_label(src, ps, np, H, W, Wp, RM, conn8, ws, wsbuf, s);
  hipLaunchKernelGGL(lay_stats_kernel, rows, dim3(256), 0, s, src, ps, H, W, Wp, RM, hole, ws, stride, euler);
  if (mode == LAY_LARGEST) hipLaunchKernelGGL(lay_best_kernel, rows, dim3(256), 0, s, H, RM, ws, stride, best);
  hipLaunchKernelGGL(lay_decide_kernel, rows, dim3(256), 0, s, H, W, RM, mode, ws, stride, (const int*)euler,
                     (const u64*)best, wsbuf);
  cc_paint(np, H, W, Wp, RM, ws, nullptr, dst, ps, s);
  return ink_launch_status();
}

// ------------------------------------------------------------------------------------------------------------------
// 5x5 chamfer distance (cv2.distanceTransform(DIST_L2, 5)) as int32 16.16: weights 65536, 91750, 143976.
// Tiled relaxation: a workgroup loads its 64x64 tile with a halo of 16 into LDS, runs 8 Jacobi passes there (a move
// spans at most 2 pixels, so the tile's pixels see every path of up to 8 moves) and writes back what got smaller.
// The image is relaxed IN PLACE: a halo value read while its owner rewrites it is the old or the new one, both are
// upper bounds of the distance, and the fixed point does not depend on which was seen.  Launch r runs only if launch
// r - 1 changed a value below the bound still needed (flags), which is 1 + the smallest stroke distance so far (mins).
#define CH_T 64
#define CH_P 8
#define CH_HALO (2 * CH_P)
#define CH_R (CH_T + 2 * CH_HALO)          // 96
#define CH_S (CH_R + 4)                    // LDS row: 2 never-written INF cells on each side
#define CH_INF 0x1fffffff                  // INT_MAX >> 2, cv2's initial value
#define CH_A 65536
#define CH_B 91750
#define CH_C 143976

__global__ __launch_bounds__(256) void lay_chamfer_init_kernel(const u64* __restrict__ mask, int H, int W, int Wp,
                                                               int* __restrict__ dist) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)H * W) return;
  const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
  const u64 wd = mask[(int64_t)blockIdx.y * H * Wp + (int64_t)y * Wp + (x >> 6)];
  dist[(int64_t)blockIdx.y * H * W + i] = (wd >> (x & 63)) & 1ull ? CH_INF : 0;
}

__global__ __launch_bounds__(256) void lay_chamfer_relax_kernel(int* __restrict__ dist_all,
                                                                const u64* __restrict__ strokes, int n, int H, int W,
                                                                int Wp, int r, int full, int* __restrict__ flags,
                                                                int* __restrict__ mins) {
  __shared__ int buf[2][CH_S * CH_S];
  __shared__ int any_fg;
  const int plane = blockIdx.z;
  if (r > 0 && flags[(r - 1) * n + plane] == 0) return;      // uniform over the workgroup
  const int bound = (full || r == 0) ? 0x7fffffff : mins[(r - 1) * n + plane] + CH_A;
  int* dist = dist_all + (int64_t)plane * H * W;
  const int ty0 = blockIdx.y * CH_T, tx0 = blockIdx.x * CH_T;
  const int tid = threadIdx.x;
  if (tid == 0) any_fg = 0;
  for (int i = tid; i < CH_S * CH_S; i += 256) buf[0][i] = buf[1][i] = CH_INF;
  __syncthreads();
  int fg = 0;
  for (int i = tid; i < CH_R * CH_R; i += 256) {
    const int ry = i / CH_R, rx = i - ry * CH_R;
    const int gy = ty0 - CH_HALO + ry, gx = tx0 - CH_HALO + rx;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const int v = dist[(int64_t)gy * W + gx];
      buf[0][(ry + 2) * CH_S + rx + 2] = v;
      if (v > 0 && ry >= CH_HALO && ry < CH_HALO + CH_T && rx >= CH_HALO && rx < CH_HALO + CH_T) fg = 1;
    }
  }
  if (fg) any_fg = 1;
  __syncthreads();
  if (!any_fg) return;                                       // a tile of zeros never changes and holds no stroke
  for (int p = 0; p < CH_P; ++p) {
    const int* src = buf[p & 1];
    int* dst = buf[(p & 1) ^ 1];
    for (int i = tid; i < CH_R * CH_R; i += 256) {
      const int ry = i / CH_R, rx = i - ry * CH_R;
      const int gy = ty0 - CH_HALO + ry, gx = tx0 - CH_HALO + rx;
      const int c = (ry + 2) * CH_S + rx + 2;
      int v = src[c];
      if (v > 0 && gy >= 0 && gy < H && gx >= 0 && gx < W) {  // pixels outside the image stay unreachable
        int m = min(min(src[c - 1], src[c + 1]), min(src[c - CH_S], src[c + CH_S])) + CH_A;
        const int d = min(min(src[c - CH_S - 1], src[c - CH_S + 1]), min(src[c + CH_S - 1], src[c + CH_S + 1])) + CH_B;
        const int k = min(min(min(src[c - 2 * CH_S - 1], src[c - 2 * CH_S + 1]), min(src[c + 2 * CH_S - 1], src[c + 2 * CH_S + 1])),
                          min(min(src[c - CH_S - 2], src[c - CH_S + 2]), min(src[c + CH_S - 2], src[c + CH_S + 2]))) + CH_C;
        m = min(m, min(d, k));
        v = min(v, m);
      }
      dst[c] = v;
    }
    __syncthreads();
  }
  const int* fin = buf[CH_P & 1];
  int changed = 0, smin = 0x7fffffff;
  const u64* sp = strokes + (int64_t)plane * H * Wp;
  for (int i = tid; i < CH_T * CH_T; i += 256) {
    const int ry = i / CH_T, rx = i - ry * CH_T;
    const int gy = ty0 + ry, gx = tx0 + rx;
    if (gy >= H || gx >= W) continue;
    const int v = fin[(ry + CH_HALO + 2) * CH_S + rx + CH_HALO + 2];
    const int64_t g = (int64_t)gy * W + gx;
    if (v < dist[g]) {
      dist[g] = v;
      if (v < bound) changed = 1;
    }
    if ((sp[(int64_t)gy * Wp + (gx >> 6)] >> (gx & 63)) & 1ull) smin = min(smin, v);
  }
  if (changed) atomicOr(&flags[r * n + plane], 1);
  if (smin != 0x7fffffff) atomicMin(&mins[r * n + plane], smin);
}

__global__ __launch_bounds__(256) void lay_chamfer_min_kernel(const int* __restrict__ dist, const u64* __restrict__ strokes,
                                                              int H, int W, int Wp, int* __restrict__ minv) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)H * W) return;
  const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
  if ((strokes[(int64_t)blockIdx.y * H * Wp + (int64_t)y * Wp + (x >> 6)] >> (x & 63)) & 1ull)
    atomicMin(&minv[blockIdx.y], dist[(int64_t)blockIdx.y * H * W + i]);
}

// shrink_by = max(0, floor(min distance as float32) - safety_margin); out = shrink_by > 0 ? dist >= shrink_by : mask,
// the comparison made on float32(dist) * 2^-16 as cv2 hands the image out (fill_object_bg_mask.py:103-107)
__global__ __launch_bounds__(256) void lay_chamfer_thresh_kernel(const int* __restrict__ dist, const u64* __restrict__ mask,
                                                                 int H, int W, int Wp, int margin,
                                                                 const int* __restrict__ minv, int* __restrict__ min_out,
                                                                 int* __restrict__ shrink_out, u64* __restrict__ out) {
  const int word = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (word >= H * Wp) return;
  const int y = word / Wp, w = word - y * Wp, x = w * 64 + lane;
  const int mv = minv[blockIdx.y];
  int shrink = 0;
  if (mv <= CH_INF) {                                        // above CH_INF: no stroke pixel at all (the memset value)
    shrink = (int)floorf((float)mv * (1.0f / 65536.0f)) - margin;
    if (shrink < 0) shrink = 0;
  }
  const int64_t po = (int64_t)blockIdx.y * H * Wp + word;
  bool on = false;
  if (x < W) {
    if (shrink > 0) on = (float)dist[((int64_t)blockIdx.y * H + y) * W + x] * (1.0f / 65536.0f) >= (float)shrink;
    else on = (mask[po] >> lane) & 1ull;
  }
  const u64 m = __ballot(on);
  if (lane == 0) out[po] = m;
  if (word == 0 && lane == 0) {
    min_out[blockIdx.y] = mv;
    shrink_out[blockIdx.y] = shrink;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// pixel kernels
// bbox[m] = (x1, y1, x2, y2) of mask > 127 with INCLUSIVE maxima (util.py:198-204); (W, H, -1, -1) when empty
__global__ __launch_bounds__(256) void lay_bbox_kernel(const uint8_t* __restrict__ masks, int H, int W,
                                                       int* __restrict__ bbox) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)H * W) return;
  if (masks[(int64_t)blockIdx.y * H * W + i] > 127) {
    const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
    int* b = bbox + 4 * blockIdx.y;
    atomicMin(&b[0], x);
    atomicMin(&b[1], y);
    atomicMax(&b[2], x);
    atomicMax(&b[3], y);
  }
}
__global__ void lay_bbox_init_kernel(int n, int H, int W, int* __restrict__ bbox) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n) return;
  bbox[4 * m] = W; bbox[4 * m + 1] = H; bbox[4 * m + 2] = -1; bbox[4 * m + 3] = -1;
}

// overlap[i, j] = 1 iff j < i and mask i has a pixel in rows [y1, y2) and columns [x1, x2) of mask j's box: the box is
// sliced exclusively, its last row and column drop out (util.py:40-55, 148-157)
__global__ __launch_bounds__(256) void lay_overlap_kernel(const uint8_t* __restrict__ masks, int n, int H, int W,
                                                          const int* __restrict__ bbox, int* __restrict__ overlap) {
  const int i = blockIdx.x / n, j = blockIdx.x - i * n;
  if (j >= i) return;                                        // the table was zeroed
  const int x1 = bbox[4 * j], y1 = bbox[4 * j + 1], x2 = bbox[4 * j + 2], y2 = bbox[4 * j + 3];
  const int bw = x2 - x1, bh = y2 - y1;
  if (bw <= 0 || bh <= 0) return;
  const uint8_t* mi = masks + (int64_t)i * H * W;
  int hit = 0;
  for (int k = threadIdx.x; k < bw * bh && !hit; k += 256) {
    const int yy = y1 + k / bw, xx = x1 + k % bw;
    if (mi[(int64_t)yy * W + xx] > 0) hit = 1;
  }
  if (hit) atomicOr(&overlap[i * n + j], 1);
}

// per layer i: sketch layer (the sketch's B, G, R inside mask i, 255 outside: util.py:31-34), edit mask (OR of the
// overlapped background planes, inside mask i's exclusively sliced box, minus mask i: util.py:94-98) and debug image
// (white mask, edit region (0, 0, 255): util.py:242-260; a layer without overlaps gets its mask as 0 / 255)
__global__ __launch_bounds__(256) void lay_assemble_kernel(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ masks,
                                                           const u64* __restrict__ bg, const int* __restrict__ bbox,
                                                           const int* __restrict__ overlap, int n, int H, int W, int Wp,
                                                           uint8_t* __restrict__ sketch, uint8_t* __restrict__ edit,
                                                           uint8_t* __restrict__ debug) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int i = blockIdx.y;
  const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
  const bool m = masks[(int64_t)i * H * W + p] > 0;
  const int64_t o3 = ((int64_t)i * H * W + p) * 3;
  sketch[o3] = m ? rgb[p * 3 + 2] : 255;
  sketch[o3 + 1] = m ? rgb[p * 3 + 1] : 255;
  sketch[o3 + 2] = m ? rgb[p * 3] : 255;
  const bool inbox = x >= bbox[4 * i] && x < bbox[4 * i + 2] && y >= bbox[4 * i + 1] && y < bbox[4 * i + 3];
  bool any = false, e = false;
  for (int j = 0; j < i; ++j) {
    if (!overlap[i * n + j]) continue;
    any = true;
    if (inbox && !m && ((bg[((int64_t)j * H + y) * Wp + (x >> 6)] >> (x & 63)) & 1ull)) e = true;
  }
  edit[(int64_t)i * H * W + p] = e ? 255 : 0;
  uint8_t d0 = m ? 255 : 0, d1 = d0, d2 = d0;
  if (any && e) { d0 = 0; d1 = 0; d2 = 255; }
  debug[o3] = d0; debug[o3 + 1] = d1; debug[o3 + 2] = d2;
}

// final = inpainted with the sketch layer's pixels (swapped back to R, G, B) wherever a channel of it is < 255
// (util.py:101, 109-133)
__global__ __launch_bounds__(256) void lay_composite_kernel(const uint8_t* __restrict__ inpainted, const uint8_t* __restrict__ sketch,
                                                            int64_t npix, uint8_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= npix) return;
  const uint8_t b = sketch[p * 3], g = sketch[p * 3 + 1], r = sketch[p * 3 + 2];
  const bool keep = b < 255 || g < 255 || r < 255;
  out[p * 3] = keep ? r : inpainted[p * 3];
  out[p * 3 + 1] = keep ? g : inpainted[p * 3 + 1];
  out[p * 3 + 2] = keep ? b : inpainted[p * 3 + 2];
}

// cv2.imread(IMREAD_GRAYSCALE) of an 8-bit RGB file: cv_gray15
__global__ __launch_bounds__(256) void lay_gray_kernel(const uint8_t* __restrict__ rgb, int64_t npix, uint8_t* __restrict__ gray) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= npix) return;
  gray[p] = (uint8_t)cv_gray15(rgb[p * 3], rgb[p * 3 + 1], rgb[p * 3 + 2]);
}

// RGBA layer (fill_object_bg_mask.py:141, 165-177): alpha = grey < 240 or background; colour = grey on sketch pixels,
// white on the remaining background pixels, 0 elsewhere
__global__ __launch_bounds__(256) void lay_rgba_kernel(const uint8_t* __restrict__ gray, const u64* __restrict__ bg, int H,
                                                       int W, int Wp, uint8_t* __restrict__ rgba) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
  const int g = gray[(int64_t)blockIdx.y * H * W + p];
  const bool b = (bg[((int64_t)blockIdx.y * H + y) * Wp + (x >> 6)] >> (x & 63)) & 1ull;
  const bool sk = g < 240;
  const uint8_t c = sk ? (uint8_t)g : (b ? 255 : 0);
  uint8_t* o = rgba + ((int64_t)blockIdx.y * H * W + p) * 4;
  o[0] = c; o[1] = c; o[2] = c; o[3] = (sk || b) ? 255 : 0;
}

static inline bool lay_dims_ok(int n, int H, int W) { return n > 0 && n <= 254 && H > 0 && W > 0 && H <= 16383 && W <= 16383; }
static inline unsigned lay_blocks(int64_t items) { return (unsigned)((items + 255) / 256); }

}  // namespace

extern "C" int ink_layers_otsu_planes(const void* gray_u8, int32_t n, int32_t H, int32_t W, int32_t invert,
                                      int32_t* hist, int32_t* thresh, void* out_planes, void* stream) {
  INK_CHECK_ARG(gray_u8 && hist && thresh && out_planes && lay_dims_ok(n, H, W));
  hipStream_t s = (hipStream_t)stream;
  const int Wp = (W + 63) / 64;
  const int64_t npix = (int64_t)H * W;
  if (hipMemsetAsync(hist, 0, (size_t)n * 256 * sizeof(int32_t), s) != hipSuccess) return INK_ERR_LAUNCH;
  const unsigned hb = (unsigned)((npix + 256 * 16 - 1) / (256 * 16));
  hipLaunchKernelGGL(lay_hist_kernel, dim3(hb, n), dim3(256), 0, s, (const uint8_t*)gray_u8, npix, invert, hist);
  hipLaunchKernelGGL(lay_otsu_kernel, dim3((n + 63) / 64), dim3(64), 0, s, (const int*)hist, n, thresh);
  hipLaunchKernelGGL(lay_pack_kernel, dim3((H * Wp + 3) / 4, n), dim3(256), 0, s, (const uint8_t*)gray_u8, H, W, Wp,
                     invert, (const int*)thresh, (u64*)out_planes);
  return ink_launch_status();
}

extern "C" int ink_layers_dilate(const void* planes, int32_t n, int32_t H, int32_t W, int32_t kernel_size,
                                 int32_t iterations, void* tmp_planes, void* out_planes, void* stream) {
  INK_CHECK_ARG(planes && tmp_planes && out_planes && lay_dims_ok(n, H, W));
  INK_CHECK_ARG((kernel_size == 3 || kernel_size == 5) && iterations >= 1 && iterations <= 64);
  INK_CHECK_ARG(planes != out_planes && planes != tmp_planes && tmp_planes != out_planes);
  hipStream_t s = (hipStream_t)stream;
  const int Wp = (W + 63) / 64;
  const BpShape sh = kernel_size == 3 ? bp_shape_cross() : bp_shape_ellipse5();
  const u64* src = (const u64*)planes;
  for (int it = 0; it < iterations; ++it) {                 // the last pass lands in out_planes
    u64* dst = ((iterations - 1 - it) & 1) ? (u64*)tmp_planes : (u64*)out_planes;
    hipLaunchKernelGGL(bp_morph_kernel, dim3((H * Wp + 255) / 256, n), dim3(256), 0, s, src, dst, H, W, Wp, sh, 0,
                       (int64_t)H * Wp);
    src = dst;
  }
  return ink_launch_status();
}

extern "C" int ink_layers_border_band(const void* planes, int32_t n, int32_t H, int32_t W, int32_t band, int32_t* flags,
                                      void* stream) {
  INK_CHECK_ARG(planes && flags && lay_dims_ok(n, H, W) && band >= 1);
  hipStream_t s = (hipStream_t)stream;
  const int Wp = (W + 63) / 64;
  if (hipMemsetAsync(flags, 0, (size_t)n * sizeof(int32_t), s) != hipSuccess) return INK_ERR_LAUNCH;
  hipLaunchKernelGGL(lay_band_kernel, dim3((H * Wp + 255) / 256, n), dim3(256), 0, s, (const u64*)planes, H, W, Wp, band,
                     flags);
  return ink_launch_status();
}

extern "C" int ink_layers_components_workspace_ints(int32_t n, int32_t H, int32_t W, int64_t* out_ints) {
  INK_CHECK_ARG(out_ints && lay_dims_ok(n, H, W));
  const int RM = lay_rm(W);
  *out_ints = LAY_HDR + (int64_t)n * (cc_ws_ints_per_plane(H, RM) + (int64_t)H * RM);
  return INK_OK;
}

extern "C" int ink_layers_components(const void* planes, int32_t n, int32_t H, int32_t W, int32_t mode, void* tmp_planes3,
                                     int32_t* workspace, void* out_planes, void* stream) {
  INK_CHECK_ARG(planes && tmp_planes3 && workspace && out_planes && lay_dims_ok(n, H, W));
  INK_CHECK_ARG(mode >= LAY_FLOOD && mode <= LAY_LARGEST && planes != out_planes);
  hipStream_t s = (hipStream_t)stream;
  const int Wp = (W + 63) / 64;
  INK_CHECK_ARG(4 * Wp * sizeof(u64) <= 64 * 1024);
  const int64_t ps = (int64_t)H * Wp;
  const u64* in = (const u64*)planes;
  u64* out = (u64*)out_planes;
  u64* ta = (u64*)tmp_planes3;
  u64* tb = ta + (int64_t)n * ps;
  u64* tc = tb + (int64_t)n * ps;
  if (hipMemsetAsync(workspace, 0, LAY_HDR * sizeof(int32_t), s) != hipSuccess) return INK_ERR_LAUNCH;
  int rc;
  if (mode == LAY_LARGEST) {
    // the component with the largest outer contour area, then what it surrounds (drawContours of an external contour)
    if ((rc = lay_cc(in, ta, n, H, W, Wp, 1, LAY_LARGEST, 0, workspace, s)) != INK_OK) return rc;
    bp_logic(BP_NOT, ta, nullptr, nullptr, tb, n, H, W, s);
    if ((rc = lay_cc(tb, tc, n, H, W, Wp, 0, LAY_FILL_ALL, 1, workspace, s)) != INK_OK) return rc;
    bp_logic(BP_OR, ta, tc, nullptr, out, n, H, W, s);
    return ink_launch_status();
  }
  bp_logic(BP_NOT, in, nullptr, nullptr, ta, n, H, W, s);
  if ((rc = lay_cc(ta, tb, n, H, W, Wp, 0, mode, 1, workspace, s)) != INK_OK) return rc;
  if (mode == LAY_FLOOD) {     // ~flooded | planes = everything but the flooded background component
    bp_logic(BP_NOT, tb, nullptr, nullptr, out, n, H, W, s);
    return ink_launch_status();
  }
  if (mode == LAY_FILL_ALL) {
    bp_logic(BP_OR, in, tb, nullptr, out, n, H, W, s);
    return ink_launch_status();
  }
  // a filled hole is filled as a polygon: with everything it surrounds = the 8-connected components of the
  // complement of the filled holes that do not reach the image edge
  bp_logic(BP_NOT, tb, nullptr, nullptr, ta, n, H, W, s);
  // (the header keeps the undecided-hole records of the first pass: lay_cc does not clear it)
  if ((rc = lay_cc(ta, tc, n, H, W, Wp, 1, LAY_FILL_ALL, 0, workspace, s)) != INK_OK) return rc;
  bp_logic(BP_OR3, in, tb, tc, out, n, H, W, s);
  return ink_launch_status();
}

extern "C" int ink_layers_chamfer_workspace_ints(int32_t n, int32_t H, int32_t W, int64_t* out_ints) {
  INK_CHECK_ARG(out_ints && lay_dims_ok(n, H, W));
  const int L = ((H > W ? H : W) + CH_P - 1) / CH_P + 1;
  *out_ints = (int64_t)n * (2 * L + 1);
  return INK_OK;
}

extern "C" int ink_layers_chamfer(const void* mask_planes, const void* stroke_planes, int32_t n, int32_t H, int32_t W,
                                  int32_t safety_margin, int32_t full, int32_t* dist, int32_t* workspace, int32_t* min_out,
                                  int32_t* shrink_out, void* out_planes, void* stream) {
  INK_CHECK_ARG(mask_planes && stroke_planes && dist && workspace && min_out && shrink_out && out_planes);
  INK_CHECK_ARG(lay_dims_ok(n, H, W) && safety_margin >= 0);
  hipStream_t s = (hipStream_t)stream;
  const int Wp = (W + 63) / 64;
  const int L = ((H > W ? H : W) + CH_P - 1) / CH_P + 1;
  int* flags = workspace;
  int* mins = workspace + (int64_t)L * n;                    // L rows + the final minimum
  if (hipMemsetAsync(flags, 0, (size_t)L * n * sizeof(int), s) != hipSuccess) return INK_ERR_LAUNCH;
  if (hipMemsetAsync(mins, 0x7f, (size_t)(L + 1) * n * sizeof(int), s) != hipSuccess) return INK_ERR_LAUNCH;
  const dim3 px(lay_blocks((int64_t)H * W), n);
  hipLaunchKernelGGL(lay_chamfer_init_kernel, px, dim3(256), 0, s, (const u64*)mask_planes, H, W, Wp, dist);
  const dim3 tiles((W + CH_T - 1) / CH_T, (H + CH_T - 1) / CH_T, n);
  for (int r = 0; r < L; ++r)
    hipLaunchKernelGGL(lay_chamfer_relax_kernel, tiles, dim3(256), 0, s, dist, (const u64*)stroke_planes, n, H, W, Wp, r,
                       full, flags, mins);
  int* minv = mins + (int64_t)L * n;
  hipLaunchKernelGGL(lay_chamfer_min_kernel, px, dim3(256), 0, s, (const int*)dist, (const u64*)stroke_planes, H, W, Wp, minv);
  hipLaunchKernelGGL(lay_chamfer_thresh_kernel, dim3((H * Wp + 3) / 4, n), dim3(256), 0, s, (const int*)dist,
                     (const u64*)mask_planes, H, W, Wp, safety_margin, (const int*)minv, min_out, shrink_out,
                     (u64*)out_planes);
  return ink_launch_status();
}

extern "C" int ink_layers_mask_tables(const void* masks_u8, int32_t n, int32_t H, int32_t W, int32_t* bbox,
                                      int32_t* overlap, void* stream) {
  INK_CHECK_ARG(masks_u8 && bbox && overlap && lay_dims_ok(n, H, W));
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(overlap, 0, (size_t)n * n * sizeof(int32_t), s) != hipSuccess) return INK_ERR_LAUNCH;
  hipLaunchKernelGGL(lay_bbox_init_kernel, dim3((n + 63) / 64), dim3(64), 0, s, n, H, W, bbox);
  hipLaunchKernelGGL(lay_bbox_kernel, dim3(lay_blocks((int64_t)H * W), n), dim3(256), 0, s, (const uint8_t*)masks_u8, H, W, bbox);
  hipLaunchKernelGGL(lay_overlap_kernel, dim3(n * n), dim3(256), 0, s, (const uint8_t*)masks_u8, n, H, W, (const int*)bbox,
                     overlap);
  return ink_launch_status();
}

extern "C" int ink_layers_assemble(const void* sketch_rgb_u8, const void* masks_u8, const void* bg_planes,
                                   const int32_t* bbox, const int32_t* overlap, int32_t n, int32_t H, int32_t W,
                                   void* sketch_layers_u8, void* edit_masks_u8, void* debug_u8, void* stream) {
  INK_CHECK_ARG(sketch_rgb_u8 && masks_u8 && bg_planes && bbox && overlap && sketch_layers_u8 && edit_masks_u8 && debug_u8);
  INK_CHECK_ARG(lay_dims_ok(n, H, W));
  hipLaunchKernelGGL(lay_assemble_kernel, dim3(lay_blocks((int64_t)H * W), n), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)sketch_rgb_u8, (const uint8_t*)masks_u8, (const u64*)bg_planes, bbox, overlap, n, H, W,
                     (W + 63) / 64, (uint8_t*)sketch_layers_u8, (uint8_t*)edit_masks_u8, (uint8_t*)debug_u8);
  return ink_launch_status();
}

extern "C" int ink_layers_composite(const void* inpainted_rgb_u8, const void* sketch_layer_u8, int32_t H, int32_t W,
                                    void* out_rgb_u8, void* stream) {
  INK_CHECK_ARG(inpainted_rgb_u8 && sketch_layer_u8 && out_rgb_u8 && H > 0 && W > 0);
  hipLaunchKernelGGL(lay_composite_kernel, dim3(lay_blocks((int64_t)H * W)), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)inpainted_rgb_u8, (const uint8_t*)sketch_layer_u8, (int64_t)H * W, (uint8_t*)out_rgb_u8);
  return ink_launch_status();
}

extern "C" int ink_layers_gray(const void* rgb_u8, int32_t n, int32_t H, int32_t W, void* gray_u8, void* stream) {
  INK_CHECK_ARG(rgb_u8 && gray_u8 && n > 0 && H > 0 && W > 0);
  const int64_t npix = (int64_t)n * H * W;
  hipLaunchKernelGGL(lay_gray_kernel, dim3(lay_blocks(npix)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)rgb_u8,
                     npix, (uint8_t*)gray_u8);
  return ink_launch_status();
}

extern "C" int ink_layers_rgba(const void* gray_u8, const void* bg_planes, int32_t n, int32_t H, int32_t W, void* rgba_u8,
                               void* stream) {
  INK_CHECK_ARG(gray_u8 && bg_planes && rgba_u8 && lay_dims_ok(n, H, W));
  hipLaunchKernelGGL(lay_rgba_kernel, dim3(lay_blocks((int64_t)H * W), n), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)gray_u8, (const u64*)bg_planes, H, W, (W + 63) / 64, (uint8_t*)rgba_u8);
  return ink_launch_status();
}
