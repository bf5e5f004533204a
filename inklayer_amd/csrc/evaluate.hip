// Evaluation stage: scoring a run against a ground-truth label image (InkScenes' INSTANCE_GT / CLASS_GT, or
// the masks_final/ of another run) is counting - how many pixels does prediction i share with ground-truth instance u -
// and everything else (IoU, AP / AR, PQ) is float64 arithmetic on that small integer table on the host
// (inklayer_amd/evaluate.py).  Four integer passes over the flat pixel array, results exact and order-independent:
//   label ranks    the distinct values of the label image (0 .. 65535) as a sorted table, and per pixel the index of its
//                  value in that table: presence bitmap (65536 bits, per workgroup in LDS, OR-ed into global memory) ->
//                  word prefix counts (one workgroup) -> rank = prefix[v >> 5] + popcount(word below the bit)
//   contingency    T[i, u] = pixels inside prediction i with ground-truth rank u; row n = every counted pixel
//   label boxes    per rank the bounding box of its pixels
//   paint          rank -> colour (the reference's InkScenes/read_GT_mat_file.py:40-70 picture)
// Every phase is its own launch and no workgroup reads what another workgroup of the same launch wrote (bitplane.h);
// cross-workgroup sums are device-scope integer atomics into buffers cleared by an earlier memset or launch, after a
// reduction in LDS (one global atomic per non-zero bin and workgroup).
// A lane owns four consecutive pixels, moved as one word per array where the base address allows it, as single
// elements otherwise and for the last H W % 4 pixels.
#include "common.h"
#include "../../include/inklayer_hip.h"

namespace {

#define EVAL_STROKE 250              // inklayer_amd/visualize.py STROKE_BELOW: a stroke pixel has grey < 250
#define EVAL_BITMAP_WORDS 2048       // 65536 bits
#define EVAL_MAX_U 256
#define EVAL_TILE 32                 // prediction rows per workgroup of the contingency kernel
#define EVAL_CHUNK 1024              // pixels per workgroup step: 256 lanes x 4
enum { EVAL_AL_LABELS = 1, EVAL_AL_RANK = 2, EVAL_AL_PRED = 4, EVAL_AL_SKETCH = 8, EVAL_AL_OUT = 16 };

// bit j set: pixel p + j exists and is a stroke pixel (grey < 250; cv_gray14, as csrc/visualize.hip and
// visualize.gray_host)
__device__ __forceinline__ unsigned eval_strokes4(const uint8_t* __restrict__ sk, int channels, int64_t p, int count,
                                                  bool wide) {
  int g[4];
  if (wide && count == 4) {
    if (channels == 3) {
      const uint32_t* w = (const uint32_t*)(sk + 3 * p);
      const uint32_t a = w[0], b = w[1], c = w[2];           // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
      g[0] = cv_gray14(a & 255u, (a >> 8) & 255u, (a >> 16) & 255u);
      g[1] = cv_gray14(a >> 24, b & 255u, (b >> 8) & 255u);
      g[2] = cv_gray14((b >> 16) & 255u, b >> 24, c & 255u);
      g[3] = cv_gray14((c >> 8) & 255u, (c >> 16) & 255u, c >> 24);
    } else {
      const uint32_t a = *(const uint32_t*)(sk + p);
      g[0] = a & 255u; g[1] = (a >> 8) & 255u; g[2] = (a >> 16) & 255u; g[3] = a >> 24;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      g[j] = 255;
      if (j < count) {
        const uint8_t* q = sk + (p + j) * channels;
        g[j] = channels == 3 ? cv_gray14(q[0], q[1], q[2]) : (int)q[0];
      }
    }
  }
  unsigned m = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (g[j] < EVAL_STROKE) m |= 1u << j;
  return m;
}

// four bytes at q as one little-endian word (zeros past `count`)
__device__ __forceinline__ uint32_t eval_bytes4(const uint8_t* __restrict__ q, int count, bool wide) {
  if (wide && count == 4) return *(const uint32_t*)q;
  uint32_t w = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < count) w |= (uint32_t)q[j] << (8 * j);
  return w;
}

// the ranks of the pixels p .. p + 3 (0 past `count`)
__device__ __forceinline__ void eval_ranks4(const uint16_t* __restrict__ rank, int64_t p, int count, bool wide, int r[4]) {
  if (wide && count == 4) {
    const uint2 w = *(const uint2*)(rank + p);
    r[0] = w.x & 0xffffu; r[1] = w.x >> 16; r[2] = w.y & 0xffffu; r[3] = w.y >> 16;
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = j < count ? (int)rank[p + j] : 0;
}

// the label values of the pixels p .. p + 3 (uint8 / uint16 / int32 elements; 0 past `count`)
__device__ __forceinline__ void eval_labels4(const void* __restrict__ labels, int esize, int64_t p, int count, bool wide,
                                             int v[4]) {
  if (wide && count == 4) {
    if (esize == 1) {
      const uint32_t w = *(const uint32_t*)((const uint8_t*)labels + p);
      v[0] = w & 255u; v[1] = (w >> 8) & 255u; v[2] = (w >> 16) & 255u; v[3] = w >> 24;
    } else if (esize == 2) {
      const uint2 w = *(const uint2*)((const uint16_t*)labels + p);
      v[0] = w.x & 0xffffu; v[1] = w.x >> 16; v[2] = w.y & 0xffffu; v[3] = w.y >> 16;
    } else {
      const int4 w = *(const int4*)((const int32_t*)labels + p);
      v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = 0;
    if (j < count) {
      // the label image may start at any byte: wider elements are put together from bytes
      const uint8_t* q = (const uint8_t*)labels + esize * (p + j);
      if (esize == 1) v[j] = q[0];
      else if (esize == 2) v[j] = (int)((uint32_t)q[0] | ((uint32_t)q[1] << 8));
      else v[j] = (int)((uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24));
    }
  }
}

__device__ __forceinline__ int eval_count(int64_t npix, int64_t p) {
  const int64_t left = npix - p;
  return left >= 4 ? 4 : (left > 0 ? (int)left : 0);
}

// (a) 1/3: which of the 65536 values occur.  A workgroup walks steps of 1024 pixels (grid-stride), marks its values in
// an LDS bitmap (an LDS atomic only where the bit is not seen set: a stale read costs one needless atomic, never a missed
// one) and ORs its non-zero words into the global bitmap; info[1] is raised for a value outside 0 .. 65535.
__global__ __launch_bounds__(256) void eval_presence_kernel(const void* __restrict__ labels, int esize, int64_t npix,
                                                            int aligned, uint32_t* __restrict__ bitmap,
                                                            int32_t* __restrict__ info) {
  __shared__ uint32_t bm[EVAL_BITMAP_WORDS];
  __shared__ int bad_any;
  for (int i = threadIdx.x; i < EVAL_BITMAP_WORDS; i += 256) bm[i] = 0;
  if (threadIdx.x == 0) bad_any = 0;
  __syncthreads();
  const int64_t chunks = (npix + EVAL_CHUNK - 1) / EVAL_CHUNK;
  bool bad = false;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int64_t p = (c * 256 + threadIdx.x) * 4;
    const int count = eval_count(npix, p);
    if (count == 0) continue;
    int v[4];
    eval_labels4(labels, esize, p, count, aligned & EVAL_AL_LABELS, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= count) continue;
      if (v[j] < 0 || v[j] > 65535) { bad = true; continue; }
      const uint32_t bit = 1u << (v[j] & 31);
      volatile uint32_t* word = &bm[v[j] >> 5];
      if (!(*word & bit)) atomicOr(&bm[v[j] >> 5], bit);
    }
  }
  if (bad) bad_any = 1;                                    // every writer stores the same value
  __syncthreads();
  for (int i = threadIdx.x; i < EVAL_BITMAP_WORDS; i += 256)
    if (bm[i]) atomicOr(&bitmap[i], bm[i]);
  if (threadIdx.x == 0 && bad_any) atomicOr((unsigned*)&info[1], 1u);
}

// (a) 2/3: one workgroup.  prefix[w] = number of set bits in the words before w; values[k] = the k-th set bit (the
// first `cap` of them); info[0] = their number U.  Thread t owns the words 8 t .. 8 t + 7.
__global__ __launch_bounds__(256) void eval_prefix_kernel(const uint32_t* __restrict__ bitmap, uint32_t* __restrict__ prefix,
                                                          int32_t* __restrict__ values, int cap, int32_t* __restrict__ info) {
  __shared__ int part[256];
  uint32_t w[8];
  int mine = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    w[k] = bitmap[8 * threadIdx.x + k];
    mine += __popc(w[k]);
  }
  part[threadIdx.x] = mine;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {                      // inclusive scan over the 256 threads
    const int add = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  int at = part[threadIdx.x] - mine;
  if (threadIdx.x == 255) info[0] = part[255];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    prefix[8 * threadIdx.x + k] = (uint32_t)at;
    uint32_t rest = w[k];
    while (rest) {
      const int b = __ffs(rest) - 1;
      rest &= rest - 1;
      if (at < cap) values[at] = 32 * (8 * threadIdx.x + k) + b;
      ++at;
    }
  }
}

// (a) 3/3: rank = index of the pixel's value in the sorted table (0 for a value outside 0 .. 65535: info[1] is set then)
__global__ __launch_bounds__(256) void eval_rank_kernel(const void* __restrict__ labels, int esize, int64_t npix, int aligned,
                                                        const uint32_t* __restrict__ bitmap,
                                                        const uint32_t* __restrict__ prefix, uint16_t* __restrict__ rank) {
  const int64_t p = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  const int count = eval_count(npix, p);
  if (count == 0) return;
  int v[4];
  eval_labels4(labels, esize, p, count, aligned & EVAL_AL_LABELS, v);
  uint32_t r[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    r[j] = 0;
    if (j < count && v[j] >= 0 && v[j] <= 65535) {
      const int w = v[j] >> 5;
      r[j] = prefix[w] + (uint32_t)__popc(bitmap[w] & ((1u << (v[j] & 31)) - 1u));
    }
  }
  if ((aligned & EVAL_AL_RANK) && count == 4) {
    *(uint2*)(rank + p) = make_uint2(r[0] | (r[1] << 16), r[2] | (r[3] << 16));
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < count) rank[p + j] = (uint16_t)r[j];
  }
}

// (b) blockIdx.y = tile of 32 table rows (row n, "every counted pixel", is the last row of the last tile), blockIdx.x
// walks steps of 1024 pixels grid-stride.  Per pixel a 32-bit membership word of the tile's rows; per bit the wave adds
// into the workgroup's LDS table [32][U]: where every lane holding the bit has the same column, its first lane adds their
// number, otherwise each lane adds 1.  At the end the non-zero bins go to T by one global atomicAdd each.
__global__ __launch_bounds__(256) void eval_contingency_kernel(const uint8_t* __restrict__ pred, int n, int by_label,
                                                               const uint16_t* __restrict__ rank, int U,
                                                               const uint8_t* __restrict__ sk, int channels, int64_t npix,
                                                               int aligned, int32_t* __restrict__ T) {
  __shared__ int tab[EVAL_TILE * EVAL_MAX_U];
  const int row0 = (int)blockIdx.y * EVAL_TILE;
  const int nmask = min(EVAL_TILE, max(0, n - row0));                  // mask rows of this tile
  const int nbits = min(EVAL_TILE, n + 1 - row0);                      // its rows, row n included
  const unsigned allbit = (n - row0 < EVAL_TILE) ? (1u << (n - row0)) : 0u;
  for (int i = threadIdx.x; i < EVAL_TILE * U; i += 256) tab[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t chunks = (npix + EVAL_CHUNK - 1) / EVAL_CHUNK;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {          // uniform trip count: the ballots below see whole waves
    const int64_t p = (c * 256 + threadIdx.x) * 4;
    const int count = eval_count(npix, p);
    unsigned m[4] = {0u, 0u, 0u, 0u};
    int col[4] = {0, 0, 0, 0};
    unsigned counted = 0;
    if (count) counted = sk ? eval_strokes4(sk, channels, p, count, aligned & EVAL_AL_SKETCH) : ((1u << count) - 1u);
    if (counted) {
      eval_ranks4(rank, p, count, aligned & EVAL_AL_RANK, col);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (col[j] >= U) { counted &= ~(1u << j); col[j] = 0; }       // not a rank of this table: the pixel is left out
      const bool wide = aligned & EVAL_AL_PRED;
      if (by_label) {
        const uint32_t w = eval_bytes4(pred + p, count, wide);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int l = (int)((w >> (8 * j)) & 255u);
          const int b = l - 1 - row0;
          if (l >= 1 && l <= n && b >= 0 && b < EVAL_TILE) m[j] = 1u << b;
        }
      } else {
#pragma unroll 4
        for (int k = 0; k < nmask; ++k) {
          const uint32_t w = eval_bytes4(pred + (int64_t)(row0 + k) * npix + p, count, wide);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if ((w >> (8 * j)) & 255u) m[j] |= 1u << k;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) m[j] = ((counted >> j) & 1u) ? (m[j] | allbit) : 0u;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (__ballot(m[j] != 0u) == 0ull) continue;
      for (int b = 0; b < nbits; ++b) {
        const bool has = (m[j] >> b) & 1u;
        const unsigned long long holders = __ballot(has);
        if (holders == 0ull) continue;
        const int leader = __ffsll((long long)holders) - 1;
        const int lcol = __builtin_amdgcn_readlane(col[j], leader);
        const unsigned long long same = __ballot(has && col[j] == lcol);
        if (same == holders) {
          if (lane == leader) atomicAdd(&tab[b * U + lcol], (int)__popcll(holders));
        } else if (has) {
          atomicAdd(&tab[b * U + col[j]], 1);
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nbits * U; i += 256) {
    const int v = tab[i];
    if (v) atomicAdd(&T[(int64_t)row0 * U + i], v);                    // (row0 + i / U) U + i % U
  }
}

// (c) boxes[u] = (INT_MAX, INT_MAX, -1, -1): the identities of min and max, written by a launch of its own
__global__ __launch_bounds__(256) void eval_boxes_init_kernel(int32_t* __restrict__ boxes, int U) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 4 * U) boxes[i] = (i & 3) < 2 ? 0x7fffffff : -1;
}

// (c) per rank xmin, ymin, xmax, ymax: LDS min / max per workgroup (an LDS atomic only where it moves the bound: the bounds
// are monotone, a stale read costs one needless atomic), then one global atomic per bound of the ranks the workgroup met.
__global__ __launch_bounds__(256) void eval_boxes_kernel(const uint16_t* __restrict__ rank, int U, int W, int64_t npix,
                                                         int aligned, int32_t* __restrict__ boxes) {
  __shared__ int box[EVAL_MAX_U * 4];
  for (int i = threadIdx.x; i < 4 * U; i += 256) box[i] = (i & 3) < 2 ? 0x7fffffff : -1;
  __syncthreads();
  const int64_t chunks = (npix + EVAL_CHUNK - 1) / EVAL_CHUNK;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int64_t p = (c * 256 + threadIdx.x) * 4;
    const int count = eval_count(npix, p);
    if (count == 0) continue;
    int r[4];
    eval_ranks4(rank, p, count, aligned & EVAL_AL_RANK, r);
    int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < count && r[j] < U) {
        volatile int* b = &box[4 * r[j]];
        if (x < b[0]) atomicMin(&box[4 * r[j]], x);
        if (y < b[1]) atomicMin(&box[4 * r[j] + 1], y);
        if (x > b[2]) atomicMax(&box[4 * r[j] + 2], x);
        if (y > b[3]) atomicMax(&box[4 * r[j] + 3], y);
      }
      if (++x == W) { x = 0; ++y; }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 4 * U; i += 256) {
    const int v = box[i];
    if ((i & 3) < 2) {
      if (v != 0x7fffffff) atomicMin(&boxes[i], v);
    } else if (v >= 0) {
      atomicMax(&boxes[i], v);
    }
  }
}

// (d) out[p] = colors[rank[p]] (white for a rank outside the table)
__global__ __launch_bounds__(256) void eval_paint_kernel(const uint16_t* __restrict__ rank, const uint8_t* __restrict__ colors,
                                                         int U, int64_t npix, int aligned, uint8_t* __restrict__ out) {
  const int64_t p = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  const int count = eval_count(npix, p);
  if (count == 0) return;
  int r[4];
  eval_ranks4(rank, p, count, aligned & EVAL_AL_RANK, r);
  uint8_t px[12];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    px[3 * j] = px[3 * j + 1] = px[3 * j + 2] = 255;
    if (j < count && r[j] < U) {
      const uint8_t* t = colors + 3 * r[j];
      px[3 * j] = t[0]; px[3 * j + 1] = t[1]; px[3 * j + 2] = t[2];
    }
  }
  uint8_t* o = out + 3 * p;
  if ((aligned & EVAL_AL_OUT) && count == 4) {
    uint32_t* ow = (uint32_t*)o;
#pragma unroll
    for (int d = 0; d < 3; ++d)
      ow[d] = (uint32_t)px[4 * d] | ((uint32_t)px[4 * d + 1] << 8) | ((uint32_t)px[4 * d + 2] << 16) |
              ((uint32_t)px[4 * d + 3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 12; ++j)
      if (j < 3 * count) o[j] = px[j];
  }
}

static inline bool eval_dims_ok(int H, int W) { return H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31); }
static inline bool eval_rank_ok(const void* rank, int U) { return rank && ink_aligned<2>(rank) && U >= 1 && U <= EVAL_MAX_U; }
// workgroups of a grid-stride pass: two steps of 1024 pixels each where the image has them, at most 1024 workgroups
static inline unsigned eval_strips(int64_t npix) {
  const int64_t chunks = (npix + EVAL_CHUNK - 1) / EVAL_CHUNK;
  const int64_t g = (chunks + 1) / 2;
  return (unsigned)(g < 1 ? 1 : (g > 1024 ? 1024 : g));
}

}  // namespace

extern "C" int ink_eval_label_ranks(const void* labels, int32_t elem_size, int32_t H, int32_t W, uint32_t* workspace,
                                    int32_t* values, int32_t values_cap, int32_t* info, uint16_t* rank, void* stream) {
  INK_CHECK_ARG(labels && workspace && values && info && rank && eval_dims_ok(H, W));
  INK_CHECK_ARG((elem_size == 1 || elem_size == 2 || elem_size == 4) && values_cap >= 1 && ink_aligned<2>(rank));
  hipStream_t s = (hipStream_t)stream;
  const int64_t npix = (int64_t)H * W;
  uint32_t* bitmap = workspace;
  uint32_t* prefix = workspace + EVAL_BITMAP_WORDS;
  if (hipMemsetAsync(bitmap, 0, EVAL_BITMAP_WORDS * sizeof(uint32_t), s) != hipSuccess) return INK_ERR_LAUNCH;
  if (hipMemsetAsync(info, 0, 2 * sizeof(int32_t), s) != hipSuccess) return INK_ERR_LAUNCH;
  const bool labels4 =      // four labels per load
      elem_size == 1 ? ink_aligned<4>(labels) : elem_size == 2 ? ink_aligned<8>(labels) : ink_aligned<16>(labels);
  const int aligned = (labels4 ? EVAL_AL_LABELS : 0) | (ink_aligned<8>(rank) ? EVAL_AL_RANK : 0);
  hipLaunchKernelGGL(eval_presence_kernel, dim3(eval_strips(npix)), dim3(256), 0, s, labels, elem_size, npix, aligned,
                     bitmap, info);
  hipLaunchKernelGGL(eval_prefix_kernel, dim3(1), dim3(256), 0, s, (const uint32_t*)bitmap, prefix, values, values_cap, info);
  hipLaunchKernelGGL(eval_rank_kernel, dim3((unsigned)((npix + EVAL_CHUNK - 1) / EVAL_CHUNK)), dim3(256), 0, s, labels,
                     elem_size, npix, aligned, (const uint32_t*)bitmap, (const uint32_t*)prefix, rank);
  return ink_launch_status();
}

extern "C" int ink_eval_contingency(const void* pred_u8, int32_t n, int32_t by_label, const void* rank_u16, int32_t U,
                                    const void* sketch_u8, int32_t channels, int32_t stroke_only, int32_t H, int32_t W,
                                    int32_t* table, void* stream) {
  INK_CHECK_ARG(table && eval_rank_ok(rank_u16, U) && eval_dims_ok(H, W) && n >= 0 && n <= (1 << 20));
  INK_CHECK_ARG(by_label ? (pred_u8 && n <= 255) : (pred_u8 || n == 0));
  INK_CHECK_ARG(!stroke_only || (sketch_u8 && (channels == 1 || channels == 3)));
  hipStream_t s = (hipStream_t)stream;
  const int64_t npix = (int64_t)H * W;
  if (hipMemsetAsync(table, 0, (size_t)(n + 1) * U * sizeof(int32_t), s) != hipSuccess) return INK_ERR_LAUNCH;
  int aligned = (ink_aligned<8>(rank_u16) ? EVAL_AL_RANK : 0) | (ink_aligned<4>(sketch_u8) ? EVAL_AL_SKETCH : 0);
  if (ink_aligned<4>(pred_u8) && (by_label || (npix & 3) == 0)) aligned |= EVAL_AL_PRED;
  const unsigned tiles = (unsigned)((n + 1 + EVAL_TILE - 1) / EVAL_TILE);
  hipLaunchKernelGGL(eval_contingency_kernel, dim3(eval_strips(npix), tiles), dim3(256), 0, s, (const uint8_t*)pred_u8, n,
                     by_label ? 1 : 0, (const uint16_t*)rank_u16, U, stroke_only ? (const uint8_t*)sketch_u8 : nullptr,
                     channels, npix, aligned, table);
  return ink_launch_status();
}

extern "C" int ink_eval_label_boxes(const void* rank_u16, int32_t U, int32_t H, int32_t W, int32_t* boxes, void* stream) {
  INK_CHECK_ARG(boxes && eval_rank_ok(rank_u16, U) && eval_dims_ok(H, W));
  hipStream_t s = (hipStream_t)stream;
  const int64_t npix = (int64_t)H * W;
  hipLaunchKernelGGL(eval_boxes_init_kernel, dim3((unsigned)((4 * U + 255) / 256)), dim3(256), 0, s, boxes, U);
  hipLaunchKernelGGL(eval_boxes_kernel, dim3(eval_strips(npix)), dim3(256), 0, s, (const uint16_t*)rank_u16, U, W, npix,
                     ink_aligned<8>(rank_u16) ? EVAL_AL_RANK : 0, boxes);
  return ink_launch_status();
}

extern "C" int ink_eval_paint_labels(const void* rank_u16, const void* colors_u8, int32_t U, int32_t H, int32_t W,
                                     void* out_rgb_u8, void* stream) {
  INK_CHECK_ARG(colors_u8 && out_rgb_u8 && eval_rank_ok(rank_u16, U) && eval_dims_ok(H, W));
  const int64_t npix = (int64_t)H * W;
  const int aligned = (ink_aligned<8>(rank_u16) ? EVAL_AL_RANK : 0) | (ink_aligned<4>(out_rgb_u8) ? EVAL_AL_OUT : 0);
  hipLaunchKernelGGL(eval_paint_kernel, dim3((unsigned)((npix + EVAL_CHUNK - 1) / EVAL_CHUNK)), dim3(256), 0,
                     (hipStream_t)stream, (const uint16_t*)rank_u16, (const uint8_t*)colors_u8, U, npix, aligned,
                     (uint8_t*)out_rgb_u8);
  return ink_launch_status();
}
