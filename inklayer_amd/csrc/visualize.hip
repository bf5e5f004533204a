// Visualisation stage: the reference's coloured sketch (segmented_sketch.png, segmented_sketch_final.png) as
// two streaming kernels over the flat pixel array.
//   reference: InkLayer/utils/visualization.py:63-167 (color_sketch_by_masks), :169-180 (get_background_idxs)
// The reference paints every mask with a Python loop over H x W.  Its output pixel is a function of the pixel's grey
// value, of the LAST mask holding the pixel and of one image-wide flag (max_stroke_opacity > 0.1, i.e. some stroke pixel
// has grey <= 229), so the host evaluates both branches once per (mask, grey) pair with the reference's own float steps
// (inklayer_amd/visualize.py::colour_tables) and the device only selects: integer work, bit-exact.
// A lane owns four consecutive pixels: 12 bytes of sketch and of output, 4 bytes of every mask plane or of the label
// image, moved as dwords where the base address (and for plane k its offset k H W) is 4-byte aligned, as bytes otherwise
// and for the last H W % 4 pixels.
#include "common.h"
#include "../../include/inklayer_hip.h"

namespace {

#define VIS_MIN_INIT 0x7f7f7f7f      // what hipMemsetAsync(0x7f) leaves: "no stroke pixel seen"
#define VIS_STROKE 250               // visualization.py:92
#define VIS_FAINT 229                // (255 - 229) / 255 > 0.1 >= (255 - 230) / 255  (visualization.py:109)
enum { VIS_AL_SKETCH = 1, VIS_AL_MASKS = 2, VIS_AL_OUT = 4 };

// grey (cv_gray14: the cv2.cvtColor(COLOR_RGB2GRAY) of visualization.py:83) of the pixels p .. p + 3 (255 for the ones
// past `count`)
__device__ __forceinline__ void vis_gray4(const uint8_t* __restrict__ sk, int channels, int64_t p, int count, bool wide,
                                          int g[4]) {
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
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    g[j] = 255;
    if (j < count) {
      const uint8_t* q = sk + (p + j) * channels;
      g[j] = channels == 3 ? cv_gray14(q[0], q[1], q[2]) : (int)q[0];
    }
  }
}

// four bytes at q as one little-endian word (zeros past `count`)
__device__ __forceinline__ uint32_t vis_bytes4(const uint8_t* __restrict__ q, int count, bool wide) {
  if (wide && count == 4) return *(const uint32_t*)q;
  uint32_t w = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < count) w |= (uint32_t)q[j] << (8 * j);
  return w;
}

// smallest grey over the stroke pixels (grey < 250) of the image -> *minv (left at VIS_MIN_INIT when there is none).
// A workgroup covers 4 x 1024 pixels; wave reduction, then LDS across the four waves, then at most one atomicMin per
// workgroup: only where it lowers the word.
__global__ __launch_bounds__(256) void vis_gray_min_kernel(const uint8_t* __restrict__ sk, int channels, int64_t npix,
                                                           int aligned, int* __restrict__ minv) {
  __shared__ int part[4];
  int m = VIS_MIN_INIT;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int64_t p = (((int64_t)blockIdx.x * 4 + c) * 256 + threadIdx.x) * 4;
    if (p < npix) {
      const int64_t left = npix - p;
      int g[4];
      vis_gray4(sk, channels, p, left < 4 ? (int)left : 4, aligned & VIS_AL_SKETCH, g);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (g[j] < VIS_STROKE) m = min(m, g[j]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = min(min(part[0], part[1]), min(part[2], part[3]));
    // the word only ever falls: a workgroup whose minimum is not below what it reads there has nothing to add (a stale
    // read is a larger value and costs one needless atomic, never a missed one)
    if (m < __atomic_load_n(minv, __ATOMIC_RELAXED)) atomicMin(minv, m);
  }
}

// out = white off the strokes, tables[variant][row][grey] on them: row = the last mask holding the pixel (stack form:
// planes walked from the last one backwards, four at a time, until every stroke pixel of the lane is settled, never
// read for a lane without strokes; label form: label - 1), n for a stroke in no mask; variant 0 iff *minv <= 229.
__global__ __launch_bounds__(256) void vis_colour_kernel(const uint8_t* __restrict__ sk, int channels,
                                                         const uint8_t* __restrict__ masks, int n, int by_label,
                                                         const uint8_t* __restrict__ tables, const int* __restrict__ minv,
                                                         int64_t npix, int aligned, uint8_t* __restrict__ out) {
  const int64_t p = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p >= npix) return;
  const int64_t left = npix - p;
  const int count = left < 4 ? (int)left : 4;
  int g[4], row[4];
  vis_gray4(sk, channels, p, count, aligned & VIS_AL_SKETCH, g);
  unsigned need = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    row[j] = n;
    if (g[j] < VIS_STROKE) need |= 1u << j;                  // pixels past `count` have grey 255
  }
  if (need) {
    const bool wide = aligned & VIS_AL_MASKS;
    if (by_label) {
      const uint32_t w = vis_bytes4(masks + p, count, wide);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int l = (w >> (8 * j)) & 255u;
        if (l >= 1 && l <= n) row[j] = l - 1;
      }
    } else {
      // four planes per step: their loads are in flight together (one dependent round trip per four planes instead
      // of one per plane), then they are tested in order, the last plane first
      for (int k = n - 1; k >= 0 && need; k -= 4) {
        uint32_t w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          w[u] = k - u >= 0 ? vis_bytes4(masks + (int64_t)(k - u) * npix + p, count, wide) : 0u;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (((need >> j) & 1u) && ((w[u] >> (8 * j)) & 255u)) {
              row[j] = k - u;
              need &= ~(1u << j);
            }
        }
      }
    }
  }
  const uint8_t* tab = tables + (*minv <= VIS_FAINT ? 0 : (int64_t)(n + 1) * 768);
  uint8_t px[12];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    px[3 * j] = px[3 * j + 1] = px[3 * j + 2] = 255;
    if (g[j] < VIS_STROKE) {
      const uint8_t* t = tab + ((int64_t)row[j] * 256 + g[j]) * 3;
      px[3 * j] = t[0]; px[3 * j + 1] = t[1]; px[3 * j + 2] = t[2];
    }
  }
  uint8_t* o = out + 3 * p;
  if ((aligned & VIS_AL_OUT) && count == 4) {
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

static inline bool vis_dims_ok(int channels, int H, int W) {
  return (channels == 1 || channels == 3) && H > 0 && W > 0 && (int64_t)H * W <= ((int64_t)1 << 40);
}

}  // namespace

extern "C" int ink_vis_gray_min(const void* sketch_u8, int32_t channels, int32_t H, int32_t W, int32_t* gray_min,
                                void* stream) {
  INK_CHECK_ARG(sketch_u8 && gray_min && vis_dims_ok(channels, H, W));
  hipStream_t s = (hipStream_t)stream;
  const int64_t npix = (int64_t)H * W;
  if (hipMemsetAsync(gray_min, 0x7f, sizeof(int32_t), s) != hipSuccess) return INK_ERR_LAUNCH;
  hipLaunchKernelGGL(vis_gray_min_kernel, dim3((unsigned)((npix + 4095) / 4096)), dim3(256), 0, s,
                     (const uint8_t*)sketch_u8, channels, npix, ink_aligned<4>(sketch_u8) ? VIS_AL_SKETCH : 0, gray_min);
  return ink_launch_status();
}

extern "C" int ink_vis_colour(const void* sketch_u8, int32_t channels, const void* masks_or_label_u8, int32_t n,
                              int32_t by_label, const void* tables_u8, const int32_t* gray_min, int32_t H, int32_t W,
                              void* out_rgb_u8, void* stream) {
  INK_CHECK_ARG(sketch_u8 && tables_u8 && gray_min && out_rgb_u8 && vis_dims_ok(channels, H, W) && n >= 0);
  INK_CHECK_ARG(by_label ? (masks_or_label_u8 && n <= 255) : (masks_or_label_u8 || n == 0));
  const int64_t npix = (int64_t)H * W;
  int aligned = (ink_aligned<4>(sketch_u8) ? VIS_AL_SKETCH : 0) | (ink_aligned<4>(out_rgb_u8) ? VIS_AL_OUT : 0);
  if (ink_aligned<4>(masks_or_label_u8) && (by_label || (npix & 3) == 0)) aligned |= VIS_AL_MASKS;
  hipLaunchKernelGGL(vis_colour_kernel, dim3((unsigned)((npix + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)sketch_u8, channels, (const uint8_t*)masks_or_label_u8, n, by_label ? 1 : 0,
                     (const uint8_t*)tables_u8, gray_min, npix, aligned, (uint8_t*)out_rgb_u8);
  return ink_launch_status();
}
