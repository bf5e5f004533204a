// Pre- and post-processing of the inpainting stage around the diffusion pipe: what
// ControlNet_inpaint, inpaint_single_layer and SDXL_inpaint do to the image and the mask before and after the model call.
// Images stay on the device: uint8 [H, W, 3] (R, G, B) and uint8 [H, W].
//   reference: InkLayer/inpainting/inpaint_ControlNet.py:49-65   (contrast, bilateral)
//              InkLayer/inpainting/inpaint_ControlNet.py:67-75   (mask dilation and blur)
//              InkLayer/inpainting/inpaint_ControlNet.py:77-90   (condition tensor)
//              InkLayer/inpainting/inpaint_ControlNet.py:92-124  (adaptive-threshold clean-up, soft-mask blend)
//              InkLayer/inpainting/inpaint_ControlNet.py:150-151, 161, 176, 181-182 (Lanczos resizes, grey round trip,
//              unsharp mask); inpaint_single_layer.py:43-44, 63, 68-78; inpaint_SDXL.py:23-24, 31-32
// Third-party algorithms restated: Pillow 12.2 (ImageEnhance.Contrast / Image.blend, BoxBlur.c,
// UnsharpMask.c, the "L" conversion) and OpenCV (bilateralFilter, dilate, GaussianBlur, adaptiveThreshold, cvtColor).
// Every kernel does only + - x /, compares and conversions in a fixed order; every table of exponentials comes from the
// host, rounded once to its type (inklayer_amd/inpaint.py).  The library is built with -ffp-contract=off, so a product
// and the sum it feeds are rounded separately: the results equal tests/inpaint_ref.py bit for bit.
#include "common.h"
#include "../../include/inklayer_hip.h"

namespace {

typedef unsigned long long inp_u64;

__device__ __forceinline__ int inp_r101(int i, int n) {      // cv2.BORDER_REFLECT_101; |i - [0, n)| < n - 1
  i = i < 0 ? -i : i;
  return i >= n ? 2 * n - 2 - i : i;
}
__device__ __forceinline__ int inp_rep(int i, int n) { return min(max(i, 0), n - 1); }   // replicate

// ------------------------------------------------------------------------------------------------------------------
// (a) ImageEnhance.Contrast(img).enhance(f): the mean of the L image as an integer sum (order-free, so deterministic),
// then Image.blend of the constant mean image and the input with a factor outside [0, 1]
__global__ __launch_bounds__(256) void inp_luma_sum_kernel(const uint8_t* __restrict__ rgb, int64_t npix,
                                                           inp_u64* __restrict__ sum) {
  __shared__ unsigned part[256];
  unsigned s = 0;                                             // < 2^32: a thread sees at most 2^28 / (256 blocks) pixels
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256)
    s += pil_luma(rgb[i * 3], rgb[i * 3 + 1], rgb[i * 3 + 2]);
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    inp_u64 t = 0;
    for (int k = 0; k < 256; ++k) t += part[k];
    atomicAdd(sum, t);
  }
}

__global__ __launch_bounds__(256) void inp_contrast_kernel(const uint8_t* __restrict__ rgb, int64_t npix, float factor,
                                                           const inp_u64* __restrict__ sum, uint8_t* __restrict__ out) {
  __shared__ int mean_s;
  if (threadIdx.x == 0) mean_s = (int)((2ull * sum[0] + (inp_u64)npix) / (2ull * (inp_u64)npix));
  __syncthreads();
  const int mean = mean_s;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix * 3) return;
  const float d = (float)((int)rgb[i] - mean);
  const float p = factor * d;
  const float t = (float)mean + p;
  out[i] = t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (uint8_t)(int)t);
}

// ------------------------------------------------------------------------------------------------------------------
// (b) cv2.bilateralFilter(rgb, 5, sigma, sigma) on 3-channel u8: the 13 taps of the radius-2 disc in row-major order,
// tab = 13 space weights | 768 colour weights (f32, from the host)
__global__ __launch_bounds__(256) void inp_bilateral_kernel(const uint8_t* __restrict__ rgb, int H, int W,
                                                            const float* __restrict__ tab, uint8_t* __restrict__ out) {
  __shared__ float t[13 + 768];
  for (int k = threadIdx.x; k < 13 + 768; k += 256) t[k] = tab[k];
  __syncthreads();
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
  const uint8_t* c = rgb + p * 3;
  const int c0 = c[0], c1 = c[1], c2 = c[2];
  float wsum = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
  int k = 0;
  for (int i = -2; i <= 2; ++i) {
    const int yy = inp_r101(y + i, H);
    for (int j = -2; j <= 2; ++j) {
      if (i * i + j * j > 4) continue;
      const uint8_t* q = rgb + ((int64_t)yy * W + inp_r101(x + j, W)) * 3;
      const int q0 = q[0], q1 = q[1], q2 = q[2];
      const float w = t[k] * t[13 + abs(q0 - c0) + abs(q1 - c1) + abs(q2 - c2)];
      ++k;
      wsum += w;
      const float a0 = (float)q0 * w, a1 = (float)q1 * w, a2 = (float)q2 * w;
      s0 += a0;
      s1 += a1;
      s2 += a2;
    }
  }
  const float inv = 1.0f / wsum;
  uint8_t* o = out + p * 3;
  o[0] = (uint8_t)(int)rintf(s0 * inv);
  o[1] = (uint8_t)(int)rintf(s1 * inv);
  o[2] = (uint8_t)(int)rintf(s2 * inv);
}

// ------------------------------------------------------------------------------------------------------------------
// (c) preprocess_mask: cv2.dilate with a 3x3 block of ones (pixels outside the image do not take part), then
// cv2.GaussianBlur((3, 3), 0) on u8 = the integer kernel [1 2 1]^T [1 2 1] / 16, rounded, reflect-101
__global__ __launch_bounds__(256) void inp_dilate3_kernel(const uint8_t* __restrict__ in, int H, int W,
                                                          uint8_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
  int m = 0;
  for (int i = -1; i <= 1; ++i)
    for (int j = -1; j <= 1; ++j) {
      const int yy = y + i, xx = x + j;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) m = max(m, (int)in[(int64_t)yy * W + xx]);
    }
  out[p] = (uint8_t)m;
}

__global__ __launch_bounds__(256) void inp_blur3_kernel(const uint8_t* __restrict__ in, int H, int W,
                                                        uint8_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
  int s = 8;
  for (int i = -1; i <= 1; ++i) {
    const uint8_t* row = in + (int64_t)inp_r101(y + i, H) * W;
    const int r = row[inp_r101(x - 1, W)] + 2 * row[x] + row[inp_r101(x + 1, W)];
    s += i == 0 ? 2 * r : r;
  }
  out[p] = (uint8_t)(s >> 4);
}

// ------------------------------------------------------------------------------------------------------------------
// (d) the bicubic / Lanczos resizes of images and masks: Pillow's resampler, ink_resize_u8 (image_ops.hip)

// ------------------------------------------------------------------------------------------------------------------
// (e) make_inpaint_condition: planar f32 [3, H, W] = v / 255, -1 where the mask / 255 > 0.5 (mask >= 128)
__global__ __launch_bounds__(256) void inp_condition_kernel(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ mask,
                                                            int64_t npix, float* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= npix) return;
  const bool m = mask[p] >= 128;
  for (int c = 0; c < 3; ++c) out[c * npix + p] = m ? -1.0f : (float)rgb[p * 3 + c] / 255.0f;
}

// ------------------------------------------------------------------------------------------------------------------
// (f) cv2.adaptiveThreshold(grey, 255, GAUSSIAN_C, BINARY, 11, 2): the 11-tap Gaussian (sigma 2, f32 taps k from the
// host) of the grey image in f32 with a replicated border - rows left to right, columns from the centre outwards - the
// blurred value rounded half-even to u8, thresh = grey > mean - 2; clean = 255 where thresh, else the pixel
__global__ __launch_bounds__(256) void inp_gauss11_rows_kernel(const uint8_t* __restrict__ rgb, int H, int W,
                                                               const float* __restrict__ k, float* __restrict__ rows) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
  const uint8_t* row = rgb + (int64_t)y * W * 3;
  auto grey = [&](int xx) {
    const uint8_t* q = row + inp_rep(xx, W) * 3;
    return (float)cv_gray15(q[0], q[1], q[2]);
  };
  float s = k[0] * grey(x - 5);
  for (int t = 1; t < 11; ++t) {
    const float a = k[t] * grey(x + t - 5);
    s += a;
  }
  rows[p] = s;
}

__global__ __launch_bounds__(256) void inp_cleanup_kernel(const uint8_t* __restrict__ rgb, const float* __restrict__ rows,
                                                          int H, int W, const float* __restrict__ k,
                                                          uint8_t* __restrict__ thresh, uint8_t* __restrict__ clean) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
  float s = k[5] * rows[p];
  for (int t = 1; t <= 5; ++t) {
    const float pair = rows[(int64_t)inp_rep(y + t, H) * W + x] + rows[(int64_t)inp_rep(y - t, H) * W + x];
    const float a = k[5 + t] * pair;
    s += a;
  }
  const int mean = min(max((int)rintf(s), 0), 255);
  const bool on = cv_gray15(rgb[p * 3], rgb[p * 3 + 1], rgb[p * 3 + 2]) > mean - 2;
  thresh[p] = on ? 255 : 0;
  for (int c = 0; c < 3; ++c) clean[p * 3 + c] = on ? 255 : rgb[p * 3 + c];
}

// ------------------------------------------------------------------------------------------------------------------
// (g) soft = clip(cv2.GaussianBlur(mask / 255.0, (3, 3), 1), 0, 1) in f64 (k2 = centre, side weight from the host),
// reflect-101; out = trunc(clean * soft + original * (1 - soft))
__global__ __launch_bounds__(256) void inp_soft_rows_kernel(const uint8_t* __restrict__ mask, int H, int W,
                                                            const double* __restrict__ k2, double* __restrict__ rows) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
  const uint8_t* row = mask + (int64_t)y * W;
  const double c = (double)row[x] / 255.0;
  const double l = (double)row[inp_r101(x - 1, W)] / 255.0, r = (double)row[inp_r101(x + 1, W)] / 255.0;
  const double a = c * k2[0], b = (l + r) * k2[1];
  rows[p] = a + b;
}

__global__ __launch_bounds__(256) void inp_soft_blend_kernel(const uint8_t* __restrict__ clean, const uint8_t* __restrict__ orig,
                                                             const double* __restrict__ rows, int H, int W,
                                                             const double* __restrict__ k2, uint8_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
  const double up = rows[(int64_t)inp_r101(y - 1, H) * W + x], dn = rows[(int64_t)inp_r101(y + 1, H) * W + x];
  const double a = rows[p] * k2[0], b = (up + dn) * k2[1];
  double soft = a + b;
  soft = soft < 0.0 ? 0.0 : (soft > 1.0 ? 1.0 : soft);
  const double rest = 1.0 - soft;
  for (int c = 0; c < 3; ++c) {
    const double u = (double)clean[p * 3 + c] * soft, v = (double)orig[p * 3 + c] * rest;
    out[p * 3 + c] = (uint8_t)(int)(u + v);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// (h) convert("L") (.convert("RGB")): Pillow's luma, written to 1 or 3 channels
__global__ __launch_bounds__(256) void inp_luma_kernel(const uint8_t* __restrict__ rgb, int64_t npix, int oc,
                                                       uint8_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= npix) return;
  const uint8_t l = (uint8_t)pil_luma(rgb[p * 3], rgb[p * 3 + 1], rgb[p * 3 + 2]);
  for (int c = 0; c < oc; ++c) out[p * oc + c] = l;
}

// One pass of Pillow's box blur with a box radius below 1 (BoxBlur.c ImagingLineBoxBlur8, radius 0):
// (ww * p + fw * (p[-1] + p[+1]) + 2^23) >> 24 in uint32, replicated border, stored as u8.  C interleaved channels.
__global__ __launch_bounds__(256) void inp_box_pass_kernel(const uint8_t* __restrict__ in, int H, int W, int C, int axis,
                                                           uint32_t ww, uint32_t fw, uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)H * W * C) return;
  const int c = (int)(i % C);
  const int64_t pix = i / C;
  const int y = (int)(pix / W), x = (int)(pix - (int64_t)y * W);
  uint32_t a, b;
  if (axis == 0) {
    a = in[((int64_t)y * W + inp_rep(x - 1, W)) * C + c];
    b = in[((int64_t)y * W + inp_rep(x + 1, W)) * C + c];
  } else {
    a = in[((int64_t)inp_rep(y - 1, H) * W + x) * C + c];
    b = in[((int64_t)inp_rep(y + 1, H) * W + x) * C + c];
  }
  out[i] = (uint8_t)((ww * (uint32_t)in[i] + fw * (a + b) + (1u << 23)) >> 24);
}

// UnsharpMask.c: d = in - blur; |d| > threshold: clip8(in + d * percent / 100) (C division), else in
__global__ __launch_bounds__(256) void inp_unsharp_kernel(const uint8_t* __restrict__ in, const uint8_t* __restrict__ blur,
                                                          int64_t n, int percent, int threshold, uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int v = in[i], d = v - (int)blur[i];
  out[i] = abs(d) > threshold ? (uint8_t)min(max(v + d * percent / 100, 0), 255) : (uint8_t)v;
}

// inpaint_single_layer.py:74-78: the result inside mask > 128 with alpha 255, zeros elsewhere
__global__ __launch_bounds__(256) void inp_rgba_cut_kernel(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ mask,
                                                           int64_t npix, uint8_t* __restrict__ rgba) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= npix) return;
  const bool in = mask[p] > 128;
  for (int c = 0; c < 3; ++c) rgba[p * 4 + c] = in ? rgb[p * 3 + c] : 0;
  rgba[p * 4 + 3] = in ? 255 : 0;
}

// an image side of 1 or 2 has no reflect-101 neighbour at distance 2; 16384 x 16384 x 4 bytes stays below 2^31 samples
static inline bool inp_dims_ok(int H, int W) { return H >= 3 && W >= 3 && H <= 16384 && W <= 16384; }
static inline unsigned inp_blocks(int64_t items) { return (unsigned)((items + 255) / 256); }

}  // namespace

extern "C" int ink_inp_contrast(const void* rgb_u8, int32_t H, int32_t W, float factor, void* sum_u64, void* out_rgb_u8,
                                void* stream) {
  INK_CHECK_ARG(rgb_u8 && sum_u64 && out_rgb_u8 && inp_dims_ok(H, W) && factor == factor);
  hipStream_t s = (hipStream_t)stream;
  const int64_t npix = (int64_t)H * W;
  if (hipMemsetAsync(sum_u64, 0, sizeof(inp_u64), s) != hipSuccess) return INK_ERR_LAUNCH;
  const unsigned rb = inp_blocks(npix) < 256u ? inp_blocks(npix) : 256u;
  hipLaunchKernelGGL(inp_luma_sum_kernel, dim3(rb), dim3(256), 0, s, (const uint8_t*)rgb_u8, npix, (inp_u64*)sum_u64);
  hipLaunchKernelGGL(inp_contrast_kernel, dim3(inp_blocks(npix * 3)), dim3(256), 0, s, (const uint8_t*)rgb_u8, npix, factor,
                     (const inp_u64*)sum_u64, (uint8_t*)out_rgb_u8);
  return ink_launch_status();
}

extern "C" int ink_inp_bilateral(const void* rgb_u8, int32_t H, int32_t W, const float* tables, void* out_rgb_u8,
                                 void* stream) {
  INK_CHECK_ARG(rgb_u8 && tables && out_rgb_u8 && rgb_u8 != out_rgb_u8 && inp_dims_ok(H, W));
  hipLaunchKernelGGL(inp_bilateral_kernel, dim3(inp_blocks((int64_t)H * W)), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)rgb_u8, H, W, tables, (uint8_t*)out_rgb_u8);
  return ink_launch_status();
}

extern "C" int ink_inp_mask_prepare(const void* mask_u8, int32_t H, int32_t W, int32_t dilate_iterations, int32_t blur,
                                    void* tmp2_u8, void* out_u8, void* stream) {
  INK_CHECK_ARG(mask_u8 && tmp2_u8 && out_u8 && inp_dims_ok(H, W));
  INK_CHECK_ARG(dilate_iterations >= 0 && dilate_iterations <= 64 && (blur == 0 || blur == 1));
  INK_CHECK_ARG(dilate_iterations + blur >= 1 && mask_u8 != out_u8 && mask_u8 != tmp2_u8 && tmp2_u8 != out_u8);
  hipStream_t s = (hipStream_t)stream;
  const int64_t npix = (int64_t)H * W;
  const dim3 grid(inp_blocks(npix));
  uint8_t* ta = (uint8_t*)tmp2_u8;
  uint8_t* tb = ta + npix;
  const uint8_t* cur = (const uint8_t*)mask_u8;
  for (int it = 0; it < dilate_iterations; ++it) {           // the last step of all lands in out_u8
    uint8_t* dst = (it == dilate_iterations - 1 && !blur) ? (uint8_t*)out_u8 : (cur == ta ? tb : ta);
    hipLaunchKernelGGL(inp_dilate3_kernel, grid, dim3(256), 0, s, cur, H, W, dst);
    cur = dst;
  }
  if (blur) hipLaunchKernelGGL(inp_blur3_kernel, grid, dim3(256), 0, s, cur, H, W, (uint8_t*)out_u8);
  return ink_launch_status();
}

extern "C" int ink_inp_condition(const void* rgb_u8, const void* mask_u8, int32_t H, int32_t W, float* out_f32,
                                 void* stream) {
  INK_CHECK_ARG(rgb_u8 && mask_u8 && out_f32 && H > 0 && W > 0 && H <= 16384 && W <= 16384);
  hipLaunchKernelGGL(inp_condition_kernel, dim3(inp_blocks((int64_t)H * W)), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)rgb_u8, (const uint8_t*)mask_u8, (int64_t)H * W, out_f32);
  return ink_launch_status();
}

extern "C" int ink_inp_cleanup(const void* result_rgb_u8, int32_t H, int32_t W, const float* taps11, float* tmp_f32,
                               void* thresh_u8, void* clean_rgb_u8, void* stream) {
  INK_CHECK_ARG(result_rgb_u8 && taps11 && tmp_f32 && thresh_u8 && clean_rgb_u8 && inp_dims_ok(H, W));
  INK_CHECK_ARG(result_rgb_u8 != clean_rgb_u8);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(inp_blocks((int64_t)H * W));
  hipLaunchKernelGGL(inp_gauss11_rows_kernel, grid, dim3(256), 0, s, (const uint8_t*)result_rgb_u8, H, W, taps11, tmp_f32);
  hipLaunchKernelGGL(inp_cleanup_kernel, grid, dim3(256), 0, s, (const uint8_t*)result_rgb_u8, (const float*)tmp_f32, H, W,
                     taps11, (uint8_t*)thresh_u8, (uint8_t*)clean_rgb_u8);
  return ink_launch_status();
}

extern "C" int ink_inp_soft_blend(const void* clean_rgb_u8, const void* original_rgb_u8, const void* mask_u8, int32_t H,
                                  int32_t W, const double* taps2, double* tmp_f64, void* out_rgb_u8, void* stream) {
  INK_CHECK_ARG(clean_rgb_u8 && original_rgb_u8 && mask_u8 && taps2 && tmp_f64 && out_rgb_u8 && inp_dims_ok(H, W));
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(inp_blocks((int64_t)H * W));
  hipLaunchKernelGGL(inp_soft_rows_kernel, grid, dim3(256), 0, s, (const uint8_t*)mask_u8, H, W, taps2, tmp_f64);
  hipLaunchKernelGGL(inp_soft_blend_kernel, grid, dim3(256), 0, s, (const uint8_t*)clean_rgb_u8,
                     (const uint8_t*)original_rgb_u8, (const double*)tmp_f64, H, W, taps2, (uint8_t*)out_rgb_u8);
  return ink_launch_status();
}

extern "C" int ink_inp_luma(const void* rgb_u8, int32_t H, int32_t W, int32_t out_channels, void* out_u8, void* stream) {
  INK_CHECK_ARG(rgb_u8 && out_u8 && H > 0 && W > 0 && H <= 16384 && W <= 16384 && (out_channels == 1 || out_channels == 3));
  hipLaunchKernelGGL(inp_luma_kernel, dim3(inp_blocks((int64_t)H * W)), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)rgb_u8, (int64_t)H * W, out_channels, (uint8_t*)out_u8);
  return ink_launch_status();
}

extern "C" int ink_inp_unsharp(const void* img_u8, int32_t H, int32_t W, int32_t channels, uint32_t ww, uint32_t fw,
                               int32_t percent, int32_t threshold, void* tmp2_u8, void* out_u8, void* stream) {
  INK_CHECK_ARG(img_u8 && tmp2_u8 && out_u8 && H > 0 && W > 0 && H <= 16384 && W <= 16384);
  INK_CHECK_ARG((channels == 1 || channels == 3) && img_u8 != tmp2_u8 && out_u8 != tmp2_u8);
  // the weights of a box of radius below 1: ww + 2 fw = 2^24 (or one less), so a pass stays inside uint32
  INK_CHECK_ARG(ww <= (1u << 24) && fw == ((1u << 24) - ww) / 2 && percent >= 0 && percent <= 10000 && threshold >= 0);
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)H * W * channels;
  const dim3 grid(inp_blocks(n));
  uint8_t* ta = (uint8_t*)tmp2_u8;
  uint8_t* tb = ta + n;
  const uint8_t* cur = (const uint8_t*)img_u8;
  for (int pass = 0; pass < 6; ++pass) {                     // three passes along x, then three along y
    uint8_t* dst = cur == ta ? tb : ta;
    hipLaunchKernelGGL(inp_box_pass_kernel, grid, dim3(256), 0, s, cur, H, W, channels, pass < 3 ? 0 : 1, ww, fw, dst);
    cur = dst;
  }
  hipLaunchKernelGGL(inp_unsharp_kernel, grid, dim3(256), 0, s, (const uint8_t*)img_u8, cur, n, percent, threshold,
                     (uint8_t*)out_u8);
  return ink_launch_status();
}

extern "C" int ink_inp_rgba_cut(const void* rgb_u8, const void* mask_u8, int32_t H, int32_t W, void* rgba_u8,
                                void* stream) {
  INK_CHECK_ARG(rgb_u8 && mask_u8 && rgba_u8 && H > 0 && W > 0 && H <= 16384 && W <= 16384);
  hipLaunchKernelGGL(inp_rgba_cut_kernel, dim3(inp_blocks((int64_t)H * W)), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)rgb_u8, (const uint8_t*)mask_u8, (int64_t)H * W, (uint8_t*)rgba_u8);
  return ink_launch_status();
}
