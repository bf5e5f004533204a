// Shared device helpers for the InkLayer gfx950 (MI355X / CDNA4) kernels.
// wave = 64 lanes; all reductions below are wave64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef _Float16 f16;
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

#define INK_OK 0
#define INK_ERR_ARG 1
#define INK_ERR_LAUNCH 2

#define INK_CHECK_ARG(cond)            \
  do {                                 \
    if (!(cond)) return INK_ERR_ARG;   \
  } while (0)

static inline int ink_launch_status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? INK_OK : INK_ERR_LAUNCH;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// erf-form GELU, as torch.nn.GELU() default.  erf by Abramowitz-Stegun 7.1.26 (|abs err| <= 1.5e-7, i.e.
// f32-rounding level for GELU's use) with v_rcp / v_exp: branch-free, 12 VALU + 2 transcendental ops instead of
// libm's erff.  With e = 1 - erf(|x| / sqrt 2):  gelu(x) = max(x, 0) - (|x| / 2) e  for either sign of x, and the
// exponent's log2(e) is folded into the argument: u = |x| sqrt(log2(e) / 2), e = poly(t) t 2^(-u u),
// t = 1 / (1 + p |x| / sqrt 2) = 1 / (1 + (p / sqrt(log2 e)) u).
__device__ __forceinline__ float gelu_erf(float x) {
  const float u = fabsf(x) * 0.84932180028801904272f;                  // sqrt(log2(e) / 2)
  const float t = __builtin_amdgcn_rcpf(fmaf(0.27273748087922250f, u, 1.0f));   // 0.3275911 / sqrt(log2 e)
  float pl = fmaf(1.061405429f, t, -1.453152027f);
  pl = fmaf(pl, t, 1.421413741f);
  pl = fmaf(pl, t, -0.284496736f);
  pl = fmaf(pl, t, 0.254829592f);
  const float e = pl * t * __builtin_amdgcn_exp2f(-(u * u));           // 1 - erf(|x| / sqrt 2)
  return fmaf(-0.5f * fabsf(x), e, fmaxf(x, 0.0f));
}

// RGB -> grey of 8-bit pixels: the three fixed-point forms of (0.299, 0.587, 0.114) that the reference's libraries
// use.  They are DIFFERENT functions - pil_luma differs from the other two in the coefficients' rounding, and the two
// cv2 forms can differ by one grey level ((0, 3, 217) is 26 in 15 bits and 27 in 14) - and every call site is pinned
// bit for bit, by its own test, to the one its reference call produces.  Do not swap one for another.
//   pil_luma    Pillow, Image.convert("L") (Convert.c rgb2l): the sketch's stroke test of the mask cleaner and the
//               refinement stage (luma < 250 / <= 250), the inpainting stage's contrast mean and grey round trip.
//   cv_gray15   OpenCV's 15-bit form: what cv2.imread(path, IMREAD_GRAYSCALE) returns for an 8-bit RGB file (libpng's
//               rgb_to_gray with OpenCV's coefficients) - the refinement stage's fourth sketch plane and the layer
//               stage's grey sketch - and cv2.cvtColor(COLOR_RGB2GRAY) as the layer stage and the inpainting
//               stage's adaptive-threshold clean-up are pinned to it (tests/layers_ref.py, tests/inpaint_ref.py).
//   cv_gray14   OpenCV's 14-bit form: cv2.cvtColor(COLOR_RGB2GRAY) as the visualisation and the evaluation stage are
//               pinned to it (visualization.py:83; tests/vis_ref.py, tests/evaluate_ref.py, visualize.gray_host).
__device__ __forceinline__ int pil_luma(unsigned r, unsigned g, unsigned b) {
  return (int)((19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16);
}
__device__ __forceinline__ int cv_gray15(unsigned r, unsigned g, unsigned b) {
  return (int)((9798u * r + 19235u * g + 3735u * b + 16384u) >> 15);
}
__device__ __forceinline__ int cv_gray14(unsigned r, unsigned g, unsigned b) {
  return (int)((4899u * r + 9617u * g + 1868u * b + 8192u) >> 14);
}

// bijective XCD-aware block remap: blocks b and b+8 share an XCD (round-robin
// dispatch); give every XCD a contiguous chunk of logical tiles so neighbouring
// tiles (sharing an operand panel) hit the same 4 MiB L2.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, x = bid & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}
