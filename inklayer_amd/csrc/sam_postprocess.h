// Per-pixel arithmetic of Sam.postprocess_masks (SA/modeling/sam.py:133-162): low [S, S] -> (virtual) [L, L] -> crop
// [in_h, in_w] -> [out_h, out_w], both bilinear stages (align_corners=False) composed per output pixel.  Shared by the
// mask kernels of sam_decoder.hip and the mask-statistics kernels of amg.hip, so that both threshold the SAME floats
// (the library is built with -ffp-contract=off: the expression below is evaluated as written in every kernel).
#pragma once
#include "common.h"

namespace {

// torch bilinear (align_corners=False) source index + weights
__device__ __forceinline__ void bil(int dst, float scale, int in_size, int& i0, int& i1, float& l1) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = (int)src;
  i0 = i0 < in_size - 1 ? i0 : in_size - 1;
  i1 = i0 < in_size - 1 ? i0 + 1 : i0;
  l1 = src - (float)i0;
}

struct PostScales {
  float sA, sBh, sBw;
};
__device__ __forceinline__ PostScales post_scales(int S, int L, int in_h, int in_w, int out_h, int out_w) {
  return PostScales{(float)S / (float)L, (float)in_h / (float)out_h, (float)in_w / (float)out_w};
}

// One output pixel (Y, X) of mask lp: every index and weight computed at the pixel (the one-pixel form).
__device__ __forceinline__ float post_pixel(const float* __restrict__ lp, int S, const PostScales& sc, int in_h, int in_w,
                                            int Y, int X) {
  int y0, y1, x0, x1;
  float ly, lx;
  bil(Y, sc.sBh, in_h, y0, y1, ly);
  bil(X, sc.sBw, in_w, x0, x1, lx);
  auto stageA = [&](int yy, int xx) {
    int a0, a1, c0, c1;
    float la, lc;
    bil(yy, sc.sA, S, a0, a1, la);
    bil(xx, sc.sA, S, c0, c1, lc);
    const float v00 = lp[a0 * S + c0], v01 = lp[a0 * S + c1];
    const float v10 = lp[a1 * S + c0], v11 = lp[a1 * S + c1];
    return (1.f - la) * ((1.f - lc) * v00 + lc * v01) + la * ((1.f - lc) * v10 + lc * v11);
  };
  const float v00 = stageA(y0, x0), v01 = stageA(y0, x1), v10 = stageA(y1, x0), v11 = stageA(y1, x1);
  return (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
}

// The rows form: PX consecutive output pixels of one row per thread.  Everything that depends on the column only - the
// second-stage source columns and weights and, for each of them, the first-stage columns and weights - is computed once
// per thread (post_cols) and reused for every row (post_row).
constexpr int POST_PX = 4;
struct PostCols {
  float lx[POST_PX], lc[POST_PX][2];
  int c0[POST_PX][2], c1[POST_PX][2];
};
__device__ __forceinline__ void post_cols(int xq, int S, const PostScales& sc, int in_w, PostCols& c) {
#pragma unroll
  for (int px = 0; px < POST_PX; ++px) {
    int x0, x1;
    bil(xq * POST_PX + px, sc.sBw, in_w, x0, x1, c.lx[px]);
    bil(x0, sc.sA, S, c.c0[px][0], c.c1[px][0], c.lc[px][0]);
    bil(x1, sc.sA, S, c.c0[px][1], c.c1[px][1], c.lc[px][1]);
  }
}
__device__ __forceinline__ void post_row(const float* __restrict__ lp, int S, const PostScales& sc, int in_h, int Y,
                                         const PostCols& c, float (&vals)[POST_PX]) {
  int y0, y1;
  float ly;
  bil(Y, sc.sBh, in_h, y0, y1, ly);
  int a0[2], a1[2];
  float la[2];
  bil(y0, sc.sA, S, a0[0], a1[0], la[0]);
  bil(y1, sc.sA, S, a0[1], a1[1], la[1]);
  const float* r00 = lp + a0[0] * S;
  const float* r01 = lp + a1[0] * S;
  const float* r10 = lp + a0[1] * S;
  const float* r11 = lp + a1[1] * S;
#pragma unroll
  for (int px = 0; px < POST_PX; ++px) {
    auto stageA = [&](const float* ra, const float* rb, float lav, int k) {
      const float v00 = ra[c.c0[px][k]], v01 = ra[c.c1[px][k]];
      const float v10 = rb[c.c0[px][k]], v11 = rb[c.c1[px][k]];
      return (1.f - lav) * ((1.f - c.lc[px][k]) * v00 + c.lc[px][k] * v01) + lav * ((1.f - c.lc[px][k]) * v10 + c.lc[px][k] * v11);
    };
    const float v00 = stageA(r00, r01, la[0], 0), v01 = stageA(r00, r01, la[0], 1);
    const float v10 = stageA(r10, r11, la[1], 0), v11 = stageA(r10, r11, la[1], 1);
    vals[px] = (1.f - ly) * ((1.f - c.lx[px]) * v00 + c.lx[px] * v01) + ly * ((1.f - c.lx[px]) * v10 + c.lx[px] * v11);
  }
}

}  // namespace
