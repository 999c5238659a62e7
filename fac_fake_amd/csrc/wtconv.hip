// WTConv2d(C, kernel_size 5, wt_levels 1, db1) -> BatchNorm2d (eval) -> ReLU
// (-> MaxPool2d(2,2)) of CViT-main/model/other/cvit_GGCA_ADD_WTConv.py
// (:167-328), behind fac_wtconv.  Per channel c of a map x with even sides,
// cross-correlation as in F.conv2d:
//
//   s_k[y][x]       = sum_{i,j in {0,1}} dwt[c][k][i][j] x[2y+i][2x+j]      k = 0..3, half resolution
//   t_k             = depthwise 5x5 of s_k with wtaps[c][k], zero padding 2 at the HALF-resolution border
//   u[2y+i][2x+j]   = sum_k iwt[c][k][i][j] t_k[y][x]
//   b               = depthwise 5x5 of x with btaps[c], zero padding 2
//   out             = maxpool?(relu(scale[c] (u + b) + shift[c]))             (one 16-bit rounding)
//
// on 16-bit channels-last maps [n][h][w][c].  The host folds wavelet_scale into
// wtaps, base_scale into btaps and base_scale * bias * scale into shift.  The
// 2x2 filters are operands (the reference keeps them in the state_dict), not
// constants.  Every sum is an fp32 fma chain from 0 in index order (i, j row
// major; the 25 taps row major; k = 0..3), then u + b, one fma(scale, ., shift),
// ReLU, the window max, one rounding.  A pixel outside the map enters as 0; the
// filters are linear and bias-free, so a half-resolution pixel outside the map
// is then 0 as well, which is the reference's zero padding of the subbands for
// even sides (odd sides are refused).
//
// Decomposition.  A workgroup (256 threads, 4 waves) owns an 8 x 8 tile of
// half-resolution pixels (16 x 16 outputs, or 8 x 8 pooled ones: the pool
// window is exactly one half-resolution pixel's four outputs) and 16
// channels; wave q owns channels 4q .. 4q + 3 of the 16, its 64 lanes are the
// 64 half-resolution pixels.  The channel quad is wave-uniform, so every
// filter and tap is a scalar operand read with scalar loads, none sits in LDS
// or in a vector register, and a lane's LDS reads are conflict-free runs of
// float4 over consecutive pixels.  Four phases, three barriers:
//
//   1  global -> LDS: the 24 x 24 input tile (16 + the 4-pixel halo each side:
//      2 half-resolution pixels of the wavelet path, which covers the base
//      path's 2), 16 channels, as 16-bit, zeros outside the map; 16-byte
//      vectors with the channel fastest over the lanes (xs, 18 KB);
//   2  the four subbands of the 12 x 12 half-resolution tile in fp32, LDS ->
//      LDS (sb, 36 KB): never rounded;
//   3  per lane one half-resolution pixel: the four 5 x 5 sums over sb, the
//      inverse transform to its four outputs, the base 5 x 5 over a 6 x 6
//      window of xs, the affine, ReLU (and max), rounded once into os (8 KB);
//   4  os -> global in 16-byte vectors, the channel fastest.
//
// 62 KB of LDS per workgroup: two workgroups per CU (160 KB).  The halo costs
// 2.25 x the tile in phase 1 / 2 work (L2 reads and 16 of ~236 fma per
// half-resolution pixel and channel); the sibling workgroup of the other 16
// channels is the next block index, so the second half of each pixel's line
// comes from L2.  Every output element is computed by one lane from the input
// alone in one fixed order, no atomics: a crop's bits do not depend on n.
#include "common.hpp"
#include "fac_cvit.h"
#include "fac_ops.h"

namespace fac {

constexpr int WT_T = 256;                              // threads per workgroup: wave q owns channel quad q
constexpr int WT_CB = 16;                              // channels per workgroup
constexpr int WT_TH = 8, WT_TW = 8;                    // half-resolution pixels per tile (one per lane)
constexpr int WT_SH = WT_TH + 4, WT_SW = WT_TW + 4;    // the subband tile with its halo of 2
constexpr int WT_XH = 2 * WT_SH, WT_XW = 2 * WT_SW;    // the input tile
constexpr int WT_NS = WT_SH * WT_SW, WT_NX = WT_XH * WT_XW;
static_assert(WT_TH * WT_TW == 64 && WT_T == 4 * 64 && WT_CB == 16, "one lane per half-resolution pixel, one wave per quad");

typedef uint16_t wt_u16x4 __attribute__((ext_vector_type(4)));
typedef uint16_t wt_u16x8 __attribute__((ext_vector_type(8)));
typedef float wt_f32x4 __attribute__((ext_vector_type(4)));

template <class T, bool POOL>
__global__ __launch_bounds__(WT_T, 2) void wtconv_k(const uint16_t* __restrict__ in, uint16_t* __restrict__ out, int H,
                                                   int W, int C, const float* __restrict__ dwt,
                                                   const float* __restrict__ wtaps, const float* __restrict__ iwt,
                                                   const float* __restrict__ btaps, const float* __restrict__ scale,
                                                   const float* __restrict__ shift, int ncb, int ntx, int nty) {
  __shared__ __attribute__((aligned(16))) uint16_t xs[4 * WT_NX * 4];   // [quad][y][x][4 channels]
  __shared__ __attribute__((aligned(16))) float sb[4 * 4 * WT_NS * 4];  // [quad][k][y][x][4 channels]
  __shared__ __attribute__((aligned(16))) uint16_t os[4 * WT_TH * WT_TW * WT_CB];   // [y][x][16 channels]
  const int tid = threadIdx.x;
  long blk = blockIdx.x;
  const int cb = (int)(blk % ncb);
  blk /= ncb;
  const int tx = (int)(blk % ntx);
  blk /= ntx;
  const int ty = (int)(blk % nty);
  const long img = blk / nty;
  const int cb0 = cb * WT_CB;
  const int y0 = 2 * WT_TH * ty - 4, x0 = 2 * WT_TW * tx - 4;   // the input tile's origin in the map
  const uint16_t* ib = in + (size_t)img * H * W * C + cb0;

  // phase 1: the input tile, zeros outside the map
  for (int i = tid; i < WT_NX * 2; i += WT_T) {
    const int v = i & 1, p = i >> 1;
    const int py = p / WT_XW, px = p - py * WT_XW;
    const int gy = y0 + py, gx = x0 + px;
    wt_u16x8 d = (wt_u16x8)(0);
    if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) d = *(const wt_u16x8*)(ib + ((size_t)gy * W + gx) * C + v * 8);
    *(wt_u16x4*)(xs + ((2 * v) * WT_NX + p) * 4) = d.lo;
    *(wt_u16x4*)(xs + ((2 * v + 1) * WT_NX + p) * 4) = d.hi;
  }
  __syncthreads();

  const int q = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int quad = cb0 / 4 + q;                          // of the map's c / 4; wave-uniform
  const uint16_t* xq = xs + q * WT_NX * 4;
  float* sq = sb + q * 4 * WT_NS * 4;

  // phase 2: the subbands of the 12 x 12 half-resolution tile
  {
    const float* f = dwt + (size_t)quad * 64;            // [k][i * 2 + j][4]
    for (int p = lane; p < WT_NS; p += 64) {
      const int sy = p / WT_SW, sx = p - sy * WT_SW;
      float xv[4][4];
#pragma unroll
      for (int ij = 0; ij < 4; ++ij) {
        const wt_u16x4 r = *(const wt_u16x4*)(xq + ((2 * sy + (ij >> 1)) * WT_XW + 2 * sx + (ij & 1)) * 4);
#pragma unroll
        for (int c = 0; c < 4; ++c) xv[ij][c] = T::to_f32(r[c]);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        wt_f32x4 s = (wt_f32x4)(0.0f);
#pragma unroll
        for (int ij = 0; ij < 4; ++ij)
#pragma unroll
          for (int c = 0; c < 4; ++c) s[c] = fmaf(f[(k * 4 + ij) * 4 + c], xv[ij][c], s[c]);
        *(wt_f32x4*)(sq + (k * WT_NS + p) * 4) = s;
      }
    }
  }
  __syncthreads();

  // phase 3: one half-resolution pixel per lane
  const int hy = lane >> 3, hx = lane & 7;
  float o[4][4];                                         // [i * 2 + j][channel]: u, then u + b
#pragma unroll
  for (int ij = 0; ij < 4; ++ij)
#pragma unroll
    for (int c = 0; c < 4; ++c) o[ij][c] = 0.0f;
  {
    const float* wq = wtaps + (size_t)quad * 400;        // [k][25][4]
    const float* fi = iwt + (size_t)quad * 64;           // [k][i * 2 + j][4]
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      const float* sk = sq + (k * WT_NS + hy * WT_SW + hx) * 4;
#pragma unroll
      for (int tap = 0; tap < 25; ++tap) {
        const wt_f32x4 s = *(const wt_f32x4*)(sk + ((tap / 5) * WT_SW + tap % 5) * 4);
#pragma unroll
        for (int c = 0; c < 4; ++c) t[c] = fmaf(wq[(k * 25 + tap) * 4 + c], s[c], t[c]);
      }
#pragma unroll
      for (int ij = 0; ij < 4; ++ij)
#pragma unroll
        for (int c = 0; c < 4; ++c) o[ij][c] = fmaf(fi[(k * 4 + ij) * 4 + c], t[c], o[ij][c]);
    }
  }
  {
    const float* bq = btaps + (size_t)quad * 100;        // [25][4]
    float b[4][4];
#pragma unroll
    for (int ij = 0; ij < 4; ++ij)
#pragma unroll
      for (int c = 0; c < 4; ++c) b[ij][c] = 0.0f;
    // the 6 x 6 window of the lane's four outputs, a row at a time: window row r
    // is tap row r - i of output row i, so every chain runs in tap order
    const uint16_t* xw = xq + ((2 * hy + 2) * WT_XW + 2 * hx + 2) * 4;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      float row[6][4];
#pragma unroll
      for (int e = 0; e < 6; ++e) {
        const wt_u16x4 d = *(const wt_u16x4*)(xw + (r * WT_XW + e) * 4);
#pragma unroll
        for (int c = 0; c < 4; ++c) row[e][c] = T::to_f32(d[c]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int a = r - i;
        if (a < 0 || a > 4) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int e = 0; e < 5; ++e)
#pragma unroll
            for (int c = 0; c < 4; ++c) b[i * 2 + j][c] = fmaf(bq[(a * 5 + e) * 4 + c], row[j + e][c], b[i * 2 + j][c]);
      }
    }
#pragma unroll
    for (int ij = 0; ij < 4; ++ij)
#pragma unroll
      for (int c = 0; c < 4; ++c) o[ij][c] += b[ij][c];
  }
  {
    float sc[4], sh[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      sc[c] = scale[quad * 4 + c];
      sh[c] = shift[quad * 4 + c];
    }
    if (POOL) {
      wt_u16x4 r;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float best = 0.0f;                               // ReLU outputs are >= 0
#pragma unroll
        for (int ij = 0; ij < 4; ++ij) best = fmaxf(best, relu(fmaf(sc[c], o[ij][c], sh[c])));
        r[c] = T::from_f32(best);
      }
      *(wt_u16x4*)(os + (hy * WT_TW + hx) * WT_CB + q * 4) = r;
    } else {
#pragma unroll
      for (int ij = 0; ij < 4; ++ij) {
        wt_u16x4 r;
#pragma unroll
        for (int c = 0; c < 4; ++c) r[c] = T::from_f32(relu(fmaf(sc[c], o[ij][c], sh[c])));
        *(wt_u16x4*)(os + ((2 * hy + (ij >> 1)) * (2 * WT_TW) + 2 * hx + (ij & 1)) * WT_CB + q * 4) = r;
      }
    }
  }
  __syncthreads();

  // phase 4: the output tile, pixels outside the map dropped
  const int OTH = POOL ? WT_TH : 2 * WT_TH, OTW = POOL ? WT_TW : 2 * WT_TW;
  const int Ho = POOL ? H / 2 : H, Wo = POOL ? W / 2 : W;
  uint16_t* ob = out + (size_t)img * Ho * Wo * C + cb0;
  for (int i = tid; i < OTH * OTW * 2; i += WT_T) {
    const int v = i & 1, p = i >> 1;
    const int py = p / OTW, px = p - py * OTW;
    const int gy = OTH * ty + py, gx = OTW * tx + px;
    if (gy < Ho && gx < Wo) *(wt_u16x8*)(ob + ((size_t)gy * Wo + gx) * C + v * 8) = *(const wt_u16x8*)(os + p * WT_CB + v * 8);
  }
}

template <class T>
static hipError_t launch_wt(const uint16_t* in, uint16_t* out, int n, int h, int w, int c, const float* dwt,
                            const float* wtaps, const float* iwt, const float* btaps, const float* scale,
                            const float* shift, bool pool, hipStream_t st) {
  const int ncb = c / WT_CB, ntx = (w / 2 + WT_TW - 1) / WT_TW, nty = (h / 2 + WT_TH - 1) / WT_TH;
  const long blocks = (long)n * nty * ntx * ncb;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  if (pool)
    wtconv_k<T, true><<<(unsigned)blocks, WT_T, 0, st>>>(in, out, h, w, c, dwt, wtaps, iwt, btaps, scale, shift, ncb, ntx, nty);
  else
    wtconv_k<T, false><<<(unsigned)blocks, WT_T, 0, st>>>(in, out, h, w, c, dwt, wtaps, iwt, btaps, scale, shift, ncb, ntx, nty);
  return hipGetLastError();
}

}  // namespace fac

extern "C" int fac_wtconv(int dtype, const void* in, void* out, int n, int h, int w, int c, const float* dwt,
                          const float* wtaps, const float* iwt, const float* btaps, const float* scale,
                          const float* shift, int pool, void* stream) {
  using namespace fac;
  if (!in || !out || !dwt || !wtaps || !iwt || !btaps || !scale || !shift || n <= 0 || (dtype != 0 && dtype != 1) ||
      (pool != 0 && pool != 1))
    return FAC_ERR_ARG;
  if (((uintptr_t)in | (uintptr_t)out) % 16) return FAC_ERR_ARG;
  if (((uintptr_t)dwt | (uintptr_t)wtaps | (uintptr_t)iwt | (uintptr_t)btaps | (uintptr_t)scale | (uintptr_t)shift) % 4)
    return FAC_ERR_ARG;
  if (c < 32 || c > 256 || c % 32 || h < 2 || w < 2 || h > 224 || w > 224 || ((h | w) & 1)) return FAC_ERR_SHAPE;
  const uint16_t* i16 = (const uint16_t*)in;
  uint16_t* o16 = (uint16_t*)out;
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = dtype == 0 ? launch_wt<BF16>(i16, o16, n, h, w, c, dwt, wtaps, iwt, btaps, scale, shift, pool != 0, st)
                                  : launch_wt<F16>(i16, o16, n, h, w, c, dwt, wtaps, iwt, btaps, scale, shift, pool != 0, st);
  if (e == hipErrorInvalidValue) return FAC_ERR_SHAPE;
  return e == hipSuccess ? FAC_OK : FAC_ERR_HIP;
}
