// InceptionDWConv2d -> BatchNorm2d (eval) -> ReLU (-> MaxPool2d(2,2)) of
// CViT-main/model/cvit_GGCA_ADD_DConv.py (:157-177, :186-256), behind
// fac_idwconv:
//
//   channels [0, 5c/8)        y = x                         (identity)
//   the next gc = c/8         y = depthwise 3x3,  padding 1
//   the next gc               y = depthwise 1x11 along W, padding 5
//   the last gc               y = depthwise 11x1 along H, padding 5
//   out = maxpool?(relu(scale[c] * y + shift[c]))           (one 16-bit rounding)
//
// on 16-bit channels-last maps [n][h][w][c].  The taps are used as given (NOT
// pre-multiplied by scale): y is an fp32 fma chain over the taps in index
// order starting from 0 (t = 0..8 row-major for the 3x3, t = 0..10 for the
// bands), a tap that falls outside the map enters as 0 (zero padding of the
// conv's input, so it contributes 0 and never `shift`), then one
// fma(scale, y, shift), ReLU, the max over the 2x2 window, one rounding.  The
// host folds the conv bias and the BatchNorm into scale / shift.
//
// Layout.  The layer is depthwise, 2 / 8 of its channels read 11 pixels and
// 5 / 8 read one, so it is load/store work with little arithmetic per byte.
// A thread owns V consecutive channels of a pixel (V = 8, one 16-byte vector,
// when c is a multiple of 64; V = 4 otherwise: at c = 32, gc = 4, a 16-byte
// vector would straddle two branches, and 5c/8 and gc are multiples of 4 for
// every multiple of 32), so a thread has exactly one branch.  From c = 128,
// two launches:
//
//   idw_id_k    the 5c/8 identity channels: affine, ReLU, pool.  Threads are
//               (pixel, vector) with the vector fastest, a pixel's identity
//               channels are one contiguous run (320 bytes at c = 256).
//   idw_conv_k  the 3c/8 conv channels, also (pixel, vector): a pixel's three
//               branches are one contiguous run of 3c/4 bytes.  The branches
//               share one unrolled loop of 11 taps whose per-lane offset is
//               (t/3 - 1, t%3 - 1), (0, t - 5) or (t - 5, 0); the 3x3 lanes
//               have 9 live taps.  The loop has no branches: a dead or padded
//               tap re-loads the lane's own pixel (a line the wave has just
//               fetched) and is selected to 0, so the 11 loads issue back to
//               back.  The element offset of every tap is a per-thread
//               constant, computed once.  The taps sit in LDS ([tap][conv
//               channel], 4.1 KB at c = 256; per thread they cost 88
//               registers).  The halo re-reads (rows / columns +-5) hit in L2
//               / the vector cache; no activation goes through LDS.
//
// Below c = 128 one launch, idw_all_k, covers all channels with the same
// branch-free tap loop; its identity lanes (one live tap of weight 1) idle
// through the other ten taps.  That costs VALU time at every c, but at c = 32
// and 64 a pixel's identity / conv runs are 40-80 / 24-48 bytes, the two
// launches each touch every cache line of the map, and the single launch is
// faster there; from c = 128 the split is 1.7-2.5 x faster.
// Both routes compute the same bits, and the route depends on c alone.
// A thread walks IDW_K pixels ppb apart; with pool it evaluates the window's
// four input pixels itself.
//
// Every output element is computed by one thread from the input alone in one
// fixed order: a crop's bits do not depend on n.
#include "common.hpp"
#include "fac_cvit.h"
#include "fac_ops.h"

namespace fac {

constexpr int IDW_T = 256;   // at most this many threads per workgroup
constexpr int IDW_K = 8;     // output pixels per thread
constexpr int IDW_TAPS = 11;
constexpr int IDW_MAX_C = 256;
constexpr int IDW_SPLIT_C = 128;   // from this many channels: two launches (identity, conv)

// All channels in one launch (c < 128).  Threads are (pixel, vector) over the
// whole pixel; identity lanes have one live tap (weight 1) and idle through
// the other ten.
template <class T, int V, bool POOL>
__global__ __launch_bounds__(IDW_T) void idw_all_k(const uint16_t* __restrict__ in, uint16_t* __restrict__ out,
                                                   long npix, int H, int W, int C, const float* __restrict__ w_hw,
                                                   const float* __restrict__ w_w, const float* __restrict__ w_h,
                                                   const float* __restrict__ scale, const float* __restrict__ shift,
                                                   int ppb) {
  typedef uint16_t vec __attribute__((ext_vector_type(V)));
  const int nv = C / V, gc = C / 8, cid = C - 3 * gc;
  const int tid = threadIdx.x, v = tid % nv, p = tid / nv;
  const int ch0 = v * V;
  const int br = ch0 < cid ? 0 : (ch0 - cid) / gc + 1;   // 0 identity, 1 3x3, 2 1x11, 3 11x1
  const int nt = br == 0 ? 1 : (br == 1 ? 9 : IDW_TAPS);
  // taps[t][channel] in LDS (identity channels: tap 0 = 1), read back as V
  // consecutive floats per tap: 88 fewer registers than keeping them per thread
  __shared__ __attribute__((aligned(16))) float taps[IDW_TAPS * IDW_SPLIT_C];   // c < IDW_SPLIT_C here
  for (int i = tid; i < IDW_TAPS * C; i += blockDim.x) {
    const int t = i / C, ch = i - t * C;
    const int b = ch < cid ? 0 : (ch - cid) / gc + 1;
    const int cb = b == 0 ? 0 : ch - cid - (b - 1) * gc;   // channel within its conv branch
    float wv;
    if (b == 0) wv = t == 0 ? 1.0f : 0.0f;
    else if (b == 1) wv = t < 9 ? w_hw[cb * 9 + t] : 0.0f;
    else wv = (b == 2 ? w_w : w_h)[cb * IDW_TAPS + t];
    taps[i] = wv;
  }
  float sc[V], sh[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    sc[j] = scale[ch0 + j];
    sh[j] = shift[ch0 + j];
  }
  __syncthreads();
  const int Ho = POOL ? H / 2 : H, Wo = POOL ? W / 2 : W;
  const long per_img = (long)Ho * Wo;

  for (int i = 0; i < IDW_K; ++i) {
    const long pix = ((long)blockIdx.x * IDW_K + i) * ppb + p;
    if (pix >= npix) break;
    const long img = pix / per_img;
    const int rem = (int)(pix - img * per_img);
    const int yo = rem / Wo, xo = rem - yo * Wo;
    const uint16_t* ib = in + (size_t)img * H * W * C + ch0;
    float best[V];
#pragma unroll
    for (int j = 0; j < V; ++j) best[j] = 0.0f;   // ReLU outputs are >= 0
#pragma unroll 1
    for (int q = 0; q < (POOL ? 4 : 1); ++q) {
      const int y = POOL ? 2 * yo + (q >> 1) : yo, x = POOL ? 2 * xo + (q & 1) : xo;
      float acc[V];
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] = 0.0f;
      // Branch-free: a tap this lane does not have (t >= nt) or that falls
      // outside the map loads the lane's own pixel instead and enters the
      // chain as 0 (fma(w, 0, acc) == acc), so the 11 loads issue back to
      // back instead of one load and one wait per predicated block.
      vec d[IDW_TAPS];
      bool on[IDW_TAPS];
#pragma unroll
      for (int t = 0; t < IDW_TAPS; ++t) {
        const int dy = br == 1 ? t / 3 - 1 : (br == 3 ? t - 5 : 0);
        const int dx = br == 1 ? t % 3 - 1 : (br == 2 ? t - 5 : 0);
        const int yy = y + dy, xx = x + dx;
        on[t] = t < nt && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
        d[t] = *(const vec*)(ib + ((size_t)(on[t] ? yy : y) * W + (on[t] ? xx : x)) * C);
      }
#pragma unroll
      for (int t = 0; t < IDW_TAPS; ++t) {
        const float* wt = taps + t * C + ch0;
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = fmaf(wt[j], on[t] ? T::to_f32(d[t][j]) : 0.0f, acc[j]);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) best[j] = fmaxf(best[j], relu(fmaf(sc[j], acc[j], sh[j])));
    }
    vec o;
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = T::from_f32(best[j]);
    *(vec*)(out + (size_t)pix * C + ch0) = o;
  }
}

// The two launches of c >= 128.  nvr: vectors per pixel the launch covers.
template <class T, int V, bool POOL>
__global__ __launch_bounds__(IDW_T) void idw_id_k(const uint16_t* __restrict__ in, uint16_t* __restrict__ out, long npix,
                                                  int H, int W, int C, const float* __restrict__ scale,
                                                  const float* __restrict__ shift, int nvr, int ppb) {
  typedef uint16_t vec __attribute__((ext_vector_type(V)));
  const int tid = threadIdx.x, p = tid / nvr, ch0 = (tid - p * nvr) * V;
  float sc[V], sh[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    sc[j] = scale[ch0 + j];
    sh[j] = shift[ch0 + j];
  }
  const int Ho = POOL ? H / 2 : H, Wo = POOL ? W / 2 : W;
  const long per_img = (long)Ho * Wo;
  for (int i = 0; i < IDW_K; ++i) {
    const long pix = ((long)blockIdx.x * IDW_K + i) * ppb + p;
    if (pix >= npix) break;
    const long img = pix / per_img;
    const int rem = (int)(pix - img * per_img);
    const int yo = rem / Wo, xo = rem - yo * Wo;
    const uint16_t* ib = in + (size_t)img * H * W * C + ch0;
    float best[V];
#pragma unroll
    for (int j = 0; j < V; ++j) best[j] = 0.0f;   // ReLU outputs are >= 0
#pragma unroll
    for (int q = 0; q < (POOL ? 4 : 1); ++q) {
      const int y = POOL ? 2 * yo + (q >> 1) : yo, x = POOL ? 2 * xo + (q & 1) : xo;
      const vec d = *(const vec*)(ib + ((size_t)y * W + x) * C);
#pragma unroll
      for (int j = 0; j < V; ++j) best[j] = fmaxf(best[j], relu(fmaf(sc[j], T::to_f32(d[j]), sh[j])));
    }
    vec o;
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = T::from_f32(best[j]);
    *(vec*)(out + (size_t)pix * C + ch0) = o;
  }
}

template <class T, int V, bool POOL>
__global__ __launch_bounds__(IDW_T) void idw_conv_k(const uint16_t* __restrict__ in, uint16_t* __restrict__ out,
                                                    long npix, int H, int W, int C, const float* __restrict__ w_hw,
                                                    const float* __restrict__ w_w, const float* __restrict__ w_h,
                                                    const float* __restrict__ scale, const float* __restrict__ shift,
                                                    int nvr, int ppb) {
  typedef uint16_t vec __attribute__((ext_vector_type(V)));
  const int gc = C / 8, cid = C - 3 * gc, CC = 3 * gc;   // CC conv channels, from channel cid
  const int tid = threadIdx.x, p = tid / nvr, k0 = (tid - p * nvr) * V, ch0 = cid + k0;
  const int br = k0 / gc;                                // 0 3x3, 1 1x11, 2 11x1
  const int nt = br == 0 ? 9 : IDW_TAPS;
  // taps[t][conv channel]; read back as V consecutive floats per tap
  __shared__ __attribute__((aligned(16))) float taps[IDW_TAPS * (3 * IDW_MAX_C / 8)];
  for (int i = tid; i < IDW_TAPS * CC; i += blockDim.x) {
    const int t = i / CC, k = i - t * CC;
    const int b = k / gc, cb = k - b * gc;               // branch, channel within it
    taps[i] = b == 0 ? (t < 9 ? w_hw[cb * 9 + t] : 0.0f) : (b == 1 ? w_w : w_h)[cb * IDW_TAPS + t];
  }
  float sc[V], sh[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    sc[j] = scale[ch0 + j];
    sh[j] = shift[ch0 + j];
  }
  int dys[IDW_TAPS], dxs[IDW_TAPS], doff[IDW_TAPS];       // per-thread constants of the tap loop
#pragma unroll
  for (int t = 0; t < IDW_TAPS; ++t) {
    dys[t] = br == 0 ? t / 3 - 1 : (br == 2 ? t - 5 : 0);
    dxs[t] = br == 0 ? t % 3 - 1 : (br == 1 ? t - 5 : 0);
    doff[t] = (dys[t] * W + dxs[t]) * C;                  // |.| <= 5 * 224 * 256
  }
  __syncthreads();
  const int Ho = POOL ? H / 2 : H, Wo = POOL ? W / 2 : W;
  const long per_img = (long)Ho * Wo;

  for (int i = 0; i < IDW_K; ++i) {
    const long pix = ((long)blockIdx.x * IDW_K + i) * ppb + p;
    if (pix >= npix) break;
    const long img = pix / per_img;
    const int rem = (int)(pix - img * per_img);
    const int yo = rem / Wo, xo = rem - yo * Wo;
    const uint16_t* ib = in + (size_t)img * H * W * C + ch0;
    float best[V];
#pragma unroll
    for (int j = 0; j < V; ++j) best[j] = 0.0f;   // ReLU outputs are >= 0
#pragma unroll 1
    for (int q = 0; q < (POOL ? 4 : 1); ++q) {
      const int y = POOL ? 2 * yo + (q >> 1) : yo, x = POOL ? 2 * xo + (q & 1) : xo;
      const uint16_t* pb = ib + ((size_t)y * W + x) * C;
      float acc[V];
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] = 0.0f;
      vec d[IDW_TAPS];
      bool on[IDW_TAPS];
#pragma unroll
      for (int t = 0; t < IDW_TAPS; ++t) {
        on[t] = t < nt && (unsigned)(y + dys[t]) < (unsigned)H && (unsigned)(x + dxs[t]) < (unsigned)W;
        d[t] = *(const vec*)(pb + (on[t] ? doff[t] : 0));
      }
#pragma unroll
      for (int t = 0; t < IDW_TAPS; ++t) {
        const float* wt = taps + t * CC + k0;
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = fmaf(wt[j], on[t] ? T::to_f32(d[t][j]) : 0.0f, acc[j]);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) best[j] = fmaxf(best[j], relu(fmaf(sc[j], acc[j], sh[j])));
    }
    vec o;
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = T::from_f32(best[j]);
    *(vec*)(out + (size_t)pix * C + ch0) = o;
  }
}

template <class T, int V>
static hipError_t launch_idw_all(const uint16_t* in, uint16_t* out, int n, int h, int w, int c, const float* w_hw,
                                 const float* w_w, const float* w_h, const float* scale, const float* shift, bool pool,
                                 hipStream_t st) {
  const int nv = c / V, ppb = IDW_T / nv;
  const long npix = (long)n * (pool ? h / 2 : h) * (pool ? w / 2 : w);
  const long per_block = (long)ppb * IDW_K;
  const long blocks = (npix + per_block - 1) / per_block;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  if (pool)
    idw_all_k<T, V, true><<<(unsigned)blocks, ppb * nv, 0, st>>>(in, out, npix, h, w, c, w_hw, w_w, w_h, scale, shift, ppb);
  else
    idw_all_k<T, V, false><<<(unsigned)blocks, ppb * nv, 0, st>>>(in, out, npix, h, w, c, w_hw, w_w, w_h, scale, shift, ppb);
  return hipGetLastError();
}

template <class T, int V>
static hipError_t launch_idw_split(const uint16_t* in, uint16_t* out, int n, int h, int w, int c, const float* w_hw,
                                 const float* w_w, const float* w_h, const float* scale, const float* shift, bool pool,
                                 hipStream_t st) {
  const long npix = (long)n * (pool ? h / 2 : h) * (pool ? w / 2 : w);
  const int nv_id = 5 * (c / 8) / V, nv_cv = 3 * (c / 8) / V;
  const int ppb_id = IDW_T / nv_id, ppb_cv = IDW_T / nv_cv;
  const long blk_id = (npix + (long)ppb_id * IDW_K - 1) / ((long)ppb_id * IDW_K);
  const long blk_cv = (npix + (long)ppb_cv * IDW_K - 1) / ((long)ppb_cv * IDW_K);
  if (blk_id > 0x7fffffffL || blk_cv > 0x7fffffffL) return hipErrorInvalidValue;
  if (pool) {
    idw_id_k<T, V, true><<<(unsigned)blk_id, ppb_id * nv_id, 0, st>>>(in, out, npix, h, w, c, scale, shift, nv_id, ppb_id);
    idw_conv_k<T, V, true><<<(unsigned)blk_cv, ppb_cv * nv_cv, 0, st>>>(in, out, npix, h, w, c, w_hw, w_w, w_h, scale,
                                                                        shift, nv_cv, ppb_cv);
  } else {
    idw_id_k<T, V, false><<<(unsigned)blk_id, ppb_id * nv_id, 0, st>>>(in, out, npix, h, w, c, scale, shift, nv_id, ppb_id);
    idw_conv_k<T, V, false><<<(unsigned)blk_cv, ppb_cv * nv_cv, 0, st>>>(in, out, npix, h, w, c, w_hw, w_w, w_h, scale,
                                                                         shift, nv_cv, ppb_cv);
  }
  return hipGetLastError();
}

}  // namespace fac

extern "C" int fac_idwconv(int dtype, const void* in, void* out, int n, int h, int w, int c, const float* w_hw,
                           const float* w_w, const float* w_h, const float* scale, const float* shift, int pool,
                           void* stream) {
  using namespace fac;
  if (!in || !out || !w_hw || !w_w || !w_h || !scale || !shift || n <= 0 || (dtype != 0 && dtype != 1))
    return FAC_ERR_ARG;
  if (((uintptr_t)in | (uintptr_t)out) % 16) return FAC_ERR_ARG;
  if (c < 32 || c > 256 || c % 32 || h < 1 || w < 1 || h > 224 || w > 224) return FAC_ERR_SHAPE;
  if (pool && ((h | w) & 1)) return FAC_ERR_SHAPE;
  const uint16_t* i16 = (const uint16_t*)in;
  uint16_t* o16 = (uint16_t*)out;
  hipStream_t st = (hipStream_t)stream;
  const bool pl = pool != 0;
  hipError_t e;
  // the route depends on c alone, and both routes compute the same bits
  if (c >= IDW_SPLIT_C)   // multiples of 32 from 128: V = 8 when c % 64 == 0
    e = c % 64 == 0 ? (dtype == 0 ? launch_idw_split<BF16, 8>(i16, o16, n, h, w, c, w_hw, w_w, w_h, scale, shift, pl, st)
                                  : launch_idw_split<F16, 8>(i16, o16, n, h, w, c, w_hw, w_w, w_h, scale, shift, pl, st))
                    : (dtype == 0 ? launch_idw_split<BF16, 4>(i16, o16, n, h, w, c, w_hw, w_w, w_h, scale, shift, pl, st)
                                  : launch_idw_split<F16, 4>(i16, o16, n, h, w, c, w_hw, w_w, w_h, scale, shift, pl, st));
  else
    e = c % 64 == 0 ? (dtype == 0 ? launch_idw_all<BF16, 8>(i16, o16, n, h, w, c, w_hw, w_w, w_h, scale, shift, pl, st)
                                  : launch_idw_all<F16, 8>(i16, o16, n, h, w, c, w_hw, w_w, w_h, scale, shift, pl, st))
                    : (dtype == 0 ? launch_idw_all<BF16, 4>(i16, o16, n, h, w, c, w_hw, w_w, w_h, scale, shift, pl, st)
                                  : launch_idw_all<F16, 4>(i16, o16, n, h, w, c, w_hw, w_w, w_h, scale, shift, pl, st));
  if (e == hipErrorInvalidValue) return FAC_ERR_SHAPE;
  return e == hipSuccess ? FAC_OK : FAC_ERR_HIP;
}
