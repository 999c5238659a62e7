// ODConv2d(c, c, 3, padding 1) -> affine(scale, shift) -> optional ReLU ->
// optional 2x2 max-pool of CViT-main/model/other/cvit_GGCA_ADD_ODConv.py
// (:158-292, built with its defaults: kernel_num 4, reduction 1/16 with
// min_channel 16, temperature 1, no conv bias) on a 16-bit channels-last map
// [n][h][w][c], behind fac_odconv.
//
// The reference block, per crop b, in eval mode:
//   p   = mean over h x w of x[b]                                   [c]
//   hid = ReLU(bn_scale (fc p) + bn_shift)        fc [16][c]; BatchNorm2d(16) folded on the host
//   ca  = sigmoid(channel_fc hid + channel_b) [c]   fa = sigmoid(filter_fc hid + filter_b) [c]
//   sa  = sigmoid(spatial_fc hid + spatial_b) [9]   ka = softmax(kernel_fc hid + kernel_b) [4]
//   out[b,o,y,x] = fa[o] sum_tap sa[tap] sum_i (sum_k ka[k] W[k,o,i,tap]) ca[i] x[b,i,y+dy,x+dx]
// with zero padding.  This is the first block here whose conv weights differ
// per crop.
//
// Route A of the three the design names (B, four accumulator sets,
// and C, aggregation in LDS inside the conv, were not built): aggregate, then
// convolve with per-crop weights.  2 + 2 ceil(n / chunk) launches on one stream
// behind one call, nothing allocated:
//   odconv_mean_k   per (crop, chunk of 512 pixels): the chunk's channel sums,
//                   fp32, a thread's pixels in order, then the threads in order;
//   odconv_att_k    per crop: the chunks in order -> p; hid (16 lanes per
//                   output, a strided sum each, then the xor butterfly); the
//                   2c + 13 head logits, sigmoid / softmax -> ca | fa | sa | ka
//                   (scratch, and att_out);
//   per chunk of crops (od_chunk: as many crops as keep the aggregated weights
//   within OD_WS_BYTES):
//   odconv_agg_k    W^_b[o][tap][i] = sa[tap] ca[i] sum_k ka[k] W_k[o][i][tap] in
//                   fp32 from the fp32 W_k of the blob, rounded to 16 bits once,
//                   written in the MFMA's fragment order; a thread keeps its 32
//                   W_k values in registers for OD_AGG_CROPS crops, so the four
//                   W_k are read once per eight crops, not once per crop;
//   odconv_conv_k   implicit GEMM over K = (tap, input channel): a wave owns 32
//                   rows of ONE crop and 64 output channels, reads that crop's
//                   W^_b as the A operand and the raw 16-bit x as the B operand
//                   (ca and sa live in the weight, so x is not rounded again);
//                   epilogue act((acc fa) scale + shift); with pool the rows
//                   are ordered window by window and the max is two lane
//                   exchanges (scconv_out_k's).
// Row tiles are per crop (grid z = the crop), so no tile straddles a crop
// boundary; a crop of fewer than 32 rows leaves lanes idle.  Rows past the
// crop's end load its last row and store nothing.  A tap outside the map
// re-reads the row's own pixel and enters the MFMA as 0.  No LDS and no barrier
// in the conv: mdfa.hip's layout.
//
// Roundings to 16 bits, all declared (tests/odconv_ref.py emulates exactly
// these): the input; the AGGREGATED weight W^_b, once (the four W_k stay fp32
// in the blob and are never rounded); the output.  Everything else is fp32: the
// means, hid, the four attentions, fa, scale, shift, the aggregation and all
// accumulation.  Every reduction has a fixed order that depends on (h, w, c)
// alone and there are no atomics; a crop's values depend on no other crop and
// not on the chunk it falls in: its bits do not depend on n or on its position.
#include "common.hpp"
#include "fac_cvit.h"
#include "fac_ops.h"

namespace fac {

constexpr int OD_T = 256;             // threads per workgroup: 4 waves, 32 rows each
constexpr int OD_ROWS = 32;           // rows per wave
constexpr int OD_NT = 4;              // 16-channel column fragments per wave
constexpr int OD_COLS = OD_NT * 16;
constexpr int OD_MEAN_PIX = 512;      // pixels per workgroup in odconv_mean_k
constexpr int OD_HID = 16;            // the attention width for c = 64, 128, 256
constexpr int OD_KN = 4;              // kernel_num
constexpr int OD_AGG_CROPS = 8;       // crops a workgroup of odconv_agg_k aggregates per load of the four W_k
constexpr size_t OD_WS_BYTES = (size_t)48 << 20;   // bound of the aggregated-weight scratch

__host__ __device__ inline size_t od_up(size_t v) { return (v + 255) & ~(size_t)255; }
__host__ __device__ inline int od_quads(int c) { return 9 * c / 32; }          // MFMA K steps: 9 taps x c / 32
__host__ __device__ inline int od_natt(int c) { return 2 * c + 13; }           // ca | fa | sa | ka
__host__ __device__ inline int od_att_stride(int c) { return 2 * c + 16; }     // rows of the scratch copy, 16-byte aligned
__host__ __device__ inline int od_mean_parts(int hw) { return (hw + OD_MEAN_PIX - 1) / OD_MEAN_PIX; }
__host__ __device__ inline size_t od_wagg_elems(int c) { return (size_t)9 * c * c; }
// Crops whose aggregated weights are alive at once: 682 / 170 / 42 for c = 64 / 128 / 256.
__host__ __device__ inline int od_chunk(int n, int c) {
  const size_t fit = OD_WS_BYTES / (od_wagg_elems(c) * 2);
  return (size_t)n < fit ? n : (int)fit;
}

// The packed blob of fac_odconv_pack, byte offsets (all multiples of 256):
//   wf   fp32 [4 kernels][c / 64][od_quads][OD_NT][64 lanes][8]: lane l, element j of fragment (nb, q, tn) is,
//        for output channel co = nb * 64 + tn * 16 + (l & 15) and K chunk jj = 4 q + (l >> 4), W[k][co][ci][tap]
//        with tap = jj / (c / 8), ci = (jj % (c / 8)) * 8 + j
//   fp32: fc [16][c], bn_scale, bn_shift [16], channel_fc [c][16], channel_b [c], filter_fc [c][16], filter_b [c],
//        spatial_fc [9][16], spatial_b [9], kernel_fc [4][16], kernel_b [4], scale, shift [c]
struct OdBlob {
  size_t wf, fc, bns, bnb, cfc, cb, ffc, fb, sfc, sb, kfc, kb, scale, shift, bytes;
};

__host__ __device__ inline OdBlob od_blob(int c) {
  OdBlob b;
  size_t o = 0;
  b.wf = o;    o += od_up((size_t)OD_KN * od_wagg_elems(c) * 4);
  b.fc = o;    o += od_up((size_t)OD_HID * c * 4);
  b.bns = o;   o += od_up(OD_HID * 4);
  b.bnb = o;   o += od_up(OD_HID * 4);
  b.cfc = o;   o += od_up((size_t)c * OD_HID * 4);
  b.cb = o;    o += od_up((size_t)c * 4);
  b.ffc = o;   o += od_up((size_t)c * OD_HID * 4);
  b.fb = o;    o += od_up((size_t)c * 4);
  b.sfc = o;   o += od_up(9 * OD_HID * 4);
  b.sb = o;    o += od_up(9 * 4);
  b.kfc = o;   o += od_up(OD_KN * OD_HID * 4);
  b.kb = o;    o += od_up(OD_KN * 4);
  b.scale = o; o += od_up((size_t)c * 4);
  b.shift = o; o += od_up((size_t)c * 4);
  b.bytes = o;
  return b;
}

// fac_odconv's scratch, byte offsets (multiples of 256): mpart fp32 [n][mean parts][c]; att fp32 [n][2c + 16]
// (ca | fa | sa | ka | 3 unused); wagg 16-bit [od_chunk][9 c c] in the fragment order of the blob's wf
struct OdScratch {
  size_t mpart, att, wagg, bytes;
};

__host__ __device__ inline OdScratch od_scratch(int n, int h, int w, int c) {
  OdScratch s;
  size_t o = 0;
  s.mpart = o; o += od_up((size_t)n * od_mean_parts(h * w) * c * 4);
  s.att = o;   o += od_up((size_t)n * od_att_stride(c) * 4);
  s.wagg = o;  o += od_up((size_t)od_chunk(n, c) * od_wagg_elems(c) * 2);
  s.bytes = o;
  return s;
}

// grid (mean parts, n)
template <class T>
__global__ __launch_bounds__(OD_T) void odconv_mean_k(const uint16_t* __restrict__ x, float* __restrict__ mpart, int hw,
                                                     int c) {
  __shared__ float red[OD_T * 8];
  const int part = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int lpp = c / 8, ppi = OD_T / lpp;             // lanes per pixel (8 channels each), pixels per iteration
  const int sub = tid % lpp, pl = tid / lpp;
  const int p0 = part * OD_MEAN_PIX, npix = min(OD_MEAN_PIX, hw - p0);
  const uint16_t* xb = x + ((size_t)b * hw + p0) * c + sub * 8;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int p = pl; p < npix; p += ppi) {
    const u16x8 r = *(const u16x8*)(xb + (size_t)p * c);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += T::to_f32(r[j]);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[pl * c + sub * 8 + j] = acc[j];
  __syncthreads();
  if (tid < c) {
    float s = red[tid];
    for (int k = 1; k < ppi; ++k) s += red[k * c + tid];
    mpart[((size_t)b * gridDim.x + part) * c + tid] = s;
  }
}

// One workgroup per crop.
__global__ __launch_bounds__(OD_T) void odconv_att_k(const float* __restrict__ mpart, const float* __restrict__ fc,
                                                    const float* __restrict__ bns, const float* __restrict__ bnb,
                                                    const float* __restrict__ cfc, const float* __restrict__ cb,
                                                    const float* __restrict__ ffc, const float* __restrict__ fb,
                                                    const float* __restrict__ sfc, const float* __restrict__ sb,
                                                    const float* __restrict__ kfc, const float* __restrict__ kb,
                                                    float* __restrict__ att, float* __restrict__ att_out, int hw, int c,
                                                    int parts) {
  __shared__ float pm[256];
  __shared__ float hid[OD_HID];
  __shared__ float kl[OD_KN];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid < c) {
    float s = 0.f;
    for (int p = 0; p < parts; ++p) s += mpart[((size_t)b * parts + p) * c + tid];
    pm[tid] = s / (float)hw;
  }
  __syncthreads();
  {
    const int j = tid >> 4, l = tid & 15;            // 16 lanes per hidden unit
    float a = 0.f;
    for (int i = l; i < c; i += 16) a += fc[(size_t)j * c + i] * pm[i];
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
    if (l == 0) hid[j] = fmaxf(a * bns[j] + bnb[j], 0.f);
  }
  __syncthreads();
  const int natt = od_natt(c);
  float* ab = att + (size_t)b * od_att_stride(c);
  float* ao = att_out ? att_out + (size_t)b * natt : nullptr;
  for (int i = tid; i < natt; i += OD_T) {
    const float* wr;
    float z;
    if (i < c) {
      wr = cfc + (size_t)i * OD_HID;
      z = cb[i];
    } else if (i < 2 * c) {
      wr = ffc + (size_t)(i - c) * OD_HID;
      z = fb[i - c];
    } else if (i < 2 * c + 9) {
      wr = sfc + (i - 2 * c) * OD_HID;
      z = sb[i - 2 * c];
    } else {
      wr = kfc + (i - 2 * c - 9) * OD_HID;
      z = kb[i - 2 * c - 9];
    }
    float a = 0.f;
#pragma unroll
    for (int j = 0; j < OD_HID; ++j) a += wr[j] * hid[j];
    z += a;
    if (i < 2 * c + 9) {
      const float v = 1.f / (1.f + expf(-z));
      ab[i] = v;
      if (ao) ao[i] = v;
    } else {
      kl[i - 2 * c - 9] = z;
    }
  }
  __syncthreads();
  if (tid < OD_KN) {
    const float mx = fmaxf(fmaxf(kl[0], kl[1]), fmaxf(kl[2], kl[3]));
    const float e0 = expf(kl[0] - mx), e1 = expf(kl[1] - mx), e2 = expf(kl[2] - mx), e3 = expf(kl[3] - mx);
    const float den = ((e0 + e1) + e2) + e3;
    const float v = expf(kl[tid] - mx) / den;
    ab[2 * c + 9 + tid] = v;
    if (ao) ao[2 * c + 9 + tid] = v;
  }
}

// grid (9 c c / 8 / OD_T, ceil(nb / OD_AGG_CROPS)), nb = the crops of the chunk; a thread writes the eight
// elements of one lane of one fragment, for up to OD_AGG_CROPS crops
template <class T>
__global__ __launch_bounds__(OD_T) void odconv_agg_k(const float* __restrict__ wf, const float* __restrict__ att,
                                                    uint16_t* __restrict__ wagg, int c, int b0, int nb) {
  const size_t g = (size_t)blockIdx.x * OD_T + threadIdx.x;     // 9 c c / 8 is a multiple of OD_T for c >= 64
  const int cpt = c / 8;
  const int l = (int)(g & 63), q = (int)((g >> 8) % (size_t)od_quads(c));
  const int jj = 4 * q + (l >> 4), tap = jj / cpt, ci0 = (jj - tap * cpt) * 8;
  const size_t per = od_wagg_elems(c);
  const float* w = wf + g * 8;
  f32x4 wk[OD_KN][2];
#pragma unroll
  for (int k = 0; k < OD_KN; ++k)
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) wk[k][hh] = *(const f32x4*)(w + k * per + hh * 4);
  for (int r = 0; r < OD_AGG_CROPS; ++r) {
    const int lb = blockIdx.y * OD_AGG_CROPS + r;
    if (lb >= nb) break;
    const float* ab = att + (size_t)(b0 + lb) * od_att_stride(c);
    const float k0 = ab[2 * c + 9], k1 = ab[2 * c + 10], k2 = ab[2 * c + 11], k3 = ab[2 * c + 12];
    const float sa = ab[2 * c + tap];
    f32x4 v[2];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const f32x4 ca = *(const f32x4*)(ab + ci0 + hh * 4);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        v[hh][i] = ((((k0 * wk[0][hh][i] + k1 * wk[1][hh][i]) + k2 * wk[2][hh][i]) + k3 * wk[3][hh][i]) * sa) * ca[i];
    }
    const u16x4 lo = T::pack4(v[0]), hi = T::pack4(v[1]);
    *(u16x8*)(wagg + (size_t)lb * per + g * 8) = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  }
}

// grid (row tiles of 128 per crop, c / 64, crops of the chunk)
template <class T, int C>
__global__ __launch_bounds__(OD_T) void odconv_conv_k(const uint16_t* __restrict__ x, const uint16_t* __restrict__ wagg,
                                                     const float* __restrict__ att, const float* __restrict__ scale,
                                                     const float* __restrict__ shift, uint16_t* __restrict__ out, int H,
                                                     int W, int b0, int act, int pool) {
  constexpr int CPT = C / 8, QPT = CPT / 4, NQ = 9 * QPT;     // 8-channel chunks and MFMA K steps per tap
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int hw = H * W;
  const int r0 = (blockIdx.x * (OD_T / 64) + wave) * OD_ROWS;
  if (r0 >= hw) return;                        // no barrier below
  const int nb = blockIdx.y, lb = blockIdx.z, b = b0 + lb;
  int m[2], yy[2], xx[2], win[2];
  const uint16_t* xp[2];                       // the row's own pixel
  const uint16_t* xb = x + (size_t)b * hw * C;
#pragma unroll
  for (int rf = 0; rf < 2; ++rf) {
    m[rf] = r0 + rf * 16 + lr;
    const int p = m[rf] < hw ? m[rf] : hw - 1;
    if (pool) {                                // four consecutive rows are one 2x2 window
      const int wq = p >> 2, sub = p & 3, W2 = W >> 1;
      const int wy = wq / W2, wx = wq - wy * W2;
      yy[rf] = 2 * wy + (sub >> 1);
      xx[rf] = 2 * wx + (sub & 1);
      win[rf] = wq;
    } else {
      yy[rf] = p / W;
      xx[rf] = p - yy[rf] * W;
      win[rf] = 0;
    }
    xp[rf] = xb + ((size_t)yy[rf] * W + xx[rf]) * C + lg * 8;
  }
  f32x4 acc[2][OD_NT];
#pragma unroll
  for (int rf = 0; rf < 2; ++rf)
#pragma unroll
    for (int tn = 0; tn < OD_NT; ++tn) acc[rf][tn] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const u16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  const uint16_t* wp = wagg + (size_t)lb * (9 * C * C) + (size_t)nb * NQ * (OD_NT * 512) + lane * 8;
  for (int tap = 0; tap < 9; ++tap) {
    const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
    bool in[2];
    const uint16_t* tp[2];
#pragma unroll
    for (int rf = 0; rf < 2; ++rf) {
      in[rf] = (unsigned)(yy[rf] + dy) < (unsigned)H && (unsigned)(xx[rf] + dx) < (unsigned)W;
      tp[rf] = xp[rf] + (in[rf] ? (dy * W + dx) * C : 0);
    }
#pragma unroll
    for (int qq = 0; qq < QPT; ++qq) {
      u16x8 af[2];
#pragma unroll
      for (int rf = 0; rf < 2; ++rf) {
        const u16x8 v = *(const u16x8*)(tp[rf] + qq * 32);
        af[rf] = in[rf] ? v : zero;
      }
      const uint16_t* wq = wp + (size_t)(tap * QPT + qq) * (OD_NT * 512);
#pragma unroll
      for (int tn = 0; tn < OD_NT; ++tn) {
        const u16x8 wfr = *(const u16x8*)(wq + tn * 512);
        acc[0][tn] = T::mfma(wfr, af[0], acc[0][tn]);
        acc[1][tn] = T::mfma(wfr, af[1], acc[1][tn]);
      }
    }
  }
  // D[ch][row]: this lane has row lane & 15 of the fragment and channels nb * 64 + 16 tn + 4 (lane >> 4) + 0..3
  const float* fa = att + (size_t)b * od_att_stride(C) + C;
#pragma unroll
  for (int rf = 0; rf < 2; ++rf) {
#pragma unroll
    for (int tn = 0; tn < OD_NT; ++tn) {
      const int ch = nb * OD_COLS + tn * 16 + lg * 4;
      const f32x4 f = *(const f32x4*)(fa + ch), sc = *(const f32x4*)(scale + ch), sh = *(const f32x4*)(shift + ch);
      f32x4 v;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float t = (acc[rf][tn][i] * f[i]) * sc[i] + sh[i];
        v[i] = act ? relu(t) : t;
      }
      if (pool) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          v[i] = fmaxf(v[i], __shfl_xor(v[i], 1, 64));
          v[i] = fmaxf(v[i], __shfl_xor(v[i], 2, 64));
        }
        if ((lr & 3) == 0 && m[rf] < hw) *(u16x4*)(out + ((size_t)b * (hw >> 2) + win[rf]) * C + ch) = T::pack4(v);
      } else if (m[rf] < hw) {
        *(u16x4*)(out + ((size_t)b * hw + m[rf]) * C + ch) = T::pack4(v);
      }
    }
  }
}

static bool od_width_ok(int c) { return c == 64 || c == 128 || c == 256; }

static bool od_shape_ok(int h, int w, int c, int pool) {
  return od_width_ok(c) && h >= 2 && h <= 224 && w >= 2 && w <= 224 && (!pool || (h % 2 == 0 && w % 2 == 0));
}

template <class T, int C>
static void od_conv_launch(const uint16_t* x, const uint16_t* wagg, const float* att, const float* scale,
                           const float* shift, uint16_t* out, int h, int w, int b0, int nb, int relu, int pool,
                           hipStream_t st) {
  const unsigned tiles = (unsigned)((h * w + OD_ROWS * (OD_T / 64) - 1) / (OD_ROWS * (OD_T / 64)));
  odconv_conv_k<T, C><<<dim3(tiles, (unsigned)(C / OD_COLS), (unsigned)nb), OD_T, 0, st>>>(x, wagg, att, scale, shift, out,
                                                                                         h, w, b0, relu, pool);
}

template <class T>
static void od_launch(const uint16_t* x, int n, int h, int w, int c, const char* pk, int relu, int pool, uint16_t* out,
                      float* att_out, char* scr, hipStream_t st) {
  const OdBlob b = od_blob(c);
  const OdScratch s = od_scratch(n, h, w, c);
  const int hw = h * w, parts = od_mean_parts(hw), chunk = od_chunk(n, c);
  auto F = [&](size_t off) { return (const float*)(pk + off); };
  float *mpart = (float*)(scr + s.mpart), *att = (float*)(scr + s.att);
  uint16_t* wagg = (uint16_t*)(scr + s.wagg);
  odconv_mean_k<T><<<dim3((unsigned)parts, (unsigned)n), OD_T, 0, st>>>(x, mpart, hw, c);
  odconv_att_k<<<(unsigned)n, OD_T, 0, st>>>(mpart, F(b.fc), F(b.bns), F(b.bnb), F(b.cfc), F(b.cb), F(b.ffc), F(b.fb),
                                           F(b.sfc), F(b.sb), F(b.kfc), F(b.kb), att, att_out, hw, c, parts);
  const unsigned agg_blocks = (unsigned)(od_wagg_elems(c) / 8 / OD_T);
  for (int b0 = 0; b0 < n; b0 += chunk) {
    const int nb = n - b0 < chunk ? n - b0 : chunk;
    odconv_agg_k<T><<<dim3(agg_blocks, (unsigned)((nb + OD_AGG_CROPS - 1) / OD_AGG_CROPS)), OD_T, 0, st>>>(F(b.wf), att, wagg,
                                                                                                         c, b0, nb);
    if (c == 64) od_conv_launch<T, 64>(x, wagg, att, F(b.scale), F(b.shift), out, h, w, b0, nb, relu, pool, st);
    else if (c == 128) od_conv_launch<T, 128>(x, wagg, att, F(b.scale), F(b.shift), out, h, w, b0, nb, relu, pool, st);
    else od_conv_launch<T, 256>(x, wagg, att, F(b.scale), F(b.shift), out, h, w, b0, nb, relu, pool, st);
  }
}

}  // namespace fac

extern "C" size_t fac_odconv_packed_bytes(int c) { return fac::od_width_ok(c) ? fac::od_blob(c).bytes : 0; }

extern "C" int fac_odconv_chunk(int n, int c) { return n > 0 && fac::od_width_ok(c) ? fac::od_chunk(n, c) : 0; }

extern "C" size_t fac_odconv_scratch_bytes(int n, int h, int w, int c) {
  if (n <= 0 || !fac::od_shape_ok(h, w, c, 0) || (long)n * h * w > 0x3fffffffL || n > 65535) return 0;
  return fac::od_scratch(n, h, w, c).bytes;
}

extern "C" int fac_odconv_pack(int dtype, int c, const float* weight, const float* fc, const float* bn_scale,
                               const float* bn_shift, const float* channel_fc, const float* channel_b,
                               const float* filter_fc, const float* filter_b, const float* spatial_fc,
                               const float* spatial_b, const float* kernel_fc, const float* kernel_b, const float* scale,
                               const float* shift, void* out) {
  using namespace fac;
  if (!weight || !fc || !bn_scale || !bn_shift || !channel_fc || !channel_b || !filter_fc || !filter_b || !spatial_fc ||
      !spatial_b || !kernel_fc || !kernel_b || !scale || !shift || !out || (dtype != 0 && dtype != 1))
    return FAC_ERR_ARG;
  if (!od_width_ok(c)) return FAC_ERR_SHAPE;
  const OdBlob b = od_blob(c);
  char* base = (char*)out;
  __builtin_memset(base, 0, b.bytes);
  const int cpt = c / 8, NQ = od_quads(c);
  float* o = (float*)(base + b.wf);
  for (int k = 0; k < OD_KN; ++k)
    for (int nb = 0; nb < c / OD_COLS; ++nb)
      for (int q = 0; q < NQ; ++q)
        for (int tn = 0; tn < OD_NT; ++tn)
          for (int l = 0; l < 64; ++l) {
            const int co = nb * OD_COLS + tn * 16 + (l & 15), jj = q * 4 + (l >> 4);
            const int tap = jj / cpt, ci0 = (jj - tap * cpt) * 8;
            for (int j = 0; j < 8; ++j) *o++ = weight[(((size_t)k * c + co) * c + ci0 + j) * 9 + tap];
          }
  auto F = [&](size_t off) { return (float*)(base + off); };
  __builtin_memcpy(F(b.fc), fc, sizeof(float) * OD_HID * c);
  __builtin_memcpy(F(b.bns), bn_scale, sizeof(float) * OD_HID);
  __builtin_memcpy(F(b.bnb), bn_shift, sizeof(float) * OD_HID);
  __builtin_memcpy(F(b.cfc), channel_fc, sizeof(float) * c * OD_HID);
  __builtin_memcpy(F(b.cb), channel_b, sizeof(float) * c);
  __builtin_memcpy(F(b.ffc), filter_fc, sizeof(float) * c * OD_HID);
  __builtin_memcpy(F(b.fb), filter_b, sizeof(float) * c);
  __builtin_memcpy(F(b.sfc), spatial_fc, sizeof(float) * 9 * OD_HID);
  __builtin_memcpy(F(b.sb), spatial_b, sizeof(float) * 9);
  __builtin_memcpy(F(b.kfc), kernel_fc, sizeof(float) * OD_KN * OD_HID);
  __builtin_memcpy(F(b.kb), kernel_b, sizeof(float) * OD_KN);
  __builtin_memcpy(F(b.scale), scale, sizeof(float) * c);
  __builtin_memcpy(F(b.shift), shift, sizeof(float) * c);
  return FAC_OK;
}

extern "C" int fac_odconv(int dtype, const void* x, int n, int h, int w, int c, const void* packed, int relu, int pool,
                          void* out, float* att_out, void* scratch, void* stream) {
  using namespace fac;
  if (!x || !packed || !out || !scratch || n <= 0 || (dtype != 0 && dtype != 1) || (pool != 0 && pool != 1) ||
      (relu != 0 && relu != 1))
    return FAC_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)packed | (uintptr_t)out | (uintptr_t)scratch) % 16 || (uintptr_t)att_out % 4)
    return FAC_ERR_ARG;
  if (!od_shape_ok(h, w, c, pool)) return FAC_ERR_SHAPE;
  if ((long)n * h * w > 0x3fffffffL || n > 65535) return FAC_ERR_SHAPE;   // n is a grid's y
  const size_t bytes = (size_t)n * h * w * c * 2, obytes = pool ? bytes / 4 : bytes;
  const uintptr_t xb = (uintptr_t)x, ob = (uintptr_t)out;
  if (xb < ob + obytes && ob < xb + bytes) return FAC_ERR_ARG;           // not in place
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0)
    od_launch<BF16>((const uint16_t*)x, n, h, w, c, (const char*)packed, relu, pool, (uint16_t*)out, att_out,
                    (char*)scratch, st);
  else
    od_launch<F16>((const uint16_t*)x, n, h, w, c, (const char*)packed, relu, pool, (uint16_t*)out, att_out, (char*)scratch,
                   st);
  return hipGetLastError() == hipSuccess ? FAC_OK : FAC_ERR_HIP;
}
