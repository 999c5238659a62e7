// MDFA(c, c) of CViT-main/model/other/cvit_GGCA4_MDFA5.py (:158-261) on a
// 16-bit channels-last map [n][h][w][c] with 7 <= h, w <= 14, behind fac_mdfa.
//
// The reference block: four conv branches of the same map (a 1x1 and three 3x3
// with padding = dilation = 6, 12, 18), each conv -> BatchNorm -> ReLU; a fifth
// branch, the crop's channel means through a 1x1 conv, BN and ReLU, broadcast
// over the map; cat = [b1 b2 b3 b4 g] (5c channels); larry = max(cat * t_b,
// cat * s_p) with s_p = sigmoid(w_s . cat_p) per pixel and t_b = ReLU(w_t .
// mean_p cat_p) per crop; out = ReLU(BN(conv_cat(larry * cat))).
//
// What is computed here is the same function, smaller:
//   * a dilated tap at (dy, dx) with |dy| >= h or |dx| >= w is outside the map
//     for every pixel and is dropped when the launch is planned (20 of the 28
//     taps stay at 14x14, 12 at 7x7); the rest take bfm.hip's per-row in-map
//     test, and a row tile with no in-map row skips the tap, wave-uniformly;
//   * cat >= 0 after the ReLUs, so max(cat t, cat s) = cat max(t, s) exactly,
//     larry * cat = m_p cat^2 with ONE scalar m_p = max(t_b, s_p) per pixel,
//     which commutes with the 1x1 conv_cat:
//       out = ReLU(m_p (W'cat . cat_p^2) + b'cat);
//   * branch 5 is one vector g_b per crop, so its share of conv_cat is a
//     vector e_b = W'cat[:, 4c:5c] g_b^2 added in the epilogue and its shares
//     of the two dots are two scalars per crop: the GEMM has K = 4c.
//
// Four launches on one stream behind one call, nothing allocated:
//   mdfa_crop_k    per crop: channel means of x, g_b, e_b and g's shares of the
//                  two dots (fp32 throughout, one workgroup per crop);
//   mdfa_branch_k  implicit GEMM, rows = pixels of the flattened batch, columns
//                  = the 4c branch channels (a wave's 64 columns lie in one
//                  branch), K = (kept tap, c); + bias, ReLU in fp32; writes q =
//                  cat^2 rounded to 16 bits and, per pixel and 64-column tile,
//                  the partial dots w_s . cat and w_t . cat from the fp32 cat;
//   mdfa_gate_k    per crop: sums the partial dots in column-tile order, t_b
//                  over the crop's pixels, m_p per pixel;
//   mdfa_cat_k     GEMM [n h w, 4c] x [4c, c] on q; epilogue
//                  ReLU(m_p (acc + e_b) + b'cat), ONE rounding at the store.
// Fusing the last three through LDS is the next step; it is not done here.
//
// GEMM layout: bfm.hip's.  No LDS and no barrier: a wave owns 32 rows x 64
// columns, the weight is the MFMA's A operand packed in fragment order (a
// wave's fragment is one contiguous 1 KiB read), the activation the B operand,
// so a lane holds four consecutive channels of one row.  Rows span crops; a tap
// outside the map re-reads the row's own pixel (an address inside x) and enters
// the MFMA as 0.  Rows past the end load row M - 1 and store nothing.
//
// Rounding: 16-bit input and folded branch / conv_cat[:, :4c] weights; branch
// sums, bias, ReLU fp32; both dots, the crop means, g_b, e_b, t_b, the sigmoid
// and m_p fp32 from the fp32 cat, every sum in a fixed order, no atomics: a
// crop's bits do not depend on n.  q = cat^2 is rounded once to 16 bits (fp16:
// clamped to 65504, the largest finite value, so no inf or NaN is produced for
// cat above 255.9).  The output is rounded once at the store.
#include "common.hpp"
#include "fac_cvit.h"
#include "fac_ops.h"

namespace fac {

constexpr int MDFA_T = 256;        // threads per workgroup: 4 waves, 32 rows each
constexpr int MDFA_ROWS = 32;      // rows per wave
constexpr int MDFA_NT = 4;         // 16-channel column fragments per wave
constexpr int MDFA_COLS = MDFA_NT * 16;
constexpr int MDFA_TAPS = 1 + 9 + 9 + 9;
constexpr float F16_MAX = 65504.f;

// The packed blob of fac_mdfa_pack, byte offsets (all multiples of 256):
//   wbr   16-bit [28 taps][c / 64][c / 32][MDFA_NT][64 lanes][8]: tap 0 is
//         branch 1, taps 1 + 9 (b - 2) + 3 ky + kx branch b's; lane l, element j
//         of fragment (tap, nb, kc, tn) is w[nb * 64 + tn * 16 + (l & 15)][kc * 32 + (l >> 4) * 8 + j][tap]
//   wcat  16-bit [c / 64][4c / 32][MDFA_NT][64][8], the same order over W'cat[:, :4c]
//   fp32: bias4 [4][c]; w5t [c in][c out]; b5 [c]; wcat5t [c in][c out] =
//         W'cat[:, 4c:5c] transposed; bcat [c]; ws [5c]; wt [5c]
struct MdfaBlob {
  size_t wbr, wcat, bias4, w5t, b5, wcat5t, bcat, ws, wt, bytes;
};

__host__ __device__ inline MdfaBlob mdfa_blob(int c) {
  const size_t cc = (size_t)c * c;
  MdfaBlob b;
  size_t o = 0;
  b.wbr = o;    o += MDFA_TAPS * cc * 2;
  b.wcat = o;   o += 4 * cc * 2;
  b.bias4 = o;  o += 4 * (size_t)c * 4;
  b.w5t = o;    o += cc * 4;
  b.b5 = o;     o += (size_t)c * 4;
  b.wcat5t = o; o += cc * 4;
  b.bcat = o;   o += (size_t)c * 4;
  b.ws = o;     o += 5 * (size_t)c * 4;
  b.wt = o;     o += 5 * (size_t)c * 4;   // c >= 64: every section is a multiple of 256 bytes
  b.bytes = o;
  return b;
}

// fac_mdfa's scratch, byte offsets (multiples of 256): q 16-bit [M][4c];
// ps, pt fp32 [M][4c / 64]; m fp32 [M]; e fp32 [n][c]; gs, gt fp32 [n]
struct MdfaScratch {
  size_t q, ps, pt, m, e, gs, gt, bytes;
};

__host__ __device__ inline size_t mdfa_up(size_t v) { return (v + 255) & ~(size_t)255; }

__host__ __device__ inline MdfaScratch mdfa_scratch(int n, int h, int w, int c) {
  const size_t M = (size_t)n * h * w, nct = (size_t)(4 * c / MDFA_COLS);
  MdfaScratch s;
  size_t o = 0;
  s.q = o;  o += mdfa_up(M * 4 * c * 2);
  s.ps = o; o += mdfa_up(M * nct * 4);
  s.pt = o; o += mdfa_up(M * nct * 4);
  s.m = o;  o += mdfa_up(M * 4);
  s.e = o;  o += mdfa_up((size_t)n * c * 4);
  s.gs = o; o += mdfa_up((size_t)n * 4);
  s.gt = o; o += mdfa_up((size_t)n * 4);
  s.bytes = o;
  return s;
}

// Sum over the workgroup in a fixed order: every thread's value to LDS, wave 0
// adds four of them per lane in index order, then the xor butterfly.
__device__ __forceinline__ float mdfa_block_sum(float v, float* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  float s = 0.f;
  if (threadIdx.x < 64) {
    s = ((red[threadIdx.x] + red[threadIdx.x + 64]) + red[threadIdx.x + 128]) + red[threadIdx.x + 192];
    s = wave_sum(s);
  }
  return s;   // valid in wave 0
}

// One workgroup per crop.
template <class T>
__global__ __launch_bounds__(MDFA_T) void mdfa_crop_k(const uint16_t* __restrict__ x, const float* __restrict__ w5t,
                                                     const float* __restrict__ b5, const float* __restrict__ wcat5t,
                                                     const float* __restrict__ ws5, const float* __restrict__ wt5,
                                                     float* __restrict__ e, float* __restrict__ gs,
                                                     float* __restrict__ gt, int hw, int c) {
  __shared__ float mean[512], g2[512], red[MDFA_T];
  const int b = blockIdx.x, tid = threadIdx.x;
  const uint16_t* xb = x + (size_t)b * hw * c;
  for (int j = tid; j < c; j += MDFA_T) {
    float s = 0.f;
    for (int p = 0; p < hw; ++p) s += T::to_f32(xb[(size_t)p * c + j]);
    mean[j] = s / (float)hw;
  }
  __syncthreads();
  float ds = 0.f, dt = 0.f;
  for (int j = tid; j < c; j += MDFA_T) {
    float s = 0.f;
    for (int i = 0; i < c; ++i) s += w5t[(size_t)i * c + j] * mean[i];
    const float g = relu(s + b5[j]);
    g2[j] = g * g;
    ds += ws5[j] * g;
    dt += wt5[j] * g;
  }
  const float sds = mdfa_block_sum(ds, red);
  const float sdt = mdfa_block_sum(dt, red);
  if (tid == 0) {
    gs[b] = sds;
    gt[b] = sdt;
  }
  __syncthreads();
  for (int j = tid; j < c; j += MDFA_T) {
    float s = 0.f;
    for (int i = 0; i < c; ++i) s += wcat5t[(size_t)i * c + j] * g2[i];
    e[(size_t)b * c + j] = s;
  }
}

template <class T>
__device__ __forceinline__ void mdfa_tap(const uint16_t* __restrict__ xa0, const uint16_t* __restrict__ xa1, bool in0,
                                         bool in1, const uint16_t* __restrict__ wp, int KC, f32x4 (&acc)[2][MDFA_NT]) {
  const u16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 2
  for (int kc = 0; kc < KC; ++kc) {
    u16x8 af[2];
    af[0] = *(const u16x8*)(xa0 + kc * 32);
    af[1] = *(const u16x8*)(xa1 + kc * 32);
    af[0] = in0 ? af[0] : zero;
    af[1] = in1 ? af[1] : zero;
    const size_t wo = (size_t)kc * (MDFA_NT * 512);
#pragma unroll
    for (int tn = 0; tn < MDFA_NT; ++tn) {
      const u16x8 wf = *(const u16x8*)(wp + wo + tn * 512);
      acc[0][tn] = T::mfma(wf, af[0], acc[0][tn]);
      acc[1][tn] = T::mfma(wf, af[1], acc[1][tn]);
    }
  }
}

// grid (row tiles of 128, 4c / 64): blockIdx.y = branch * (c / 64) + column block
template <class T>
__global__ __launch_bounds__(MDFA_T, 2) void mdfa_branch_k(const uint16_t* __restrict__ x,
                                                         const uint16_t* __restrict__ wbr,
                                                         const float* __restrict__ bias4, const float* __restrict__ ws,
                                                         const float* __restrict__ wt, uint16_t* __restrict__ q,
                                                         float* __restrict__ ps, float* __restrict__ pt, int M, int H,
                                                         int W, int c) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lk = (lane >> 4) * 8;
  const long r0 = ((long)blockIdx.x * (MDFA_T / 64) + wave) * MDFA_ROWS;
  if (r0 >= M) return;                         // no barrier below
  const int KC = c >> 5, NB = c / MDFA_COLS;
  const int br = blockIdx.y / NB, nb = blockIdx.y - br * NB;      // branch 0..3
  const int hw = H * W;
  int m[2], yy[2], xx[2];
  const uint16_t* xp[2];                       // the row's own pixel, this lane's k offset
#pragma unroll
  for (int rf = 0; rf < 2; ++rf) {
    m[rf] = (int)r0 + rf * 16 + lr;
    const int mc = m[rf] < M ? m[rf] : M - 1;
    const int p = mc % hw;
    yy[rf] = p / W;
    xx[rf] = p - yy[rf] * W;
    xp[rf] = x + (size_t)mc * c + lk;
  }
  f32x4 acc[2][MDFA_NT];
#pragma unroll
  for (int rf = 0; rf < 2; ++rf)
#pragma unroll
    for (int tn = 0; tn < MDFA_NT; ++tn) acc[rf][tn] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const size_t frag = (size_t)KC * (MDFA_NT * 512);            // elements per (tap, column block)
  const uint16_t* wb = wbr + lane * 8;
  if (br == 0) {
    mdfa_tap<T>(xp[0], xp[1], true, true, wb + (size_t)nb * frag, KC, acc);
  } else {
    const int d = 6 * br;
    for (int ky = -1; ky <= 1; ++ky) {
      const int dy = ky * d;
      if (dy >= H || -dy >= H) continue;       // outside the map for every pixel
      for (int kx = -1; kx <= 1; ++kx) {
        const int dx = kx * d;
        if (dx >= W || -dx >= W) continue;
        const int off = (dy * W + dx) * c;     // elements; used only where the tap is inside the row's own map
        bool in[2];
        const uint16_t* xa[2];
#pragma unroll
        for (int rf = 0; rf < 2; ++rf) {
          in[rf] = (unsigned)(yy[rf] + dy) < (unsigned)H && (unsigned)(xx[rf] + dx) < (unsigned)W;
          xa[rf] = xp[rf] + (in[rf] ? off : 0);
        }
        if (!__any(in[0] || in[1])) continue;  // wave-uniform: no row of this tile sees the tap
        const int tap = 1 + 9 * (br - 1) + (ky + 1) * 3 + kx + 1;
        mdfa_tap<T>(xa[0], xa[1], in[0], in[1], wb + ((size_t)tap * NB + nb) * frag, KC, acc);
      }
    }
  }

  // D[ch][row]: this lane has row lane & 15 of the fragment and channels nb * 64 + 16 tn + 4 (lane >> 4) + 0..3
  const int C4 = 4 * c, nct = C4 / MDFA_COLS;
#pragma unroll
  for (int rf = 0; rf < 2; ++rf) {
    float ds = 0.f, dt = 0.f;
#pragma unroll
    for (int tn = 0; tn < MDFA_NT; ++tn) {
      const int ch = br * c + nb * MDFA_COLS + tn * 16 + (lane >> 4) * 4;
      const f32x4 bb = *(const f32x4*)(bias4 + ch), vs = *(const f32x4*)(ws + ch), vt = *(const f32x4*)(wt + ch);
      f32x4 v;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float cat = relu(acc[rf][tn][i] + bb[i]);
        ds += vs[i] * cat;
        dt += vt[i] * cat;
        const float sq = cat * cat;
        v[i] = T::id == 1 ? fminf(sq, F16_MAX) : sq;
      }
      if (m[rf] < M) *(u16x4*)(q + (size_t)m[rf] * C4 + ch) = T::pack4(v);
    }
    // the four lane groups of a row, in a fixed order
    ds += __shfl_xor(ds, 16, 64);
    dt += __shfl_xor(dt, 16, 64);
    ds += __shfl_xor(ds, 32, 64);
    dt += __shfl_xor(dt, 32, 64);
    if (lane < 16 && m[rf] < M) {
      ps[(size_t)m[rf] * nct + blockIdx.y] = ds;
      pt[(size_t)m[rf] * nct + blockIdx.y] = dt;
    }
  }
}

// One workgroup per crop: z_p = sum over column tiles in order, + g's share.
__global__ __launch_bounds__(MDFA_T) void mdfa_gate_k(const float* __restrict__ ps, const float* __restrict__ pt,
                                                     const float* __restrict__ gs, const float* __restrict__ gt,
                                                     float* __restrict__ mm, int hw, int nct) {
  __shared__ float red[MDFA_T];
  __shared__ float tb;
  const int b = blockIdx.x, tid = threadIdx.x;
  float zs = 0.f, zt = 0.f;                    // hw <= 196 < MDFA_T: one pixel per thread
  if (tid < hw) {
    const size_t r = ((size_t)b * hw + tid) * nct;
    for (int k = 0; k < nct; ++k) {
      zs += ps[r + k];
      zt += pt[r + k];
    }
  }
  const float tot = mdfa_block_sum(zt, red);
  if (tid == 0) tb = relu(tot / (float)hw + gt[b]);
  __syncthreads();
  if (tid < hw) {
    const float s = 1.f / (1.f + __expf(-(zs + gs[b])));
    mm[(size_t)b * hw + tid] = fmaxf(tb, s);
  }
}

// grid (row tiles of 128, c / 64)
template <class T>
__global__ __launch_bounds__(MDFA_T, 2) void mdfa_cat_k(const uint16_t* __restrict__ q, const uint16_t* __restrict__ wcat,
                                                      const float* __restrict__ bcat, const float* __restrict__ e,
                                                      const float* __restrict__ mm, uint16_t* __restrict__ out, int M,
                                                      int hw, int c) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lk = (lane >> 4) * 8;
  const long r0 = ((long)blockIdx.x * (MDFA_T / 64) + wave) * MDFA_ROWS;
  if (r0 >= M) return;
  const int C4 = 4 * c, KC = C4 >> 5, nb = blockIdx.y;
  int m[2], mc[2];
  const uint16_t* qp[2];
#pragma unroll
  for (int rf = 0; rf < 2; ++rf) {
    m[rf] = (int)r0 + rf * 16 + lr;
    mc[rf] = m[rf] < M ? m[rf] : M - 1;
    qp[rf] = q + (size_t)mc[rf] * C4 + lk;
  }
  f32x4 acc[2][MDFA_NT];
#pragma unroll
  for (int rf = 0; rf < 2; ++rf)
#pragma unroll
    for (int tn = 0; tn < MDFA_NT; ++tn) acc[rf][tn] = (f32x4){0.f, 0.f, 0.f, 0.f};
  mdfa_tap<T>(qp[0], qp[1], true, true, wcat + (size_t)nb * KC * (MDFA_NT * 512) + lane * 8, KC, acc);
#pragma unroll
  for (int rf = 0; rf < 2; ++rf) {
    if (m[rf] >= M) continue;
    const float mp = mm[m[rf]];
    const float* eb = e + (size_t)(m[rf] / hw) * c;
#pragma unroll
    for (int tn = 0; tn < MDFA_NT; ++tn) {
      const int ch = nb * MDFA_COLS + tn * 16 + (lane >> 4) * 4;
      const f32x4 ev = *(const f32x4*)(eb + ch), bv = *(const f32x4*)(bcat + ch);
      f32x4 v;
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = relu(mp * (acc[rf][tn][i] + ev[i]) + bv[i]);
      *(u16x4*)(out + (size_t)m[rf] * c + ch) = T::pack4(v);
    }
  }
}

static bool mdfa_width_ok(int c) { return c == 64 || c == 128 || c == 256 || c == 512; }

static bool mdfa_shape_ok(int h, int w, int c) { return h >= 7 && h <= 14 && w >= 7 && w <= 14 && mdfa_width_ok(c); }

static uint16_t mdfa_h16(int dtype, float v) { return dtype == 0 ? fac_host::f32_to_bf16(v) : fac_host::f32_to_f16(v); }

// [co][ci] (element stride `es`, row stride `rs`) -> fragment order [co / 64][ci / 32][MDFA_NT][64][8]
static uint16_t* mdfa_pack_frag(int dtype, const float* w, int co_n, int ci_n, size_t rs, size_t es, uint16_t* o) {
  for (int nb = 0; nb < co_n / MDFA_COLS; ++nb)
    for (int kc = 0; kc < ci_n / 32; ++kc)
      for (int tn = 0; tn < MDFA_NT; ++tn)
        for (int l = 0; l < 64; ++l) {
          const int co = nb * MDFA_COLS + tn * 16 + (l & 15), ci0 = kc * 32 + (l >> 4) * 8;
          for (int j = 0; j < 8; ++j) *o++ = mdfa_h16(dtype, w[(size_t)co * rs + (size_t)(ci0 + j) * es]);
        }
  return o;
}

template <class T>
static void mdfa_launch(const uint16_t* x, int n, int h, int w, int c, const char* pk, uint16_t* out, char* scr,
                        hipStream_t st) {
  const MdfaBlob b = mdfa_blob(c);
  const MdfaScratch s = mdfa_scratch(n, h, w, c);
  const int hw = h * w, M = n * hw, nct = 4 * c / MDFA_COLS;
  auto F = [&](size_t off) { return (const float*)(pk + off); };
  float *e = (float*)(scr + s.e), *gs = (float*)(scr + s.gs), *gt = (float*)(scr + s.gt);
  float *ps = (float*)(scr + s.ps), *pt = (float*)(scr + s.pt), *mm = (float*)(scr + s.m);
  uint16_t* q = (uint16_t*)(scr + s.q);
  const unsigned tiles = (unsigned)((M + MDFA_ROWS * (MDFA_T / 64) - 1) / (MDFA_ROWS * (MDFA_T / 64)));
  mdfa_crop_k<T><<<n, MDFA_T, 0, st>>>(x, F(b.w5t), F(b.b5), F(b.wcat5t), F(b.ws) + 4 * c, F(b.wt) + 4 * c, e, gs, gt,
                                       hw, c);
  mdfa_branch_k<T><<<dim3(tiles, (unsigned)nct), MDFA_T, 0, st>>>(x, (const uint16_t*)(pk + b.wbr), F(b.bias4), F(b.ws),
                                                                F(b.wt), q, ps, pt, M, h, w, c);
  mdfa_gate_k<<<n, MDFA_T, 0, st>>>(ps, pt, gs, gt, mm, hw, nct);
  mdfa_cat_k<T><<<dim3(tiles, (unsigned)(c / MDFA_COLS)), MDFA_T, 0, st>>>(q, (const uint16_t*)(pk + b.wcat), F(b.bcat),
                                                                         e, mm, out, M, hw, c);
}

}  // namespace fac

extern "C" size_t fac_mdfa_packed_bytes(int c) { return fac::mdfa_width_ok(c) ? fac::mdfa_blob(c).bytes : 0; }

extern "C" size_t fac_mdfa_scratch_bytes(int n, int h, int w, int c) {
  if (n <= 0 || !fac::mdfa_shape_ok(h, w, c) || (long)n * h * w > 0x3fffffffL) return 0;
  return fac::mdfa_scratch(n, h, w, c).bytes;
}

extern "C" int fac_mdfa_pack(int dtype, int c, const float* w1, const float* w2, const float* w3, const float* w4,
                             const float* bias4, const float* w5, const float* b5, const float* wcat,
                             const float* bcat, const float* ws, const float* wt, void* out) {
  using namespace fac;
  if (!w1 || !w2 || !w3 || !w4 || !bias4 || !w5 || !b5 || !wcat || !bcat || !ws || !wt || !out ||
      (dtype != 0 && dtype != 1))
    return FAC_ERR_ARG;
  if (!mdfa_width_ok(c)) return FAC_ERR_SHAPE;
  const MdfaBlob b = mdfa_blob(c);
  char* base = (char*)out;
  uint16_t* o = (uint16_t*)(base + b.wbr);
  o = mdfa_pack_frag(dtype, w1, c, c, (size_t)c, 1, o);
  const float* w3x3[3] = {w2, w3, w4};
  for (int br = 0; br < 3; ++br)
    for (int tap = 0; tap < 9; ++tap) o = mdfa_pack_frag(dtype, w3x3[br] + tap, c, c, (size_t)c * 9, 9, o);
  mdfa_pack_frag(dtype, wcat, c, 4 * c, (size_t)5 * c, 1, (uint16_t*)(base + b.wcat));
  auto F = [&](size_t off) { return (float*)(base + off); };
  __builtin_memcpy(F(b.bias4), bias4, sizeof(float) * 4 * c);
  __builtin_memcpy(F(b.b5), b5, sizeof(float) * c);
  __builtin_memcpy(F(b.bcat), bcat, sizeof(float) * c);
  __builtin_memcpy(F(b.ws), ws, sizeof(float) * 5 * c);
  __builtin_memcpy(F(b.wt), wt, sizeof(float) * 5 * c);
  for (int i = 0; i < c; ++i)
    for (int j = 0; j < c; ++j) {
      F(b.w5t)[(size_t)i * c + j] = w5[(size_t)j * c + i];
      F(b.wcat5t)[(size_t)i * c + j] = wcat[(size_t)j * 5 * c + 4 * c + i];
    }
  return FAC_OK;
}

extern "C" int fac_mdfa(int dtype, const void* x, int n, int h, int w, int c, const void* packed, void* out,
                        void* scratch, void* stream) {
  using namespace fac;
  if (!x || !packed || !out || !scratch || n <= 0 || (dtype != 0 && dtype != 1)) return FAC_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)packed | (uintptr_t)out | (uintptr_t)scratch) % 16) return FAC_ERR_ARG;
  if (!mdfa_shape_ok(h, w, c)) return FAC_ERR_SHAPE;
  if ((long)n * h * w > 0x3fffffffL) return FAC_ERR_SHAPE;           // rows x 4c are indexed in 32 bits per row
  const size_t bytes = (size_t)n * h * w * c * 2;
  const uintptr_t xb = (uintptr_t)x, ob = (uintptr_t)out;
  if (xb < ob + bytes && ob < xb + bytes) return FAC_ERR_ARG;      // the branch kernel reads halos: not in place
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0)
    mdfa_launch<BF16>((const uint16_t*)x, n, h, w, c, (const char*)packed, (uint16_t*)out, (char*)scratch, st);
  else
    mdfa_launch<F16>((const uint16_t*)x, n, h, w, c, (const char*)packed, (uint16_t*)out, (char*)scratch, st);
  return hipGetLastError() == hipSuccess ? FAC_OK : FAC_ERR_HIP;
}
