// ScConv(c) -> affine(scale, shift) -> ReLU -> optional 2x2 max-pool of
// CViT-main/model/other/cvit_GGCA_ADD_ScConv.py (:311-353, built with its
// defaults) on a 16-bit channels-last map [n][h][w][c], behind fac_scconv.
//
// The reference block, per crop:
//   1. GroupNorm(4, c), eps 1e-5: t = gamma_c (x - mu_g) rstd_g + beta_c, the
//      statistics over a group's c/4 channels x h x w (biased variance);
//   2. gate: z = t k_c with k_c = gamma_c / sum(gamma), r = sigmoid(z);
//      w1 = 1, w2 = 0 where r > 0.5 (in exact arithmetic: z > 0), else w1 =
//      w2 = r; with c' = c +- c/2 the partner channel,
//      y[c] = w1[c] x[c] + w2[c'] x[c'];
//   3. u = squeeze1 y[:c/2], l = squeeze2 y[c/2:] (1x1, c/2 -> c/4, no bias);
//   4. Y1 = GWC(u) + PWC1(u) (GWC: 3x3, padding 1, 2 groups, bias), Y2 =
//      cat[PWC2(l), l];
//   5. s = softmax over the 2c per-crop means of cat[Y1, Y2]; the result is
//      s[:c] Y1 + s[c:] Y2.
//
// The means of step 5 are linear in u and l: mean(Y2) is [PWC2; I] mean(l),
// and the sum of a zero-padded 3x3 conv over the map is, per tap (dy, dx), the
// sum of u minus its last / first row (dy = -1 / +1) and last / first column
// (dx = -1 / +1) plus the corner both took away.  So s is known before any Y
// is formed and scales the two accumulators of the last launch's epilogue.
//
// Route A of the two the design names (route B, recomputing gate
// and squeeze on a halo in LDS, was not built).  Six launches on one stream
// behind one call, nothing allocated:
//   scconv_stat_k    per (crop, group, chunk of pixels): the chunk's mean and
//                    centred sum of squares, the chunk held in registers for
//                    the second pass;
//   scconv_stat2_k   per (crop, group): the chunks merged in chunk order
//                    (Chan's pairwise update) -> mu_g, rstd_g; stats_out;
//   scconv_gate_k    gate + both squeezes.  Rows = pixels of the flattened
//                    batch, a wave owns 32 rows and all c/2 outputs; a lane
//                    gates exactly the eight (channel, partner) pairs of its
//                    MFMA B fragment, so y never leaves registers; writes
//                    ul = [u | l] [n h w][c/2] in 16 bits;
//   scconv_mean_k    per (crop, chunk of 1024 pixels): sums of ul over the
//                    chunk, its first / last row and first / last column;
//   scconv_soft_k    per crop: the chunks in order, the tap sums, the 2c means
//                    with the weights the GEMM uses, the softmax -> s [n][2c];
//   scconv_out_k     implicit GEMM, a wave owns 32 rows x 64 output channels
//                    and two accumulators: Y1 over K = (tap, group channels) +
//                    (PWC1 channels) and Y2 over K = c/4 against [PWC2; I];
//                    epilogue ReLU((s1 (Y1 + b) + s2 Y2) scale + shift); with
//                    pool the rows are ordered window by window (four
//                    consecutive rows = one 2x2 window) and the max is two
//                    lane exchanges.
// The map crosses HBM as: x read twice (statistics, gate), ul (half a map)
// written once and read twice (means; the GEMM, its halo from cache), the
// output written once.  Folding scconv_mean_k's sums into scconv_gate_k is the
// next step; it is not done here.
//
// GEMM layout: mdfa.hip's.  No LDS and no barrier in the two GEMM kernels: the
// weight is the MFMA's A operand packed in fragment order, the activation the B
// operand, so a lane holds eight consecutive channels of one row.  A tap outside
// the map re-reads the row's own pixel (an address inside ul) and enters the
// MFMA as 0.  Rows past the end load row M - 1 and store nothing.  For c = 64 a
// wave's 64 columns span both GWC groups, so there GWC is packed as a dense
// c/4 -> c conv with zeros across the groups.
//
// Variance: two passes over the chunk cached in registers (sum -> chunk mean,
// then the sum of (x - mean)^2), and Chan's update between chunks, so a mean
// that is large against the deviation (post-ReLU maps) costs no digits.  The
// in-chunk sums are fp32 in a fixed order; the merge of a group's few chunks and
// 1 / sqrt(var + eps) run in double in one thread, then round to fp32.
//
// Roundings to 16 bits, all declared (tests/scconv_ref.py emulates exactly
// these): the input and the five conv weights (packed); y, the gated map, as
// the squeeze MFMA's operand; u | l at the store; the output.  Everything else
// is fp32: t, z, the sigmoid, the gate (z > 0), all sums, the means (from the
// 16-bit u | l and the 16-bit weights, so s belongs to the Y that is formed),
// the softmax, the epilogue.  Every reduction has a fixed order that depends on
// (h, w, c) alone and there are no atomics: a crop's bits do not depend on n or
// on its position in the batch.
#include "common.hpp"
#include "fac_cvit.h"
#include "fac_ops.h"

namespace fac {

constexpr int SC_T = 256;           // threads per workgroup: 4 waves, 32 rows each
constexpr int SC_ROWS = 32;         // rows per wave
constexpr int SC_NT = 4;            // 16-channel column fragments per wave in scconv_out_k
constexpr int SC_COLS = SC_NT * 16;
constexpr int SC_STAT_IT = 8;       // 16-byte loads per thread in scconv_stat_k
constexpr int SC_MEAN_PIX = 1024;   // pixels per workgroup in scconv_mean_k
constexpr double SC_EPS = 1e-5;

__host__ __device__ inline size_t sc_up(size_t v) { return (v + 255) & ~(size_t)255; }

// Channels of u that one wave of scconv_out_k reads per tap, and where they start.
__host__ __device__ inline int sc_gin(int c) { return c == 64 ? c / 4 : c / 8; }
// 8-channel K chunks of the Y1 GEMM: 9 taps x sc_gin / 8, then PWC1's c/4 / 8; in quads of 4 (one MFMA).
__host__ __device__ inline int sc_chunks(int c) { return 9 * (sc_gin(c) / 8) + c / 32; }
__host__ __device__ inline int sc_quads(int c) { return (sc_chunks(c) + 3) / 4; }
__host__ __device__ inline int sc_quads2(int c) { return (c / 4 + 31) / 32; }

// The packed blob of fac_scconv_pack, byte offsets (all multiples of 256):
//   wsq   16-bit [2 halves][c / 64][c / 64][64 lanes][8]: lane l, element j of fragment (half, kc, tn) is
//         squeeze{half + 1}[tn * 16 + (l & 15)][kc * 32 + (l >> 4) * 8 + j]
//   wy1   16-bit [c / 64][sc_quads][SC_NT][64][8]: lane l, element j of (nb, q, tn) is, for output channel co =
//         nb * 64 + tn * 16 + (l & 15) and chunk jj = 4 q + (l >> 4): GWC[co][.][tap] of chunk jj's channel (zero
//         across groups), PWC1[co][.] for the chunks after the taps, zero for the padding chunks
//   wy2   16-bit [c / 64][sc_quads2][SC_NT][64][8] over [PWC2; I] [c][c / 4], zero past K = c / 4
//   fp32: gamma, beta, kc, scale, shift, gwc_b [c]; the 16-bit values of GWC [c][c/8][9], PWC1 [c][c/4] and
//         PWC2 [3c/4][c/4] as fp32, for the means
struct ScBlob {
  size_t wsq, wy1, wy2, gamma, beta, kc, scale, shift, gwcb, gwcf, pwc1f, pwc2f, bytes;
};

__host__ __device__ inline ScBlob sc_blob(int c) {
  ScBlob b;
  size_t o = 0;
  b.wsq = o;   o += sc_up((size_t)2 * (c / 4) * (c / 2) * 2);
  b.wy1 = o;   o += sc_up((size_t)c * sc_quads(c) * 32 * 2);
  b.wy2 = o;   o += sc_up((size_t)c * sc_quads2(c) * 32 * 2);
  b.gamma = o; o += sc_up((size_t)c * 4);
  b.beta = o;  o += sc_up((size_t)c * 4);
  b.kc = o;    o += sc_up((size_t)c * 4);
  b.scale = o; o += sc_up((size_t)c * 4);
  b.shift = o; o += sc_up((size_t)c * 4);
  b.gwcb = o;  o += sc_up((size_t)c * 4);
  b.gwcf = o;  o += sc_up((size_t)c * (c / 8) * 9 * 4);
  b.pwc1f = o; o += sc_up((size_t)c * (c / 4) * 4);
  b.pwc2f = o; o += sc_up((size_t)(3 * c / 4) * (c / 4) * 4);
  b.bytes = o;
  return b;
}

__host__ __device__ inline int sc_stat_pix(int c) { return SC_T / (c / 32) * SC_STAT_IT; }   // pixels per chunk
__host__ __device__ inline int sc_stat_parts(int hw, int c) { return (hw + sc_stat_pix(c) - 1) / sc_stat_pix(c); }
__host__ __device__ inline int sc_mean_parts(int hw) { return (hw + SC_MEAN_PIX - 1) / SC_MEAN_PIX; }

// fac_scconv's scratch, byte offsets (multiples of 256): spart fp32 [n][4][stat parts][2] (mean, centred
// sum of squares); stats fp32 [n][4][2] (mu, rstd); ul 16-bit [n h w][c / 2]; mpart fp32 [n][mean parts][5]
// [c / 2] (sum over the chunk, row 0, row h - 1, column 0, column w - 1); s fp32 [n][2c]
struct ScScratch {
  size_t spart, stats, ul, mpart, s, bytes;
};

__host__ __device__ inline ScScratch sc_scratch(int n, int h, int w, int c) {
  const size_t hw = (size_t)h * w;
  ScScratch s;
  size_t o = 0;
  s.spart = o; o += sc_up((size_t)n * 4 * sc_stat_parts((int)hw, c) * 2 * 4);
  s.stats = o; o += sc_up((size_t)n * 4 * 2 * 4);
  s.ul = o;    o += sc_up((size_t)n * hw * (c / 2) * 2);
  s.mpart = o; o += sc_up((size_t)n * sc_mean_parts((int)hw) * 5 * (c / 2) * 4);
  s.s = o;     o += sc_up((size_t)n * 2 * c * 4);
  s.bytes = o;
  return s;
}

// Sum over the workgroup in a fixed order, returned to every thread: every
// thread's value to LDS, wave 0 adds four of them per lane in index order, then
// the xor butterfly.  red: SC_T + 1 floats.
__device__ __forceinline__ float sc_block_sum(float v, float* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  if (threadIdx.x < 64) {
    float s = ((red[threadIdx.x] + red[threadIdx.x + 64]) + red[threadIdx.x + 128]) + red[threadIdx.x + 192];
    s = wave_sum(s);
    if (threadIdx.x == 0) red[SC_T] = s;
  }
  __syncthreads();
  return red[SC_T];
}

// grid (stat parts, 4 groups, n)
template <class T>
__global__ __launch_bounds__(SC_T) void scconv_stat_k(const uint16_t* __restrict__ x, float* __restrict__ spart, int hw,
                                                     int c) {
  __shared__ float red[SC_T + 1];
  const int part = blockIdx.x, g = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int lpp = c / 32, ppi = SC_T / lpp;            // lanes per pixel (8 channels each), pixels per iteration
  const int sub = tid % lpp, pl = tid / lpp;
  const int p0 = part * ppi * SC_STAT_IT;
  const int npix = min(ppi * SC_STAT_IT, hw - p0);
  const uint16_t* xb = x + (size_t)b * hw * c + (size_t)g * (c / 4) + sub * 8;
  float v[SC_STAT_IT][8];
  float sum = 0.f;
#pragma unroll
  for (int it = 0; it < SC_STAT_IT; ++it) {
    const int p = it * ppi + pl;
    const bool in = p < npix;
    u16x8 r = {0, 0, 0, 0, 0, 0, 0, 0};
    if (in) r = *(const u16x8*)(xb + (size_t)(p0 + p) * c);
    float s8 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[it][j] = T::to_f32(r[j]);
      s8 += v[it][j];
    }
    sum += s8;
  }
  const float cnt = (float)npix * (float)(c / 4);
  const float mean = sc_block_sum(sum, red) / cnt;
  float m2 = 0.f;
#pragma unroll
  for (int it = 0; it < SC_STAT_IT; ++it) {
    const bool in = it * ppi + pl < npix;
    float s8 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = v[it][j] - mean;
      s8 += d * d;
    }
    m2 += in ? s8 : 0.f;
  }
  m2 = sc_block_sum(m2, red);
  if (tid == 0) {
    float* o = spart + (((size_t)b * 4 + g) * gridDim.x + part) * 2;
    o[0] = mean;
    o[1] = m2;
  }
}

// one thread per (crop, group)
__global__ void scconv_stat2_k(const float* __restrict__ spart, float* __restrict__ stats, float* __restrict__ stats_out,
                               int n4, int hw, int c, int parts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const int chunk = sc_stat_pix(c);
  double na = 0.0, mean = 0.0, m2 = 0.0;
  for (int p = 0; p < parts; ++p) {
    const double nb = (double)min(chunk, hw - p * chunk) * (double)(c / 4);
    const double mb = spart[((size_t)i * parts + p) * 2], qb = spart[((size_t)i * parts + p) * 2 + 1];
    const double d = mb - mean, nn = na + nb;
    mean += d * (nb / nn);
    m2 += qb + d * d * (na * nb / nn);
    na = nn;
  }
  const float mu = (float)mean, rstd = (float)(1.0 / sqrt(m2 / na + SC_EPS));
  stats[(size_t)i * 2] = mu;
  stats[(size_t)i * 2 + 1] = rstd;
  if (stats_out) {
    stats_out[(size_t)i * 2] = mu;
    stats_out[(size_t)i * 2 + 1] = rstd;
  }
}

// y for the eight channels k0 .. k0 + 7 of the upper half (xa) and their partners in the lower half (xb)
template <class T>
__device__ __forceinline__ void sc_gate8(u16x8 xa, u16x8 xb, float mua, float rsa, float mub, float rsb,
                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                         const float* __restrict__ kcv, int k0, int half, u16x8& yup, u16x8& ylo) {
  float yu[8], yl[8];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const f32x4 ga = *(const f32x4*)(gamma + k0 + 4 * q), gb = *(const f32x4*)(gamma + half + k0 + 4 * q);
    const f32x4 ba = *(const f32x4*)(beta + k0 + 4 * q), bb = *(const f32x4*)(beta + half + k0 + 4 * q);
    const f32x4 ka = *(const f32x4*)(kcv + k0 + 4 * q), kb = *(const f32x4*)(kcv + half + k0 + 4 * q);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = 4 * q + i;
      const float a = T::to_f32(xa[j]), bv = T::to_f32(xb[j]);
      const float za = (((a - mua) * rsa) * ga[i] + ba[i]) * ka[i];
      const float zb = (((bv - mub) * rsb) * gb[i] + bb[i]) * kb[i];
      const float ra = 1.f / (1.f + __expf(-za)), rb = 1.f / (1.f + __expf(-zb));
      const float w1a = za > 0.f ? 1.f : ra, w2a = za > 0.f ? 0.f : ra;
      const float w1b = zb > 0.f ? 1.f : rb, w2b = zb > 0.f ? 0.f : rb;
      yu[j] = w1a * a + w2b * bv;
      yl[j] = w1b * bv + w2a * a;
    }
  }
  const u16x4 u0 = T::pack4((f32x4){yu[0], yu[1], yu[2], yu[3]}), u1 = T::pack4((f32x4){yu[4], yu[5], yu[6], yu[7]});
  const u16x4 l0 = T::pack4((f32x4){yl[0], yl[1], yl[2], yl[3]}), l1 = T::pack4((f32x4){yl[4], yl[5], yl[6], yl[7]});
  yup = __builtin_shufflevector(u0, u1, 0, 1, 2, 3, 4, 5, 6, 7);
  ylo = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// grid (row tiles of 128); C: the width, NF = C / 64 fragments of 16 outputs per half and K chunks of 32
template <class T, int C>
__global__ __launch_bounds__(SC_T) void scconv_gate_k(const uint16_t* __restrict__ x, const float* __restrict__ stats,
                                                     const uint16_t* __restrict__ wsq, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, const float* __restrict__ kcv,
                                                     uint16_t* __restrict__ ul, int M, int hw) {
  constexpr int NF = C / 64, HALF = C / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lk = (lane >> 4) * 8;
  const long r0 = ((long)blockIdx.x * (SC_T / 64) + wave) * SC_ROWS;
  if (r0 >= M) return;                         // no barrier below
  int m[2];
  const uint16_t* xp[2];
  const float* sp[2];
#pragma unroll
  for (int rf = 0; rf < 2; ++rf) {
    m[rf] = (int)r0 + rf * 16 + lr;
    const int mc = m[rf] < M ? m[rf] : M - 1;
    xp[rf] = x + (size_t)mc * C + lk;
    sp[rf] = stats + (size_t)(mc / hw) * 8;
  }
  f32x4 au[2][NF], al[2][NF];
#pragma unroll
  for (int rf = 0; rf < 2; ++rf)
#pragma unroll
    for (int tn = 0; tn < NF; ++tn) au[rf][tn] = al[rf][tn] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const uint16_t* wu = wsq + lane * 8;
  const uint16_t* wl = wsq + (size_t)NF * NF * 512 + lane * 8;
#pragma unroll
  for (int kc = 0; kc < NF; ++kc) {
    const int k0 = kc * 32 + lk;               // a channel of the upper half; its group is 0 or 1, the partner's 2 or 3
    const int ga = k0 / (C / 4);
    u16x8 yu[2], yl[2];
#pragma unroll
    for (int rf = 0; rf < 2; ++rf) {
      const u16x8 xa = *(const u16x8*)(xp[rf] + kc * 32), xb = *(const u16x8*)(xp[rf] + HALF + kc * 32);
      sc_gate8<T>(xa, xb, sp[rf][2 * ga], sp[rf][2 * ga + 1], sp[rf][4 + 2 * ga], sp[rf][5 + 2 * ga], gamma, beta, kcv,
                  k0, HALF, yu[rf], yl[rf]);
    }
#pragma unroll
    for (int tn = 0; tn < NF; ++tn) {
      const u16x8 fu = *(const u16x8*)(wu + (size_t)(kc * NF + tn) * 512);
      const u16x8 fl = *(const u16x8*)(wl + (size_t)(kc * NF + tn) * 512);
#pragma unroll
      for (int rf = 0; rf < 2; ++rf) {
        au[rf][tn] = T::mfma(fu, yu[rf], au[rf][tn]);
        al[rf][tn] = T::mfma(fl, yl[rf], al[rf][tn]);
      }
    }
  }
  // D[ch][row]: this lane has row lane & 15 of the fragment and channels 16 tn + 4 (lane >> 4) + 0..3
#pragma unroll
  for (int rf = 0; rf < 2; ++rf) {
    if (m[rf] >= M) continue;
    uint16_t* o = ul + (size_t)m[rf] * HALF + (lane >> 4) * 4;
#pragma unroll
    for (int tn = 0; tn < NF; ++tn) {
      *(u16x4*)(o + tn * 16) = T::pack4(au[rf][tn]);
      *(u16x4*)(o + C / 4 + tn * 16) = T::pack4(al[rf][tn]);
    }
  }
}

// grid (mean parts, n)
template <class T>
__global__ __launch_bounds__(SC_T) void scconv_mean_k(const uint16_t* __restrict__ ul, float* __restrict__ mpart, int H,
                                                     int W, int c) {
  __shared__ float red[5][SC_T];
  const int part = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int ch2 = c / 2, npl = SC_T / ch2;
  const int ch = tid % ch2, pl = tid / ch2;
  const int hw = H * W, p0 = part * SC_MEAN_PIX, p1 = min(p0 + SC_MEAN_PIX, hw);
  const uint16_t* ub = ul + (size_t)b * hw * ch2 + ch;
  float tot = 0.f, r0 = 0.f, rl = 0.f, c0 = 0.f, cl = 0.f;
  for (int p = p0 + pl; p < p1; p += npl) {
    const float v = T::to_f32(ub[(size_t)p * ch2]);
    const int y = p / W, xx = p - y * W;
    tot += v;
    r0 += y == 0 ? v : 0.f;
    rl += y == H - 1 ? v : 0.f;
    c0 += xx == 0 ? v : 0.f;
    cl += xx == W - 1 ? v : 0.f;
  }
  red[0][tid] = tot;
  red[1][tid] = r0;
  red[2][tid] = rl;
  red[3][tid] = c0;
  red[4][tid] = cl;
  __syncthreads();
  if (pl == 0) {
    float* o = mpart + ((size_t)b * gridDim.x + part) * 5 * ch2 + ch;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      float s = red[q][ch];
      for (int k = 1; k < npl; ++k) s += red[q][k * ch2 + ch];
      o[(size_t)q * ch2] = s;
    }
  }
}

// One workgroup per crop.
template <class T>
__global__ __launch_bounds__(SC_T) void scconv_soft_k(const uint16_t* __restrict__ ul, const float* __restrict__ mpart,
                                                     const float* __restrict__ gwcf, const float* __restrict__ pwc1f,
                                                     const float* __restrict__ pwc2f, const float* __restrict__ gwcb,
                                                     float* __restrict__ sout, int H, int W, int c, int parts) {
  __shared__ float sums[5][128];      // per channel of ul: total, row 0, row H - 1, column 0, column W - 1
  __shared__ float corner[4][64];     // u at (0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)
  __shared__ float S[9][64];          // per tap, the sum of u over the pixels the tap reads inside the map
  __shared__ float logit[512];
  __shared__ float red[SC_T + 1];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int ch2 = c / 2, c4 = c / 4, c8 = c / 8, hw = H * W;
  const float inv = 1.f / (float)hw;
  for (int ch = tid; ch < ch2; ch += SC_T)
    for (int q = 0; q < 5; ++q) {
      float s = 0.f;
      for (int p = 0; p < parts; ++p) s += mpart[(((size_t)b * parts + p) * 5 + q) * ch2 + ch];
      sums[q][ch] = s;
    }
  const uint16_t* ub = ul + (size_t)b * hw * ch2;
  for (int i = tid; i < 4 * c4; i += SC_T) {
    const int k = i / c4, ch = i - k * c4;
    const int y = k < 2 ? 0 : H - 1, xx = (k & 1) ? W - 1 : 0;
    corner[k][ch] = T::to_f32(ub[(size_t)(y * W + xx) * ch2 + ch]);
  }
  __syncthreads();
  for (int i = tid; i < 9 * c4; i += SC_T) {
    const int tap = i / c4, ch = i - tap * c4;
    const int ky = tap / 3, kx = tap - ky * 3;
    float s = sums[0][ch];
    s -= ky == 0 ? sums[2][ch] : 0.f;          // dy = -1 never reads the last row
    s -= ky == 2 ? sums[1][ch] : 0.f;          // dy = +1 never reads the first row
    s -= kx == 0 ? sums[4][ch] : 0.f;
    s -= kx == 2 ? sums[3][ch] : 0.f;
    if (ky != 1 && kx != 1) s += corner[(ky == 0 ? 2 : 0) + (kx == 0 ? 1 : 0)][ch];
    S[tap][ch] = s;
  }
  __syncthreads();
  for (int co = tid; co < c; co += SC_T) {
    const int gb = (co / ch2) * c8;
    float a = 0.f;
    for (int ci = 0; ci < c8; ++ci)
      for (int tap = 0; tap < 9; ++tap) a += gwcf[((size_t)co * c8 + ci) * 9 + tap] * S[tap][gb + ci];
    for (int ci = 0; ci < c4; ++ci) a += pwc1f[(size_t)co * c4 + ci] * sums[0][ci];
    logit[co] = a * inv + gwcb[co];
    float l2;
    if (co < 3 * c4) {
      l2 = 0.f;
      for (int ci = 0; ci < c4; ++ci) l2 += pwc2f[(size_t)co * c4 + ci] * sums[0][c4 + ci];
    } else {
      l2 = sums[0][c4 + co - 3 * c4];
    }
    logit[c + co] = l2 * inv;
  }
  __syncthreads();
  float mx = -3.4e38f;
  for (int i = tid; i < 2 * c; i += SC_T) mx = fmaxf(mx, logit[i]);
  __syncthreads();
  red[tid] = mx;
  __syncthreads();
  if (tid == 0) {
    float t = red[0];
    for (int i = 1; i < SC_T; ++i) t = fmaxf(t, red[i]);
    red[SC_T] = t;
  }
  __syncthreads();
  mx = red[SC_T];
  float e[2] = {0.f, 0.f}, part = 0.f;         // 2c <= 512: at most two values per thread
  for (int k = 0; k < 2; ++k) {
    const int i = tid + k * SC_T;
    if (i < 2 * c) e[k] = expf(logit[i] - mx);
    part += e[k];
  }
  const float den = sc_block_sum(part, red);
  for (int k = 0; k < 2; ++k) {
    const int i = tid + k * SC_T;
    if (i < 2 * c) sout[(size_t)b * 2 * c + i] = e[k] / den;
  }
}

// grid (row tiles of 128, c / 64)
template <class T>
__global__ __launch_bounds__(SC_T) void scconv_out_k(const uint16_t* __restrict__ ul, const uint16_t* __restrict__ wy1,
                                                      const uint16_t* __restrict__ wy2, const float* __restrict__ sv,
                                                      const float* __restrict__ gwcb, const float* __restrict__ scale,
                                                      const float* __restrict__ shift, uint16_t* __restrict__ out, int M,
                                                      int H, int W, int c, int pool) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const long r0 = ((long)blockIdx.x * (SC_T / 64) + wave) * SC_ROWS;
  if (r0 >= M) return;                         // no barrier below
  const int hw = H * W, ch2 = c / 2, c4 = c / 4, nb = blockIdx.y;
  const int gin = sc_gin(c), cpt = gin / 8, ntap = 9 * cpt, nch = sc_chunks(c), NQ = sc_quads(c), NQ2 = sc_quads2(c);
  const int gbase = c == 64 ? 0 : (nb * SC_COLS / ch2) * gin;
  int m[2], yy[2], xx[2], bb[2], win[2];
  const uint16_t* up[2];                       // the row's own pixel in ul
#pragma unroll
  for (int rf = 0; rf < 2; ++rf) {
    m[rf] = (int)r0 + rf * 16 + lr;
    const int mc = m[rf] < M ? m[rf] : M - 1;
    bb[rf] = mc / hw;
    const int p = mc - bb[rf] * hw;
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
    up[rf] = ul + ((size_t)bb[rf] * hw + (size_t)yy[rf] * W + xx[rf]) * ch2;
  }
  f32x4 a1[2][SC_NT], a2[2][SC_NT];
#pragma unroll
  for (int rf = 0; rf < 2; ++rf)
#pragma unroll
    for (int tn = 0; tn < SC_NT; ++tn) a1[rf][tn] = a2[rf][tn] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const u16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};

  const uint16_t* w1p = wy1 + (size_t)nb * NQ * (SC_NT * 512) + lane * 8;
  for (int q = 0; q < NQ; ++q) {
    const int jj = q * 4 + lg;                 // this lane group's 8-channel chunk
    int dy = 0, dx = 0, chan = 0;
    bool live = jj < nch;
    if (jj < ntap) {
      const int tap = jj / cpt;
      dy = tap / 3 - 1;
      dx = tap - (tap / 3) * 3 - 1;
      chan = gbase + (jj - tap * cpt) * 8;
    } else if (live) {
      chan = (jj - ntap) * 8;                  // PWC1: every channel of u, the row's own pixel
    }
    u16x8 af[2];
#pragma unroll
    for (int rf = 0; rf < 2; ++rf) {
      const bool in = live && (unsigned)(yy[rf] + dy) < (unsigned)H && (unsigned)(xx[rf] + dx) < (unsigned)W;
      const u16x8 v = *(const u16x8*)(up[rf] + (in ? (dy * W + dx) * ch2 : 0) + chan);
      af[rf] = in ? v : zero;
    }
#pragma unroll
    for (int tn = 0; tn < SC_NT; ++tn) {
      const u16x8 wf = *(const u16x8*)(w1p + ((size_t)q * SC_NT + tn) * 512);
      a1[0][tn] = T::mfma(wf, af[0], a1[0][tn]);
      a1[1][tn] = T::mfma(wf, af[1], a1[1][tn]);
    }
  }
  const uint16_t* w2p = wy2 + (size_t)nb * NQ2 * (SC_NT * 512) + lane * 8;
  for (int q = 0; q < NQ2; ++q) {
    const int k = q * 32 + lg * 8;
    const bool in = k < c4;
    u16x8 af[2];
#pragma unroll
    for (int rf = 0; rf < 2; ++rf) {
      const u16x8 v = *(const u16x8*)(up[rf] + c4 + (in ? k : 0));
      af[rf] = in ? v : zero;
    }
#pragma unroll
    for (int tn = 0; tn < SC_NT; ++tn) {
      const u16x8 wf = *(const u16x8*)(w2p + ((size_t)q * SC_NT + tn) * 512);
      a2[0][tn] = T::mfma(wf, af[0], a2[0][tn]);
      a2[1][tn] = T::mfma(wf, af[1], a2[1][tn]);
    }
  }

  // D[ch][row]: this lane has row lane & 15 of the fragment and channels nb * 64 + 16 tn + 4 (lane >> 4) + 0..3
#pragma unroll
  for (int rf = 0; rf < 2; ++rf) {
    const float* sb = sv + (size_t)bb[rf] * 2 * c;
#pragma unroll
    for (int tn = 0; tn < SC_NT; ++tn) {
      const int ch = nb * SC_COLS + tn * 16 + lg * 4;
      const f32x4 s1 = *(const f32x4*)(sb + ch), s2 = *(const f32x4*)(sb + c + ch);
      const f32x4 bg = *(const f32x4*)(gwcb + ch), sc = *(const f32x4*)(scale + ch), sh = *(const f32x4*)(shift + ch);
      f32x4 v;
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = relu((s1[i] * (a1[rf][tn][i] + bg[i]) + s2[i] * a2[rf][tn][i]) * sc[i] + sh[i]);
      if (pool) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          v[i] = fmaxf(v[i], __shfl_xor(v[i], 1, 64));
          v[i] = fmaxf(v[i], __shfl_xor(v[i], 2, 64));
        }
        if ((lr & 3) == 0 && m[rf] < M)
          *(u16x4*)(out + ((size_t)bb[rf] * (hw >> 2) + win[rf]) * c + ch) = T::pack4(v);
      } else if (m[rf] < M) {
        *(u16x4*)(out + (size_t)m[rf] * c + ch) = T::pack4(v);
      }
    }
  }
}

static bool sc_width_ok(int c) { return c == 64 || c == 128 || c == 256; }

static bool sc_shape_ok(int h, int w, int c, int pool) {
  return sc_width_ok(c) && h >= 2 && h <= 224 && w >= 2 && w <= 224 && (!pool || (h % 2 == 0 && w % 2 == 0));
}

static float sc_r16(int dtype, float v) {
  if (dtype == 0) {
    const uint32_t u = (uint32_t)fac_host::f32_to_bf16(v) << 16;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
  }
  return (float)(_Float16)v;
}

static uint16_t sc_h16(int dtype, float v) { return dtype == 0 ? fac_host::f32_to_bf16(v) : fac_host::f32_to_f16(v); }

template <class T, int C>
static void sc_gate_launch(const uint16_t* x, const float* stats, const char* pk, const ScBlob& b, uint16_t* ul, int M,
                           int hw, unsigned tiles, hipStream_t st) {
  scconv_gate_k<T, C><<<tiles, SC_T, 0, st>>>(x, stats, (const uint16_t*)(pk + b.wsq), (const float*)(pk + b.gamma),
                                              (const float*)(pk + b.beta), (const float*)(pk + b.kc), ul, M, hw);
}

template <class T>
static void sc_launch(const uint16_t* x, int n, int h, int w, int c, const char* pk, int pool, uint16_t* out,
                      float* stats_out, char* scr, hipStream_t st) {
  const ScBlob b = sc_blob(c);
  const ScScratch s = sc_scratch(n, h, w, c);
  const int hw = h * w, M = n * hw, sparts = sc_stat_parts(hw, c), mparts = sc_mean_parts(hw);
  auto F = [&](size_t off) { return (const float*)(pk + off); };
  float *spart = (float*)(scr + s.spart), *stats = (float*)(scr + s.stats), *mpart = (float*)(scr + s.mpart);
  float* sv = (float*)(scr + s.s);
  uint16_t* ul = (uint16_t*)(scr + s.ul);
  const unsigned tiles = (unsigned)((M + SC_ROWS * (SC_T / 64) - 1) / (SC_ROWS * (SC_T / 64)));
  scconv_stat_k<T><<<dim3((unsigned)sparts, 4, (unsigned)n), SC_T, 0, st>>>(x, spart, hw, c);
  scconv_stat2_k<<<(unsigned)((n * 4 + 63) / 64), 64, 0, st>>>(spart, stats, stats_out, n * 4, hw, c, sparts);
  if (c == 64) sc_gate_launch<T, 64>(x, stats, pk, b, ul, M, hw, tiles, st);
  else if (c == 128) sc_gate_launch<T, 128>(x, stats, pk, b, ul, M, hw, tiles, st);
  else sc_gate_launch<T, 256>(x, stats, pk, b, ul, M, hw, tiles, st);
  scconv_mean_k<T><<<dim3((unsigned)mparts, (unsigned)n), SC_T, 0, st>>>(ul, mpart, h, w, c);
  scconv_soft_k<T><<<(unsigned)n, SC_T, 0, st>>>(ul, mpart, F(b.gwcf), F(b.pwc1f), F(b.pwc2f), F(b.gwcb), sv, h, w, c,
                                                mparts);
  scconv_out_k<T><<<dim3(tiles, (unsigned)(c / SC_COLS)), SC_T, 0, st>>>(ul, (const uint16_t*)(pk + b.wy1),
                                                                       (const uint16_t*)(pk + b.wy2), sv, F(b.gwcb),
                                                                       F(b.scale), F(b.shift), out, M, h, w, c, pool);
}

}  // namespace fac

extern "C" size_t fac_scconv_packed_bytes(int c) { return fac::sc_width_ok(c) ? fac::sc_blob(c).bytes : 0; }

extern "C" size_t fac_scconv_scratch_bytes(int n, int h, int w, int c) {
  if (n <= 0 || !fac::sc_shape_ok(h, w, c, 0) || (long)n * h * w > 0x3fffffffL || n > 65535) return 0;
  return fac::sc_scratch(n, h, w, c).bytes;
}

extern "C" int fac_scconv_pack(int dtype, int c, const float* gamma, const float* beta, const float* kc,
                               const float* squeeze1, const float* squeeze2, const float* gwc_w, const float* gwc_b,
                               const float* pwc1, const float* pwc2, const float* scale, const float* shift, void* out) {
  using namespace fac;
  if (!gamma || !beta || !kc || !squeeze1 || !squeeze2 || !gwc_w || !gwc_b || !pwc1 || !pwc2 || !scale || !shift ||
      !out || (dtype != 0 && dtype != 1))
    return FAC_ERR_ARG;
  if (!sc_width_ok(c)) return FAC_ERR_SHAPE;
  const ScBlob b = sc_blob(c);
  char* base = (char*)out;
  __builtin_memset(base, 0, b.bytes);
  const int c2 = c / 2, c4 = c / 4, c8 = c / 8, nf = c / 64;
  uint16_t* o = (uint16_t*)(base + b.wsq);
  for (int half = 0; half < 2; ++half) {
    const float* w = half ? squeeze2 : squeeze1;           // [c4][c2]
    for (int kcn = 0; kcn < nf; ++kcn)
      for (int tn = 0; tn < nf; ++tn)
        for (int l = 0; l < 64; ++l)
          for (int j = 0; j < 8; ++j)
            *o++ = sc_h16(dtype, w[(size_t)(tn * 16 + (l & 15)) * c2 + kcn * 32 + (l >> 4) * 8 + j]);
  }
  const int gin = sc_gin(c), cpt = gin / 8, ntap = 9 * cpt, nch = sc_chunks(c), NQ = sc_quads(c), NQ2 = sc_quads2(c);
  o = (uint16_t*)(base + b.wy1);
  for (int nb = 0; nb < c / SC_COLS; ++nb)
    for (int q = 0; q < NQ; ++q)
      for (int tn = 0; tn < SC_NT; ++tn)
        for (int l = 0; l < 64; ++l) {
          const int co = nb * SC_COLS + tn * 16 + (l & 15), jj = q * 4 + (l >> 4), g = co / c2;
          const int gbase = c == 64 ? 0 : g * gin;
          for (int j = 0; j < 8; ++j) {
            float v = 0.f;
            if (jj < ntap) {
              const int tap = jj / cpt, ci = gbase + (jj - tap * cpt) * 8 + j - g * c8;   // GWC's input within co's group
              if (ci >= 0 && ci < c8) v = gwc_w[((size_t)co * c8 + ci) * 9 + tap];
            } else if (jj < nch) {
              v = pwc1[(size_t)co * c4 + (jj - ntap) * 8 + j];
            }
            *o++ = sc_h16(dtype, v);
          }
        }
  o = (uint16_t*)(base + b.wy2);
  for (int nb = 0; nb < c / SC_COLS; ++nb)
    for (int q = 0; q < NQ2; ++q)
      for (int tn = 0; tn < SC_NT; ++tn)
        for (int l = 0; l < 64; ++l) {
          const int co = nb * SC_COLS + tn * 16 + (l & 15);
          for (int j = 0; j < 8; ++j) {
            const int k = q * 32 + (l >> 4) * 8 + j;
            float v = 0.f;
            if (k < c4) v = co < 3 * c4 ? pwc2[(size_t)co * c4 + k] : (k == co - 3 * c4 ? 1.f : 0.f);
            *o++ = sc_h16(dtype, v);
          }
        }
  auto F = [&](size_t off) { return (float*)(base + off); };
  __builtin_memcpy(F(b.gamma), gamma, sizeof(float) * c);
  __builtin_memcpy(F(b.beta), beta, sizeof(float) * c);
  __builtin_memcpy(F(b.kc), kc, sizeof(float) * c);
  __builtin_memcpy(F(b.scale), scale, sizeof(float) * c);
  __builtin_memcpy(F(b.shift), shift, sizeof(float) * c);
  __builtin_memcpy(F(b.gwcb), gwc_b, sizeof(float) * c);
  for (size_t i = 0; i < (size_t)c * c8 * 9; ++i) F(b.gwcf)[i] = sc_r16(dtype, gwc_w[i]);
  for (size_t i = 0; i < (size_t)c * c4; ++i) F(b.pwc1f)[i] = sc_r16(dtype, pwc1[i]);
  for (size_t i = 0; i < (size_t)3 * c4 * c4; ++i) F(b.pwc2f)[i] = sc_r16(dtype, pwc2[i]);
  return FAC_OK;
}

extern "C" int fac_scconv(int dtype, const void* x, int n, int h, int w, int c, const void* packed, int pool, void* out,
                          float* stats_out, void* scratch, void* stream) {
  using namespace fac;
  if (!x || !packed || !out || !scratch || n <= 0 || (dtype != 0 && dtype != 1) || (pool != 0 && pool != 1))
    return FAC_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)packed | (uintptr_t)out | (uintptr_t)scratch) % 16 || (uintptr_t)stats_out % 4)
    return FAC_ERR_ARG;
  if (!sc_shape_ok(h, w, c, pool)) return FAC_ERR_SHAPE;
  if ((long)n * h * w > 0x3fffffffL || n > 65535) return FAC_ERR_SHAPE;   // rows are indexed in 32 bits; n is a grid's y / z
  const size_t bytes = (size_t)n * h * w * c * 2;
  const uintptr_t xb = (uintptr_t)x, ob = (uintptr_t)out;
  if (xb < ob + bytes && ob < xb + bytes) return FAC_ERR_ARG;            // not in place
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0)
    sc_launch<BF16>((const uint16_t*)x, n, h, w, c, (const char*)packed, pool, (uint16_t*)out, stats_out,
                    (char*)scratch, st);
  else
    sc_launch<F16>((const uint16_t*)x, n, h, w, c, (const char*)packed, pool, (uint16_t*)out, stats_out, (char*)scratch,
                   st);
  return hipGetLastError() == hipSuccess ? FAC_OK : FAC_ERR_HIP;
}
