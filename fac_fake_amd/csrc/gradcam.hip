// Grad-CAM (CViT-main/figure/utils.py:57-166, gradcam_cnn.py) on gfx950: the
// input-gradient kernels of the CViT tail and the CAM arithmetic.
//
// The library is forward-only everywhere else; Grad-CAM needs d logit[target]
// / d A for A the last BatchNorm's 512 x 14 x 14 map.  That gradient runs back
// through the head, the six pre-norm encoder layers on 2 tokens, the patch
// embedding, x * GGCA(x) (RepBn8) and the fused ReLU + MaxPool2d(2,2).  Only
// input gradients exist (no weight gradients) and the batch is <= 32 crops,
// so every kernel here is small and the GEMMs are weight-bandwidth-bound.
//
// Conventions:
//  * gradients are fp32 from the logit to the map (|g| peaks at ~5e-3: too
//    close to fp16's subnormals); the forward's 16-bit roundings of GEMM
//    inputs count as identity (straight-through);
//  * no atomics: every sum has one fixed order that depends on nothing but
//    the element's own row, so a crop's gradient and heatmap are
//    bit-reproducible and independent of the batch it is computed in;
//  * weights are read exactly as gemm_nt stores them (16-bit [N][K] rows);
//    no transposed copy exists.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/fac_cvit.h"
#include "common.hpp"

namespace fac {

// ---------------------------------------------------------------- dgrad GEMM
// dX[M][K] = dY[M][N] . W[N][K]  (the input gradient of y = x . W^T).
// A workgroup owns kDgCols consecutive columns k (4 per thread: one 8-byte
// load of a weight row per thread, a wave reads 512 contiguous bytes), a row
// range [s*NC, (s+1)*NC) of W (blockIdx.y = split s) and kDgMT rows m
// (blockIdx.z); the dY tile goes through LDS ([n][m], read as two broadcast
// ds_read_b128 per weight row).  Each (m, k) is summed over its split's n in
// ascending order into P[s][m][k]; the consumer adds the splits in ascending
// s.  The split count depends on (N, K) alone (dgrad_splits), never on M.
constexpr int kDgThreads = 256, kDgCols = kDgThreads * 4, kDgMT = 8, kDgNCH = 64;

// Rows of W per split (a multiple of kDgNCH) and the number of splits: enough
// workgroups to stream W from many CUs (about 256 over columns x splits).
void dgrad_plan(int N, int K, int* nc, int* splits) {
  const int colblocks = (K + kDgCols - 1) / kDgCols;
  int s = std::min((N + kDgNCH - 1) / kDgNCH, std::max(1, 256 / colblocks));
  int per = (N + s - 1) / s;
  per = (per + kDgNCH - 1) / kDgNCH * kDgNCH;
  *nc = per;
  *splits = (N + per - 1) / per;
}

template <class T>
__global__ __launch_bounds__(kDgThreads) void dgrad_partial(const float* __restrict__ dY, int ldy,
                                                            const uint16_t* __restrict__ W, float* __restrict__ P,
                                                            int M, int N, int K, int NC) {
  __shared__ __attribute__((aligned(16))) float sdy[kDgNCH][kDgMT];
  const int tid = threadIdx.x;
  const int k = (blockIdx.x * kDgThreads + tid) * 4;
  const int s = blockIdx.y, m0 = blockIdx.z * kDgMT;
  const int n_lo = s * NC, n_hi = min(N, n_lo + NC);
  const bool act = k < K;  // K % 4 == 0: a thread's 4 columns are all inside or all outside
  float acc[kDgMT][4];
#pragma unroll
  for (int i = 0; i < kDgMT; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int nb = n_lo; nb < n_hi; nb += kDgNCH) {
    __syncthreads();
    for (int i = tid; i < kDgNCH * kDgMT; i += kDgThreads) {
      const int nn = i & (kDgNCH - 1), mi = i / kDgNCH;
      const int m = m0 + mi, n = nb + nn;
      sdy[nn][mi] = (m < M && n < n_hi) ? dY[(size_t)m * ldy + n] : 0.f;
    }
    __syncthreads();
    const int cnt = min(kDgNCH, n_hi - nb);
    if (act) {
      const uint16_t* wp = W + (size_t)nb * K + k;
#pragma unroll 4
      for (int nn = 0; nn < cnt; ++nn) {
        const uint2 w = *(const uint2*)(wp + (size_t)nn * K);
        const float wv[4] = {T::to_f32((uint16_t)(w.x & 0xffffu)), T::to_f32((uint16_t)(w.x >> 16)),
                             T::to_f32((uint16_t)(w.y & 0xffffu)), T::to_f32((uint16_t)(w.y >> 16))};
        const f32x4 d0 = *(const f32x4*)&sdy[nn][0], d1 = *(const f32x4*)&sdy[nn][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            acc[i][j] = fmaf(d0[i], wv[j], acc[i][j]);
            acc[i + 4][j] = fmaf(d1[i], wv[j], acc[i + 4][j]);
          }
      }
    }
  }
  if (!act) return;
#pragma unroll
  for (int i = 0; i < kDgMT; ++i) {
    const int m = m0 + i;
    if (m < M) *(f32x4*)(P + ((size_t)s * M + m) * K + k) = (f32x4){acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
  }
}

// Sum of the S partials of element i of an [M][K] result (MK = M*K), ascending s.
__device__ __forceinline__ float psum(const float* __restrict__ P, int S, size_t MK, size_t i) {
  float v = P[i];
  for (int s = 1; s < S; ++s) v += P[(size_t)s * MK + i];
  return v;
}

// out[i] = sum_s P[s][i]                                        (mode 0)
// out[i] = (sum_s P[s][i]) * GELU'(pre[i]), exact-erf GELU     (mode 1)
// out = dx [2B][1024]: row 2b = sum_s P[s][b], row 2b+1 = 0    (mode 2: the
//   head's gradient enters the residual stream at the CLS rows only)
template <int MODE>
__global__ __launch_bounds__(256) void dgrad_reduce(const float* __restrict__ P, int S, size_t MK,
                                                    const float* __restrict__ pre, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= MK) return;
  float v = psum(P, S, MK, i);
  if constexpr (MODE == 1) {
    const float x = pre[i];
    // d/dx 0.5 x (1 + erf(x / sqrt 2)) = 0.5 (1 + erf(x / sqrt 2)) + x exp(-x^2 / 2) / sqrt(2 pi)
    v *= 0.5f * (1.0f + erff(x * 0.70710678118654752440f)) + x * expf(-0.5f * x * x) * 0.39894228040143267794f;
  }
  if constexpr (MODE == 2) {
    const size_t b = i >> 10, c = i & 1023;
    out[(2 * b) * 1024 + c] = v;
    out[(2 * b + 1) * 1024 + c] = 0.f;
  } else {
    out[i] = v;
  }
}

// ------------------------------------------------------- LayerNorm backward
// y = (x - mean) * rstd * g + b over 1024 columns; input gradient only:
//   dxhat = dy * g,  dx = rstd * (dxhat - mean(dxhat) - xhat * mean(dxhat * xhat))
// added to the residual gradient dx[row].  dy = sum_s P[s][row] (the partials
// of the dgrad GEMM before it).  One wave per row, the forward's column
// layout (ln_row_store: 16 floats per lane), mean / rstd recomputed from the
// saved residual row with the forward's own arithmetic.
__global__ __launch_bounds__(64) void ln_bwd(const float* __restrict__ x, const float* __restrict__ g, float eps,
                                             const float* __restrict__ P, int S, int R, float* __restrict__ dx) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const float* xr = x + (size_t)row * 1024;
  f32x4 v[4], d[4];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = i * 256 + lane * 4;
    v[i] = *(const f32x4*)(xr + c);
    f32x4 p = *(const f32x4*)(P + (size_t)row * 1024 + c);
    for (int k = 1; k < S; ++k) p += *(const f32x4*)(P + ((size_t)k * R + row) * 1024 + c);
    d[i] = p * *(const f32x4*)(g + c);
    s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
  }
  const float mean = wave_sum(s) * (1.0f / 1024.0f);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[i][j] -= mean;
      q += v[i][j] * v[i][j];
    }
  const float rstd = 1.0f / sqrtf(wave_sum(q) * (1.0f / 1024.0f) + eps);
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[i][j] *= rstd;  // xhat
      s1 += d[i][j];
      s2 += d[i][j] * v[i][j];
    }
  const float m1 = wave_sum(s1) * (1.0f / 1024.0f), m2 = wave_sum(s2) * (1.0f / 1024.0f);
  float* dr = dx + (size_t)row * 1024;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = i * 256 + lane * 4;
    f32x4 o = *(const f32x4*)(dr + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] += rstd * (d[i][j] - m1 - v[i][j] * m2);
    *(f32x4*)(dr + c) = o;
  }
}

// -------------------------------------------------------- attention backward
// n = 2 tokens, 8 heads x 128 (attention2's forward, cvit.py:43-60).  One wave
// per (crop, head); a lane holds dims lane and lane + 64.  The softmax is
// recomputed from the saved q, k; do = sum_s P[s] (to_out's dgrad partials,
// [2B][1024] rows).  dqkv fp32 [2B][3072] in the forward's (qkv h d) layout.
__global__ __launch_bounds__(256) void attn2_bwd(const float* __restrict__ qkv, const float* __restrict__ P, int S,
                                                 int B, float scale, float* __restrict__ dqkv) {
  const int wid = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (wid >= B * 8) return;
  const int b = wid >> 3, h = wid & 7;
  const float* r0 = qkv + (size_t)(2 * b) * 3072 + h * 128;
  const float* r1 = r0 + 3072;
  const size_t MK = (size_t)2 * B * 1024, o0i = (size_t)(2 * b) * 1024 + h * 128;
  float q0[2], q1[2], k0[2], k1[2], v0[2], v1[2], g0[2], g1[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int d = lane + 64 * i;
    q0[i] = r0[d];
    k0[i] = r0[1024 + d];
    v0[i] = r0[2048 + d];
    q1[i] = r1[d];
    k1[i] = r1[1024 + d];
    v1[i] = r1[2048 + d];
    g0[i] = psum(P, S, MK, o0i + d);
    g1[i] = psum(P, S, MK, o0i + 1024 + d);
  }
  float s00 = 0.f, s01 = 0.f, s10 = 0.f, s11 = 0.f, t00 = 0.f, t01 = 0.f, t10 = 0.f, t11 = 0.f;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    s00 += q0[i] * k0[i];
    s01 += q0[i] * k1[i];
    s10 += q1[i] * k0[i];
    s11 += q1[i] * k1[i];
    t00 += g0[i] * v0[i];  // d a00 = do0 . v0
    t01 += g0[i] * v1[i];
    t10 += g1[i] * v0[i];
    t11 += g1[i] * v1[i];
  }
  s00 = wave_sum(s00) * scale;
  s01 = wave_sum(s01) * scale;
  s10 = wave_sum(s10) * scale;
  s11 = wave_sum(s11) * scale;
  t00 = wave_sum(t00);
  t01 = wave_sum(t01);
  t10 = wave_sum(t10);
  t11 = wave_sum(t11);
  const float m0 = fmaxf(s00, s01), m1 = fmaxf(s10, s11);
  const float e00 = expf(s00 - m0), e01 = expf(s01 - m0);
  const float e10 = expf(s10 - m1), e11 = expf(s11 - m1);
  const float a00 = e00 / (e00 + e01), a01 = e01 / (e00 + e01);
  const float a10 = e10 / (e10 + e11), a11 = e11 / (e10 + e11);
  // softmax backward per row, then the 1/32 scale of the scores
  const float c0 = a00 * t00 + a01 * t01, c1 = a10 * t10 + a11 * t11;
  const float u00 = a00 * (t00 - c0) * scale, u01 = a01 * (t01 - c0) * scale;
  const float u10 = a10 * (t10 - c1) * scale, u11 = a11 * (t11 - c1) * scale;
  float* w0 = dqkv + (size_t)(2 * b) * 3072 + h * 128;
  float* w1 = w0 + 3072;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int d = lane + 64 * i;
    w0[d] = u00 * k0[i] + u01 * k1[i];
    w1[d] = u10 * k0[i] + u11 * k1[i];
    w0[1024 + d] = u00 * q0[i] + u10 * q1[i];
    w1[1024 + d] = u01 * q0[i] + u11 * q1[i];
    w0[2048 + d] = a00 * g0[i] + a10 * g1[i];
    w1[2048 + d] = a01 * g0[i] + a11 * g1[i];
  }
}

// ------------------------------------------------------------ head backward
// logits = hid . w2^T + b2 with hid = ReLU(.) fp32 [B][2048]; the seed is the
// one-hot of the target (GradCAM.get_loss sums output[i, target[i]]):
//   dhid[b][j] = w2[t_b][j] if hid[b][j] > 0 else 0
// t_b = target[b], or for target[b] < 0 the argmax of the crop's logits
// (np.argmax: the first maximum).
__global__ __launch_bounds__(256) void head_bwd(const float* __restrict__ hid, const float* __restrict__ w2,
                                                const int32_t* __restrict__ target,
                                                const float* __restrict__ logits, int B, float* __restrict__ dhid) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * 2048) return;
  const int b = i >> 11, j = i & 2047;
  int t = target[b];
  if (t < 0) t = logits[2 * b + 1] > logits[2 * b] ? 1 : 0;
  t = t > 1 ? 1 : t;
  dhid[i] = hid[i] > 0.f ? w2[t * 2048 + j] : 0.f;
}

// ---------------------------------------------------- x * GGCA(x) backward
// The forward (ggca_k, ops.hip) is out = x * x * a_h[y] * a_w[x] per channel,
// a_h = sigmoid(z(avg_x x) + z(max_x x)), a_w likewise over y, z the shared
// 1x1 -> BN(eval) -> ReLU -> 1x1.  With g = d out (fp32):
//   dx  = 2 x a_h a_w g                              (direct)
//       + dpool[h_avg][y] / W + dpool[w_avg][x] / H  (average pools)
//       + dpool[h_max][y] at the row's first maximum, dpool[w_max][x] at the
//         column's first maximum (AdaptiveMaxPool2d's scan order)
//   s = g x^2, da_h[y] = sum_x s a_w[x], da_w[x] = sum_y s a_h[y],
//   dz = da a (1 - a) for both arguments of the sigmoid, and each pooled
//   vector's dz goes back through w2^T, its own ReLU mask, the BN scale, w1^T.
// One workgroup per (crop, group); the group's features, the 2H + 2W vectors
// and their gradients live in LDS.  Every sum runs in ascending index order.
constexpr int kGgX = 6272, kGgV = 3584, kGgH = 448;  // 7*7*128 features, 28*128 pooled, 28*16 hidden

template <class T>
__global__ __launch_bounds__(256) void ggca_mul_bwd(const uint16_t* __restrict__ x, const float* __restrict__ g,
                                                    int H, int W, int C, int groups, const float* __restrict__ w1,
                                                    const float* __restrict__ b1, const float* __restrict__ bn4,
                                                    const float* __restrict__ w2, const float* __restrict__ b2,
                                                    float* __restrict__ dx) {
  __shared__ float xs[kGgX];
  __shared__ float pv[kGgV];   // pooled -> z -> attention (rows 0..H-1: a_h, 2H..2H+W-1: a_w)
  __shared__ float dv[kGgV];   // dz -> dpool
  __shared__ float hid[kGgH];  // ReLU'd hidden (its sign is the mask)
  __shared__ float dh[kGgH];
  const int img = blockIdx.x / groups, gr = blockIdx.x - img * groups;
  const int CG = C / groups, CR = CG / 16, P = H * W, NV = 2 * H + 2 * W;
  const int tid = threadIdx.x;
  const size_t base = (size_t)img * P * C + gr * CG;
  const uint16_t* xb = x + base;
  const float* gb = g + base;
  for (int i = tid; i < P * CG; i += 256) {
    const int pix = i / CG, c = i - pix * CG;
    xs[i] = T::to_f32(xb[(size_t)pix * C + c]);
  }
  __syncthreads();
  // the forward's pooled vectors, hidden layer and z, as ggca_k computes them
  for (int i = tid; i < NV * CG; i += 256) {
    const int v = i / CG, c = i - v * CG;
    float acc;
    if (v < 2 * H) {
      const int y = v < H ? v : v - H;
      acc = xs[(y * W) * CG + c];
      for (int xx = 1; xx < W; ++xx) {
        const float e = xs[(y * W + xx) * CG + c];
        acc = v < H ? acc + e : fmaxf(acc, e);
      }
      if (v < H) acc = acc / (float)W;
    } else {
      const int u = v - 2 * H, xx = u < W ? u : u - W;
      acc = xs[xx * CG + c];
      for (int y = 1; y < H; ++y) {
        const float e = xs[(y * W + xx) * CG + c];
        acc = u < W ? acc + e : fmaxf(acc, e);
      }
      if (u < W) acc = acc / (float)H;
    }
    pv[i] = acc;
  }
  __syncthreads();
  for (int i = tid; i < NV * CR; i += 256) {
    const int v = i / CR, r = i - v * CR;
    float a = 0.f;
    for (int c = 0; c < CG; ++c) a += w1[r * CG + c] * pv[v * CG + c];
    a += b1[r];
    const float inv = 1.0f / sqrtf(bn4[CR + r] + 1e-5f);
    a = (a - bn4[r]) * inv * bn4[2 * CR + r] + bn4[3 * CR + r];
    hid[i] = fmaxf(a, 0.f);
  }
  __syncthreads();
  for (int i = tid; i < NV * CG; i += 256) {
    const int v = i / CG, c = i - v * CG;
    float a = 0.f;
    for (int r = 0; r < CR; ++r) a += w2[c * CR + r] * hid[v * CR + r];
    pv[i] = a + b2[c];
  }
  __syncthreads();
  // attention values in place: a thread reads the two z rows of its (axis index, channel) and writes the first
  for (int i = tid; i < (H + W) * CG; i += 256) {
    const int u = i / CG, c = i - u * CG;
    const int va = u < H ? u : 2 * H + (u - H), vm = u < H ? H + u : 2 * H + W + (u - H);
    pv[va * CG + c] = 1.0f / (1.0f + expf(-(pv[va * CG + c] + pv[vm * CG + c])));
  }
  __syncthreads();
  // d a_h / d a_w -> dz of both pooled vectors of that axis index
  for (int i = tid; i < (H + W) * CG; i += 256) {
    const int u = i / CG, c = i - u * CG;
    float acc = 0.f, a;
    int va, vm;
    if (u < H) {
      const int y = u;
      for (int xx = 0; xx < W; ++xx) {
        const int e = (y * W + xx) * CG + c;
        const float xv = xs[e];
        acc += gb[(size_t)(y * W + xx) * C + c] * xv * xv * pv[(2 * H + xx) * CG + c];
      }
      va = y;
      vm = H + y;
    } else {
      const int xx = u - H;
      for (int y = 0; y < H; ++y) {
        const int e = (y * W + xx) * CG + c;
        const float xv = xs[e];
        acc += gb[(size_t)(y * W + xx) * C + c] * xv * xv * pv[y * CG + c];
      }
      va = 2 * H + xx;
      vm = 2 * H + W + xx;
    }
    a = pv[va * CG + c];
    const float dz = acc * a * (1.0f - a);
    dv[va * CG + c] = dz;
    dv[vm * CG + c] = dz;
  }
  __syncthreads();
  for (int i = tid; i < NV * CR; i += 256) {  // through w2^T, the ReLU mask and the BN scale
    const int v = i / CR, r = i - v * CR;
    float a = 0.f;
    for (int c = 0; c < CG; ++c) a += w2[c * CR + r] * dv[v * CG + c];
    const float inv = 1.0f / sqrtf(bn4[CR + r] + 1e-5f);
    dh[i] = hid[i] > 0.f ? a * (inv * bn4[2 * CR + r]) : 0.f;
  }
  __syncthreads();
  for (int i = tid; i < NV * CG; i += 256) {  // through w1^T: the pooled vectors' gradients
    const int v = i / CG, c = i - v * CG;
    float a = 0.f;
    for (int r = 0; r < CR; ++r) a += w1[r * CG + c] * dh[v * CR + r];
    dv[i] = a;
  }
  __syncthreads();
  float* ob = dx + base;
  for (int i = tid; i < P * CG; i += 256) {
    const int pix = i / CG, c = i - pix * CG;
    const int y = pix / W, xx = pix - y * W;
    const float xv = xs[i];
    float o = 2.0f * xv * pv[y * CG + c] * pv[(2 * H + xx) * CG + c] * gb[(size_t)pix * C + c];
    o += dv[y * CG + c] / (float)W;
    o += dv[(2 * H + xx) * CG + c] / (float)H;
    int ax = 0, ay = 0;  // first maximum of the row (over x) and of the column (over y)
    float mx = xs[(y * W) * CG + c], my = xs[xx * CG + c];
    for (int k = 1; k < W; ++k) {
      const float e = xs[(y * W + k) * CG + c];
      if (e > mx) {
        mx = e;
        ax = k;
      }
    }
    for (int k = 1; k < H; ++k) {
      const float e = xs[(k * W + xx) * CG + c];
      if (e > my) {
        my = e;
        ay = k;
      }
    }
    if (ax == xx) o += dv[(H + y) * CG + c];
    if (ay == y) o += dv[(2 * H + W + xx) * CG + c];
    ob[(size_t)pix * C + c] = o;
  }
}

// -------------------------------------------------- ReLU + MaxPool2d backward
// A: the pre-ReLU map, 16-bit channels-last [n][2h][2h][c]; dP fp32 [n][h][h][c];
// dA fp32 [n][2h][2h][c]: dP goes to the first maximum (row-major scan, strict
// >, as PyTorch's max_pool2d) of the ReLU'd window if A is positive there.
template <class T>
__global__ __launch_bounds__(256) void relu_pool_bwd(const uint16_t* __restrict__ A, const float* __restrict__ dP,
                                                     int n, int h, int c, float* __restrict__ dA) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n * h * h * c) return;
  const int ch = (int)(i % c);
  size_t r = i / c;
  const int j = (int)(r % h);
  r /= h;
  const int ii = (int)(r % h), b = (int)(r / h);
  const int H2 = 2 * h;
  const size_t p00 = (((size_t)b * H2 + 2 * ii) * H2 + 2 * j) * c + ch;
  const size_t off[4] = {p00, p00 + c, p00 + (size_t)H2 * c, p00 + (size_t)H2 * c + c};
  float best = 0.f;
  int arg = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float v = fmaxf(T::to_f32(A[off[k]]), 0.f);
    if (k == 0 || v > best) {
      best = v;
      arg = k;
    }
  }
  const float gp = dP[i];
#pragma unroll
  for (int k = 0; k < 4; ++k) dA[off[k]] = (k == arg && best > 0.f) ? gp : 0.f;
}

// ------------------------------------------------------------------ the CAM
// figure/utils.py:76-134,165-166 for one crop per workgroup, all fp32:
//   w[c]   = mean_p G[p][c]                        (row sums over x, then over the rows y)
//   cam[p] = max(sum_c w[c] A[p][c], 0)            (a wave per p; lane sums c = lane + 64 i, then the butterfly)
//   cam    = (cam - min) / (1e-7 + max(cam - min))
//   heat   = bilinear 14 -> 224 (half-pixel centres, clamped edges), max(., 0),
//            then the same min/max scaling over the 224^2 map.
// A 16-bit [n][14][14][512], G fp32 the same shape; w_out [n][512], cam14
// [n][196], heat [n][224][224].
constexpr int kCamP = 196, kCamC = 512, kCamS = 14, kCamO = 224;

__device__ __forceinline__ float cam_pixel(const float* __restrict__ cam, int oy, int ox) {
  // torch upsample_bilinear2d, align_corners = False (= cv2 INTER_LINEAR when upscaling)
  const float sy = fmaxf((oy + 0.5f) * 0.0625f - 0.5f, 0.f), sx = fmaxf((ox + 0.5f) * 0.0625f - 0.5f, 0.f);
  const int y0 = (int)sy, x0 = (int)sx;
  const int y1 = y0 + (y0 < kCamS - 1 ? 1 : 0), x1 = x0 + (x0 < kCamS - 1 ? 1 : 0);
  const float ly = sy - (float)y0, lx = sx - (float)x0, hy = 1.0f - ly, hx = 1.0f - lx;
  return hy * (hx * cam[y0 * kCamS + x0] + lx * cam[y0 * kCamS + x1]) +
         ly * (hx * cam[y1 * kCamS + x0] + lx * cam[y1 * kCamS + x1]);
}

__device__ __forceinline__ void block_minmax(float& lo, float& hi, float* red, int tid) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o, 64));
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
  }
  __syncthreads();
  if ((tid & 63) == 0) {
    red[(tid >> 6) * 2] = lo;
    red[(tid >> 6) * 2 + 1] = hi;
  }
  __syncthreads();
  lo = fminf(fminf(red[0], red[2]), fminf(red[4], red[6]));
  hi = fmaxf(fmaxf(red[1], red[3]), fmaxf(red[5], red[7]));
}

template <class T>
__global__ __launch_bounds__(256) void cam_k(const uint16_t* __restrict__ A, const float* __restrict__ G,
                                             float* __restrict__ w_out, float* __restrict__ cam14,
                                             float* __restrict__ heat) {
  __shared__ float ws[kCamC];
  __shared__ float cam[kCamP];
  __shared__ float red[8];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint16_t* Ab = A + (size_t)b * kCamP * kCamC;
  const float* Gb = G + (size_t)b * kCamP * kCamC;
  for (int c = tid; c < kCamC; c += 256) {
    float s = 0.f;
    for (int y = 0; y < kCamS; ++y) {  // a row's sum, then the rows: shorter chains than one run over 196
      float r = 0.f;
      for (int xx = 0; xx < kCamS; ++xx) r += Gb[(size_t)(y * kCamS + xx) * kCamC + c];
      s += r;
    }
    s *= (1.0f / (float)kCamP);
    ws[c] = s;
    if (w_out) w_out[(size_t)b * kCamC + c] = s;
  }
  __syncthreads();
  for (int p = wave; p < kCamP; p += 4) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kCamC / 64; ++i) {
      const int c = lane + 64 * i;
      s += ws[c] * T::to_f32(Ab[(size_t)p * kCamC + c]);
    }
    s = wave_sum(s);
    if (lane == 0) cam[p] = fmaxf(s, 0.f);
  }
  __syncthreads();
  float lo = tid < kCamP ? cam[tid] : INFINITY, hi = tid < kCamP ? cam[tid] : -INFINITY;
  block_minmax(lo, hi, red, tid);
  const float den = 1e-7f + (hi - lo);
  __syncthreads();
  if (tid < kCamP) {
    const float v = (cam[tid] - lo) / den;
    cam[tid] = v;
    cam14[(size_t)b * kCamP + tid] = v;
  }
  __syncthreads();
  float lo2 = INFINITY, hi2 = -INFINITY;
  for (int i = tid; i < kCamO * kCamO; i += 256) {
    const float v = fmaxf(cam_pixel(cam, i / kCamO, i % kCamO), 0.f);
    lo2 = fminf(lo2, v);
    hi2 = fmaxf(hi2, v);
  }
  block_minmax(lo2, hi2, red, tid);
  const float den2 = 1e-7f + (hi2 - lo2);
  float* hb = heat + (size_t)b * kCamO * kCamO;
  for (int i = tid; i < kCamO * kCamO; i += 256) {
    const float v = fmaxf(cam_pixel(cam, i / kCamO, i % kCamO), 0.f);
    hb[i] = (v - lo2) / den2;
  }
}

// ------------------------------------------------------------------ launchers
static hipError_t last() { return hipGetLastError(); }

size_t dgrad_partial_floats(int M, int N, int K) {
  int nc, s;
  dgrad_plan(N, K, &nc, &s);
  return (size_t)s * M * K;
}

// The partials of dX = dY . W into P ([splits][M][K]); returns the split count in *splits.
hipError_t launch_dgrad(int dtype, const float* dY, int ldy, const uint16_t* W, float* P, int M, int N, int K,
                        int* splits, hipStream_t st) {
  if (M <= 0 || N <= 0 || K <= 0 || K % 4 != 0 || ldy < N) return hipErrorInvalidValue;
  int nc, s;
  dgrad_plan(N, K, &nc, &s);
  *splits = s;
  const dim3 grid((K + kDgCols - 1) / kDgCols, s, (M + kDgMT - 1) / kDgMT);
  if (dtype == 0) dgrad_partial<BF16><<<grid, kDgThreads, 0, st>>>(dY, ldy, W, P, M, N, K, nc);
  else dgrad_partial<F16><<<grid, kDgThreads, 0, st>>>(dY, ldy, W, P, M, N, K, nc);
  return last();
}

hipError_t launch_dgrad_reduce(int mode, const float* P, int S, size_t MK, const float* pre, float* out,
                               hipStream_t st) {
  const unsigned nb = (unsigned)((MK + 255) / 256);
  if (mode == 0) dgrad_reduce<0><<<nb, 256, 0, st>>>(P, S, MK, pre, out);
  else if (mode == 1) dgrad_reduce<1><<<nb, 256, 0, st>>>(P, S, MK, pre, out);
  else dgrad_reduce<2><<<nb, 256, 0, st>>>(P, S, MK, pre, out);
  return last();
}

hipError_t launch_ln_bwd(const float* x, const float* g, float eps, const float* P, int S, int R, float* dx,
                         hipStream_t st) {
  ln_bwd<<<R, 64, 0, st>>>(x, g, eps, P, S, R, dx);
  return last();
}

hipError_t launch_attn2_bwd(const float* qkv, const float* P, int S, int B, float scale, float* dqkv,
                            hipStream_t st) {
  attn2_bwd<<<(B * 8 + 3) / 4, 256, 0, st>>>(qkv, P, S, B, scale, dqkv);
  return last();
}

hipError_t launch_head_bwd(const float* hid, const float* w2, const int32_t* target, const float* logits, int B,
                           float* dhid, hipStream_t st) {
  head_bwd<<<(B * 2048 + 255) / 256, 256, 0, st>>>(hid, w2, target, logits, B, dhid);
  return last();
}

}  // namespace fac

namespace {
bool dt_ok(int dtype) { return dtype == FAC_DTYPE_BF16 || dtype == FAC_DTYPE_F16; }
int status(hipError_t e) { return e == hipSuccess ? FAC_OK : (e == hipErrorInvalidValue ? FAC_ERR_ARG : FAC_ERR_HIP); }
}  // namespace

extern "C" {

size_t fac_gradcam_dgrad_scratch_floats(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  return fac::dgrad_partial_floats(M, N, K);
}

int fac_gradcam_dgrad(int dtype, const float* d_dy, int ldy, const uint16_t* d_w, float* d_scratch, float* d_dx,
                      int M, int N, int K, void* stream) {
  if (!d_dy || !d_w || !d_scratch || !d_dx || !dt_ok(dtype) || M <= 0 || N <= 0 || K <= 0 || ldy < N)
    return FAC_ERR_ARG;
  if (K % 4 != 0 || M > 64 || ((uintptr_t)d_w & 7) || ((uintptr_t)d_scratch & 15)) return FAC_ERR_SHAPE;
  int s = 0;
  hipError_t e = fac::launch_dgrad(dtype, d_dy, ldy, d_w, d_scratch, M, N, K, &s, (hipStream_t)stream);
  if (e != hipSuccess) return status(e);
  return status(fac::launch_dgrad_reduce(0, d_scratch, s, (size_t)M * K, nullptr, d_dx, (hipStream_t)stream));
}

int fac_gradcam_gelu_bwd(const float* d_pre, const float* d_dh, long long n, float* d_dpre, void* stream) {
  if (!d_pre || !d_dh || !d_dpre || n <= 0) return FAC_ERR_ARG;
  return status(fac::launch_dgrad_reduce(1, d_dh, 1, (size_t)n, d_pre, d_dpre, (hipStream_t)stream));
}

int fac_gradcam_ln_bwd(const float* d_x, const float* d_g, float eps, const float* d_dy, int R, float* d_dx,
                       void* stream) {
  if (!d_x || !d_g || !d_dy || !d_dx || R <= 0 || !(eps > 0.f)) return FAC_ERR_ARG;
  return status(fac::launch_ln_bwd(d_x, d_g, eps, d_dy, 1, R, d_dx, (hipStream_t)stream));
}

int fac_gradcam_attention_bwd(const float* d_qkv, const float* d_do, int B, float scale, float* d_dqkv,
                              void* stream) {
  if (!d_qkv || !d_do || !d_dqkv || B <= 0) return FAC_ERR_ARG;
  return status(fac::launch_attn2_bwd(d_qkv, d_do, 1, B, scale, d_dqkv, (hipStream_t)stream));
}

int fac_gradcam_head_bwd(const float* d_hid, const float* d_w2, const int32_t* d_target, const float* d_logits,
                         int B, float* d_dhid, void* stream) {
  if (!d_hid || !d_w2 || !d_target || !d_logits || !d_dhid || B <= 0) return FAC_ERR_ARG;
  return status(fac::launch_head_bwd(d_hid, d_w2, d_target, d_logits, B, d_dhid, (hipStream_t)stream));
}

int fac_ggca_mul_bwd(int dtype, const void* x, const float* g, int n, int h, int w, int c, int groups,
                     const float* w1, const float* b1, const float* bn4, const float* w2, const float* b2, float* dx,
                     void* stream) {
  if (!x || !g || !dx || !w1 || !b1 || !bn4 || !w2 || !b2 || n <= 0 || h <= 0 || w <= 0 || c <= 0 || groups <= 0 ||
      c % groups || !dt_ok(dtype))
    return FAC_ERR_ARG;
  const int cg = c / groups;
  if (cg % 16 || h * w * cg > fac::kGgX || (2 * h + 2 * w) * cg > fac::kGgV || (2 * h + 2 * w) * (cg / 16) > fac::kGgH)
    return FAC_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0)
    fac::ggca_mul_bwd<fac::BF16><<<n * groups, 256, 0, st>>>((const uint16_t*)x, g, h, w, c, groups, w1, b1, bn4, w2,
                                                            b2, dx);
  else
    fac::ggca_mul_bwd<fac::F16><<<n * groups, 256, 0, st>>>((const uint16_t*)x, g, h, w, c, groups, w1, b1, bn4, w2,
                                                           b2, dx);
  return status(hipGetLastError());
}

int fac_relu_pool_bwd(int dtype, const void* a, const float* dp, int n, int h, int c, float* da, void* stream) {
  if (!a || !dp || !da || n <= 0 || h <= 0 || c <= 0 || !dt_ok(dtype)) return FAC_ERR_ARG;
  const size_t work = (size_t)n * h * h * c;
  if (work >= ((size_t)1 << 31)) return FAC_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const unsigned nb = (unsigned)((work + 255) / 256);
  if (dtype == 0) fac::relu_pool_bwd<fac::BF16><<<nb, 256, 0, st>>>((const uint16_t*)a, dp, n, h, c, da);
  else fac::relu_pool_bwd<fac::F16><<<nb, 256, 0, st>>>((const uint16_t*)a, dp, n, h, c, da);
  return status(hipGetLastError());
}

int fac_gradcam_cam(int dtype, const void* a, const float* da, int n, float* w_out, float* cam14, float* heat,
                    void* stream) {
  if (!a || !da || !cam14 || !heat || n <= 0 || !dt_ok(dtype)) return FAC_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0) fac::cam_k<fac::BF16><<<n, 256, 0, st>>>((const uint16_t*)a, da, w_out, cam14, heat);
  else fac::cam_k<fac::F16><<<n, 256, 0, st>>>((const uint16_t*)a, da, w_out, cam14, heat);
  return status(hipGetLastError());
}

}  // extern "C"
