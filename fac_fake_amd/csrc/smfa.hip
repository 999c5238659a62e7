// x (+)= SMFA(x) of CViT-main/model/other/cvit_GGCA_SMFA.py (:160-203) on a
// 16-bit channels-last map [n][h][w][c] with 8 <= h, w <= 15, behind fac_smfa.
//
// In that range h // 8 == w // 8 == 1: adaptive_max_pool2d gives the
// per-channel global max, dw_conv (3x3, padding 1) on a 1x1 map is its centre
// tap plus its bias, linear_1 acts on one vector per crop and the nearest
// interpolation broadcasts it.  With t = linear_0(f), y = t[:, :c], x = t[:, c:]:
//
//   u[b,ch] = alpha[ch] * (cw[ch] * max_p x[b,p,ch] + cb[ch]) + belt[ch] * var_p x[b,p,ch]
//   g[b,:]  = GELU(W1 u[b,:] + b1)                       one c-vector per crop
//   d       = depthwise 3x3 of y, zero padding, 2 outputs per input channel
//             (output j reads y channel j / 2), + its bias
//   hmap    = GELU(Wpw d + bpw)                          1x1, 2c -> 2c
//   out     = [f +] Wcat [x * g | hmap] + bcat           1x1, 3c -> c
//
// Wcat = [linear_2.W | linear_2.W conv_1.W] and bcat = linear_2.b + linear_2.W
// conv_1.b are folded by the caller in fp32 (other.smfa_fold): linear_2(x g +
// conv_1(hmap)) is linear in both terms.  linear_0's bias is NOT folded into
// the depthwise conv: the conv pads y, which already carries the bias, so a
// padded tap contributes 0.
//
// Four launches, nothing allocated, no atomics:
//   1. smfa_gemm_k<LIN0>   t = f W0^T + b0                         -> scratch
//   2. smfa_gate_k         max / variance per (crop, channel), u, the gate
//                          GEMV and GELU, all fp32                 -> scratch
//   3. smfa_gemm_k<DW>     the depthwise taps computed in registers as the
//                          activation operand of the 2c -> 2c GEMM, GELU
//                          epilogue: d never reaches memory        -> scratch
//   4. smfa_gemm_k<CAT>    K = 3c: x * g applied on load for k < c, hmap for
//                          k >= c; bcat and the residual f in the epilogue
//
// Rounding points (tests/smfa_ref.py emulates exactly these; everything else
// is fp32): the 16-bit weights W0, Wpw, Wcat; t at its store; the depthwise
// operand d; hmap at its store; the x * g operand; the one output rounding.
// The statistics are taken from the STORED 16-bit x (the x half of t), not
// from linear_0's accumulators: max is exact on those values, the variance is
// two-pass (mean first, then sum (x - mean)^2 / (N - 1), unbiased as
// torch.var), summed over the positions in index order by one thread per
// channel.  The depthwise sum is an fp32 fma chain over the taps t = 0..8
// (row-major) from 0, padded taps entering as 0, then + bias.
//
// GEMM layout.  No LDS and no barrier: a wave owns 32 rows (positions of the
// flattened batch) x NT*16 output channels and reads its fragments straight
// from global memory; the weights (<= 512 KB) stay in L2.  The weight is the
// MFMA's A operand and the activation its B operand, so a lane holds four
// consecutive output channels of one row and stores them as 8 bytes.  Rows
// span crops (196 rows per crop is no multiple of 32): the crop, the position
// and the tap mask are per row, rows past the end load row M - 1 and store
// nothing.  Every output element is one fixed-order sum: a crop's bits do not
// depend on n.
#include "common.hpp"
#include "fac_cvit.h"
#include "fac_ops.h"

namespace fac {

constexpr int SMFA_T = 256;        // threads per workgroup: 4 waves, 32 rows each
constexpr int SMFA_ROWS = 32;      // rows per wave
constexpr int SMFA_MAX_C = 256;
enum { SMFA_LIN0 = 0, SMFA_DW = 1, SMFA_CAT = 2 };

__device__ __forceinline__ float smfa_gelu(float v) { return v * 0.5f * (1.f + erff(v * 0.70710678118654752440f)); }

// Byte offsets into fac_smfa_pack's blob; every block is a multiple of 256 bytes (c % 64 == 0).
struct SmfaLayout {
  size_t w0, wpw, wcat, b0, bpw, bcat, dwt, dwb, gate, w1t, b1, total;
  __host__ __device__ explicit SmfaLayout(int c) {
    const size_t C = (size_t)c;
    w0 = 0;
    wpw = w0 + 2 * C * C * 2;
    wcat = wpw + 4 * C * C * 2;
    b0 = wcat + 3 * C * C * 2;
    bpw = b0 + 2 * C * 4;
    bcat = bpw + 2 * C * 4;
    dwt = bcat + C * 4;
    dwb = dwt + 9 * 2 * C * 4;
    gate = dwb + 2 * C * 4;
    w1t = gate + 4 * C * 4;
    b1 = w1t + C * C * 4;
    total = b1 + C * 4;
  }
};

struct SmfaGemmArgs {
  const uint16_t* a0;      // LIN0: f [M][c]; DW, CAT: t [M][2c]
  const uint16_t* a1;      // CAT: hmap [M][2c]
  const float* g;          // CAT: gate [n][c]
  const uint16_t* w;       // [N][K]
  const float* bias;       // [N]
  const float* dwt;        // DW: taps [9][2c]
  const float* dwb;        // DW: bias [2c]
  const uint16_t* resid;   // CAT: f [M][c] or null
  uint16_t* out;           // [M][N]
  int M, N, K, c, H, W;
};

template <class T, int MODE, int NT>
__global__ __launch_bounds__(SMFA_T) void smfa_gemm_k(SmfaGemmArgs A) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lk = (lane >> 4) * 8;
  const long r0 = ((long)blockIdx.x * (SMFA_T / 64) + wave) * SMFA_ROWS;
  if (r0 >= A.M) return;                       // no barrier below
  const int n0 = blockIdx.y * (NT * 16);
  const int c = A.c, c2 = 2 * A.c, K = A.K;
  int m[2], mc[2], crop[2];
  unsigned on[2] = {0, 0};                     // DW: bit t set when tap t is inside the map
#pragma unroll
  for (int rf = 0; rf < 2; ++rf) {
    m[rf] = (int)r0 + rf * 16 + lr;
    mc[rf] = m[rf] < A.M ? m[rf] : A.M - 1;
    const int hw = A.H * A.W;
    crop[rf] = mc[rf] / hw;
    if (MODE == SMFA_DW) {
      const int p = mc[rf] - crop[rf] * hw, yy = p / A.W, xx = p - yy * A.W;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int y2 = yy + t / 3 - 1, x2 = xx + t % 3 - 1;
        if ((unsigned)y2 < (unsigned)A.H && (unsigned)x2 < (unsigned)A.W) on[rf] |= 1u << t;
      }
    }
  }
  f32x4 acc[2][NT];
#pragma unroll
  for (int rf = 0; rf < 2; ++rf)
#pragma unroll
    for (int tn = 0; tn < NT; ++tn) acc[rf][tn] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < K; k0 += 32) {
    const int kk = k0 + lk;
    u16x8 af[2];
    if (MODE == SMFA_LIN0) {
#pragma unroll
      for (int rf = 0; rf < 2; ++rf) af[rf] = *(const u16x8*)(A.a0 + (size_t)mc[rf] * K + kk);
    } else if (MODE == SMFA_DW) {
      // outputs kk .. kk+7 read y channels kk/2 .. kk/2+3
      float d[2][8];
#pragma unroll
      for (int rf = 0; rf < 2; ++rf)
#pragma unroll
        for (int j = 0; j < 8; ++j) d[rf][j] = 0.f;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const f32x4 wl = *(const f32x4*)(A.dwt + t * c2 + kk), wh = *(const f32x4*)(A.dwt + t * c2 + kk + 4);
        const int off = ((t / 3 - 1) * A.W + (t % 3 - 1)) * c2;
#pragma unroll
        for (int rf = 0; rf < 2; ++rf) {
          const bool in = (on[rf] >> t) & 1u;
          // a padded tap re-loads the row's own pixel and enters as 0
          const u16x4 y = *(const u16x4*)(A.a0 + ((long)mc[rf] * c2 + (in ? off : 0) + (kk >> 1)));
#pragma unroll
          for (int j = 0; j < 8; ++j)
            d[rf][j] = fmaf(j < 4 ? wl[j] : wh[j - 4], in ? T::to_f32(y[j >> 1]) : 0.f, d[rf][j]);
        }
      }
      const f32x4 bl = *(const f32x4*)(A.dwb + kk), bh = *(const f32x4*)(A.dwb + kk + 4);
#pragma unroll
      for (int rf = 0; rf < 2; ++rf)
#pragma unroll
        for (int j = 0; j < 8; ++j) af[rf][j] = T::from_f32(d[rf][j] + (j < 4 ? bl[j] : bh[j - 4]));
    } else {
      if (k0 < c) {                            // wave-uniform: c % 32 == 0
#pragma unroll
        for (int rf = 0; rf < 2; ++rf) {
          const u16x8 x = *(const u16x8*)(A.a0 + (size_t)mc[rf] * c2 + c + kk);
          const float* gp = A.g + (size_t)crop[rf] * c + kk;
          const f32x4 gl = *(const f32x4*)gp, gh = *(const f32x4*)(gp + 4);
#pragma unroll
          for (int j = 0; j < 8; ++j) af[rf][j] = T::from_f32(T::to_f32(x[j]) * (j < 4 ? gl[j] : gh[j - 4]));
        }
      } else {
#pragma unroll
        for (int rf = 0; rf < 2; ++rf) af[rf] = *(const u16x8*)(A.a1 + (size_t)mc[rf] * c2 + (kk - c));
      }
    }
#pragma unroll
    for (int tn = 0; tn < NT; ++tn) {
      const u16x8 wf = *(const u16x8*)(A.w + (size_t)(n0 + tn * 16 + lr) * K + kk);
#pragma unroll
      for (int rf = 0; rf < 2; ++rf) acc[rf][tn] = T::mfma(wf, af[rf], acc[rf][tn]);
    }
  }

  // D[n][m]: this lane has row m = lane & 15 of the fragment and channels n0 + 16 tn + 4 (lane >> 4) + 0..3
#pragma unroll
  for (int rf = 0; rf < 2; ++rf) {
    if (m[rf] >= A.M) continue;
#pragma unroll
    for (int tn = 0; tn < NT; ++tn) {
      const int n = n0 + tn * 16 + (lane >> 4) * 4;
      const f32x4 b = *(const f32x4*)(A.bias + n);
      f32x4 v = acc[rf][tn] + b;
      if (MODE == SMFA_DW) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = smfa_gelu(v[i]);
      }
      if (MODE == SMFA_CAT && A.resid) {
        const u16x4 r = *(const u16x4*)(A.resid + (size_t)m[rf] * A.N + n);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] += T::to_f32(r[i]);
      }
      *(u16x4*)(A.out + (size_t)m[rf] * A.N + n) = T::pack4(v);
    }
  }
}

// One workgroup per crop; thread ch < c owns a channel of x = t[:, c:].
template <class T>
__global__ __launch_bounds__(SMFA_MAX_C) void smfa_gate_k(const uint16_t* __restrict__ t, int hw, int c,
                                                          const float* __restrict__ gate4,
                                                          const float* __restrict__ w1t, const float* __restrict__ b1,
                                                          float* __restrict__ g, float* __restrict__ gate_out) {
  __shared__ float u[SMFA_MAX_C];
  const int ch = threadIdx.x, b = blockIdx.x;
  const uint16_t* xp = t + (size_t)b * hw * 2 * c + c + ch;
  if (ch < c) {
    float mx = -__builtin_inff(), s = 0.f;
    for (int p = 0; p < hw; ++p) {
      const float v = T::to_f32(xp[(size_t)p * 2 * c]);
      mx = fmaxf(mx, v);
      s += v;
    }
    const float mean = s / (float)hw;
    float ss = 0.f;
    for (int p = 0; p < hw; ++p) {
      const float dv = T::to_f32(xp[(size_t)p * 2 * c]) - mean;
      ss = fmaf(dv, dv, ss);
    }
    const float var = ss / (float)(hw - 1);
    const float alpha = gate4[ch], cw = gate4[c + ch], cb = gate4[2 * c + ch], belt = gate4[3 * c + ch];
    u[ch] = fmaf(belt, var, alpha * fmaf(cw, mx, cb));
  }
  __syncthreads();
  if (ch < c) {
    float a = 0.f;
    for (int i = 0; i < c; ++i) a = fmaf(w1t[(size_t)i * c + ch], u[i], a);
    const float gv = smfa_gelu(a + b1[ch]);
    g[(size_t)b * c + ch] = gv;
    if (gate_out) gate_out[(size_t)b * c + ch] = gv;
  }
}

template <class T, int MODE>
static void launch_smfa_gemm(const SmfaGemmArgs& A, hipStream_t st) {
  const unsigned gx = (unsigned)((A.M + SMFA_ROWS * (SMFA_T / 64) - 1) / (SMFA_ROWS * (SMFA_T / 64)));
  if (A.N % 128 == 0)
    smfa_gemm_k<T, MODE, 8><<<dim3(gx, A.N / 128), SMFA_T, 0, st>>>(A);
  else
    smfa_gemm_k<T, MODE, 4><<<dim3(gx, A.N / 64), SMFA_T, 0, st>>>(A);
}

template <class T>
static hipError_t launch_smfa(const uint16_t* x, int n, int h, int w, int c, const char* wpk, bool residual, uint16_t* out,
                              float* gate_out, char* scratch, hipStream_t st) {
  const SmfaLayout L(c);
  const int M = n * h * w;
  uint16_t* t = (uint16_t*)scratch;
  uint16_t* hm = t + (size_t)M * 2 * c;
  float* g = (float*)(hm + (size_t)M * 2 * c);
  const auto F = [&](size_t off) { return (const float*)(wpk + off); };
  const auto U = [&](size_t off) { return (const uint16_t*)(wpk + off); };

  SmfaGemmArgs a{};
  a.M = M, a.c = c, a.H = h, a.W = w;
  a.a0 = x, a.w = U(L.w0), a.bias = F(L.b0), a.out = t, a.N = 2 * c, a.K = c;
  launch_smfa_gemm<T, SMFA_LIN0>(a, st);
  smfa_gate_k<T><<<n, SMFA_MAX_C, 0, st>>>(t, h * w, c, F(L.gate), F(L.w1t), F(L.b1), g, gate_out);
  a.a0 = t, a.w = U(L.wpw), a.bias = F(L.bpw), a.dwt = F(L.dwt), a.dwb = F(L.dwb), a.out = hm, a.N = 2 * c, a.K = 2 * c;
  launch_smfa_gemm<T, SMFA_DW>(a, st);
  a.a1 = hm, a.g = g, a.w = U(L.wcat), a.bias = F(L.bcat), a.resid = residual ? x : nullptr, a.out = out, a.N = c, a.K = 3 * c;
  launch_smfa_gemm<T, SMFA_CAT>(a, st);
  return hipGetLastError();
}

static bool smfa_shape_ok(int h, int w, int c) {
  return h >= 8 && h <= 15 && w >= 8 && w <= 15 && c >= 64 && c <= SMFA_MAX_C && c % 64 == 0;
}

}  // namespace fac

extern "C" size_t fac_smfa_scratch_bytes(int n, int h, int w, int c) {
  if (n <= 0 || !fac::smfa_shape_ok(h, w, c)) return 0;
  return (size_t)n * h * w * 2 * c * 2 * 2 + (size_t)n * c * 4;   // t, hmap (16-bit [M][2c]) and the gate (fp32 [n][c])
}

extern "C" size_t fac_smfa_packed_bytes(int c) {
  if (c < 64 || c > fac::SMFA_MAX_C || c % 64) return 0;
  return fac::SmfaLayout(c).total;
}

extern "C" int fac_smfa_pack(int dtype, int c, const float* w0, const float* b0, const float* gate4, const float* w1,
                             const float* b1, const float* dww, const float* dwb, const float* wpw, const float* bpw,
                             const float* wcat, const float* bcat, void* out) {
  if (!w0 || !b0 || !gate4 || !w1 || !b1 || !dww || !dwb || !wpw || !bpw || !wcat || !bcat || !out ||
      (dtype != 0 && dtype != 1))
    return FAC_ERR_ARG;
  if (c < 64 || c > fac::SMFA_MAX_C || c % 64) return FAC_ERR_SHAPE;
  const fac::SmfaLayout L(c);
  char* o = (char*)out;
  const auto to16 = [&](const float* src, size_t off, size_t count) {
    uint16_t* dst = (uint16_t*)(o + off);
    for (size_t i = 0; i < count; ++i) dst[i] = dtype == 0 ? fac_host::f32_to_bf16(src[i]) : fac_host::f32_to_f16(src[i]);
  };
  const auto f32 = [&](const float* src, size_t off, size_t count) { __builtin_memcpy(o + off, src, count * 4); };
  const size_t C = (size_t)c;
  to16(w0, L.w0, 2 * C * C);
  to16(wpw, L.wpw, 4 * C * C);
  to16(wcat, L.wcat, 3 * C * C);
  f32(b0, L.b0, 2 * C);
  f32(bpw, L.bpw, 2 * C);
  f32(bcat, L.bcat, C);
  float* dwt = (float*)(o + L.dwt);                                // [2c][9] -> [9][2c]
  for (size_t j = 0; j < 2 * C; ++j)
    for (int t = 0; t < 9; ++t) dwt[t * 2 * C + j] = dww[j * 9 + t];
  f32(dwb, L.dwb, 2 * C);
  f32(gate4, L.gate, 4 * C);
  float* w1t = (float*)(o + L.w1t);                                // [out][in] -> [in][out]
  for (size_t i = 0; i < C; ++i)
    for (size_t k = 0; k < C; ++k) w1t[k * C + i] = w1[i * C + k];
  f32(b1, L.b1, C);
  return FAC_OK;
}

extern "C" int fac_smfa(int dtype, const void* x, int n, int h, int w, int c, const void* wpk, int residual, void* out,
                        float* gate_out, void* scratch, void* stream) {
  using namespace fac;
  if (!x || !wpk || !out || !scratch || n <= 0 || (dtype != 0 && dtype != 1)) return FAC_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)wpk | (uintptr_t)out | (uintptr_t)scratch) % 16) return FAC_ERR_ARG;
  if (!smfa_shape_ok(h, w, c)) return FAC_ERR_SHAPE;
  if ((long)n * h * w > 0x3fffffffL) return FAC_ERR_SHAPE;        // rows are indexed in 32 bits
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = dtype == 0 ? launch_smfa<BF16>((const uint16_t*)x, n, h, w, c, (const char*)wpk, residual != 0,
                                                      (uint16_t*)out, gate_out, (char*)scratch, st)
                                  : launch_smfa<F16>((const uint16_t*)x, n, h, w, c, (const char*)wpk, residual != 0,
                                                     (uint16_t*)out, gate_out, (char*)scratch, st);
  return e == hipSuccess ? FAC_OK : FAC_ERR_HIP;
}
