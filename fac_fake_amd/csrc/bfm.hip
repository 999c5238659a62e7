// BFM(x, x) of CViT-main/model/other/cvit_GGCA4_BFM5.py (:162-272) on a 16-bit
// channels-last map [n][h][w][c] with 7 <= h, w <= 14, behind fac_bfm.
//
// Every call site of the reference is self.bfm(x, x).  With t1 is t2 both
// MultiScaleFeatureExtractor outputs are the same tensor t, and TFAM returns
// (cs[0] + ss[0] + 1) t + (cs[1] + ss[1] + 1) t where cs and ss are softmaxes
// over the stacking dimension of size 2: each pair sums to 1, so the block is
// 4 t whatever the TFAM weights are.  What is computed here:
//
//   out = scale * (ReLU(conv3(x) + b3) + ReLU(conv5(x) + b5) + ReLU(conv7(x) + b7))
//
// three full c -> c convs (3x3 / 5x5 / 7x7, zero padding 1 / 2 / 3) of the
// same map, each ReLU'd alone BEFORE the sum (they do not merge into one 7x7
// conv), scale = 4 in the models.
//
// One launch, one implicit GEMM over the 7x7 window.  Rows are the pixels of
// the flattened batch (n h w), columns the output channels, K = 49 offsets x c.
// The 3x3 and 5x5 taps are subsets of the window's 49 offsets, so the shifted
// input fragment of an offset and 32-channel chunk is fetched once and feeds
// one, two or three MFMAs (16x16x32) into three fp32 accumulator sets: 49
// pixel-fragment fetches per chunk where three separate convs make 83.
//
// Layout (smfa.hip's GEMM).  No LDS and no barrier: a wave owns 32 rows x 64
// output channels x 3 accumulator sets (96 accumulator registers) and reads
// its fragments straight from global memory.  The weight is the MFMA's A
// operand, packed by fac_bfm_pack in fragment order so that a wave's fragment
// is one contiguous 1 KiB read; the four waves of a workgroup walk the same
// weights at the same time.  The activation is the B operand, so a lane holds
// four consecutive output channels of one row and stores them as 8 bytes.
// Rows span crops (49 or 196 rows per crop are no multiple of 32): the crop,
// the position and the in-map test are per row.  A tap outside the map re-reads
// the row's own pixel (an address inside x) and enters the MFMA as 0: the halo
// never sees a neighbouring crop, a wrapped row or a bias.  Rows past the end
// load row M - 1 and store nothing.
//
// Rounding: the 16-bit weights and input; every sum is fp32 in a fixed order
// (offsets row-major over the window, chunks inside); + bias, ReLU, the sum
// (3x3 + 5x5) + 7x7 and x scale in fp32; ONE rounding to 16 bits at the store.
// No atomics: a crop's bits do not depend on n.
#include "common.hpp"
#include "fac_cvit.h"
#include "fac_ops.h"

namespace fac {

constexpr int BFM_T = 256;        // threads per workgroup: 4 waves, 32 rows each
constexpr int BFM_ROWS = 32;      // rows per wave
constexpr int BFM_NT = 4;         // 16-channel column fragments per wave
constexpr int BFM_COLS = BFM_NT * 16;
constexpr int BFM_TAPS = 9 + 25 + 49;

// fac_bfm_pack's layout, in 16-bit elements: the 7x7, then the 5x5, then the
// 3x3 weights, each [c / 64][k * k taps][c / 32][BFM_NT][64 lanes][8]; lane l,
// element j of fragment (nb, tap, kc, tn) is w[nb * 64 + tn * 16 + (l & 15)][kc * 32 + (l >> 4) * 8 + j][tap].
__host__ __device__ inline size_t bfm_region(int c, int k) {
  const size_t cc = (size_t)c * c;
  return k == 7 ? 0 : k == 5 ? 49 * cc : (49 + 25) * cc;
}

template <class T, int S>
__device__ __forceinline__ void bfm_tap(const uint16_t* __restrict__ xa0, const uint16_t* __restrict__ xa1, bool in0,
                                        bool in1, const uint16_t* __restrict__ w7, const uint16_t* __restrict__ w5,
                                        const uint16_t* __restrict__ w3, int KC, f32x4 (&a7)[2][BFM_NT],
                                        f32x4 (&a5)[2][BFM_NT], f32x4 (&a3)[2][BFM_NT]) {
  const u16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 2
  for (int kc = 0; kc < KC; ++kc) {
    u16x8 af[2];
    af[0] = *(const u16x8*)(xa0 + kc * 32);
    af[1] = *(const u16x8*)(xa1 + kc * 32);
    af[0] = in0 ? af[0] : zero;
    af[1] = in1 ? af[1] : zero;
    const size_t wo = (size_t)kc * (BFM_NT * 512);
#pragma unroll
    for (int tn = 0; tn < BFM_NT; ++tn) {
      const u16x8 wf = *(const u16x8*)(w7 + wo + tn * 512);
      a7[0][tn] = T::mfma(wf, af[0], a7[0][tn]);
      a7[1][tn] = T::mfma(wf, af[1], a7[1][tn]);
    }
    if (S >= 2) {
#pragma unroll
      for (int tn = 0; tn < BFM_NT; ++tn) {
        const u16x8 wf = *(const u16x8*)(w5 + wo + tn * 512);
        a5[0][tn] = T::mfma(wf, af[0], a5[0][tn]);
        a5[1][tn] = T::mfma(wf, af[1], a5[1][tn]);
      }
    }
    if (S >= 3) {
#pragma unroll
      for (int tn = 0; tn < BFM_NT; ++tn) {
        const u16x8 wf = *(const u16x8*)(w3 + wo + tn * 512);
        a3[0][tn] = T::mfma(wf, af[0], a3[0][tn]);
        a3[1][tn] = T::mfma(wf, af[1], a3[1][tn]);
      }
    }
  }
}

template <class T>
__global__ __launch_bounds__(BFM_T, 2) void bfm_k(const uint16_t* __restrict__ x, const uint16_t* __restrict__ wpk,
                                                const float* __restrict__ bias3, uint16_t* __restrict__ out, int M,
                                                int H, int W, int c, float scale) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lk = (lane >> 4) * 8;
  const long r0 = ((long)blockIdx.x * (BFM_T / 64) + wave) * BFM_ROWS;
  if (r0 >= M) return;                         // no barrier below
  const int nb = blockIdx.y, KC = c >> 5;
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
  f32x4 a7[2][BFM_NT], a5[2][BFM_NT], a3[2][BFM_NT];
#pragma unroll
  for (int rf = 0; rf < 2; ++rf)
#pragma unroll
    for (int tn = 0; tn < BFM_NT; ++tn) a7[rf][tn] = a5[rf][tn] = a3[rf][tn] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const size_t frag = (size_t)KC * (BFM_NT * 512);            // elements per (column block, tap)
  const uint16_t* w7b = wpk + bfm_region(c, 7) + (size_t)nb * 49 * frag + lane * 8;
  const uint16_t* w5b = wpk + bfm_region(c, 5) + (size_t)nb * 25 * frag + lane * 8;
  const uint16_t* w3b = wpk + bfm_region(c, 3) + (size_t)nb * 9 * frag + lane * 8;

  for (int dy = -3; dy <= 3; ++dy) {
    for (int dx = -3; dx <= 3; ++dx) {
      const int off = (dy * W + dx) * c;       // elements; used only where the tap is inside the row's own map
      bool in[2];
      const uint16_t* xa[2];
#pragma unroll
      for (int rf = 0; rf < 2; ++rf) {
        in[rf] = (unsigned)(yy[rf] + dy) < (unsigned)H && (unsigned)(xx[rf] + dx) < (unsigned)W;
        xa[rf] = xp[rf] + (in[rf] ? off : 0);
      }
      const int ady = dy < 0 ? -dy : dy, adx = dx < 0 ? -dx : dx, r = ady > adx ? ady : adx;
      const uint16_t* w7 = w7b + (size_t)((dy + 3) * 7 + dx + 3) * frag;
      const uint16_t* w5 = w5b + (size_t)(r <= 2 ? (dy + 2) * 5 + dx + 2 : 0) * frag;   // read only where r <= 2
      const uint16_t* w3 = w3b + (size_t)(r <= 1 ? (dy + 1) * 3 + dx + 1 : 0) * frag;   // read only where r <= 1
      if (r <= 1)
        bfm_tap<T, 3>(xa[0], xa[1], in[0], in[1], w7, w5, w3, KC, a7, a5, a3);
      else if (r == 2)
        bfm_tap<T, 2>(xa[0], xa[1], in[0], in[1], w7, w5, w3, KC, a7, a5, a3);
      else
        bfm_tap<T, 1>(xa[0], xa[1], in[0], in[1], w7, w5, w3, KC, a7, a5, a3);
    }
  }

  // D[ch][row]: this lane has row lane & 15 of the fragment and channels nb * 64 + 16 tn + 4 (lane >> 4) + 0..3
#pragma unroll
  for (int rf = 0; rf < 2; ++rf) {
    if (m[rf] >= M) continue;
#pragma unroll
    for (int tn = 0; tn < BFM_NT; ++tn) {
      const int ch = nb * BFM_COLS + tn * 16 + (lane >> 4) * 4;
      const f32x4 b3 = *(const f32x4*)(bias3 + ch), b5 = *(const f32x4*)(bias3 + c + ch),
                  b7 = *(const f32x4*)(bias3 + 2 * c + ch);
      f32x4 v;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        v[i] = ((relu(a3[rf][tn][i] + b3[i]) + relu(a5[rf][tn][i] + b5[i])) + relu(a7[rf][tn][i] + b7[i])) * scale;
      *(u16x4*)(out + (size_t)m[rf] * c + ch) = T::pack4(v);
    }
  }
}

static bool bfm_width_ok(int c) { return c == 64 || c == 128 || c == 256 || c == 512; }

static bool bfm_shape_ok(int h, int w, int c) { return h >= 7 && h <= 14 && w >= 7 && w <= 14 && bfm_width_ok(c); }

}  // namespace fac

extern "C" size_t fac_bfm_packed_elems(int c) {
  return fac::bfm_width_ok(c) ? (size_t)fac::BFM_TAPS * c * c : 0;
}

extern "C" int fac_bfm_pack(int dtype, int c, const float* w3, const float* w5, const float* w7, uint16_t* out) {
  using namespace fac;
  if (!w3 || !w5 || !w7 || !out || (dtype != 0 && dtype != 1)) return FAC_ERR_ARG;
  if (!bfm_width_ok(c)) return FAC_ERR_SHAPE;
  const int KC = c / 32, NB = c / BFM_COLS;
  const float* src[3] = {w7, w5, w3};
  const int ks[3] = {7, 5, 3};
  for (int s = 0; s < 3; ++s) {
    const int k = ks[s], kk = k * k;
    const float* w = src[s];
    uint16_t* o = out + bfm_region(c, k);
    for (int nb = 0; nb < NB; ++nb)
      for (int tap = 0; tap < kk; ++tap)
        for (int kc = 0; kc < KC; ++kc)
          for (int tn = 0; tn < BFM_NT; ++tn)
            for (int l = 0; l < 64; ++l) {
              const int co = nb * BFM_COLS + tn * 16 + (l & 15), ci0 = kc * 32 + (l >> 4) * 8;
              for (int j = 0; j < 8; ++j) {
                const float v = w[((size_t)co * c + ci0 + j) * kk + tap];
                *o++ = dtype == 0 ? fac_host::f32_to_bf16(v) : fac_host::f32_to_f16(v);
              }
            }
  }
  return FAC_OK;
}

extern "C" int fac_bfm(int dtype, const void* x, int n, int h, int w, int c, const void* wpk, const float* bias3,
                       float scale, void* out, void* stream) {
  using namespace fac;
  if (!x || !wpk || !bias3 || !out || n <= 0 || (dtype != 0 && dtype != 1)) return FAC_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)wpk | (uintptr_t)bias3 | (uintptr_t)out) % 16) return FAC_ERR_ARG;
  if (!bfm_shape_ok(h, w, c)) return FAC_ERR_SHAPE;
  if ((long)n * h * w > 0x3fffffffL) return FAC_ERR_SHAPE;         // rows are indexed in 32 bits
  const size_t bytes = (size_t)n * h * w * c * 2;
  const uintptr_t xb = (uintptr_t)x, ob = (uintptr_t)out;
  if (xb < ob + bytes && ob < xb + bytes) return FAC_ERR_ARG;      // the kernel reads halos: not in place
  const int M = n * h * w;
  const dim3 grid((unsigned)((M + BFM_ROWS * (BFM_T / 64) - 1) / (BFM_ROWS * (BFM_T / 64))), (unsigned)(c / BFM_COLS));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0)
    bfm_k<BF16><<<grid, BFM_T, 0, st>>>((const uint16_t*)x, (const uint16_t*)wpk, bias3, (uint16_t*)out, M, h, w, c, scale);
  else
    bfm_k<F16><<<grid, BFM_T, 0, st>>>((const uint16_t*)x, (const uint16_t*)wpk, bias3, (uint16_t*)out, M, h, w, c, scale);
  return hipGetLastError() == hipSuccess ? FAC_OK : FAC_ERR_HIP;
}
