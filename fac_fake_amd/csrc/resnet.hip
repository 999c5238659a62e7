// ResNet BasicBlock kernels (CViT-main/ResKan/kan_resnet.py:11-65, :225-256):
//
//  * conv3x3_res: the block's second conv, Conv2d(3x3, stride 1, padding 1,
//    c -> c) + folded bn2 + identity (16-bit) + ReLU, as an implicit GEMM on
//    MFMA for the four maps of a ResNet-34: 56^2 x 64, 28^2 x 128, 14^2 x 256
//    and 7^2 x 512.
//  * avgpool_f32: the global average pool, 16-bit in, fp32 out (the KAN
//    head's input is never rounded to 16 bits).
//
// GEMM view: D[channel][pixel] = sum_k W[channel][k] * X[k][pixel], k = (32-
// channel chunk, tap, channel in chunk).  The weights are the MFMA's A operand
// and the pixels its B operand, so in the 16x16 accumulator layout (row =
// 4*(lane>>4) + reg, col = lane&15) a lane holds four consecutive channels of
// one pixel: bias, residual and output are 16-/8-byte vector accesses and the
// epilogue needs no LDS staging.
//
// As in conv.hip a workgroup stages the input halo of its pixels once per
// 32-channel chunk in LDS and reads all nine taps from it.  The next chunk's
// halo is fetched into registers while the current one is multiplied and
// written to the other LDS buffer afterwards: one __syncthreads() per chunk,
// plain loads and compiler-placed waits only (no global_load_lds, no
// hand-counted s_waitcnt).  Weight fragments go from global memory (L2)
// straight to VGPRs: they are packed per (chunk, tap, 16-channel tile) in
// lane order, 1 KiB each.
//
// Pixels of a workgroup:
//  * 56^2, 28^2, 14^2: a TH x TW box of one crop (8x28, 4x28, 14x14), halo
//    (TH+2) x (TW+2), zero outside the crop.
//  * 7^2: 49 positions per crop is no multiple of 16, so the GEMM rows run
//    over the whole batch, m = crop*49 + y*7 + x, and a workgroup takes MT
//    consecutive rows, which span up to NCR crops.  Each of those crops gets
//    its own zero-bordered 9x9 halo in LDS, so a pixel at x = 6 sees zeros,
//    never the next row's or the next crop's pixel.  The batch's last
//    workgroup is partial: rows >= n*49 read halo slot 0 of the workgroup's
//    first crop (always a real crop) and are not stored; halo slots of crops
//    >= n are zero-filled without a load.
//
// Every global access is predicated on its pixel lying inside the tensor; no
// load is issued for a position outside [0, n) x [0, h) x [0, h).
#include <hip/hip_runtime.h>

#include "../../include/fac_cvit.h"
#include "../../include/fac_ops.h"
#include "common.hpp"

namespace fac {

// H: map size; C: channels (cin == cout); TH x TW: the box (unused at 7^2);
// BN: output channels per workgroup; WM x WN: the 4 waves over pixel tiles x
// channel tiles; RT: 16-pixel tiles per wave.
template <class T, int H, int C, int TH, int TW, int BN, int WM, int WN, int RT>
__global__ __launch_bounds__(256) void conv3x3_res_k(const uint16_t* __restrict__ in,
                                                     const uint16_t* __restrict__ wpk,
                                                     const float* __restrict__ bias,
                                                     const uint16_t* __restrict__ res,
                                                     uint16_t* __restrict__ out, int n) {
  static_assert(WM * WN == 4, "four waves");
  constexpr bool CROSS = H == 7;
  constexpr int CT = BN / 16 / WN;                       // 16-channel tiles per wave
  constexpr int MT = 16 * RT * WM;                       // GEMM rows (pixels) per workgroup
  constexpr int HW = CROSS ? 9 : TW + 2;                 // halo row pitch
  constexpr int NCR = CROSS ? (MT + 47) / 49 + 1 : 1;    // crops MT consecutive rows can touch
  constexpr int NPOS = CROSS ? NCR * 81 : (TH + 2) * (TW + 2);
  constexpr int PLANE = (NPOS + 15) / 16 * 16;           // q-major planes of 16-byte pieces, pitch % 16 == 0
  constexpr int NPC = (PLANE * 4 + 255) / 256;           // 16-byte pieces per thread per chunk
  constexpr int NCHUNK = C / 32;
  constexpr int BX = H / (CROSS ? 1 : TW), BY = H / (CROSS ? 1 : TH);
  static_assert(CROSS || MT >= TH * TW, "the waves cover the box");
  static_assert(C % BN == 0 && BN % (16 * WN) == 0, "channel tiling");

  __shared__ u16x8 halo[2][4 * PLANE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int n0 = blockIdx.y * BN;

  // --- where this workgroup's pixels are
  int b = 0, y0 = 0, x0 = 0;          // box mode: crop and box origin
  long m0 = 0;                        // cross mode: first GEMM row, its crop
  int c0 = 0;
  if constexpr (CROSS) {
    m0 = (long)blockIdx.x * MT;
    c0 = (int)(m0 / 49);
  } else {
    b = blockIdx.x / (BX * BY);
    const int r = blockIdx.x - b * (BX * BY);
    y0 = (r / BX) * TH;
    x0 = (r % BX) * TW;
  }
  const long mtot = (long)n * 49;

  // --- halo staging: piece i -> 16 pixels x 4 quarter-chunks per wave, so a
  // quarter's 16 pixels land contiguously in its plane
  long src[NPC];                      // element offset of the piece at chunk 0, -1: zero, -2: no slot
#pragma unroll
  for (int j = 0; j < NPC; ++j) {
    const int i = tid + j * 256;
    const int q = (i >> 4) & 3, pos = (i >> 6) * 16 + (i & 15);
    long o = -2;
    if (pos < NPOS) {
      o = -1;
      if constexpr (CROSS) {
        const int lc = pos / 81, r = pos - lc * 81;
        const int y = r / 9 - 1, x = r % 9 - 1;
        const long crop = (long)c0 + lc;
        if (crop < n && y >= 0 && y < 7 && x >= 0 && x < 7) o = ((crop * 7 + y) * 7 + x) * C + q * 8;
      } else {
        const int y = y0 + pos / HW - 1, x = x0 + pos % HW - 1;
        if (y >= 0 && y < H && x >= 0 && x < H) o = (((long)b * H + y) * H + x) * C + q * 8;
      }
    }
    src[j] = o;
  }
  auto fetch = [&](int chunk, u16x8 (&v)[NPC]) {
#pragma unroll
    for (int j = 0; j < NPC; ++j) {
      v[j] = (u16x8){0, 0, 0, 0, 0, 0, 0, 0};
      if (src[j] >= 0) v[j] = *(const u16x8*)(in + src[j] + chunk * 32);
    }
  };
  auto put = [&](int buf, const u16x8 (&v)[NPC]) {
#pragma unroll
    for (int j = 0; j < NPC; ++j) {
      const int i = tid + j * 256;
      const int q = (i >> 4) & 3, pos = (i >> 6) * 16 + (i & 15);
      if (src[j] != -2) halo[buf][q * PLANE + pos] = v[j];
    }
  };

  // --- this lane's pixel in each of its tiles: halo slot and output offset
  int base[RT];
  long opix[RT];                      // element offset of the pixel's channel 0 in out / res, -1: not stored
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int m = (wm * RT + rt) * 16 + (lane & 15);
    if constexpr (CROSS) {
      const long gm = m0 + m;
      const bool ok = gm < mtot;
      const long g = ok ? gm : m0;
      const int crop = (int)(g / 49), r = (int)(g - (long)crop * 49);
      base[rt] = (crop - c0) * 81 + (r / 7) * 9 + r % 7;
      opix[rt] = ok ? gm * C : -1;
    } else {
      const bool ok = m < TH * TW;
      const int mm = ok ? m : 0;
      const int py = mm / TW, px = mm - py * TW;
      base[rt] = py * HW + px;
      opix[rt] = ok ? (((long)b * H + y0 + py) * H + x0 + px) * C : -1;
    }
    base[rt] += (lane >> 4) * PLANE;
  }

  f32x4 acc[RT][CT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // weight fragments: [chunk][tap][C/16 tiles][64 lanes][8]
  const u16x8* wfrag = (const u16x8*)wpk + (size_t)(n0 / 16 + wn * CT) * 64 + lane;

  {
    u16x8 v[NPC];
    fetch(0, v);
    put(0, v);
  }
  __syncthreads();

#pragma unroll 1
  for (int chunk = 0; chunk < NCHUNK; ++chunk) {
    const int buf = chunk & 1;
    u16x8 wf[9][CT];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) wf[tap][ct] = wfrag[((size_t)(chunk * 9 + tap) * (C / 16) + ct) * 64];
    u16x8 nxt[NPC];
    const bool more = chunk + 1 < NCHUNK;
    if (more) fetch(chunk + 1, nxt);
    // pixel fragments: a ring of XD reads in flight ahead of the MFMAs that
    // consume them (one wave per SIMD cannot hide an LDS read behind two MFMAs)
    constexpr int NS = 9 * RT, XD = 4;
    auto xread = [&](int s) { return halo[buf][base[s % RT] + ((s / RT) / 3) * HW + (s / RT) % 3]; };
    u16x8 xr[XD];
#pragma unroll
    for (int s = 0; s < XD; ++s) xr[s] = xread(s);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const u16x8 x = xr[s % XD];
      if (s + XD < NS) xr[s % XD] = xread(s + XD);
      __builtin_amdgcn_sched_barrier(0);   // the scheduler would sink the read back to its use
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[s % RT][ct] = T::mfma(wf[s / RT][ct], x, acc[s % RT][ct]);
    }
    if (more) put(buf ^ 1, nxt);
    __syncthreads();
  }

  // --- epilogue: + bias + residual (fp32), ReLU, one rounding on the store
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int ch = n0 + (wn * CT + ct) * 16 + (lane >> 4) * 4;
    const f32x4 bv = *(const f32x4*)(bias + ch);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      if (opix[rt] < 0) continue;
      const u16x4 r = *(const u16x4*)(res + opix[rt] + ch);
      f32x4 y;
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = relu(acc[rt][ct][j] + bv[j] + T::to_f32(r[j]));
      *(u16x4*)(out + opix[rt] + ch) = T::pack4(y);
    }
  }
}

// Mean over s of x [n][s][c] (16-bit) -> y [n][c] fp32.  One thread per 8
// channels of one row block: a sequential fp32 sum over s in index order, so
// the result does not depend on the launch shape; no atomics.
template <class T>
__global__ __launch_bounds__(256) void avgpool_f32_k(const uint16_t* __restrict__ x, float* __restrict__ y, long n,
                                                     int s, int c) {
  const int c8 = c / 8;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * c8) return;
  const long b = i / c8;
  const int g = (int)(i - b * c8);
  const uint16_t* p = x + (b * s) * c + g * 8;
  float sum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < s; ++k) {
    const u16x8 v = *(const u16x8*)(p + (long)k * c);
#pragma unroll
    for (int j = 0; j < 8; ++j) sum[j] += T::to_f32(v[j]);
  }
  const float inv = 1.0f / (float)s;
  float* o = y + b * c + g * 8;
  *(f32x4*)o = (f32x4){sum[0] * inv, sum[1] * inv, sum[2] * inv, sum[3] * inv};
  *(f32x4*)(o + 4) = (f32x4){sum[4] * inv, sum[5] * inv, sum[6] * inv, sum[7] * inv};
}

static bool res_shape_ok(int h, int c) {
  return (h == 56 && c == 64) || (h == 28 && c == 128) || (h == 14 && c == 256) || (h == 7 && c == 512);
}

template <class T>
static void launch_res(const uint16_t* in, const uint16_t* wpk, const float* bias, const uint16_t* res, uint16_t* out,
                       int n, int h, hipStream_t st) {
  switch (h) {
    case 56:   // 8x28 box, 64 channels, 2x2 waves of 7 x 2 tiles
      conv3x3_res_k<T, 56, 64, 8, 28, 64, 2, 2, 7><<<dim3(n * 14, 1), 256, 0, st>>>(in, wpk, bias, res, out, n);
      break;
    case 28:   // 4x28 box, 128 channels, 1x4 waves of 7 x 2 tiles
      conv3x3_res_k<T, 28, 128, 4, 28, 128, 1, 4, 7><<<dim3(n * 7, 1), 256, 0, st>>>(in, wpk, bias, res, out, n);
      break;
    case 14:   // 14x14 box (196 of 208 rows), 128 of 256 channels, 1x4 waves of 13 x 2 tiles
      conv3x3_res_k<T, 14, 256, 14, 14, 128, 1, 4, 13><<<dim3(n, 2), 256, 0, st>>>(in, wpk, bias, res, out, n);
      break;
    default: { // 7^2: 208 rows of the batch's n*49, 128 of 512 channels, 1x4 waves of 13 x 2 tiles
      const unsigned gx = (unsigned)(((long)n * 49 + 207) / 208);
      conv3x3_res_k<T, 7, 512, 7, 7, 128, 1, 4, 13><<<dim3(gx, 4), 256, 0, st>>>(in, wpk, bias, res, out, n);
    }
  }
}

}  // namespace fac

extern "C" {

size_t fac_conv3x3_res_packed_elems(int h, int c) { return fac::res_shape_ok(h, c) ? (size_t)c * c * 9 : 0; }

int fac_conv3x3_res_pack(int dtype, int h, int c, const float* w, uint16_t* out) {
  if (!w || !out || (dtype != 0 && dtype != 1)) return FAC_ERR_ARG;
  if (!fac::res_shape_ok(h, c)) return FAC_ERR_SHAPE;
  // [chunk][tap][16-channel tile][lane][8]: lane l of a tile holds output
  // channel tile*16 + (l & 15), input channels chunk*32 + (l >> 4)*8 + 0..7
  size_t q = 0;
  for (int chunk = 0; chunk < c / 32; ++chunk)
    for (int tap = 0; tap < 9; ++tap)
      for (int tile = 0; tile < c / 16; ++tile)
        for (int l = 0; l < 64; ++l)
          for (int j = 0; j < 8; ++j) {
            const int co = tile * 16 + (l & 15), ci = chunk * 32 + (l >> 4) * 8 + j;
            const float v = w[((size_t)co * c + ci) * 9 + tap];
            out[q++] = dtype == 0 ? fac_host::f32_to_bf16(v) : fac_host::f32_to_f16(v);
          }
  return FAC_OK;
}

int fac_conv3x3_res(int dtype, const void* in, const void* wpk, const float* bias, const void* residual, void* out,
                    int n, int h, int c, void* stream) {
  if (!in || !wpk || !bias || !residual || !out || n <= 0 || (dtype != 0 && dtype != 1)) return FAC_ERR_ARG;
  if (!fac::res_shape_ok(h, c)) return FAC_ERR_SHAPE;
  if ((long)n * 14 > 0x7fffffffL) return FAC_ERR_SHAPE;   // the grid's x dimension (56^2: 14 boxes per crop)
  if (dtype == 0)
    fac::launch_res<fac::BF16>((const uint16_t*)in, (const uint16_t*)wpk, bias, (const uint16_t*)residual,
                               (uint16_t*)out, n, h, (hipStream_t)stream);
  else
    fac::launch_res<fac::F16>((const uint16_t*)in, (const uint16_t*)wpk, bias, (const uint16_t*)residual,
                              (uint16_t*)out, n, h, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? FAC_OK : FAC_ERR_HIP;
}

int fac_avgpool_f32(int dtype, const void* x, int n, int s, int c, float* y, void* stream) {
  if (!x || !y || n <= 0 || (dtype != 0 && dtype != 1)) return FAC_ERR_ARG;
  if (s < 1 || c < 8 || c % 8) return FAC_ERR_SHAPE;
  const long items = (long)n * (c / 8);
  const long blocks = (items + 255) / 256;
  if (blocks > 0x7fffffffL) return FAC_ERR_SHAPE;
  if (dtype == 0)
    fac::avgpool_f32_k<fac::BF16><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>((const uint16_t*)x, y, n, s, c);
  else
    fac::avgpool_f32_k<fac::F16><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>((const uint16_t*)x, y, n, s, c);
  return hipGetLastError() == hipSuccess ? FAC_OK : FAC_ERR_HIP;
}

}  // extern "C"
