// GGCA (Global Grouped Coordinate Attention, CViT-main/model/cvit_GGCA_ADD*.py
// :144-207) fused with the caller's combine, behind fac_ggca_apply:
//
//   att_h[y][c] = sigmoid(z(mean_x x) + z(max_x x)),  att_w[x][c] likewise over y
//   z           = 1x1 (cg -> cg/16), BatchNorm (eval, eps 1e-5), ReLU, 1x1 back,
//                 per channel group
//   g           = (x * att_h) * att_w                  (the reference's order)
//   out         = op == 0 ? x * g : x + g              (one 16-bit rounding)
//                 fac_ggca_scale (LDS route only): out = g, the module's own
//                 output, for the classes that assign x = GGCA(x)
//
// on 16-bit channels-last maps x [n][h][w][c], fp32 in between.  Two routes,
// chosen from (h, w, c, groups) alone so that a crop's bits never depend on
// the batch it sits in:
//
//   LDS        maps inside fac_ggca's limits (the 7x7x512 site of most CViT
//              variants): ggca_lds_k, the arithmetic of ops.hip's ggca_k
//              statement for statement, plus the op == 1 epilogue.  One
//              workgroup per (image, group) holds the group's map in LDS.
//   streaming  larger maps (RepBn3: 56x56x64 after features1, 401 KB per
//              crop), three launches over a library-owned fp32 workspace:
//     ggca_pool_k   one workgroup per (image, band of 16 rows, slab of 64
//                   channels).  A thread owns one 16-byte channel vector of
//                   the x positions xg, xg + 32: every row of the band is
//                   read once, fully coalesced (a pixel's slab is one
//                   128-byte line).  Row mean / max: the thread's two
//                   positions, a butterfly over the 8 positions of its wave,
//                   then the four waves in wave order.  Column sum / max:
//                   kept in registers down the band and stored per band.
//     ggca_att_k    one workgroup per (image, group, 16 positions): reduces
//                   the column partials in band order, runs the shared MLP
//                   on the avg and max vector of each position (ggca_k's
//                   loops) and stores att = sigmoid(z_avg + z_max) [h + w][c].
//     ggca_apply_k  element-wise, one 16-byte vector per thread.
//   The map is read twice and written once; the partials are 8/16 bytes per
//   2-byte element.  No atomics; every sum has one order fixed by (h, w, c).
//
// Workspace: per (device, stream), grown with hipMalloc when a call needs more
// than any before it on that stream and never freed or moved afterwards (a
// captured graph keeps pointing at the buffer it was captured with).  A call
// that would have to grow it while its stream is capturing returns
// FAC_ERR_OOM: run the shape once on that stream before capturing.
#include <mutex>
#include <vector>

#include "common.hpp"
#include "fac_cvit.h"
#include "fac_ops.h"

namespace fac {

// ---------------------------------------------------------------- LDS route
// ops.hip's ggca_k with the combine as a template parameter.  OP 0 must stay
// bit-identical to fac_ggca: keep every statement up to the epilogue as it is
// there.
template <class T, int OP>
__global__ __launch_bounds__(256) void ggca_lds_k(const uint16_t* __restrict__ x, int H, int W, int C, int groups,
                                                  const float* __restrict__ w1, const float* __restrict__ b1,
                                                  const float* __restrict__ bn4, const float* __restrict__ w2,
                                                  const float* __restrict__ b2, uint16_t* __restrict__ out) {
  constexpr int MAXP = 16 * 16, MAXCG = 256, MAXV = 64, MAXCR = 16;
  __shared__ float xs[MAXP * MAXCG / 4];      // H*W*CG <= 16384 floats (64 KB)
  __shared__ float pv[MAXV * MAXCG / 2];      // (2H + 2W) pooled vectors x CG
  __shared__ float hid[MAXV * MAXCR];
  const int img = blockIdx.x / groups, gr = blockIdx.x - img * groups;
  const int CG = C / groups, CR = CG / 16, P = H * W, NV = 2 * H + 2 * W;
  const int tid = threadIdx.x;
  const uint16_t* xb = x + (size_t)img * P * C + gr * CG;
  for (int i = tid; i < P * CG; i += 256) {
    const int pix = i / CG, c = i - pix * CG;
    xs[i] = T::to_f32(xb[(size_t)pix * C + c]);
  }
  __syncthreads();
  // pooled vectors: v = 0..H-1 h_avg, H..2H-1 h_max, 2H..2H+W-1 w_avg, 2H+W.. w_max
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
  for (int i = tid; i < NV * CR; i += 256) {  // 1x1 CG -> CR, BN (eval), ReLU
    const int v = i / CR, r = i - v * CR;
    float a = 0.f;
    for (int c = 0; c < CG; ++c) a += w1[r * CG + c] * pv[v * CG + c];
    a += b1[r];
    const float inv = 1.0f / sqrtf(bn4[CR + r] + 1e-5f);
    a = (a - bn4[r]) * inv * bn4[2 * CR + r] + bn4[3 * CR + r];
    hid[i] = fmaxf(a, 0.f);
  }
  __syncthreads();
  for (int i = tid; i < NV * CG; i += 256) {  // 1x1 CR -> CG
    const int v = i / CG, c = i - v * CG;
    float a = 0.f;
    for (int r = 0; r < CR; ++r) a += w2[c * CR + r] * hid[v * CR + r];
    pv[i] = a + b2[c];
  }
  __syncthreads();
  uint16_t* ob = out + (size_t)img * P * C + gr * CG;
  for (int i = tid; i < P * CG; i += 256) {
    const int pix = i / CG, c = i - pix * CG;
    const int y = pix / W, xx = pix - y * W;
    const float ah = 1.0f / (1.0f + expf(-(pv[y * CG + c] + pv[(H + y) * CG + c])));
    const float aw = 1.0f / (1.0f + expf(-(pv[(2 * H + xx) * CG + c] + pv[(2 * H + W + xx) * CG + c])));
    const float v = xs[i];
    if (OP == 0) ob[(size_t)pix * C + c] = T::from_f32(v * ((v * ah) * aw));
    else if (OP == 1) ob[(size_t)pix * C + c] = T::from_f32(v + (v * ah) * aw);
    else ob[(size_t)pix * C + c] = T::from_f32((v * ah) * aw);   // fac_ggca_scale: GGCA(x) itself
  }
}

// ---------------------------------------------------------------- streaming route
constexpr int GG_T = 256;              // threads of every streaming kernel
constexpr int GG_RB = 16;              // rows per band of the pooling pass
constexpr int GG_SV = 8;               // 16-byte vectors per channel slab (64 channels, one 128-byte line a pixel)
constexpr int GG_XP = GG_T / GG_SV;    // 32 x positions per pass over a row
constexpr int GG_NX = 2;               // passes per row: w <= GG_XP * GG_NX
constexpr int GG_MAX_HW = GG_XP * GG_NX;
constexpr int GG_PC = 16;              // positions (rows or columns) per ggca_att_k workgroup
constexpr int GG_MAX_CG = 256, GG_MAX_CR = 16;

// Workspace of one image, in floats (C = channels):
//   rowp [2][H][C]        row mean, row max                       (ggca_pool_k)
//   colp [nb][2][W][C]    column sum, column max of each band     (ggca_pool_k)
//   att  [H + W][C]       att_h rows, then att_w columns          (ggca_att_k)
__host__ __device__ inline int gg_bands(int H) { return (H + GG_RB - 1) / GG_RB; }
__host__ __device__ inline size_t gg_colp_off(int H, int C) { return (size_t)2 * H * C; }
__host__ __device__ inline size_t gg_att_off(int H, int W, int C) {
  return gg_colp_off(H, C) + (size_t)gg_bands(H) * 2 * W * C;
}
__host__ __device__ inline size_t gg_img_floats(int H, int W, int C) { return gg_att_off(H, W, C) + (size_t)(H + W) * C; }

template <class T>
__global__ __launch_bounds__(GG_T) void ggca_pool_k(const u16x8* __restrict__ x, int H, int W, int cv, int ns,
                                                    float* __restrict__ ws) {
  __shared__ float rs[GG_RB][4][GG_SV * 8], rm[GG_RB][4][GG_SV * 8];   // per row and wave: 64 channel sums / maxima
  const int nb = gg_bands(H), C = cv * 8;
  int b = blockIdx.x;
  const int slab = b % ns;
  b /= ns;
  const int band = b % nb, img = b / nb;
  const int tid = threadIdx.x, j = tid & (GG_SV - 1), xg = tid >> 3, wave = tid >> 6;
  const int jv = slab * GG_SV + j;
  const bool active = jv < cv;
  const int y0 = band * GG_RB, rows = min(GG_RB, H - y0);
  const u16x8* xb = x + (size_t)img * H * W * cv;
  float* wsb = ws + (size_t)img * gg_img_floats(H, W, C);
  float cs[GG_NX][8], cm[GG_NX][8];
#pragma unroll
  for (int k = 0; k < GG_NX; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) cs[k][e] = 0.f, cm[k][e] = -INFINITY;
  for (int r = 0; r < rows; ++r) {
    float s[8], m[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = 0.f, m[e] = -INFINITY;
#pragma unroll
    for (int k = 0; k < GG_NX; ++k) {
      const int xx = xg + k * GG_XP;
      if (active && xx < W) {
        const u16x8 v = xb[((size_t)(y0 + r) * W + xx) * cv + jv];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float f = T::to_f32(v[e]);
          s[e] += f;
          m[e] = fmaxf(m[e], f);
          cs[k][e] += f;
          cm[k][e] = fmaxf(cm[k][e], f);
        }
      }
    }
    // the 8 positions of this wave (lane bits 3..5); lanes 0..7 end with vector j = lane
#pragma unroll
    for (int o = 8; o <= 32; o <<= 1)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        s[e] += __shfl_xor(s[e], o, 64);
        m[e] = fmaxf(m[e], __shfl_xor(m[e], o, 64));
      }
    if ((tid & 63) < GG_SV) {
#pragma unroll
      for (int e = 0; e < 8; ++e) rs[r][wave][j * 8 + e] = s[e], rm[r][wave][j * 8 + e] = m[e];
    }
  }
  __syncthreads();
  for (int i = tid; i < rows * GG_SV * 8; i += GG_T) {
    const int r = i >> 6, cl = i & 63, ch = slab * GG_SV * 8 + cl;
    if (ch < C) {
      const float sum = ((rs[r][0][cl] + rs[r][1][cl]) + rs[r][2][cl]) + rs[r][3][cl];
      const float mx = fmaxf(fmaxf(rm[r][0][cl], rm[r][1][cl]), fmaxf(rm[r][2][cl], rm[r][3][cl]));
      wsb[(size_t)(y0 + r) * C + ch] = sum / (float)W;
      wsb[(size_t)(H + y0 + r) * C + ch] = mx;
    }
  }
  float* colp = wsb + gg_colp_off(H, C) + (size_t)band * 2 * W * C;
#pragma unroll
  for (int k = 0; k < GG_NX; ++k) {
    const int xx = xg + k * GG_XP;
    if (active && xx < W) {
      f32x4* ps = (f32x4*)(colp + (size_t)xx * C + jv * 8);
      f32x4* pm = (f32x4*)(colp + (size_t)(W + xx) * C + jv * 8);
      ps[0] = (f32x4){cs[k][0], cs[k][1], cs[k][2], cs[k][3]};
      ps[1] = (f32x4){cs[k][4], cs[k][5], cs[k][6], cs[k][7]};
      pm[0] = (f32x4){cm[k][0], cm[k][1], cm[k][2], cm[k][3]};
      pm[1] = (f32x4){cm[k][4], cm[k][5], cm[k][6], cm[k][7]};
    }
  }
}

__global__ __launch_bounds__(GG_T) void ggca_att_k(int H, int W, int C, int groups, const float* __restrict__ w1,
                                                   const float* __restrict__ b1, const float* __restrict__ bn4,
                                                   const float* __restrict__ w2, const float* __restrict__ b2,
                                                   float* __restrict__ ws) {
  __shared__ float pv[2 * GG_PC * GG_MAX_CG];   // vector 2q = avg, 2q + 1 = max of position q0 + q
  __shared__ float hid[2 * GG_PC * GG_MAX_CR];
  const int npc = (H + W + GG_PC - 1) / GG_PC, nb = gg_bands(H);
  int b = blockIdx.x;
  const int chunk = b % npc;
  b /= npc;
  const int gr = b % groups, img = b / groups;
  const int CG = C / groups, CR = CG / 16, tid = threadIdx.x;
  const int q0 = chunk * GG_PC, nq = min(GG_PC, H + W - q0), NV = 2 * nq;
  float* wsb = ws + (size_t)img * gg_img_floats(H, W, C);
  const float* colp = wsb + gg_colp_off(H, C);
  for (int i = tid; i < NV * CG; i += GG_T) {
    const int v = i / CG, c = i - v * CG, q = q0 + (v >> 1), mx = v & 1, ch = gr * CG + c;
    float acc;
    if (q < H) {
      acc = wsb[(size_t)(mx * H + q) * C + ch];
    } else {
      const float* p = colp + (size_t)(mx * W + q - H) * C + ch;
      acc = p[0];
      for (int k = 1; k < nb; ++k) {
        const float e = p[(size_t)k * 2 * W * C];
        acc = mx ? fmaxf(acc, e) : acc + e;
      }
      if (!mx) acc = acc / (float)H;
    }
    pv[i] = acc;
  }
  __syncthreads();
  for (int i = tid; i < NV * CR; i += GG_T) {  // 1x1 CG -> CR, BN (eval), ReLU
    const int v = i / CR, r = i - v * CR;
    float a = 0.f;
    for (int c = 0; c < CG; ++c) a += w1[r * CG + c] * pv[v * CG + c];
    a += b1[r];
    const float inv = 1.0f / sqrtf(bn4[CR + r] + 1e-5f);
    a = (a - bn4[r]) * inv * bn4[2 * CR + r] + bn4[3 * CR + r];
    hid[i] = fmaxf(a, 0.f);
  }
  __syncthreads();
  for (int i = tid; i < NV * CG; i += GG_T) {  // 1x1 CR -> CG
    const int v = i / CG, c = i - v * CG;
    float a = 0.f;
    for (int r = 0; r < CR; ++r) a += w2[c * CR + r] * hid[v * CR + r];
    pv[i] = a + b2[c];
  }
  __syncthreads();
  float* att = wsb + gg_att_off(H, W, C);
  for (int i = tid; i < nq * CG; i += GG_T) {
    const int q = i / CG, c = i - q * CG;
    att[(size_t)(q0 + q) * C + gr * CG + c] = 1.0f / (1.0f + expf(-(pv[2 * q * CG + c] + pv[(2 * q + 1) * CG + c])));
  }
}

template <class T, int OP>
__global__ __launch_bounds__(GG_T) void ggca_apply_k(const u16x8* __restrict__ x, int H, int W, int cv, int bpi,
                                                     const float* __restrict__ ws, u16x8* __restrict__ out) {
  const int img = blockIdx.x / bpi, vpi = H * W * cv, C = cv * 8;
  const int i = (blockIdx.x - img * bpi) * GG_T + threadIdx.x;
  if (i >= vpi) return;
  const int pix = i / cv, j = i - pix * cv, y = pix / W, xx = pix - y * W;
  const float* att = ws + (size_t)img * gg_img_floats(H, W, C) + gg_att_off(H, W, C);
  const f32x4* ah = (const f32x4*)(att + (size_t)y * C + j * 8);
  const f32x4* aw = (const f32x4*)(att + (size_t)(H + xx) * C + j * 8);
  const f32x4 h0 = ah[0], h1 = ah[1], w0 = aw[0], w1 = aw[1];
  const u16x8 v = x[(size_t)img * vpi + i];
  u16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float f = T::to_f32(v[e]);
    const float g = (f * (e < 4 ? h0[e & 3] : h1[e & 3])) * (e < 4 ? w0[e & 3] : w1[e & 3]);
    o[e] = T::from_f32(OP == 0 ? f * g : f + g);
  }
  out[(size_t)img * vpi + i] = o;
}

// One grow-only fp32 buffer per (device, stream); see the header comment.
struct GgcaWs {
  int dev;
  hipStream_t st;
  float* p;
  size_t floats;
};

static float* ggca_workspace(hipStream_t st, size_t floats, int* status) {
  static std::mutex mu;
  static std::vector<GgcaWs> all;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    *status = FAC_ERR_HIP;
    return nullptr;
  }
  std::lock_guard<std::mutex> lock(mu);
  GgcaWs* e = nullptr;
  for (auto& w : all)
    if (w.dev == dev && w.st == st) e = &w;
  if (e && e->floats >= floats) return e->p;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap) != hipSuccess) {
    *status = FAC_ERR_HIP;
    return nullptr;
  }
  float* p = nullptr;
  if (cap != hipStreamCaptureStatusNone || hipMalloc((void**)&p, floats * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    *status = FAC_ERR_OOM;
    return nullptr;
  }
  // the old buffer stays allocated: a graph captured earlier still uses it
  if (e) e->p = p, e->floats = floats;
  else all.push_back({dev, st, p, floats});
  return p;
}

inline bool ggca_lds_shape(int h, int w, int cg) {   // fac_ggca's limits
  return h <= 16 && w <= 16 && cg <= 256 && h * w * cg <= 16384 && (2 * h + 2 * w) * cg <= 8192 &&
         2 * h + 2 * w <= 64;
}

}  // namespace fac

extern "C" {

int fac_ggca_apply_route(int h, int w, int c, int groups) {
  if (h <= 0 || w <= 0 || c <= 0 || groups <= 0 || c % groups) return 0;
  const int cg = c / groups;
  if (cg % 16 || cg > fac::GG_MAX_CG) return 0;
  if (fac::ggca_lds_shape(h, w, cg)) return 1;
  return h <= fac::GG_MAX_HW && w <= fac::GG_MAX_HW && c <= 2048 ? 2 : 0;
}

int fac_ggca_apply(int dtype, const void* x, int n, int h, int w, int c, int groups, const float* w1, const float* b1,
                   const float* bn4, const float* w2, const float* b2, int op, void* out, void* stream) {
  using namespace fac;
  if (!x || !out || !w1 || !b1 || !bn4 || !w2 || !b2 || n <= 0 || h <= 0 || w <= 0 || c <= 0 || groups <= 0 ||
      c % groups || (dtype != FAC_DTYPE_BF16 && dtype != FAC_DTYPE_F16) || (op != 0 && op != 1))
    return FAC_ERR_ARG;
  const int route = fac_ggca_apply_route(h, w, c, groups);
  if (route == 0) return FAC_ERR_SHAPE;
  const hipStream_t st = (hipStream_t)stream;
  const bool bf = dtype == FAC_DTYPE_BF16;
  if (route == 1) {
    if ((long long)n * groups > 0x7fffffffLL) return FAC_ERR_SHAPE;
    const uint16_t* xi = (const uint16_t*)x;
    uint16_t* xo = (uint16_t*)out;
    const int blocks = n * groups;
    if (bf) {
      if (op == 0) ggca_lds_k<BF16, 0><<<blocks, 256, 0, st>>>(xi, h, w, c, groups, w1, b1, bn4, w2, b2, xo);
      else ggca_lds_k<BF16, 1><<<blocks, 256, 0, st>>>(xi, h, w, c, groups, w1, b1, bn4, w2, b2, xo);
    } else {
      if (op == 0) ggca_lds_k<F16, 0><<<blocks, 256, 0, st>>>(xi, h, w, c, groups, w1, b1, bn4, w2, b2, xo);
      else ggca_lds_k<F16, 1><<<blocks, 256, 0, st>>>(xi, h, w, c, groups, w1, b1, bn4, w2, b2, xo);
    }
    return hipGetLastError() == hipSuccess ? FAC_OK : FAC_ERR_HIP;
  }
  if (((uintptr_t)x | (uintptr_t)out) & 15) return FAC_ERR_ARG;   // 16-byte vector loads and stores
  const int cv = c / 8, ns = (cv + GG_SV - 1) / GG_SV, nb = gg_bands(h), npc = (h + w + GG_PC - 1) / GG_PC;
  const int bpi = (h * w * cv + GG_T - 1) / GG_T;
  const long long most = (long long)n * (bpi > nb * ns ? (bpi > groups * npc ? bpi : groups * npc)
                                                       : (nb * ns > groups * npc ? nb * ns : groups * npc));
  if (most > 0x7fffffffLL) return FAC_ERR_SHAPE;
  int status = FAC_OK;
  float* ws = ggca_workspace(st, (size_t)n * gg_img_floats(h, w, c), &status);
  if (!ws) return status;
  const u16x8* xi = (const u16x8*)x;
  u16x8* xo = (u16x8*)out;
  if (bf) ggca_pool_k<BF16><<<n * nb * ns, GG_T, 0, st>>>(xi, h, w, cv, ns, ws);
  else ggca_pool_k<F16><<<n * nb * ns, GG_T, 0, st>>>(xi, h, w, cv, ns, ws);
  ggca_att_k<<<n * groups * npc, GG_T, 0, st>>>(h, w, c, groups, w1, b1, bn4, w2, b2, ws);
  if (bf) {
    if (op == 0) ggca_apply_k<BF16, 0><<<n * bpi, GG_T, 0, st>>>(xi, h, w, cv, bpi, ws, xo);
    else ggca_apply_k<BF16, 1><<<n * bpi, GG_T, 0, st>>>(xi, h, w, cv, bpi, ws, xo);
  } else {
    if (op == 0) ggca_apply_k<F16, 0><<<n * bpi, GG_T, 0, st>>>(xi, h, w, cv, bpi, ws, xo);
    else ggca_apply_k<F16, 1><<<n * bpi, GG_T, 0, st>>>(xi, h, w, cv, bpi, ws, xo);
  }
  return hipGetLastError() == hipSuccess ? FAC_OK : FAC_ERR_HIP;
}

// GGCA(x) alone, out = (x * att_h) * att_w: the LDS route with no combine.
int fac_ggca_scale(int dtype, const void* x, int n, int h, int w, int c, int groups, const float* w1, const float* b1,
                   const float* bn4, const float* w2, const float* b2, void* out, void* stream) {
  using namespace fac;
  if (!x || !out || !w1 || !b1 || !bn4 || !w2 || !b2 || n <= 0 || h <= 0 || w <= 0 || c <= 0 || groups <= 0 ||
      c % groups || (dtype != FAC_DTYPE_BF16 && dtype != FAC_DTYPE_F16))
    return FAC_ERR_ARG;
  if (fac_ggca_apply_route(h, w, c, groups) != 1 || (long long)n * groups > 0x7fffffffLL) return FAC_ERR_SHAPE;
  const hipStream_t st = (hipStream_t)stream;
  const uint16_t* xi = (const uint16_t*)x;
  uint16_t* xo = (uint16_t*)out;
  if (dtype == FAC_DTYPE_BF16) ggca_lds_k<BF16, 2><<<n * groups, 256, 0, st>>>(xi, h, w, c, groups, w1, b1, bn4, w2, b2, xo);
  else ggca_lds_k<F16, 2><<<n * groups, 256, 0, st>>>(xi, h, w, c, groups, w1, b1, bn4, w2, b2, xo);
  return hipGetLastError() == hipSuccess ? FAC_OK : FAC_ERR_HIP;
}

}  // extern "C"
