// The iFormer / MSCA blocks of msca_S3D (sx_exp_deepfakedetect-master/S3D/
// new_model/{iformer_3d,msca_3d,Conv3d}.py) on 16-bit channels-last maps
// [n][t][h][w][ld] -- the layers that are no dense contraction:
//
//   fac_dwsep3d       DWSepConv3d: depthwise (1,k,k) then depthwise (kt,1,1)
//                     (zero padding, no bias, nothing in between), folded
//                     BatchNorm, ReLU6, then nothing | a second affine | GELU
//   fac_bn_maxpool3d  per-channel affine (BatchNorm) applied on load, then
//                     MaxPool3d((kt,3,3), 1, (kt/2,1,1))
//   fac_ew            the element-wise steps around the 1x1x1 convs
//
// Every operand takes a leading dimension and a channel offset, so a channel
// slice is read in place and a result lands in its slot of a wider tensor.
// One thread owns 8 consecutive channels (one 16-byte load / store) of one
// position; threads run along the channels first, so a wavefront reads
// consecutive 16-byte vectors of a position.  Everything between the 16-bit
// load and the one 16-bit conversion is fp32, in a fixed order that depends on
// the position alone: a clip's result does not depend on n or on its place in
// the batch.  No LDS, no atomics; the maps of this model (10x28x28 and
// 5x14x14) stay in L2, where the window's re-reads hit.
#include "common.hpp"
#include "fac_cvit.h"
#include "fac_ops.h"

namespace fac {

constexpr int MSCA_T = 256;

__device__ __forceinline__ float relu6f(float v) { return fminf(fmaxf(v, 0.f), 6.f); }
// nn.GELU() (approximate='none'): x * 0.5 * (1 + erf(x / sqrt(2)))
__device__ __forceinline__ float gelu_erf(float v) { return v * 0.5f * (1.f + erff(v * 0.70710678118654752440f)); }

__device__ __forceinline__ void ld8f(const float* p, float (&v)[8]) {
  const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = a[k];
    v[4 + k] = b[k];
  }
}

template <class DT>
__device__ __forceinline__ void store8(void* out, size_t e, const float (&v)[8], bool f32) {
  if (f32) {
    float* o = (float*)out + e;
    *(f32x4*)o = (f32x4){v[0], v[1], v[2], v[3]};
    *(f32x4*)(o + 4) = (f32x4){v[4], v[5], v[6], v[7]};
  } else {
    u16x8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = DT::from_f32(v[k]);
    *(u16x8*)((uint16_t*)out + e) = o;
  }
}

// idx -> (position, first channel of the thread's vector).  32-bit division
// when the launch has under 2^32 threads (every launch of the model): the
// 64-bit one costs some 40 instructions per thread, felt by the element-wise ops.
__device__ __forceinline__ void split_idx(size_t idx, size_t total, int cv, size_t& pos, int& c0) {
  if (total <= 0xffffffffULL) {
    const unsigned i = (unsigned)idx, p = i / (unsigned)cv;
    pos = p;
    c0 = (int)(i - p * (unsigned)cv) * 8;
  } else {
    pos = idx / cv;
    c0 = (int)(idx % cv) * 8;
  }
}
// position -> (clip, frame, row, column) of a [n][t][h][w] map
__device__ __forceinline__ void split_pos(size_t pos, size_t total, int t, int h, int w, size_t& b, int& tt, int& y, int& x) {
  if (total <= 0xffffffffULL) {
    unsigned q = (unsigned)pos;
    x = (int)(q % (unsigned)w), q /= (unsigned)w;
    y = (int)(q % (unsigned)h), q /= (unsigned)h;
    tt = (int)(q % (unsigned)t), b = q / (unsigned)t;
  } else {
    size_t q = pos;
    x = (int)(q % w), q /= w;
    y = (int)(q % h), q /= h;
    tt = (int)(q % t), b = q / t;
  }
}

struct DwArgs {
  const uint16_t* in;
  const float *ws, *wt, *scale, *shift, *scale2, *shift2;
  void* out;
  size_t total;   // n*t*h*w * (c/8) threads with work
  int ldi, i_off, t, h, w, c, act, ldo, o_off, out_f32;
};

// acc = sum over dt of wt[dt] * (sum over dy, dx of ws[dy][dx] * x): the
// reference's own order (the whole spatial conv, then the temporal one).
// Taps outside the map are skipped (zero padding), so a window larger than
// the map (7x7 on 4x4, T < kt) is right by construction.
template <class DT, int K, int KT>
__global__ __launch_bounds__(MSCA_T) void dwsep_k(const DwArgs A) {
  const size_t idx = (size_t)blockIdx.x * MSCA_T + threadIdx.x;
  if (idx >= A.total) return;
  size_t pos, b;
  int c0, x, y, tt;
  split_idx(idx, A.total, A.c >> 3, pos, c0);
  split_pos(pos, A.total, A.t, A.h, A.w, b, tt, y, x);
  float acc[8] = {};
#pragma unroll
  for (int dt = 0; dt < KT; ++dt) {
    const int tz = tt + dt - KT / 2;
    if (tz < 0 || tz >= A.t) continue;
    float sp[8] = {};
#pragma unroll
    for (int dy = 0; dy < K; ++dy) {
      const int yy = y + dy - K / 2;
      if (yy < 0 || yy >= A.h) continue;
#pragma unroll
      for (int dx = 0; dx < K; ++dx) {
        const int xx = x + dx - K / 2;
        if (xx < 0 || xx >= A.w) continue;
        const size_t p = ((b * A.t + tz) * A.h + yy) * A.w + xx;
        const u16x8 v = *(const u16x8*)(A.in + p * A.ldi + A.i_off + c0);
        float wv[8];
        ld8f(A.ws + (size_t)(dy * K + dx) * A.c + c0, wv);
#pragma unroll
        for (int k = 0; k < 8; ++k) sp[k] += wv[k] * DT::to_f32(v[k]);
      }
    }
    if (KT == 1) {
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = sp[k];
    } else {
      float tv[8];
      ld8f(A.wt + (size_t)dt * A.c + c0, tv);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += tv[k] * sp[k];
    }
  }
  float s[8], sh[8];
  ld8f(A.scale + c0, s);
  ld8f(A.shift + c0, sh);
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = relu6f(acc[k] * s[k] + sh[k]);
  if (A.act == FAC_DWSEP_AFFINE2) {
    ld8f(A.scale2 + c0, s);
    ld8f(A.shift2 + c0, sh);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = acc[k] * s[k] + sh[k];
  } else if (A.act == FAC_DWSEP_GELU) {
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = gelu_erf(acc[k]);
  }
  store8<DT>(A.out, pos * A.ldo + A.o_off + c0, acc, A.out_f32 != 0);
}

struct PoolArgs {
  const uint16_t* in;
  const float *scale, *shift;
  uint16_t* out;
  size_t total;
  int ldi, i_off, t, h, w, c, kt, ldo, o_off;
};

// max over the (kt,3,3) window of x*scale + shift (padding ignored, as
// MaxPool3d's -inf), rounded once.  The window always holds its centre.
template <class DT>
__global__ __launch_bounds__(MSCA_T) void bn_maxpool_k(const PoolArgs A) {
  const size_t idx = (size_t)blockIdx.x * MSCA_T + threadIdx.x;
  if (idx >= A.total) return;
  size_t pos, b;
  int c0, x, y, tt;
  split_idx(idx, A.total, A.c >> 3, pos, c0);
  split_pos(pos, A.total, A.t, A.h, A.w, b, tt, y, x);
  const int ht = A.kt / 2;
  float s[8], sh[8], m[8];
  ld8f(A.scale + c0, s);
  ld8f(A.shift + c0, sh);
#pragma unroll
  for (int k = 0; k < 8; ++k) m[k] = -__builtin_inff();
  for (int tz = max(tt - ht, 0); tz <= min(tt + ht, A.t - 1); ++tz)
    for (int yy = max(y - 1, 0); yy <= min(y + 1, A.h - 1); ++yy)
      for (int xx = max(x - 1, 0); xx <= min(x + 1, A.w - 1); ++xx) {
        const size_t p = ((b * A.t + tz) * A.h + yy) * A.w + xx;
        const u16x8 v = *(const u16x8*)(A.in + p * A.ldi + A.i_off + c0);
#pragma unroll
        for (int k = 0; k < 8; ++k) m[k] = fmaxf(m[k], DT::to_f32(v[k]) * s[k] + sh[k]);
      }
  store8<DT>(A.out, pos * A.ldo + A.o_off + c0, m, false);
}

struct EwArgs {
  const uint16_t *a, *b, *c3;
  const float *scale, *shift;
  uint16_t* out;
  size_t total;
  int op, c, lda, a_off, ldb, b_off, ldc, c_off, ldo, o_off;
};

template <class DT>
__global__ __launch_bounds__(MSCA_T) void ew_k(const EwArgs A) {
  const size_t idx = (size_t)blockIdx.x * MSCA_T + threadIdx.x;
  if (idx >= A.total) return;
  size_t pos;
  int c0;
  split_idx(idx, A.total, A.c >> 3, pos, c0);
  const u16x8 av = *(const u16x8*)(A.a + pos * A.lda + A.a_off + c0);
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = DT::to_f32(av[k]);
  if (A.op == FAC_EW_AFFINE) {
    float s[8], sh[8];
    ld8f(A.scale + c0, s);
    ld8f(A.shift + c0, sh);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = v[k] * s[k] + sh[k];
  } else if (A.op == FAC_EW_GELU) {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = gelu_erf(v[k]);
  } else if (A.op == FAC_EW_CLAMP6) {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = relu6f(v[k]);
  } else {
    const u16x8 bv = *(const u16x8*)(A.b + pos * A.ldb + A.b_off + c0);
    if (A.op == FAC_EW_MUL) {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] *= DT::to_f32(bv[k]);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] += DT::to_f32(bv[k]);
      if (A.op == FAC_EW_ADD_GELU) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = gelu_erf(v[k]);
      } else if (A.op == FAC_EW_ADD3) {   // (a + b) + c
        const u16x8 cvv = *(const u16x8*)(A.c3 + pos * A.ldc + A.c_off + c0);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] += DT::to_f32(cvv[k]);
      }
    }
  }
  store8<DT>(A.out, pos * A.ldo + A.o_off + c0, v, false);
}

// a [rows][ld] operand's slice [off, off + c): 16-byte vectors inside the row
static inline bool slice_ok(const void* p, int ld, int off, int c, size_t align = 16) {
  return p && !((uintptr_t)p % align) && ld >= 8 && ld % 8 == 0 && off >= 0 && off % 8 == 0 && off <= ld - c;
}
// threads = rows * c/8, in blocks of MSCA_T; 0 if the grid would not fit
static inline unsigned grid_of(size_t rows, int c, size_t* total) {
  *total = rows * (size_t)(c / 8);
  const size_t blocks = (*total + MSCA_T - 1) / MSCA_T;
  return blocks <= 0x7fffffffULL ? (unsigned)blocks : 0u;
}

template <class DT>
static void launch_dwsep(int k, int kt, unsigned grid, hipStream_t st, const DwArgs& A) {
#define FAC_DW(K, KT) dwsep_k<DT, K, KT><<<grid, MSCA_T, 0, st>>>(A)
  if (kt == 1) {
    if (k == 3) FAC_DW(3, 1);
    else if (k == 5) FAC_DW(5, 1);
    else FAC_DW(7, 1);
  } else {
    if (k == 3) FAC_DW(3, 3);
    else if (k == 5) FAC_DW(5, 3);
    else FAC_DW(7, 3);
  }
#undef FAC_DW
}

}  // namespace fac

extern "C" {

int fac_dwsep3d(const fac_dwsep_desc* d, void* stream) {
  using namespace fac;
  if (!d || (d->dtype != 0 && d->dtype != 1) || !d->ws || !d->scale || !d->shift) return FAC_ERR_ARG;
  if (d->act != FAC_DWSEP_NONE && d->act != FAC_DWSEP_AFFINE2 && d->act != FAC_DWSEP_GELU) return FAC_ERR_ARG;
  if (d->act == FAC_DWSEP_AFFINE2 && (!d->scale2 || !d->shift2)) return FAC_ERR_ARG;
  if ((d->k != 3 && d->k != 5 && d->k != 7) || (d->kt != 1 && d->kt != 3)) return FAC_ERR_SHAPE;
  if (d->kt == 3 && !d->wt) return FAC_ERR_ARG;
  if (d->n < 1 || d->t < 1 || d->h < 1 || d->w < 1 || d->c < 8 || d->c % 8) return FAC_ERR_SHAPE;
  if (!slice_ok(d->in, d->ldi, d->i_off, d->c) || !slice_ok(d->out, d->ldo, d->o_off, d->c)) return FAC_ERR_ARG;
  if (((uintptr_t)d->ws | (uintptr_t)d->wt | (uintptr_t)d->scale | (uintptr_t)d->shift | (uintptr_t)d->scale2 |
       (uintptr_t)d->shift2) & 15)
    return FAC_ERR_ARG;   // fp32 per-channel tables are read as 16-byte vectors
  DwArgs A;
  A.in = (const uint16_t*)d->in;
  A.ws = d->ws, A.wt = d->wt, A.scale = d->scale, A.shift = d->shift, A.scale2 = d->scale2, A.shift2 = d->shift2;
  A.out = d->out;
  A.ldi = d->ldi, A.i_off = d->i_off, A.t = d->t, A.h = d->h, A.w = d->w, A.c = d->c, A.act = d->act;
  A.ldo = d->ldo, A.o_off = d->o_off, A.out_f32 = d->out_f32 ? 1 : 0;
  const unsigned grid = grid_of((size_t)d->n * d->t * d->h * d->w, d->c, &A.total);
  if (!grid) return FAC_ERR_SHAPE;
  if (d->dtype == 0) launch_dwsep<BF16>(d->k, d->kt, grid, (hipStream_t)stream, A);
  else launch_dwsep<F16>(d->k, d->kt, grid, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? FAC_OK : FAC_ERR_HIP;
}

int fac_bn_maxpool3d(int dtype, const void* in, int ldi, int i_off, int n, int t, int h, int w, int c, int kt,
                     const float* scale, const float* shift, void* out, int ldo, int o_off, void* stream) {
  using namespace fac;
  if ((dtype != 0 && dtype != 1) || !scale || !shift || (((uintptr_t)scale | (uintptr_t)shift) & 15))
    return FAC_ERR_ARG;
  if ((kt != 1 && kt != 3) || n < 1 || t < 1 || h < 1 || w < 1 || c < 8 || c % 8) return FAC_ERR_SHAPE;
  if (!slice_ok(in, ldi, i_off, c) || !slice_ok(out, ldo, o_off, c)) return FAC_ERR_ARG;
  PoolArgs A;
  A.in = (const uint16_t*)in, A.scale = scale, A.shift = shift, A.out = (uint16_t*)out;
  A.ldi = ldi, A.i_off = i_off, A.t = t, A.h = h, A.w = w, A.c = c, A.kt = kt, A.ldo = ldo, A.o_off = o_off;
  const unsigned grid = grid_of((size_t)n * t * h * w, c, &A.total);
  if (!grid) return FAC_ERR_SHAPE;
  if (dtype == 0) bn_maxpool_k<BF16><<<grid, MSCA_T, 0, (hipStream_t)stream>>>(A);
  else bn_maxpool_k<F16><<<grid, MSCA_T, 0, (hipStream_t)stream>>>(A);
  return hipGetLastError() == hipSuccess ? FAC_OK : FAC_ERR_HIP;
}

int fac_ew(int dtype, int op, const void* a, int lda, int a_off, const void* b, int ldb, int b_off, const void* c3,
           int ldc, int c_off, const float* scale, const float* shift, void* out, int ldo, int o_off, long long rows,
           int c, void* stream) {
  using namespace fac;
  if ((dtype != 0 && dtype != 1) || op < FAC_EW_AFFINE || op > FAC_EW_ADD3) return FAC_ERR_ARG;
  if (rows < 1 || rows > (1LL << 40) || c < 8 || c % 8) return FAC_ERR_SHAPE;
  if (!slice_ok(a, lda, a_off, c) || !slice_ok(out, ldo, o_off, c)) return FAC_ERR_ARG;
  const bool two = op == FAC_EW_MUL || op == FAC_EW_ADD || op == FAC_EW_ADD_GELU || op == FAC_EW_ADD3;
  if (two && !slice_ok(b, ldb, b_off, c)) return FAC_ERR_ARG;
  if (op == FAC_EW_ADD3 && !slice_ok(c3, ldc, c_off, c)) return FAC_ERR_ARG;
  if (op == FAC_EW_AFFINE && (!scale || !shift || (((uintptr_t)scale | (uintptr_t)shift) & 15))) return FAC_ERR_ARG;
  EwArgs A;
  A.a = (const uint16_t*)a, A.b = (const uint16_t*)b, A.c3 = (const uint16_t*)c3;
  A.scale = scale, A.shift = shift, A.out = (uint16_t*)out;
  A.op = op, A.c = c, A.lda = lda, A.a_off = a_off, A.ldb = ldb, A.b_off = b_off, A.ldc = ldc, A.c_off = c_off;
  A.ldo = ldo, A.o_off = o_off;
  const unsigned grid = grid_of((size_t)rows, c, &A.total);
  if (!grid) return FAC_ERR_SHAPE;
  if (dtype == 0) ew_k<BF16><<<grid, MSCA_T, 0, (hipStream_t)stream>>>(A);
  else ew_k<F16><<<grid, MSCA_T, 0, (hipStream_t)stream>>>(A);
  return hipGetLastError() == hipSuccess ? FAC_OK : FAC_ERR_HIP;
}

}  // extern "C"
