// GCNet context block (ContextBlock3d, pooling 'avg', fusion 'channel_add') of
// CA_S3D_v3 on 16-bit channels-last maps x [n][s][c], s = T*H*W:
//
//   ctx[b][c]  = (sum over s of x[b][s][c]) / s
//   h[b][:]    = W0 ctx[b][:] + b0                       (p values)
//   h          = LayerNorm(h) (biased variance, eps, affine), then min(max(h, 0), 6)
//   term[b][:] = W3 h[b][:] + b3                         (c values)
//   out        = round16(float(x) + term[b][c])
//
// Everything between the 16-bit load and the 16-bit store is fp32.  Two routes
// behind fac_context_add:
//
//   per-clip  one launch, one 512-thread workgroup per clip: pool, MLP, then a
//             second pass over x (from LDS when the clip's map fits there)
//   split     partial sums over 64-row chunks -> fp32 partials [n][chunks][c],
//             one workgroup per clip reducing them in chunk order + the MLP,
//             then a vectorised apply launch
//
// No atomics: every sum has a fixed order that depends on (s, c) alone, so a
// clip's result does not depend on n or on where the clip sits in the batch.
//
// Thread layout of every pass over x (T threads, cv = c/8 16-byte vectors per
// row): cvb = min(cv, T) columns at once, rg = T / cvb row groups; thread t
// owns vector column t % cvb (+ k*cvb when cv > T) and the rows t / cvb,
// + rg, + 2 rg, ...; threads >= rg*cvb idle.  A thread so keeps its column --
// its 8 accumulators, or its 8 term values -- in registers for the whole pass.
#include "common.hpp"
#include "fac_cvit.h"
#include "fac_ops.h"

namespace fac {

constexpr int CTX_CHUNK = 64;      // rows per partial-sum / apply workgroup (split route)
constexpr int CTX_MAX_P = 64;      // widest bottleneck (p) supported
constexpr int CTX_MAX_C = 4096;    // widest map: ctx and term each live in LDS as c floats
constexpr int CTX_T_CLIP = 512;    // threads of the per-clip kernel
constexpr int CTX_T = 256;         // threads of the split route's kernels
constexpr int CTX_LDS = 64 * 1024; // dynamic LDS a launch may ask for without an attribute
constexpr size_t CTX_CLIP_BYTES = 256 * 1024;   // route 0: per-clip up to this clip size, else split

struct CtxW {
  const float *w0, *b0, *ln_w, *ln_b, *w3t, *b3;
  float eps;
  int p;
};

template <class DT>
__device__ __forceinline__ void add8(float (&a)[8], u16x8 v) {
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] += DT::to_f32(v[k]);
}

// Sum of rows [r0 + g, r0 + g + rg, ...) below r1 of vector column j into
// a[8]: four independent chains (rows taken four at a time), the rest into
// the first, combined as (a0 + a1) + (a2 + a3).  HOLD: each vector also goes
// to `hold` (LDS copy of the clip, [row][cv] vectors).
template <class DT, bool HOLD>
__device__ __forceinline__ void col_sum(const u16x8* __restrict__ x, int cv, int j, int r, int r1, int rg,
                                        float (&a)[8], u16x8* hold) {
  float a1[8] = {}, a2[8] = {}, a3[8] = {};
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] = 0.f;
  for (; r + 3 * rg < r1; r += 4 * rg) {
    const u16x8 v0 = x[(size_t)r * cv + j], v1 = x[(size_t)(r + rg) * cv + j];
    const u16x8 v2 = x[(size_t)(r + 2 * rg) * cv + j], v3 = x[(size_t)(r + 3 * rg) * cv + j];
    if (HOLD) {
      hold[r * cv + j] = v0;
      hold[(r + rg) * cv + j] = v1;
      hold[(r + 2 * rg) * cv + j] = v2;
      hold[(r + 3 * rg) * cv + j] = v3;
    }
    add8<DT>(a, v0);
    add8<DT>(a1, v1);
    add8<DT>(a2, v2);
    add8<DT>(a3, v3);
  }
  for (; r < r1; r += rg) {
    const u16x8 v = x[(size_t)r * cv + j];
    if (HOLD) hold[r * cv + j] = v;
    add8<DT>(a, v);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] = (a[k] + a1[k]) + (a2[k] + a3[k]);
}

// out = round16(float(x) + term) over the same rows of vector column j.
template <class DT, class Src>
__device__ __forceinline__ void col_apply(const Src* x, u16x8* out, int cv, int j, int r, int r1, int rg,
                                          const float (&t)[8]) {
  auto one = [&](u16x8 v) {
    u16x8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = DT::from_f32(DT::to_f32(v[k]) + t[k]);
    return o;
  };
  for (; r + 3 * rg < r1; r += 4 * rg) {
    const size_t i0 = (size_t)r * cv + j, i1 = (size_t)(r + rg) * cv + j, i2 = (size_t)(r + 2 * rg) * cv + j,
                 i3 = (size_t)(r + 3 * rg) * cv + j;
    const u16x8 v0 = x[i0], v1 = x[i1], v2 = x[i2], v3 = x[i3];
    out[i0] = one(v0);
    out[i1] = one(v1);
    out[i2] = one(v2);
    out[i3] = one(v3);
  }
  for (; r < r1; r += rg) {
    const size_t i = (size_t)r * cv + j;
    out[i] = one(x[i]);
  }
}

// The MLP of one clip, by the whole workgroup: ctx[c] (LDS) -> term[c] (LDS).
// hb: 2 * CTX_MAX_P floats of LDS.  h[q]: wave w takes q = w, w + nw, ...; a
// lane sums its c/64 products in order, then the wave butterfly -- the same
// order whatever the number of waves.  LayerNorm over exactly p values, by
// every thread for itself (p <= 64).  term[o]: thread per channel, q in order.
__device__ __forceinline__ void ctx_mlp(const CtxW& W, int c, const float* ctx, float* hb, float* term) {
  const int t = threadIdx.x, T = blockDim.x, lane = t & 63, p = W.p;
  for (int q = t >> 6; q < p; q += T >> 6) {
    const float* w = W.w0 + (size_t)q * c;
    float a = 0.f;
    for (int i = lane; i < c; i += 64) a = fmaf(w[i], ctx[i], a);
    a = wave_sum(a);
    if (lane == 0) hb[q] = a + W.b0[q];
  }
  __syncthreads();
  float mu = 0.f, var = 0.f;
  for (int q = 0; q < p; ++q) mu += hb[q];
  mu /= (float)p;
  for (int q = 0; q < p; ++q) {
    const float d = hb[q] - mu;
    var = fmaf(d, d, var);
  }
  const float rstd = 1.0f / sqrtf(var / (float)p + W.eps);
  if (t < p) {
    const float v = (hb[t] - mu) * rstd * W.ln_w[t] + W.ln_b[t];
    hb[CTX_MAX_P + t] = fminf(fmaxf(v, 0.f), 6.f);
  }
  __syncthreads();
  for (int o = t; o < c; o += T) {
    float a = 0.f;
    for (int q = 0; q < p; ++q) a = fmaf(W.w3t[(size_t)q * c + o], hb[CTX_MAX_P + q], a);
    term[o] = a + W.b3[o];
  }
  __syncthreads();
}

// LDS of ctx_clip_k (floats): red [rg][c] | ctx [c] | hb [2 * CTX_MAX_P] | hold
// (16-bit copy of the clip, HOLD only).  term reuses red's first c floats.
template <class DT, bool HOLD>
__global__ __launch_bounds__(CTX_T_CLIP) void ctx_clip_k(const uint16_t* x, int s, int c, CtxW W,
                                                         uint16_t* out, float* term_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int t = threadIdx.x, cv = c >> 3;
  const int cvb = cv < CTX_T_CLIP ? cv : CTX_T_CLIP, rg = CTX_T_CLIP / cvb;
  const int g = t / cvb, j0 = t - g * cvb;
  const bool active = g < rg;
  float* red = lds;
  float* ctx = red + (size_t)rg * c;
  float* hb = ctx + c;
  u16x8* hold = (u16x8*)(hb + 2 * CTX_MAX_P);
  const size_t clip = (size_t)blockIdx.x * s * cv;
  const u16x8* xb = (const u16x8*)x + clip;
  if (active)
    for (int j = j0; j < cv; j += cvb) {
      float a[8];
      col_sum<DT, HOLD>(xb, cv, j, g, s, rg, a, hold);
#pragma unroll
      for (int k = 0; k < 8; ++k) red[(size_t)g * c + j * 8 + k] = a[k];
    }
  __syncthreads();
  for (int o = t; o < c; o += CTX_T_CLIP) {
    float a = 0.f;
    for (int q = 0; q < rg; ++q) a += red[(size_t)q * c + o];
    ctx[o] = a / (float)s;
  }
  __syncthreads();
  float* term = red;
  ctx_mlp(W, c, ctx, hb, term);
  if (term_out)
    for (int o = t; o < c; o += CTX_T_CLIP) term_out[(size_t)blockIdx.x * c + o] = term[o];
  if (active)
    for (int j = j0; j < cv; j += cvb) {
      float tv[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) tv[k] = term[j * 8 + k];
      if (HOLD)
        col_apply<DT>((const u16x8*)hold, (u16x8*)out + clip, cv, j, g, s, rg, tv);
      else
        col_apply<DT>(xb, (u16x8*)out + clip, cv, j, g, s, rg, tv);
    }
}

// Split route, launch 1: block (clip, chunk) -> partial[clip][chunk][c], the
// fp32 sum of the chunk's rows.  LDS: red [rg][c] floats.
template <class DT>
__global__ __launch_bounds__(CTX_T) void ctx_partial_k(const uint16_t* __restrict__ x, int s, int c, int chunks,
                                                       float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int t = threadIdx.x, cv = c >> 3;
  const int cvb = cv < CTX_T ? cv : CTX_T, rg = CTX_T / cvb;
  const int g = t / cvb, j0 = t - g * cvb;
  const int clip = blockIdx.x / chunks, chunk = blockIdx.x - clip * chunks;
  const int r0 = chunk * CTX_CHUNK, r1 = min(s, r0 + CTX_CHUNK);
  const u16x8* xb = (const u16x8*)x + (size_t)clip * s * cv;
  if (g < rg)
    for (int j = j0; j < cv; j += cvb) {
      float a[8];
      col_sum<DT, false>(xb, cv, j, r0 + g, r1, rg, a, nullptr);
#pragma unroll
      for (int k = 0; k < 8; ++k) lds[(size_t)g * c + j * 8 + k] = a[k];
    }
  __syncthreads();
  for (int o = t; o < c; o += CTX_T) {
    float a = 0.f;
    for (int q = 0; q < rg; ++q) a += lds[(size_t)q * c + o];
    partial[(size_t)blockIdx.x * c + o] = a;
  }
}

// Split route, launch 2: one workgroup per clip.  The partials in chunk order
// (four chains: chunk i into chain i % 4), then the MLP.  LDS: ctx [c] |
// term [c] | hb.
__global__ __launch_bounds__(CTX_T) void ctx_mlp_k(const float* __restrict__ partial, int s, int c, int chunks, CtxW W,
                                                   float* __restrict__ term_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* ctx = lds;
  float* term = ctx + c;
  float* hb = term + c;
  const int t = threadIdx.x;
  const float* pb = partial + (size_t)blockIdx.x * chunks * c;
  for (int o = t; o < c; o += CTX_T) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int i = 0;
    for (; i + 3 < chunks; i += 4) {
      a0 += pb[(size_t)i * c + o];
      a1 += pb[(size_t)(i + 1) * c + o];
      a2 += pb[(size_t)(i + 2) * c + o];
      a3 += pb[(size_t)(i + 3) * c + o];
    }
    for (; i < chunks; ++i) a0 += pb[(size_t)i * c + o];
    ctx[o] = ((a0 + a1) + (a2 + a3)) / (float)s;
  }
  __syncthreads();
  ctx_mlp(W, c, ctx, hb, term);
  for (int o = t; o < c; o += CTX_T) term_out[(size_t)blockIdx.x * c + o] = term[o];
}

// Split route, launch 3: block (clip, chunk) adds the clip's term to its rows.
template <class DT>
__global__ __launch_bounds__(CTX_T) void ctx_apply_k(const uint16_t* x, int s, int c, int chunks,
                                                     const float* __restrict__ term, uint16_t* out) {
  const int t = threadIdx.x, cv = c >> 3;
  const int cvb = cv < CTX_T ? cv : CTX_T, rg = CTX_T / cvb;
  const int g = t / cvb, j0 = t - g * cvb;
  if (g >= rg) return;
  const int clip = blockIdx.x / chunks, chunk = blockIdx.x - clip * chunks;
  const int r0 = chunk * CTX_CHUNK, r1 = min(s, r0 + CTX_CHUNK);
  const size_t base = (size_t)clip * s * cv;
  for (int j = j0; j < cv; j += cvb) {
    float tv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) tv[k] = term[(size_t)clip * c + j * 8 + k];
    col_apply<DT>((const u16x8*)x + base, (u16x8*)out + base, cv, j, r0 + g, r1, rg, tv);
  }
}

static inline int ctx_rg(int c, int T) {
  const int cv = c / 8;
  return T / (cv < T ? cv : T);
}
// dynamic LDS of ctx_clip_k without / with the clip held
static inline size_t ctx_clip_lds(int c) { return ((size_t)ctx_rg(c, CTX_T_CLIP) * c + c + 2 * CTX_MAX_P) * 4; }
static inline bool ctx_clip_holds(int s, int c) { return ctx_clip_lds(c) + (size_t)s * c * 2 <= (size_t)CTX_LDS; }

}  // namespace fac

extern "C" {

size_t fac_context_scratch_bytes(int n, int s, int c) {
  if (n < 1 || s < 1 || c < 8 || c % 8) return 0;
  const size_t chunks = ((size_t)s + fac::CTX_CHUNK - 1) / fac::CTX_CHUNK;
  return ((size_t)n * chunks * c + (size_t)n * c) * sizeof(float);
}

// Route 0's choice.  It depends on (s, c) alone: the two routes add the pool
// in different orders, so a choice by n would let a clip's term change with
// the batch it sits in.  Measured (profiles/ca_s3d_bench.txt): per-clip wins
// on clips up to 0.2 MB at every batch size (and at 0.16 MB with 2 clips); at
// 0.8 MB the routes tie at 1536 clips and split wins with few clips, where one
// workgroup streams a large clip at only ~80 GB/s.
int fac_context_route(int s, int c) {
  if (s < 1 || c < 8 || c % 8) return 0;
  return (size_t)s * c * 2 <= fac::CTX_CLIP_BYTES ? 1 : 2;
}

int fac_context_add(int dtype, const void* x, int n, int s, int c, int p, const float* w0, const float* b0,
                    const float* ln_w, const float* ln_b, float ln_eps, const float* w3t, const float* b3, void* out,
                    float* term, void* scratch, int route, void* stream) {
  using namespace fac;
  if (!x || !out || !w0 || !b0 || !ln_w || !ln_b || !w3t || !b3 || route < 0 || route > 2 || (dtype != 0 && dtype != 1))
    return FAC_ERR_ARG;
  if (n < 1 || s < 1 || s > (1 << 30) || c < 8 || c % 8 || c > CTX_MAX_C || p < 1 || p > CTX_MAX_P)
    return FAC_ERR_SHAPE;
  const long long chunks = ((long long)s + CTX_CHUNK - 1) / CTX_CHUNK;
  if ((long long)n * chunks > 0x7fffffffLL) return FAC_ERR_SHAPE;
  if (((uintptr_t)x | (uintptr_t)out) & 15) return FAC_ERR_ARG;   // 16-byte vector loads and stores
  if (route == 0) route = fac_context_route(s, c);
  if (route == 2 && !scratch) return FAC_ERR_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const CtxW W{w0, b0, ln_w, ln_b, w3t, b3, ln_eps, p};
  const uint16_t* xi = (const uint16_t*)x;
  uint16_t* xo = (uint16_t*)out;
  if (route == 1) {
    const bool hold = ctx_clip_holds(s, c);
    const size_t lds = ctx_clip_lds(c) + (hold ? (size_t)s * c * 2 : 0);
    if (dtype == 0) {
      if (hold) ctx_clip_k<BF16, true><<<n, CTX_T_CLIP, lds, st>>>(xi, s, c, W, xo, term);
      else ctx_clip_k<BF16, false><<<n, CTX_T_CLIP, lds, st>>>(xi, s, c, W, xo, term);
    } else {
      if (hold) ctx_clip_k<F16, true><<<n, CTX_T_CLIP, lds, st>>>(xi, s, c, W, xo, term);
      else ctx_clip_k<F16, false><<<n, CTX_T_CLIP, lds, st>>>(xi, s, c, W, xo, term);
    }
    return hipGetLastError() == hipSuccess ? FAC_OK : FAC_ERR_HIP;
  }
  float* partial = (float*)scratch;
  float* tbuf = term ? term : partial + (size_t)n * chunks * c;
  const int blocks = (int)(n * chunks);
  const size_t lds_p = (size_t)ctx_rg(c, CTX_T) * c * 4, lds_m = ((size_t)2 * c + 2 * CTX_MAX_P) * 4;
  if (dtype == 0) ctx_partial_k<BF16><<<blocks, CTX_T, lds_p, st>>>(xi, s, c, (int)chunks, partial);
  else ctx_partial_k<F16><<<blocks, CTX_T, lds_p, st>>>(xi, s, c, (int)chunks, partial);
  ctx_mlp_k<<<n, CTX_T, lds_m, st>>>(partial, s, c, (int)chunks, W, tbuf);
  if (dtype == 0) ctx_apply_k<BF16><<<blocks, CTX_T, 0, st>>>(xi, s, c, (int)chunks, tbuf, xo);
  else ctx_apply_k<F16><<<blocks, CTX_T, 0, st>>>(xi, s, c, (int)chunks, tbuf, xo);
  return hipGetLastError() == hipSuccess ? FAC_OK : FAC_ERR_HIP;
}

}  // extern "C"
