// BlazeFace face detector (MediaPipe front model, 128x128, 896 anchors) and the
// tile / untile / weighted-NMS / margin flow around it, all fp32, NHWC.
//
// The net is ~35 MFLOP per tile: latency and traffic bound, so every layer is a
// plain VALU-FMA kernel (no MFMA: the 16-bit MFMA operands would move scores
// across the thresholds downstream, and the channel counts 24..96 leave the
// f32 MFMA no advantage over FMAs fed from SGPR weights).
//
//   bf_tiles    frames u8 [F,H,W,3] -> tiles u8 [F*n,128,128,3]: the reference's
//               windows (side min(H,W), n = 3 if W > H else 1, at y = 0), area
//               averaged in the exact-integer overlap arithmetic of crop.hip
//               (round half up, no channel swap).
//   bf_stem     x/127.5 - 1, pad (1,2,1,2) with zeros, conv 5x5 s2 3->24, ReLU.
//   bf_block    one BlazeBlock: depthwise 3x3 (+bias) into LDS, pointwise 1x1
//               (+bias) with wave-uniform output channels (weights come through
//               scalar loads), residual (2x2 max-pool at stride 2, zero channel
//               pad), ReLU; 64 output pixels per workgroup.
//   bf_heads    classifier_8/16 + regressor_8/16 written in anchor order.
//   bf_decode   anchors decode, clamp +-100, sigmoid, score >= threshold,
//               order-preserving compaction (ballot prefix), one block per tile.
//   bf_nms      one workgroup per frame: tile detections -> frame pixels, rank
//               sort by score, the best kCap kept, the blending loop, margin,
//               int boxes.
//
// Arithmetic that feeds a decision (decode, untile, IoU, blend, margin) uses
// explicit _rn intrinsics so nothing is contracted into an FMA: the float32
// numpy restatement (fac_fake_amd/blazeface.py) follows it operation by
// operation.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "common.hpp"
#include "fac_blazeface.h"

namespace fac {
namespace bf {

constexpr int kTile = 128;
constexpr int kAnchors = 896;
constexpr int kCap = 1024;            // NMS candidates kept per frame
constexpr int kMaxIn = 3 * kAnchors;  // most candidates a frame can have
constexpr int kChunk = 512;           // tiles per pass of the net (bounds the activation workspace)

// ------------------------------------------------------------------ tiles
// One thread per output pixel (3 channels); grid (tile, output row).  Acc is
// uint32_t for windows up to 2048 px (2 * 255 * n^2 + n^2 < 2^32: the same
// integers, without 64-bit divisions), else uint64_t.  (A variant that staged
// the covered source rows in LDS with aligned dword loads measured 2x slower
// at 1080 px, 3.55 vs 1.75 ms for 900 tiles, and was dropped.)
template <typename Acc>
__global__ __launch_bounds__(128) void bf_tiles(const uint8_t* __restrict__ frames, int H, int W, int split,
                                                int x_step, int ntiles, uint8_t* __restrict__ tiles) {
  const int t = blockIdx.x, oy = blockIdx.y, ox = threadIdx.x;
  const int f = t / ntiles, x0 = (t % ntiles) * x_step;
  const int n = split;
  const int X0 = ox * n, X1 = X0 + n, Y0 = oy * n, Y1 = Y0 + n;
  const int sx0 = X0 / kTile, sx1 = (X1 - 1) / kTile;  // covered source columns (inclusive)
  const int sy0 = Y0 / kTile, sy1 = (Y1 - 1) / kTile;
  const uint8_t* src = frames + ((size_t)f * H * W + x0) * 3;
  Acc acc0 = 0, acc1 = 0, acc2 = 0;
  for (int sy = sy0; sy <= sy1; ++sy) {
    const Acc ovy = (Acc)(min(Y1, (sy + 1) * kTile) - max(Y0, sy * kTile));
    Acc r0 = 0, r1 = 0, r2 = 0;
    const uint8_t* row = src + (size_t)sy * W * 3;
    for (int sx = sx0; sx <= sx1; ++sx) {
      const Acc ovx = (Acc)(min(X1, (sx + 1) * kTile) - max(X0, sx * kTile));
      const uint8_t* p = row + sx * 3;
      r0 += ovx * p[0];
      r1 += ovx * p[1];
      r2 += ovx * p[2];
    }
    acc0 += ovy * r0;
    acc1 += ovy * r1;
    acc2 += ovy * r2;
  }
  const Acc den = (Acc)n * (Acc)n;
  uint8_t* dst = tiles + (((size_t)t * kTile + oy) * kTile + ox) * 3;
  dst[0] = (uint8_t)((2 * acc0 + den) / (2 * den));
  dst[1] = (uint8_t)((2 * acc1 + den) / (2 * den));
  dst[2] = (uint8_t)((2 * acc2 + den) / (2 * den));
}

// ------------------------------------------------------------------- stem
// One thread per output pixel, 24 accumulators; weights [75][24] in LDS
// (every lane reads the same address: broadcast).
__global__ __launch_bounds__(256) void bf_stem(const uint8_t* __restrict__ tiles, const float* __restrict__ w,
                                               const float* __restrict__ b, float* __restrict__ out) {
  __shared__ float sw[75 * 24];
  for (int i = threadIdx.x; i < 75 * 24; i += 256) sw[i] = w[i];
  __syncthreads();
  const int gp = blockIdx.x * 256 + threadIdx.x;  // 4096 pixels per tile: never straddles the end
  const int t = gp >> 12, oy = (gp >> 6) & 63, ox = gp & 63;
  float acc[24];
#pragma unroll
  for (int co = 0; co < 24; ++co) acc[co] = b[co];
  const uint8_t* img = tiles + (size_t)t * kTile * kTile * 3;
  for (int ky = 0; ky < 5; ++ky) {
    const int iy = 2 * oy + ky - 1;
    if (iy < 0 || iy >= kTile) continue;  // padded after normalisation: the tap is 0
    for (int kx = 0; kx < 5; ++kx) {
      const int ix = 2 * ox + kx - 1;
      if (ix < 0 || ix >= kTile) continue;
      const uint8_t* p = img + (iy * kTile + ix) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float x = __fsub_rn(__fdiv_rn((float)p[c], 127.5f), 1.0f);
        const float* wr = sw + ((ky * 5 + kx) * 3 + c) * 24;
#pragma unroll
        for (int co = 0; co < 24; ++co) acc[co] = fmaf(x, wr[co], acc[co]);
      }
    }
  }
  float4* dst = reinterpret_cast<float4*>(out + (size_t)gp * 24);
#pragma unroll
  for (int q = 0; q < 6; ++q)
    dst[q] = make_float4(relu(acc[4 * q]), relu(acc[4 * q + 1]), relu(acc[4 * q + 2]), relu(acc[4 * q + 3]));
}

// -------------------------------------------------------------- BlazeBlock
// 64 consecutive output pixels per workgroup (the pixel counts per tile, 4096 /
// 1024 / 256 / 64, are multiples of 64).  Stage 1: depthwise, channel fastest
// (coalesced reads), into s_dw[c][pixel].  Stage 2: lane = pixel, each wave a
// wave-uniform run of NCO output channels (weights packed [CIN][CP], CP = COUT
// rounded up to 16, zero filled).  Stage 3: through s_out so the residual read
// and the store are coalesced.  NW waves per workgroup: 4 on the large maps; 16
// from the 16x16 maps on, where a launch has too few workgroups to hide the
// weight loads behind other waves and the per-wave chain has to be short.
template <int CIN, int COUT, int STRIDE, int HIN, int NW>
__global__ __launch_bounds__(NW * 64) void bf_block(const float* __restrict__ in, const float* __restrict__ dw_w,
                                                const float* __restrict__ dw_b, const float* __restrict__ pw_w,
                                                const float* __restrict__ pw_b, float* __restrict__ out) {
  constexpr int CP = (COUT + 15) / 16 * 16, NCO = CP / NW, NT = NW * 64;
  constexpr int DSTR = 65, OSTR = COUT + 1;
  constexpr int UNR = NCO <= 6 ? 16 : 4;  // weight rows in flight, within the SGPR budget
  __shared__ float s_dw[CIN * DSTR];
  __shared__ float s_out[64 * OSTR];
  constexpr int Hin = HIN, Ho = Hin / STRIDE, per_tile = Ho * Ho;  // powers of two: shifts, no divisions
  const int pix0 = blockIdx.x * 64;

  for (int idx = threadIdx.x; idx < 64 * CIN; idx += NT) {
    const int c = idx % CIN, p = idx / CIN;
    const int gp = pix0 + p;
    const int t = gp / per_tile, rem = gp % per_tile, oy = rem / Ho, ox = rem % Ho;
    const float* base = in + (size_t)t * Hin * Hin * CIN + c;
    float acc = dw_b[c];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = oy * STRIDE + ky - (STRIDE == 1 ? 1 : 0);
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ox * STRIDE + kx - (STRIDE == 1 ? 1 : 0);
        if (iy >= 0 && iy < Hin && ix >= 0 && ix < Hin)
          acc = fmaf(dw_w[(ky * 3 + kx) * CIN + c], base[(size_t)(iy * Hin + ix) * CIN], acc);
      }
    }
    s_dw[c * DSTR + p] = acc;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int co0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * NCO;
  if (co0 < COUT) {
    float acc[NCO];
#pragma unroll
    for (int j = 0; j < NCO; ++j) acc[j] = pw_b[co0 + j];
#pragma unroll UNR
    for (int ci = 0; ci < CIN; ++ci) {
      const float a = s_dw[ci * DSTR + lane];
      const float* wr = pw_w + ci * CP + co0;
#pragma unroll
      for (int j = 0; j < NCO; ++j) acc[j] = fmaf(a, wr[j], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < NCO; ++j)
      if (co0 + j < COUT) s_out[lane * OSTR + co0 + j] = acc[j];
  }
  __syncthreads();

  for (int idx = threadIdx.x; idx < 64 * COUT; idx += NT) {
    const int co = idx % COUT, p = idx / COUT;
    const int gp = pix0 + p;
    float v = s_out[p * OSTR + co];
    if (co < CIN) {
      const int t = gp / per_tile, rem = gp % per_tile, oy = rem / Ho, ox = rem % Ho;
      const float* base = in + (size_t)t * Hin * Hin * CIN + co;
      if (STRIDE == 1) {
        v += base[(size_t)(oy * Hin + ox) * CIN];
      } else {
        const float* q = base + (size_t)(2 * oy * Hin + 2 * ox) * CIN;
        v += fmaxf(fmaxf(q[0], q[CIN]), fmaxf(q[(size_t)Hin * CIN], q[(size_t)(Hin + 1) * CIN]));
      }
    }
    out[(size_t)gp * COUT + co] = relu(v);
  }
}

// ------------------------------------------------------------------ heads
// grid (tile, 8): parts 0..3 a quarter each of the 16x16 map (34 outputs per
// pixel: 2 scores + 32 coordinates), parts 4..7 a quarter each of the 8x8 map
// (6 + 96).  Weights are packed [cin][outputs], so consecutive lanes read
// consecutive weights and share the activation.
__global__ __launch_bounds__(256) void bf_heads(const float* __restrict__ b1, const float* __restrict__ b2,
                                                const float* __restrict__ w8, const float* __restrict__ bias8,
                                                const float* __restrict__ w16, const float* __restrict__ bias16,
                                                float* __restrict__ r, float* __restrict__ c) {
  const int t = blockIdx.x, part = blockIdx.y;
  float* rt = r + (size_t)t * kAnchors * 16;
  float* ct = c + (size_t)t * kAnchors;
  if (part < 4) {
    const float* x = b1 + (size_t)t * 256 * 88;
    for (int idx = threadIdx.x; idx < 64 * 34; idx += 256) {
      const int pix = part * 64 + idx / 34, o = idx % 34;
      const float* xp = x + pix * 88;
      float acc = bias8[o];
      for (int ci = 0; ci < 88; ++ci) acc = fmaf(xp[ci], w8[ci * 34 + o], acc);
      if (o < 2)
        ct[pix * 2 + o] = acc;
      else
        rt[pix * 32 + (o - 2)] = acc;
    }
  } else {
    const float* x = b2 + (size_t)t * 64 * 96;
    for (int idx = threadIdx.x; idx < 16 * 102; idx += 256) {
      const int pix = (part - 4) * 16 + idx / 102, o = idx % 102;
      const float* xp = x + pix * 96;
      float acc = bias16[o];
      for (int ci = 0; ci < 96; ++ci) acc = fmaf(xp[ci], w16[ci * 102 + o], acc);
      if (o < 6)
        ct[512 + pix * 6 + o] = acc;
      else
        rt[512 * 16 + pix * 96 + (o - 6)] = acc;
    }
  }
}

// ----------------------------------------------------------------- decode
// One block per tile, one thread per anchor.  dets [T][896][17], compacted in
// anchor order; counts [T].
__global__ __launch_bounds__(kAnchors) void bf_decode(const float* __restrict__ r, const float* __restrict__ c,
                                                      const float* __restrict__ anchors, float min_score,
                                                      float* __restrict__ dets, int32_t* __restrict__ counts) {
  __shared__ int s_wave[kAnchors / 64];
  const int t = blockIdx.x, a = threadIdx.x, lane = a & 63, wv = a >> 6;
  float s = c[(size_t)t * kAnchors + a];
  s = fminf(fmaxf(s, -100.0f), 100.0f);
  const float score = __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-s)));
  const bool keep = score >= min_score;
  const unsigned long long bal = __ballot(keep);
  if (lane == 0) s_wave[wv] = __popcll(bal);
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int i = 0; i < kAnchors / 64; ++i) {
    const int n = s_wave[i];
    if (i < wv) before += n;
    total += n;
  }
  if (a == 0) counts[t] = total;
  if (!keep) return;
  const int pos = before + __popcll(bal & ((1ull << lane) - 1ull));  // < 896
  const float* rr = r + ((size_t)t * kAnchors + a) * 16;
  const float ax = anchors[a * 4], ay = anchors[a * 4 + 1], aw = anchors[a * 4 + 2], ah = anchors[a * 4 + 3];
  float* d = dets + ((size_t)t * kAnchors + pos) * 17;
  const float xc = __fadd_rn(__fmul_rn(__fdiv_rn(rr[0], 128.0f), aw), ax);
  const float yc = __fadd_rn(__fmul_rn(__fdiv_rn(rr[1], 128.0f), ah), ay);
  const float hw = __fdiv_rn(__fmul_rn(__fdiv_rn(rr[2], 128.0f), aw), 2.0f);
  const float hh = __fdiv_rn(__fmul_rn(__fdiv_rn(rr[3], 128.0f), ah), 2.0f);
  d[0] = __fsub_rn(yc, hh);
  d[1] = __fsub_rn(xc, hw);
  d[2] = __fadd_rn(yc, hh);
  d[3] = __fadd_rn(xc, hw);
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    d[4 + 2 * k] = __fadd_rn(__fmul_rn(__fdiv_rn(rr[4 + 2 * k], 128.0f), aw), ax);
    d[5 + 2 * k] = __fadd_rn(__fmul_rn(__fdiv_rn(rr[5 + 2 * k], 128.0f), ah), ay);
  }
  d[16] = score;
}

// -------------------------------------------------------------------- NMS
// One workgroup per frame.  tile_dets [frames*ntiles][stride][17] with
// tile_counts valid rows each (clamped to stride; ntiles * stride <= kMaxIn is
// checked by the host).  `sorted` is a [frames][kCap][17] workspace.  Every
// index written is < kCap; out_dets / out_boxes are [frames][kCap][..]
// (out_boxes may be null).
__global__ __launch_bounds__(256) void bf_nms(const float* __restrict__ tile_dets,
                                              const int32_t* __restrict__ tile_counts, int ntiles, int stride,
                                              int map, float scale, int x_step, int H, int W, float min_iou,
                                              float* __restrict__ sorted, float* __restrict__ out_dets,
                                              int32_t* __restrict__ out_boxes, int32_t* __restrict__ out_counts,
                                              int32_t* __restrict__ out_overflow) {
  __shared__ float s_score[kMaxIn];
  __shared__ unsigned char s_alive[kCap];
  __shared__ unsigned char s_mem[kCap];
  __shared__ int s_first;
  const int f = blockIdx.x, tid = threadIdx.x;
  int start[4] = {0, 0, 0, 0};  // ntiles <= 3
  for (int h = 0; h < ntiles; ++h) start[h + 1] = start[h] + min(max(tile_counts[f * ntiles + h], 0), stride);
  const int n_in = start[ntiles];
  for (int h = ntiles; h < 3; ++h) start[h + 1] = n_in;
  const int n = min(n_in, kCap);
  float* srt = sorted + (size_t)f * kCap * 17;
  float* od = out_dets + (size_t)f * kCap * 17;

  for (int j = tid; j < n_in; j += 256) {
    const int h = (j >= start[1]) + (j >= start[2]);
    s_score[j] = tile_dets[((size_t)(f * ntiles + h) * stride + (j - start[h])) * 17 + 16];
  }
  for (int i = tid; i < kCap; i += 256) s_alive[i] = i < n;
  __syncthreads();
  // rank sort, score descending, ties by position; the best kCap are kept
  for (int j = tid; j < n_in; j += 256) {
    const float sj = s_score[j];
    int rank = 0;
    for (int k = 0; k < n_in; ++k) {
      const float sk = s_score[k];
      rank += (sk > sj) || (sk == sj && k < j);
    }
    if (rank >= kCap) continue;
    const int h = (j >= start[1]) + (j >= start[2]);
    const float* d = tile_dets + ((size_t)(f * ntiles + h) * stride + (j - start[h])) * 17;
    float* o = srt + rank * 17;
    if (map) {
      const float xoff = (float)(h * x_step);
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const float v = __fmul_rn(__fmul_rn(d[k], 128.0f), scale);
        // boxes are (y, x, y, x), keypoints (x, y): the window offset goes on x
        const bool is_x = k < 4 ? (k & 1) : !(k & 1);
        o[k] = is_x ? __fadd_rn(v, xoff) : v;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k) o[k] = d[k];
    }
    o[16] = sj;
  }
  if (tid == 0) s_first = 0;
  __syncthreads();

  int nout = 0;
  while (true) {
    // thread 0 advances to the first remaining candidate
    if (tid == 0) {
      int i = s_first;
      while (i < n && !s_alive[i]) ++i;
      s_first = i;
    }
    __syncthreads();
    const int first = s_first;
    if (first >= n) break;  // uniform
    const float fy0 = srt[first * 17], fx0 = srt[first * 17 + 1], fy1 = srt[first * 17 + 2],
                fx1 = srt[first * 17 + 3];
    const float area_a = __fmul_rn(__fsub_rn(fy1, fy0), __fsub_rn(fx1, fx0));
    for (int i = tid; i < n; i += 256) {
      unsigned char m = 0;
      if (s_alive[i]) {
        const float* b = srt + i * 17;
        const float iy = fmaxf(__fsub_rn(fminf(fy1, b[2]), fmaxf(fy0, b[0])), 0.0f);
        const float ix = fmaxf(__fsub_rn(fminf(fx1, b[3]), fmaxf(fx0, b[1])), 0.0f);
        const float inter = __fmul_rn(iy, ix);
        const float area_b = __fmul_rn(__fsub_rn(b[2], b[0]), __fsub_rn(b[3], b[1]));
        const float iou = __fdiv_rn(inter, __fsub_rn(__fadd_rn(area_a, area_b), inter));
        m = iou > min_iou;
        if (m || i == first) s_alive[i] = 0;  // the first box always leaves (a degenerate box has IoU NaN)
      }
      s_mem[i] = m;
    }
    __syncthreads();
    if (tid < 17) {
      // every sum in sorted order, one thread per output value
      float acc = 0.0f, tot = 0.0f;
      int cnt = 0;
      for (int i = first; i < n; ++i) {
        if (!s_mem[i]) continue;
        const float sc = srt[i * 17 + 16];
        if (tid < 16) acc = __fadd_rn(acc, __fmul_rn(srt[i * 17 + tid], sc));
        tot = __fadd_rn(tot, sc);
        ++cnt;
      }
      float v = srt[first * 17 + tid];
      if (cnt > 1) v = tid < 16 ? __fdiv_rn(acc, tot) : __fdiv_rn(tot, (float)cnt);
      od[nout * 17 + tid] = v;  // nout < n <= kCap
    }
    ++nout;
    __syncthreads();
  }

  // margin 0.2 of the height (twice on ymin), clamp to the frame, truncate
  for (int k = tid; k < nout; k += 256) {
    const float y0 = od[k * 17], x0 = od[k * 17 + 1], y1 = od[k * 17 + 2], x1 = od[k * 17 + 3];
    const float off = rintf(__fmul_rn(0.2f, __fsub_rn(y1, y0)));
    const float top = fmaxf(__fsub_rn(y0, __fmul_rn(off, 2.0f)), 0.0f);
    const float left = fmaxf(__fsub_rn(x0, off), 0.0f);
    const float bottom = fminf(__fadd_rn(y1, off), (float)H);
    const float right = fminf(__fadd_rn(x1, off), (float)W);
    if (!out_boxes) break;
    int32_t* b = out_boxes + ((size_t)f * kCap + k) * 5;
    b[0] = f;
    b[1] = (int32_t)left;
    b[2] = (int32_t)top;
    b[3] = (int32_t)right;
    b[4] = (int32_t)bottom;
  }
  if (tid == 0) {
    out_counts[f] = nout;
    out_overflow[f] = n_in - n;
  }
}

// ------------------------------------------------------------------- host
struct BlockSpec {
  int cin, cout, stride, hin;
  const char* prefix;
};
static const BlockSpec kBlocks[16] = {
    {24, 24, 1, 64, "backbone1.2"},  {24, 28, 1, 64, "backbone1.3"},  {28, 32, 2, 64, "backbone1.4"},
    {32, 36, 1, 32, "backbone1.5"},  {36, 42, 1, 32, "backbone1.6"},  {42, 48, 2, 32, "backbone1.7"},
    {48, 56, 1, 16, "backbone1.8"},  {56, 64, 1, 16, "backbone1.9"},  {64, 72, 1, 16, "backbone1.10"},
    {72, 80, 1, 16, "backbone1.11"}, {80, 88, 1, 16, "backbone1.12"}, {88, 96, 2, 16, "backbone2.0"},
    {96, 96, 1, 8, "backbone2.1"},   {96, 96, 1, 8, "backbone2.2"},   {96, 96, 1, 8, "backbone2.3"},
    {96, 96, 1, 8, "backbone2.4"}};
constexpr int kLastB1 = 10, kLastB2 = 15;
constexpr size_t kActMax = (size_t)64 * 64 * 28;  // largest activation of a tile, in floats
constexpr size_t kB1 = 16 * 16 * 88, kB2 = 8 * 8 * 96;

struct BlockW {
  size_t dw_w, dw_b, pw_w, pw_b;  // float offsets into the weight blob
};

}  // namespace bf
}  // namespace fac

struct fac_bf {
  int device = 0;
  bool loaded = false;
  float* d_w = nullptr;  // one blob: stem, blocks, heads, anchors
  size_t stem_w = 0, stem_b = 0, w8 = 0, bias8 = 0, w16 = 0, bias16 = 0, anchors = 0;
  fac::bf::BlockW blk[16];
  // workspace: chunk-sized activations, and buffers that grow with the tile / frame count
  float *act_a = nullptr, *act_b = nullptr, *b1 = nullptr, *b2 = nullptr, *r = nullptr, *c = nullptr;
  uint8_t* tiles = nullptr;
  float* tile_dets = nullptr;
  int32_t* tile_counts = nullptr;
  float* sorted = nullptr;
  int cap_pass = 0, cap_tiles = 0, cap_frames = 0;
};

namespace fac {
namespace bf {

template <typename T>
static bool dalloc(T** p, size_t n) {
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  return hipMalloc((void**)p, n * sizeof(T)) == hipSuccess;
}

// Grow-only workspace: `net_tiles` tiles through the net (activations for one
// pass of at most kChunk tiles), `T` tiles of detections, `F` frames of NMS.
static int ensure(fac_bf* h, int net_tiles, int T, int F) {
  const int pass = std::min(net_tiles, kChunk);
  if (pass > h->cap_pass) {
    h->cap_pass = 0;
    const size_t n = (size_t)pass;
    if (!dalloc(&h->act_a, n * kActMax) || !dalloc(&h->act_b, n * kActMax) || !dalloc(&h->b1, n * kB1) ||
        !dalloc(&h->b2, n * kB2) || !dalloc(&h->r, n * kAnchors * 16) || !dalloc(&h->c, n * kAnchors))
      return FAC_ERR_OOM;
    h->cap_pass = pass;
  }
  if (T > h->cap_tiles) {
    h->cap_tiles = 0;
    if (!dalloc(&h->tiles, (size_t)T * kTile * kTile * 3) || !dalloc(&h->tile_dets, (size_t)T * kAnchors * 17) ||
        !dalloc(&h->tile_counts, (size_t)T))
      return FAC_ERR_OOM;
    h->cap_tiles = T;
  }
  if (F > h->cap_frames) {
    h->cap_frames = 0;
    if (!dalloc(&h->sorted, (size_t)F * kCap * 17)) return FAC_ERR_OOM;
    h->cap_frames = F;
  }
  return FAC_OK;
}

template <int CIN, int COUT, int STRIDE, int HIN, int NW>
static void launch_block(const float* in, const float* w, const BlockW& o, float* out, int tiles, hipStream_t st) {
  constexpr int ho = HIN / STRIDE;
  bf_block<CIN, COUT, STRIDE, HIN, NW><<<tiles * ho * ho / 64, NW * 64, 0, st>>>(in, w + o.dw_w, w + o.dw_b,
                                                                                  w + o.pw_w, w + o.pw_b, out);
}

static bool run_block(int i, const float* in, const float* w, const BlockW& o, float* out, int tiles,
                      hipStream_t st) {
  const BlockSpec& s = kBlocks[i];
#define FAC_BF_CASE(CI, CO, S, HI, NW)                                  \
  if (s.cin == CI && s.cout == CO && s.stride == S && s.hin == HI) {    \
    launch_block<CI, CO, S, HI, NW>(in, w, o, out, tiles, st);          \
    return true;                                                        \
  }
  FAC_BF_CASE(24, 24, 1, 64, 4)
  FAC_BF_CASE(24, 28, 1, 64, 4)
  FAC_BF_CASE(28, 32, 2, 64, 4)
  FAC_BF_CASE(32, 36, 1, 32, 4)
  FAC_BF_CASE(36, 42, 1, 32, 4)
  FAC_BF_CASE(42, 48, 2, 32, 16)
  FAC_BF_CASE(48, 56, 1, 16, 16)
  FAC_BF_CASE(56, 64, 1, 16, 16)
  FAC_BF_CASE(64, 72, 1, 16, 16)
  FAC_BF_CASE(72, 80, 1, 16, 16)
  FAC_BF_CASE(80, 88, 1, 16, 16)
  FAC_BF_CASE(88, 96, 2, 16, 16)
  FAC_BF_CASE(96, 96, 1, 8, 16)
#undef FAC_BF_CASE
  return false;
}

// The net on T tiles, kChunk at a time.  Any of b1 / b2 / r / c may be null
// (the chunk workspace is used); dets / counts null skips the decode.
static int run_net(fac_bf* h, const uint8_t* tiles, int T, float* b1, float* b2, float* r, float* c, float min_score,
                   float* dets, int32_t* counts, hipStream_t st) {
  const float* w = h->d_w;
  for (int t0 = 0; t0 < T; t0 += kChunk) {
    const int n = std::min(kChunk, T - t0);
    float* b1p = b1 ? b1 + (size_t)t0 * kB1 : h->b1;
    float* b2p = b2 ? b2 + (size_t)t0 * kB2 : h->b2;
    float* rp = r ? r + (size_t)t0 * kAnchors * 16 : h->r;
    float* cp = c ? c + (size_t)t0 * kAnchors : h->c;
    bf_stem<<<n * 4096 / 256, 256, 0, st>>>(tiles + (size_t)t0 * kTile * kTile * 3, w + h->stem_w, w + h->stem_b,
                                            h->act_a);
    const float* cur = h->act_a;
    for (int i = 0; i < 16; ++i) {
      float* dst = i == kLastB1 ? b1p : i == kLastB2 ? b2p : (cur == h->act_a ? h->act_b : h->act_a);
      if (!run_block(i, cur, w, h->blk[i], dst, n, st)) return FAC_ERR_SHAPE;
      cur = dst;
    }
    bf_heads<<<dim3(n, 8), 256, 0, st>>>(b1p, b2p, w + h->w8, w + h->bias8, w + h->w16, w + h->bias16, rp, cp);
    if (dets)
      bf_decode<<<n, kAnchors, 0, st>>>(rp, cp, w + h->anchors, min_score, dets + (size_t)t0 * kAnchors * 17,
                                        counts + t0);
  }
  return hipGetLastError() == hipSuccess ? FAC_OK : FAC_ERR_HIP;
}

static int run_nms(fac_bf* h, const float* tile_dets, const int32_t* tile_counts, int F, int ntiles, int stride,
                   int map, int split, int x_step, int H, int W, float min_iou, float* dets, int32_t* boxes,
                   int32_t* counts, int32_t* overflow, hipStream_t st) {
  bf_nms<<<F, 256, 0, st>>>(tile_dets, tile_counts, ntiles, stride, map, (float)((double)split / kTile), x_step, H, W,
                            min_iou, h->sorted, dets, boxes, counts, overflow);
  return hipGetLastError() == hipSuccess ? FAC_OK : FAC_ERR_HIP;
}

static void launch_tiles(const uint8_t* frames, int T, int H, int W, int split, int x_step, int ntiles,
                         uint8_t* tiles, hipStream_t st) {
  if (split <= 2048)
    bf_tiles<uint32_t><<<dim3(T, kTile), kTile, 0, st>>>(frames, H, W, split, x_step, ntiles, tiles);
  else
    bf_tiles<uint64_t><<<dim3(T, kTile), kTile, 0, st>>>(frames, H, W, split, x_step, ntiles, tiles);
}

static bool windows(int H, int W, int* split, int* x_step, int* ntiles) {
  *split = std::min(H, W);
  *x_step = (W - *split) / 2;
  *ntiles = W > H ? 3 : 1;
  return *split >= kTile;
}

static const fac_tensor_desc* find(const fac_tensor_desc* d, int n, const std::string& name) {
  for (int i = 0; i < n; ++i)
    if (d[i].name && name == d[i].name) return &d[i];
  return nullptr;
}

static bool shape_is(const fac_tensor_desc* d, std::initializer_list<int64_t> s) {
  if (!d->data || d->ndim != (int)s.size()) return false;
  int i = 0;
  for (int64_t v : s)
    if (d->shape[i++] != v) return false;
  return true;
}

}  // namespace bf
}  // namespace fac

using namespace fac::bf;

extern "C" {

int fac_bf_capacity(void) { return kCap; }

int fac_bf_create(int device, fac_bf** out) {
  if (!out || device < 0) return FAC_ERR_ARG;
  *out = new fac_bf();
  (*out)->device = device;
  return FAC_OK;
}

void fac_bf_destroy(fac_bf* h) {
  if (!h) return;
  if (hipSetDevice(h->device) == hipSuccess) {
    void* ptrs[] = {h->d_w, h->act_a, h->act_b, h->b1, h->b2, h->r, h->c, h->tiles, h->tile_dets, h->tile_counts,
                    h->sorted};
    for (void* p : ptrs)
      if (p) (void)hipFree(p);
  }
  delete h;
}

int fac_bf_load(fac_bf* h, const fac_tensor_desc* descs, int n) {
  if (!h || !descs || n <= 0) return FAC_ERR_ARG;
  std::vector<float> blob;
  auto reserve = [&](size_t count) {
    const size_t off = blob.size();
    blob.resize(off + (count + 3) / 4 * 4, 0.0f);  // 16-byte aligned pieces
    return off;
  };
  auto get = [&](const std::string& name) { return find(descs, n, name); };

  const fac_tensor_desc *sw = get("backbone1.0.weight"), *sb = get("backbone1.0.bias");
  if (!sw || !sb) return FAC_ERR_MISSING;
  if (!shape_is(sw, {24, 3, 5, 5}) || !shape_is(sb, {24})) return FAC_ERR_SHAPE;
  h->stem_w = reserve(75 * 24);
  for (int co = 0; co < 24; ++co)
    for (int c = 0; c < 3; ++c)
      for (int k = 0; k < 25; ++k) blob[h->stem_w + (size_t)(k * 3 + c) * 24 + co] = sw->data[(co * 3 + c) * 25 + k];
  h->stem_b = reserve(24);
  memcpy(&blob[h->stem_b], sb->data, 24 * sizeof(float));

  for (int i = 0; i < 16; ++i) {
    const BlockSpec& s = kBlocks[i];
    const std::string p = s.prefix;
    const fac_tensor_desc *dw = get(p + ".convs.0.weight"), *db = get(p + ".convs.0.bias"),
                          *pw = get(p + ".convs.1.weight"), *pb = get(p + ".convs.1.bias");
    if (!dw || !db || !pw || !pb) return FAC_ERR_MISSING;
    if (!shape_is(dw, {s.cin, 1, 3, 3}) || !shape_is(db, {s.cin}) || !shape_is(pw, {s.cout, s.cin, 1, 1}) ||
        !shape_is(pb, {s.cout}))
      return FAC_ERR_SHAPE;
    const int cp = (s.cout + 15) / 16 * 16;
    BlockW& o = h->blk[i];
    o.dw_w = reserve((size_t)9 * s.cin);
    for (int c = 0; c < s.cin; ++c)
      for (int k = 0; k < 9; ++k) blob[o.dw_w + (size_t)k * s.cin + c] = dw->data[c * 9 + k];
    o.dw_b = reserve(s.cin);
    memcpy(&blob[o.dw_b], db->data, s.cin * sizeof(float));
    o.pw_w = reserve((size_t)s.cin * cp);  // channel padding lives here, zero filled
    for (int co = 0; co < s.cout; ++co)
      for (int ci = 0; ci < s.cin; ++ci) blob[o.pw_w + (size_t)ci * cp + co] = pw->data[(size_t)co * s.cin + ci];
    o.pw_b = reserve(cp);
    memcpy(&blob[o.pw_b], pb->data, s.cout * sizeof(float));
  }

  const fac_tensor_desc *c8 = get("classifier_8.weight"), *c8b = get("classifier_8.bias"),
                        *r8 = get("regressor_8.weight"), *r8b = get("regressor_8.bias"),
                        *c16 = get("classifier_16.weight"), *c16b = get("classifier_16.bias"),
                        *r16 = get("regressor_16.weight"), *r16b = get("regressor_16.bias"), *an = get("anchors");
  if (!c8 || !c8b || !r8 || !r8b || !c16 || !c16b || !r16 || !r16b || !an) return FAC_ERR_MISSING;
  if (!shape_is(c8, {2, 88, 1, 1}) || !shape_is(c8b, {2}) || !shape_is(r8, {32, 88, 1, 1}) || !shape_is(r8b, {32}) ||
      !shape_is(c16, {6, 96, 1, 1}) || !shape_is(c16b, {6}) || !shape_is(r16, {96, 96, 1, 1}) ||
      !shape_is(r16b, {96}) || !shape_is(an, {kAnchors, 4}))
    return FAC_ERR_SHAPE;
  h->w8 = reserve(88 * 34);
  h->bias8 = reserve(34);
  for (int o = 0; o < 34; ++o) {
    const float* src = o < 2 ? c8->data + o * 88 : r8->data + (o - 2) * 88;
    for (int ci = 0; ci < 88; ++ci) blob[h->w8 + (size_t)ci * 34 + o] = src[ci];
    blob[h->bias8 + o] = o < 2 ? c8b->data[o] : r8b->data[o - 2];
  }
  h->w16 = reserve(96 * 102);
  h->bias16 = reserve(102);
  for (int o = 0; o < 102; ++o) {
    const float* src = o < 6 ? c16->data + o * 96 : r16->data + (o - 6) * 96;
    for (int ci = 0; ci < 96; ++ci) blob[h->w16 + (size_t)ci * 102 + o] = src[ci];
    blob[h->bias16 + o] = o < 6 ? c16b->data[o] : r16b->data[o - 6];
  }
  h->anchors = reserve(kAnchors * 4);
  memcpy(&blob[h->anchors], an->data, kAnchors * 4 * sizeof(float));

  if (hipSetDevice(h->device) != hipSuccess) return FAC_ERR_HIP;
  if (hipDeviceSynchronize() != hipSuccess) return FAC_ERR_HIP;  // earlier launches may still read the old blob
  if (!dalloc(&h->d_w, blob.size())) return FAC_ERR_OOM;
  if (hipMemcpy(h->d_w, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
    return FAC_ERR_HIP;
  h->loaded = true;
  return FAC_OK;
}

int fac_bf_debug_tiles(fac_bf* h, const uint8_t* d_frames, int F, int H, int W, uint8_t* d_tiles, void* stream) {
  if (!h || !d_frames || !d_tiles || F <= 0 || H <= 0 || W <= 0) return FAC_ERR_ARG;
  int split, x_step, ntiles;
  if (!windows(H, W, &split, &x_step, &ntiles)) return FAC_ERR_SHAPE;  // tiles only shrink
  if ((long long)F * H * W * 3 >= (1ll << 40) || (long long)F * ntiles > (1 << 20)) return FAC_ERR_SHAPE;
  if (hipSetDevice(h->device) != hipSuccess) return FAC_ERR_HIP;
  launch_tiles(d_frames, F * ntiles, H, W, split, x_step, ntiles, d_tiles, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? FAC_OK : FAC_ERR_HIP;
}

int fac_bf_debug_net(fac_bf* h, const uint8_t* d_tiles, int T, float* d_b1, float* d_b2, float* d_r, float* d_c,
                     void* stream) {
  if (!h || !d_tiles || T <= 0 || T > (1 << 20)) return FAC_ERR_ARG;
  if (!h->loaded) return FAC_ERR_NOT_LOADED;
  if (hipSetDevice(h->device) != hipSuccess) return FAC_ERR_HIP;
  if (int rc = ensure(h, T, 0, 0)) return rc;
  return run_net(h, d_tiles, T, d_b1, d_b2, d_r, d_c, 0.0f, nullptr, nullptr, (hipStream_t)stream);
}

// One launch each, on the caller's buffers, with the loaded weights: no workspace.
int fac_bf_debug_stem(fac_bf* h, const uint8_t* d_tiles, int T, float* d_out, void* stream) {
  if (!h || !d_tiles || !d_out || T <= 0 || T > (1 << 20)) return FAC_ERR_ARG;
  if (!h->loaded) return FAC_ERR_NOT_LOADED;
  if (hipSetDevice(h->device) != hipSuccess) return FAC_ERR_HIP;
  bf_stem<<<T * 4096 / 256, 256, 0, (hipStream_t)stream>>>(d_tiles, h->d_w + h->stem_w, h->d_w + h->stem_b, d_out);
  return hipGetLastError() == hipSuccess ? FAC_OK : FAC_ERR_HIP;
}

int fac_bf_debug_block(fac_bf* h, int index, const float* d_in, int T, float* d_out, void* stream) {
  if (!h || !d_in || !d_out || T <= 0 || T > (1 << 20) || index < 0 || index > 15) return FAC_ERR_ARG;
  if (!h->loaded) return FAC_ERR_NOT_LOADED;
  if (hipSetDevice(h->device) != hipSuccess) return FAC_ERR_HIP;
  if (!run_block(index, d_in, h->d_w, h->blk[index], d_out, T, (hipStream_t)stream)) return FAC_ERR_SHAPE;
  return hipGetLastError() == hipSuccess ? FAC_OK : FAC_ERR_HIP;
}

int fac_bf_debug_heads(fac_bf* h, const float* d_b1, const float* d_b2, int T, float* d_r, float* d_c,
                       void* stream) {
  if (!h || !d_b1 || !d_b2 || !d_r || !d_c || T <= 0 || T > (1 << 20)) return FAC_ERR_ARG;
  if (!h->loaded) return FAC_ERR_NOT_LOADED;
  if (hipSetDevice(h->device) != hipSuccess) return FAC_ERR_HIP;
  const float* w = h->d_w;
  bf_heads<<<dim3(T, 8), 256, 0, (hipStream_t)stream>>>(d_b1, d_b2, w + h->w8, w + h->bias8, w + h->w16,
                                                         w + h->bias16, d_r, d_c);
  return hipGetLastError() == hipSuccess ? FAC_OK : FAC_ERR_HIP;
}

int fac_bf_tile_detections(fac_bf* h, const uint8_t* d_tiles, int T, float min_score, float* d_dets,
                           int32_t* d_counts, void* stream) {
  if (!h || !d_tiles || !d_dets || !d_counts || T <= 0 || T > (1 << 20)) return FAC_ERR_ARG;
  if (!h->loaded) return FAC_ERR_NOT_LOADED;
  if (hipSetDevice(h->device) != hipSuccess) return FAC_ERR_HIP;
  if (int rc = ensure(h, T, 0, 0)) return rc;
  return run_net(h, d_tiles, T, nullptr, nullptr, nullptr, nullptr, min_score, d_dets, d_counts,
                 (hipStream_t)stream);
}

int fac_bf_nms(fac_bf* h, const float* d_dets, const int32_t* d_counts, int G, int stride, float min_iou,
               float* d_out, int32_t* d_out_counts, int32_t* d_overflow, void* stream) {
  if (!h || !d_dets || !d_counts || !d_out || !d_out_counts || !d_overflow || G <= 0 || G > (1 << 20))
    return FAC_ERR_ARG;
  if (stride <= 0 || stride > kMaxIn) return FAC_ERR_SHAPE;
  if (hipSetDevice(h->device) != hipSuccess) return FAC_ERR_HIP;
  if (int rc = ensure(h, 0, 0, G)) return rc;
  // normalised coordinates: no window mapping, no margin boxes
  return run_nms(h, d_dets, d_counts, G, 1, stride, 0, kTile, 0, 1, 1, min_iou, d_out, nullptr, d_out_counts,
                 d_overflow, (hipStream_t)stream);
}

int fac_bf_debug_postprocess(fac_bf* h, const float* d_r, const float* d_c, int F, int H, int W, float min_score,
                             float min_iou, float* d_tile_dets, int32_t* d_tile_counts, float* d_dets,
                             int32_t* d_boxes, int32_t* d_counts, int32_t* d_overflow, void* stream) {
  if (!h || !d_r || !d_c || !d_dets || !d_boxes || !d_counts || !d_overflow || F <= 0 || H <= 0 || W <= 0)
    return FAC_ERR_ARG;
  if (!h->loaded) return FAC_ERR_NOT_LOADED;
  int split, x_step, ntiles;
  if (!windows(H, W, &split, &x_step, &ntiles)) return FAC_ERR_SHAPE;
  if ((long long)F * ntiles > (1 << 20)) return FAC_ERR_SHAPE;
  const int T = F * ntiles;
  if (hipSetDevice(h->device) != hipSuccess) return FAC_ERR_HIP;
  if (int rc = ensure(h, 0, T, F)) return rc;
  hipStream_t st = (hipStream_t)stream;
  float* td = d_tile_dets ? d_tile_dets : h->tile_dets;
  int32_t* tc = d_tile_counts ? d_tile_counts : h->tile_counts;
  bf_decode<<<T, kAnchors, 0, st>>>(d_r, d_c, h->d_w + h->anchors, min_score, td, tc);
  return run_nms(h, td, tc, F, ntiles, kAnchors, 1, split, x_step, H, W, min_iou, d_dets, d_boxes, d_counts,
                 d_overflow, st);
}

int fac_bf_detect(fac_bf* h, const uint8_t* d_frames, int F, int H, int W, float min_score, float min_iou,
                  float* d_dets, int32_t* d_boxes, int32_t* d_counts, int32_t* d_overflow, void* stream) {
  if (!h || !d_frames || !d_dets || !d_boxes || !d_counts || !d_overflow || F <= 0 || H <= 0 || W <= 0)
    return FAC_ERR_ARG;
  if (!h->loaded) return FAC_ERR_NOT_LOADED;
  int split, x_step, ntiles;
  if (!windows(H, W, &split, &x_step, &ntiles)) return FAC_ERR_SHAPE;
  if ((long long)F * H * W * 3 >= (1ll << 40) || (long long)F * ntiles > (1 << 20)) return FAC_ERR_SHAPE;
  const int T = F * ntiles;
  if (hipSetDevice(h->device) != hipSuccess) return FAC_ERR_HIP;
  if (int rc = ensure(h, T, T, F)) return rc;
  hipStream_t st = (hipStream_t)stream;
  launch_tiles(d_frames, T, H, W, split, x_step, ntiles, h->tiles, st);
  if (int rc = run_net(h, h->tiles, T, nullptr, nullptr, nullptr, nullptr, min_score, h->tile_dets, h->tile_counts,
                       st))
    return rc;
  return run_nms(h, h->tile_dets, h->tile_counts, F, ntiles, kAnchors, 1, split, x_step, H, W, min_iou, d_dets,
                 d_boxes, d_counts, d_overflow, st);
}

}  // extern "C"
