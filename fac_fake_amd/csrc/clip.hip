// Clip staging of the S3D-family models (S3D, CA_S3D_v3, msca_S3D): face
// boxes of decoded BGR frames -> the uint8 [B,3,T,224,224] clip S3D._pack
// takes.  The harness does it on the CPU, per frame: frame[top:bottom,
// left:right] (preprocessing/extract_crops.py:69), then
// IsotropicResize(224, INTER_AREA down / INTER_CUBIC up) and
// PadIfNeeded(224, 224, BORDER_CONSTANT) (S3D-test.py:65-73,
// transforms/albu.py:9-26), then the 20 frames stacked, still BGR
// (S3D-test.py:94-96).  Here every box of every clip is one launch.
//
// A box row is (frame, left, top, right, bottom, ow, oh): the box is clipped
// to the frame (cw x ch), resized to ow x oh -- the host computes them as
// isotropically_resize_image does, in float64 -- and centred in a zero
// 224 x 224 plane per channel, top = (224 - oh) / 2, left = (224 - ow) / 2
// (the remainder goes bottom / right, as PadIfNeeded's).  The resize is
//   max(cw, ch) == 224  a copy (albu.py:12-13 returns the image: ow x oh is
//                       cw x ch whatever the table says);
//   max(cw, ch)  > 224  cv2.INTER_AREA on a true downscale: crop.hip's
//                       exact-integer overlap sums with 224 replaced by ow /
//                       oh per axis, round half up over cw * ch;
//   max(cw, ch)  < 224  cv2.INTER_CUBIC's 8-bit scheme (OpenCV 4.x resize.cpp,
//                       hal::resize / interpolateCubic / HResizeCubic /
//                       VResizeCubic with FixedPtCast): fx = (float)((d + 0.5)
//                       * scale - 0.5) with scale = 1 / (dst / src) in double,
//                       four taps at floor(fx) - 1 .. + 2 clamped to the box,
//                       float coefficients with A = -0.75 rounded to 1/2048,
//                       an exact-integer horizontal pass and
//                       (sum + 2^21) >> 22 saturated for the vertical one.
// The coefficient arithmetic uses explicit _rn intrinsics and this file is
// compiled with -ffp-contract=off (build.py FILE_FLAGS: the intrinsics are
// plain operators in the HIP headers and would otherwise fuse into FMAs once
// inlined), so every tap equals the host restatement's
// (tests/clip_stage_ref.py) and the kernel is bit-identical to it.  cv2 is not
// available to the tests: its SIMD builds evaluate the cubic vertical pass in
// float and INTER_AREA with float weights, so it may differ by a count, and
// parity with cv2 itself is unpinned (as for crop.hip).
// A bad frame index, cw, ch, ow or oh <= 0, or ow or oh over 224 (no host
// table has one) gives zero planes; every byte of every plane is written.
#include "common.hpp"

namespace fac {

constexpr int kClip = 224;

// cv2's cubic taps of output pixel d, src -> dst pixels: first tap index
// s - 1 (unclamped) and the four coefficients in 1/2048 units.
__device__ inline void cubic_tap(int d, int src, int dst, int& s, int a[4]) {
  const double scale = __ddiv_rn(1.0, __ddiv_rn((double)dst, (double)src));
  const float fx = (float)__dsub_rn(__dmul_rn(__dadd_rn((double)d, 0.5), scale), 0.5);
  const float fl = floorf(fx);
  s = (int)fl;
  const float x = __fsub_rn(fx, fl);
  const float A = -0.75f;
  const float x1 = __fadd_rn(x, 1.f), xm = __fsub_rn(1.f, x);
  // ((A (x+1) - 5A)(x+1) + 8A)(x+1) - 4A
  const float c0 = __fsub_rn(
      __fmul_rn(__fadd_rn(__fmul_rn(__fsub_rn(__fmul_rn(A, x1), 5.f * A), x1), 8.f * A), x1), 4.f * A);
  // ((A+2) x - (A+3)) x x + 1, and the same in 1 - x
  const float c1 = __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(A + 2.f, x), A + 3.f), x), x), 1.f);
  const float c2 = __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(A + 2.f, xm), A + 3.f), xm), xm), 1.f);
  const float c3 = __fsub_rn(__fsub_rn(__fsub_rn(1.f, c0), c1), c2);
  a[0] = __float2int_rn(__fmul_rn(c0, 2048.f));
  a[1] = __float2int_rn(__fmul_rn(c1, 2048.f));
  a[2] = __float2int_rn(__fmul_rn(c2, 2048.f));
  a[3] = __float2int_rn(__fmul_rn(c3, 2048.f));
}

// The three bytes of the pixel at p as ONE (unaligned) dword load: with a
// load per byte the kernel was bound by its count of load instructions, not
// by bytes or arithmetic.  The fourth byte, the next pixel's first, is
// dropped; the frames' last pixel has none, so its dword starts one byte
// earlier (lim: the last address a dword may start at) and is shifted down.
__device__ inline void load_px(const uint8_t* p, const uint8_t* lim, int& c0, int& c1, int& c2) {
  const uint8_t* q = p < lim ? p : lim;
  uint32_t v;
  __builtin_memcpy(&v, q, 4);
  v >>= 8 * (unsigned)(p - q);
  c0 = v & 255;
  c1 = (v >> 8) & 255;
  c2 = (v >> 16) & 255;
}

// Area-weighted sums of one output pixel over source columns sx0..sx1 and
// rows sy0..sy1 (intervals [X0, X1) / [Y0, Y1) in 1/ow / 1/oh pixel units).
// Acc: 32 bits hold 255 * cw * ch for every box of up to 8.4 Mpixel.
template <typename Acc>
__device__ inline void area_sums(const uint8_t* __restrict__ src, const uint8_t* lim, int W, int ow, int oh, int X0,
                                 int X1, int sx0, int sx1, int Y0, int Y1, int sy0, int sy1, Acc& acc0, Acc& acc1,
                                 Acc& acc2) {
  for (int sy = sy0; sy <= sy1; ++sy) {
    const int ovy = min(Y1, (sy + 1) * oh) - max(Y0, sy * oh);
    Acc r0 = 0, r1 = 0, r2 = 0;
    const uint8_t* row = src + (size_t)sy * W * 3;
    for (int sx = sx0; sx <= sx1; ++sx) {
      const int ovx = min(X1, (sx + 1) * ow) - max(X0, sx * ow);
      int c0, c1, c2;
      load_px(row + sx * 3, lim, c0, c1, c2);
      r0 += ovx * c0;
      r1 += ovx * c1;
      r2 += ovx * c2;
    }
    acc0 += (Acc)ovy * r0;
    acc1 += (Acc)ovy * r1;
    acc2 += (Acc)ovy * r2;
  }
}

// floor(num / den) for a quotient of at most 255: a float estimate (relative
// error far under 1 / 255), then one exact step either way.
__device__ inline int div_u8(unsigned num, unsigned den, float inv) {
  int q = (int)((float)num * inv);
  const long long r = (long long)num - (long long)q * den;
  return r < 0 ? q - 1 : (r >= (long long)den ? q + 1 : q);
}

constexpr int kRows = 8;                    // output rows per workgroup
constexpr long long kDen32 = 8404991;       // 511 * den < 2^32: the rounded division fits 32 bits

// One thread per output column (all 3 channels) of kRows output rows; grid
// (box, 224 / kRows).  What depends on the column alone (the cubic x taps with
// their double divisions, the area branch's column range) is computed once
// per thread, the rows' cubic y taps once per workgroup (threads 0..kRows-1,
// through LDS).  A wave's stores go to three planes, consecutive lanes to
// consecutive x, four pixels per dword.
__global__ __launch_bounds__(256) void clip_stage_u8(const uint8_t* __restrict__ frames, int n_frames, int H, int W,
                                                     const int32_t* __restrict__ boxes, int T,
                                                     uint8_t* __restrict__ out) {
  __shared__ int ytap[kRows][5];  // per row: floor(fy) and the four y taps
  const int n = blockIdx.x, oy0 = blockIdx.y * kRows, ox = threadIdx.x;
  const int32_t* bx = boxes + 7 * n;  // (frame, left, top, right, bottom, ow, oh)
  const int f = bx[0];
  const int x0 = max(bx[1], 0), y0 = max(bx[2], 0), x1 = min(bx[3], W), y1 = min(bx[4], H);
  const int cw = x1 - x0, ch = y1 - y0;
  int ow = bx[5], oh = bx[6];
  const int big = max(cw, ch);
  if (big == kClip) {
    ow = cw;
    oh = ch;
  }
  const bool ok = f >= 0 && f < n_frames && cw > 0 && ch > 0 && ow > 0 && oh > 0 && ow <= kClip && oh <= kClip;
  const int left = (kClip - ow) / 2, top = (kClip - oh) / 2;
  const bool cubic = ok && big < kClip;  // (uniform over the workgroup)
  if (cubic) {
    if (ox < kRows) {
      const int dy = oy0 + ox - top;
      if (dy >= 0 && dy < oh) cubic_tap(dy, ch, oh, ytap[ox][0], &ytap[ox][1]);
    }
    __syncthreads();
  }
  if (ox >= kClip) return;
  const int dx = ox - left;
  const bool live = ok && dx >= 0 && dx < ow;
  // the column's share of the work
  int X0 = 0, X1 = 0, sx0 = 0, sx1 = -1, a[4] = {0, 0, 0, 0}, cx[4] = {0, 0, 0, 0};
  // an output column's interval covers at most ceil(cw / ow) + 1 source
  // columns: up to 4 (boxes of up to 3 * 224 px) they are four taps a[k] at
  // cx[k] like the cubic ones (weight 0 past the interval), so a row's four
  // loads are independent and in flight together
  const bool area4 = ok && big > kClip && (cw + ow - 1) / ow + 1 <= 4 && (long long)cw * ch <= kDen32;
  if (live && big > kClip) {
    // interval of this output column in 1/ow pixel units, relative to the box
    X0 = dx * cw;
    X1 = X0 + cw;
    sx0 = X0 / ow;
    sx1 = min((X1 - 1) / ow, cw - 1);  // covered source columns (inclusive)
    if (area4) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int sx = sx0 + k;
        a[k] = max(min(X1, (sx + 1) * ow) - max(X0, sx * ow), 0);
        cx[k] = min(sx, cw - 1) * 3;
      }
    }
  } else if (live && cubic) {
    int sx;
    cubic_tap(dx, cw, ow, sx, a);
#pragma unroll
    for (int k = 0; k < 4; ++k) cx[k] = min(max(sx - 1 + k, 0), cw - 1) * 3;
  }
  const long long den = (long long)cw * ch;
  const bool den32 = den <= kDen32;
  const float inv2 = den32 && ok ? __builtin_amdgcn_rcpf((float)(unsigned)(2 * den)) : 0.f;
  const size_t plane = (size_t)T * kClip * kClip;  // one channel of one clip
  uint8_t* dst = out + (size_t)(n / T) * 3 * plane + ((size_t)(n % T) * kClip + oy0) * kClip + ox;
  const uint8_t* src = ok ? frames + (((size_t)f * H + y0) * W + x0) * 3 : frames;
  const uint8_t* lim = frames + (size_t)n_frames * H * W * 3 - 4;  // (at least two pixels: the launcher checks)
#pragma unroll 1
  for (int r = 0; r < kRows; ++r, dst += kClip) {
    const int dy = oy0 + r - top;
    int v0 = 0, v1 = 0, v2 = 0;
    if (live && dy >= 0 && dy < oh) {
      if (big == kClip) {
        load_px(src + ((size_t)dy * W + dx) * 3, lim, v0, v1, v2);
      } else if (big > kClip) {
        const int Y0 = dy * ch, Y1 = Y0 + ch;
        const int sy0 = Y0 / oh, sy1 = min((Y1 - 1) / oh, ch - 1);
        if (den32) {
          unsigned acc0 = 0, acc1 = 0, acc2 = 0;
          if (area4) {
#pragma unroll 2
            for (int sy = sy0; sy <= sy1; ++sy) {
              const unsigned ovy = min(Y1, (sy + 1) * oh) - max(Y0, sy * oh);
              const uint8_t* row = src + (size_t)sy * W * 3;
              unsigned h0 = 0, h1 = 0, h2 = 0;
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                int c0, c1, c2;
                load_px(row + cx[k], lim, c0, c1, c2);
                h0 += a[k] * c0;
                h1 += a[k] * c1;
                h2 += a[k] * c2;
              }
              acc0 += ovy * h0;
              acc1 += ovy * h1;
              acc2 += ovy * h2;
            }
          } else {
            area_sums(src, lim, W, ow, oh, X0, X1, sx0, sx1, Y0, Y1, sy0, sy1, acc0, acc1, acc2);
          }
          const unsigned d = (unsigned)den, d2 = 2 * d;  // round half up
          v0 = div_u8(2 * acc0 + d, d2, inv2);
          v1 = div_u8(2 * acc1 + d, d2, inv2);
          v2 = div_u8(2 * acc2 + d, d2, inv2);
        } else {
          long long acc0 = 0, acc1 = 0, acc2 = 0;
          area_sums(src, lim, W, ow, oh, X0, X1, sx0, sx1, Y0, Y1, sy0, sy1, acc0, acc1, acc2);
          v0 = (int)((2 * acc0 + den) / (2 * den));
          v1 = (int)((2 * acc1 + den) / (2 * den));
          v2 = (int)((2 * acc2 + den) / (2 * den));
        }
      } else {
        const int sy = ytap[r][0];
        int s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint8_t* row = src + (size_t)min(max(sy - 1 + j, 0), ch - 1) * W * 3;
          int h0 = 0, h1 = 0, h2 = 0;  // horizontal pass, exact: |h| <= 255 * 2816
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            int c0, c1, c2;
            load_px(row + cx[k], lim, c0, c1, c2);
            h0 += a[k] * c0;
            h1 += a[k] * c1;
            h2 += a[k] * c2;
          }
          const int b = ytap[r][1 + j];
          s0 += b * h0;  // |sum| <= 255 * 2816^2 < 2^31
          s1 += b * h1;
          s2 += b * h2;
        }
        v0 = min(max((s0 + (1 << 21)) >> 22, 0), 255);
        v1 = min(max((s1 + (1 << 21)) >> 22, 0), 255);
        v2 = min(max((s2 + (1 << 21)) >> 22, 0), 255);
      }
    }
    // planar, channels stay BGR: four neighbouring lanes' pixels go out as one
    // dword per plane from the first of them (rows start at multiples of 4
    // bytes: 224 = 4 * 56, and the ABI checks the base).
    const int pk = v0 | v1 << 8 | v2 << 16;
    const int p1 = __shfl_down(pk, 1), p2 = __shfl_down(pk, 2), p3 = __shfl_down(pk, 3);
    if ((ox & 3) == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int sh = 8 * c;
        *reinterpret_cast<uint32_t*>(dst + c * plane) = (uint32_t)((pk >> sh) & 255) | (uint32_t)((p1 >> sh) & 255) << 8 |
                                                        (uint32_t)((p2 >> sh) & 255) << 16 |
                                                        (uint32_t)((p3 >> sh) & 255) << 24;
      }
    }
  }
}

static_assert(kClip % kRows == 0, "whole row groups");

hipError_t launch_clip_stage(const uint8_t* frames, int n_frames, int H, int W, const int32_t* boxes, int n_boxes,
                             int T, uint8_t* clips, hipStream_t st) {
  if (n_boxes <= 0) return hipSuccess;
  clip_stage_u8<<<dim3(n_boxes, kClip / kRows), 256, 0, st>>>(frames, n_frames, H, W, boxes, T, clips);
  return hipGetLastError();
}

}  // namespace fac

