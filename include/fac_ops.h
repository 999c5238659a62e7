/* fac_ops.h — C ABI of the layer-level gfx950 kernels behind the §8f model
 * families: ResVitKan (config 5) and S3D (config 4).
 *
 * The CViT path has one fused entry point per forward (fac_cvit.h); the
 * ResNet-50 stem of ResVitKan and the Inception-3D blocks of S3D are
 * sequences of ordinary layers, orchestrated by their Python mirrors
 * (fac_fake_amd/resvitkan.py, fac_fake_amd/s3d.py) and captured into one
 * hipGraph per forward.  Every entry point is stream-ordered, takes device
 * pointers and plain sizes, returns 0 or a negative fac_status
 * (fac_cvit.h) and never throws.
 *
 * Activations are 16-bit (bf16 or fp16, `dtype` as in fac_cvit.h)
 * channels-last N·D·H·W·C tensors, C a multiple of 8 (inputs with 3
 * channels are packed to 8 by fac_pack_input).  2-D layers are D = 1.
 */
#ifndef FAC_OPS_H
#define FAC_OPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Epilogue flags of fac_conv_nd. */
#define FAC_CONV_RELU 1      /* v = max(acc + bias, 0) */
#define FAC_CONV_RESID 2     /* v = v + residual[m][r_off + c] (16-bit) */
#define FAC_CONV_RELU2 4     /* v = max(v, 0) after the residual */
#define FAC_CONV_OUT_F32 8   /* fp32 output instead of 16-bit */
#define FAC_CONV_MAXPOOL3S2 16 /* then MaxPool2d(3, 2, 1) over H, W: out is
                                [n][od][oh/2][ow/2][ldo]; only with
                                FAC_CONV_RELU alone, on the space-to-depth
                                first conv below (ResNet-50's conv1 + bn1 +
                                relu + maxpool, ResVitKan.py:187/205);
                                FAC_ERR_ARG otherwise */
#define FAC_CONV_PREPOOL3S2 64 /* MaxPool3d((1,3,3), (1,2,2), (0,1,1)) over the
                                INPUT first, then the conv: a 1x1x1 conv,
                                cin = cout = 64, input width 56 (rows of
                                28 pooled positions); desc->d/h/w are the
                                unpooled input's, od/oh/ow the pooled
                                output's; flags FAC_CONV_RELU at most besides
                                this one; FAC_ERR_ARG otherwise.  S3D's
                                base.1 + base.2 (model.py:19-20) without
                                the pooled map in memory */
#define FAC_CONV_MAXPOOL3S1 32 /* MaxPool3d(3, 1, 1) over the INPUT first
                                (-inf padding), then the conv: a 1x1x1 conv
                                (stride 1, no padding) over an S x S map,
                                S in {14, 7, 3}, cout % 32 == 0, ldo and
                                c_off % 8 == 0, flags FAC_CONV_RELU at most
                                besides this one; FAC_ERR_ARG otherwise.
                                S3D's Inception branch3 (MaxPool3d +
                                BasicConv3d(cin, cout, 1), model.py:84-342)
                                without the pooled map in memory */

/* One N-d convolution (Conv2d / Conv3d, any kernel, stride, zero padding,
 * dilation 1, groups 1) with folded BatchNorm, as an implicit GEMM on MFMA:
 * rows = output positions (n, z, y, x), columns = output channels,
 * k = (tap, input channel).
 *
 * Replaces nn.Conv2d + nn.BatchNorm2d(eval) (+ nn.ReLU, + the residual add
 * of a ResNet Bottleneck) — CViT-main/ResVitKan/ResVitKan.py:124-152,
 * :187-200, :232-240 — and nn.Conv3d + BatchNorm3d(eval) + ReLU of S3D's
 * BasicConv3d / SepConv3d — sx_exp_deepfakedetect-master/S3D/model.py:50-82.
 *
 * weight: 16-bit [cout_pad][k_pad], row o = output channel, k index =
 *   ((tz*kh + ty)*kw + tx)*cin + c, zero beyond taps*cin; cout_pad a
 *   multiple of 128, k_pad a multiple of 64 (fac_conv_weight_layout).
 * bias: fp32 [cout_pad] (BN shift folded in), or NULL for none (every
 *   routed kernel honours NULL).
 * out: row m = ((n*Do + z)*Ho + y)*Wo + x, element [m*ldo + c_off + c];
 *   c_off lets Inception branches write straight into their concat slot.
 * residual (FAC_CONV_RESID): 16-bit [m*ldr + r_off + c].
 * Shapes with a dedicated kernel are routed to it inside this call (same
 * contract): the 4x4/1 16->64 conv over space-to-depth cells (conv_s2d4:
 * ResNet-50's / S3D's first conv) and temporal (kd,1,1) convs with 8 output
 * frames, cin % 64 == 0, cout % 64 == 0 (conv_tk), and
 * stride-1 1x1 convs with cin 64, 128 or 256, cout % 64 == 0, no fp32
 * output (conv_pw: ResNet-50's K <= 256 bottleneck 1x1s), of which the
 * residual ones with cin 128 (cout % 256 == 0) or 256 (cout % 128 == 0) take
 * pw_res (ResNet-50 layer2 / layer3 conv3 + identity; fac_set_option
 * "pw_res" 0 routes them to the generic kernel for A/B), and 1x1 residual
 * convs with cin 512, cout % 256 == 0 (layer4's conv3 + identity) take
 * pw_res2 (weights in VGPRs; "pw_res" 2 or 0 routes them to convnd_pt). */
typedef struct fac_conv_desc {
  int dtype;
  const void* in;
  int n, d, h, w, cin;          /* input dims; cin % 8 == 0 */
  const void* weight;
  const float* bias;
  int cout, k_pad;              /* k_pad: weight row length (elements) */
  int kd, kh, kw;               /* kernel */
  int sd, sh, sw;               /* stride */
  int pd, ph, pw;               /* zero padding */
  int od, oh, ow;               /* output dims (floor mode) */
  void* out;
  int ldo, c_off;
  const void* residual;
  int ldr, r_off;
  int flags;
} fac_conv_desc;

int fac_conv_nd(const fac_conv_desc* desc, void* stream);

/* fac_conv_nd whose output columns go to three tensors: [0, split1) to
 * desc->out (ldo, c_off), [split1, split2) to out1 (row stride ldo1, from
 * column 0), [split2, cout) to out2 (ldo2).  For convs that share an input,
 * e.g. the three 1x1x1 heads of an S3D Inception block (model.py:84-342:
 * branch0, branch1.0, branch2.0) as one GEMM over concatenated weights:
 * every output column is computed exactly as by its own launch.  Splits are
 * multiples of 8; no residual, no fp32 output. */
int fac_conv_nd_split(const fac_conv_desc* desc, void* out1, int ldo1, int split1, void* out2, int ldo2, int split2,
                      void* stream);

/* relu(conv(desc) + bias, if desc->flags has FAC_CONV_RELU) + conv(ds) +
 * ds bias, then ReLU if desc->flags has FAC_CONV_RELU2: a ResNet bottleneck's
 * conv3 + bn3 (+ReLU, ResVitKan.py:146-152) with its downsample branch
 * (conv + bn, ResVitKan.py:150) added in the same launch, so the downsample
 * output never goes through memory.  Both convs: cin % 64 == 0, the same
 * output positions [n, od, oh, ow] and cout (% 128 == 0); ds->out is ignored
 * and ds->flags must be 0; no FAC_CONV_RESID / FAC_CONV_OUT_F32 on desc.
 * Replaces fac_conv_nd(ds) + fac_conv_nd(desc with residual = its output).
 * Layer1's 64 -> 256 pair with a stride-1 1x1 downsample runs on pw_res
 * DUAL (both weight blocks resident in LDS), layer2's 128 -> 512 and
 * layer3's 256 -> 1024 conv3 with the stride-2 256 -> 512 / 512 -> 1024
 * downsample (cout % 256 == 0) on pw_dual2 (both weight blocks in VGPRs;
 * fac_set_option "pw_res" 2
 * routes it to convnd_pt for A/B, 0 routes both), the others on convnd_pt
 * DUAL. */
int fac_conv_nd_dual(const fac_conv_desc* desc, const fac_conv_desc* ds, void* stream);

/* The kernel family fac_conv_nd / fac_conv_nd_split would launch for this
 * descriptor ("conv_pw", "pw_res", "conv_tk2", "convnd_pt", ...; the generic
 * implicit GEMM with its tile and workgroups per CU, "convnd_igemm:128x64:3"),
 * or NULL with *status set when the call would be rejected.  split1 = split2
 * = INT_MAX asks about fac_conv_nd, anything else about fac_conv_nd_split
 * into dense segments (ldo1 = split2 - split1, ldo2 = cout - split2).
 * Launches nothing; pointers in the descriptor are only tested for NULL.
 * The answers follow fac_set_option's process-wide A/B knobs. */
const char* fac_conv_nd_route(const fac_conv_desc* desc, int split1, int split2, int* status);
/* The same for fac_conv_nd_dual and, below, fac_pool_nd. */
const char* fac_conv_nd_dual_route(const fac_conv_desc* desc, const fac_conv_desc* ds, int* status);

/* A ResNet-50 layer1 / layer2 bottleneck's conv3 and the next block's conv1
 * in one launch (ResVitKan.py:146-152; torchvision resnet50): c3 = the 1x1
 * 64 -> 256 (layer1) or 128 -> 512 (layer2) conv3 + bn3 with flags exactly
 * FAC_CONV_RELU | FAC_CONV_RESID | FAC_CONV_RELU2 (out = relu(relu(conv + b)
 * + residual), the block output, ldo = cout); c1 = the next block's 1x1
 * 256 -> 64 / 128 (layer1) or 512 -> 128 (layer2) conv1 + bn1 with
 * flags exactly FAC_CONV_RELU over the same positions: its input is c3's
 * output (c1->in is ignored), written to c1->out (ldo = cout).  Every
 * output is what fac_conv_nd(c3) then fac_conv_nd(c1) would produce up to
 * fp32 summation order; the 256-channel map is written once and not read
 * back.  FAC_ERR_ARG / FAC_ERR_SHAPE for anything else. */
int fac_bottleneck_pw2(const fac_conv_desc* c3, const fac_conv_desc* c1, void* stream);

/* S3D Mixed_3b's branch2 SepConv3d(16, 32, 3) (model.py:84-110) in one
 * launch: sdsc = the (1,3,3) conv 16 -> 32 (+ BN folded, FAC_CONV_RELU at
 * most) over desc->in = [n][8][14][14][16], tdsc = the (3,1,1) conv 32 -> 32
 * over its output (tdsc->in is ignored: the 32-channel map stays in LDS),
 * written to tdsc->out [m*ldo + c_off + c] (the block output's channel
 * slot).  Every output is what fac_conv_nd(sdsc) then fac_conv_nd(tdsc)
 * would produce up to fp32 summation order.  FAC_ERR_SHAPE for any other
 * shape. */
int fac_sep_tiny(const fac_conv_desc* sdsc, const fac_conv_desc* tdsc, void* stream);

/* S3D Mixed_3c's branch2 SepConv3d(32, 96, 3) (model.py:84-110) in one
 * launch: sdsc = the (1,3,3) conv 32 -> 96 over [n][8][14][14][32] with its
 * output channels zero-padded to 128 (cout 128: rows 96..127 zero weights
 * and bias, which this kernel skips), tdsc = the (3,1,1) conv over those 128
 * channels (cin 128) -> 96, written to tdsc->out [m*ldo + c_off + c]; the
 * middle map stays in LDS.  Every output is what fac_conv_nd(sdsc) then
 * fac_conv_nd(tdsc) would produce up to fp32 summation order.
 * FAC_ERR_SHAPE for any other shape. */
int fac_sep_mid(const fac_conv_desc* sdsc, const fac_conv_desc* tdsc, void* stream);

/* Weight packing geometry for fac_conv_nd: *cout_pad = cout rounded up to
 * 128, *k_pad = taps*cin rounded up to 64. */
int fac_conv_weight_layout(int cout, int cin, int kd, int kh, int kw, int* cout_pad, int* k_pad);

/* Max or average pooling, channels-last 16-bit (MaxPool2d/3d: padding is
 * -inf, i.e. ignored; AvgPool: count_include_pad=True, the PyTorch default).
 * mode 0 = max, 1 = avg.  out element [m*ldo + c_off + c].
 * Replaces nn.MaxPool2d(3, 2, 1) (ResVitKan.py:205), S3D's nn.MaxPool3d
 * layers and F.avg_pool3d (S3D/model.py:31-45). */
typedef struct fac_pool_desc {
  int dtype;
  const void* in;
  int n, d, h, w, c;
  int kd, kh, kw, sd, sh, sw, pd, ph, pw;
  int od, oh, ow;
  int mode;
  void* out;
  int ldo, c_off;
} fac_pool_desc;

int fac_pool_nd(const fac_pool_desc* desc, void* stream);
const char* fac_pool_nd_route(const fac_pool_desc* desc, int* status);

/* Input staging: 3-channel images -> 16-bit channels-last with c_pad
 * channels (zeros beyond 3): out[n][s][c] = (x / div - mean[c]) / std[c]
 * in fp32.  src_kind 0: uint8 [n][s][3] (face crops: div = 255 gives the
 * reference's x/255. then Normalize, cvit_prediction.py:214-215);
 * src_kind 1: fp32 planar [n][3][s] (an already normalised NCHW tensor, or
 * S3D's raw 0..255 NCTHW clip: div 1, mean 0, std 1).  s = spatial
 * positions per image; mean3/std3 may be NULL (0 / 1). */
int fac_pack_input(int dtype, const void* src, int src_kind, int n, int s, float div, const float* mean3,
                   const float* std3, void* out, int c_pad, void* stream);

/* Space-to-depth staging for a stride-2 first conv (ResNet-50's 7x7/2,
 * ResVitKan.py:187): [n][h/2 + pad_before + pad_after]^2 cells of 16
 * channels, cell (Y, X) channel ((dy*2 + dx)*4 + c) = normalised pixel
 * (2(Y - pad_before) + dy, 2(X - pad_before) + dx), channel c < 3 (zero
 * outside the image and for c = 3).  A 7x7/2 conv with padding 3 is then a
 * 4x4/1 conv without padding over this image (pad_before 2, pad_after 1),
 * with weights w'[o][ty][tx][(dy*2+dx)*4 + c] = w[o][c][2ty+dy-1][2tx+dx-1]:
 * K = 256 instead of 49 taps x 8 padded channels.  src_kind as in
 * fac_pack_input; with frames > 1 the fp32 source is a clip batch
 * [n][3][frames][h][w] (S3D's (1,7,7)/(1,2,2) first conv, model.py:18) and
 * the output [n][frames][cells][cells][16]. */
int fac_pack_input_s2d(int dtype, const void* src, int src_kind, int n, int frames, int h, int w, int pad_before,
                       int pad_after, float div, const float* mean3, const float* std3, void* out, void* stream);

/* fac_conv_nd over fac_pack_input_s2d(src_kind 1, div 1, no mean / std)'s
 * cells of the fp32 clip batch `clip` [n][3][frames][h][w], with the packing
 * folded into the conv's halo staging (S3D's base.0 spatial conv,
 * model.py:18): `desc` describes that conv exactly as fac_conv_nd would get
 * it (cells [n][frames][h/2+pad_before+pad_after]^2[16], the 4x4/1 cout-64
 * s2d kernel, flags 0 or FAC_CONV_RELU); desc->in is not read.  The output
 * is bit-identical to fac_pack_input_s2d + fac_conv_nd. */
int fac_conv_s2d4_clip(const fac_conv_desc* desc, const float* clip, int h, int w, int pad_before, void* stream);

/* fac_conv_s2d4_clip over a uint8 clip batch [n][3][frames][h][w] (decoded
 * video frames, S3D-test.py:94-96's 0..255 values before the float cast): the
 * same output as fac_conv_s2d4_clip on that clip cast to fp32, a quarter of
 * the input bytes.  Round-4 addition, no reference counterpart. */
int fac_conv_s2d4_clip_u8(const fac_conv_desc* desc, const uint8_t* clip, int h, int w, int pad_before,
                          void* stream);

/* S3D's base.0 (SepConv3d(3, 64, k 7, s 2, p 3), model.py:18,63-82) in one
 * launch from a uint8 clip batch [n][3][16][h][w] with h / 2 = w / 2 = 56
 * (the 112 x 112 clips of S3D-test.py): `sdesc` is the spatial half as
 * fac_conv_s2d4_clip_u8 takes it (the space-to-depth 4x4 conv, cout 64),
 * `tdesc` the temporal (7,1,1)/(2,1,1) conv (64 -> 64, 16 -> 8 frames, its
 * `in` unused) whose `out` receives [n][8][56][56][64].  The 16-frame
 * half-resolution map between the two never goes through HBM; the output is
 * bit-identical to fac_conv_s2d4_clip_u8 followed by fac_conv_nd(tdesc). */
int fac_s3d_base0_u8(const fac_conv_desc* sdesc, const fac_conv_desc* tdesc, const uint8_t* clip, int h, int w,
                     int pad_before, void* stream);

/* KANLinear forward (CViT-main/ResVitKan/kan.py:189-206), fp32:
 *   y = silu(x) · base_weightᵀ + b_splines(x) · (spline_weight ⊙ spline_scaler)ᵀ
 * with order-3 B-spline bases over the per-feature knot vector `grid`
 * [in][n_knots] (kan.py:90-132, the Cox–de Boor recursion in the
 * reference's operation order).  `wcat` is the fused weight, k-major
 * [in][1 + nb][out] (index 0 = base_weight[o][i], 1.. = the scaled spline
 * weights spline_weight[o][i][k] * spline_scaler[o][i], nb = n_knots - 4).
 * x [rows][in] fp32 -> y [rows][out] fp32.  `partial` is a scratch buffer of
 * fac_kan_scratch_bytes() bytes: ceil(in/32) slabs of [rows][out] fp32
 * (0 for a size <= 0).  FAC_ERR_ARG: a null pointer or a size <= 0;
 * FAC_ERR_SHAPE: n_knots != 12, or ceil(in/32)*rows*out >= 2^31 (the
 * outputs and the slabs are indexed in 32 bits). */
int fac_kan_linear(const float* x, int rows, int in_f, int out_f, const float* grid, int n_knots, const float* wcat,
                   float* y, void* partial, void* stream);
size_t fac_kan_scratch_bytes(int rows, int in_f, int out_f);

/* GGCA(c, h, w, reduction 16, groups) of the CViT RepBn8 variant fused with
 * its x = x * GGCA(x) — CViT-main/model/cvit_GGCA_ADD_DEConv_RepBn8.py:144-207,
 * :436-437 — on 16-bit channels-last features x [n][h][w][c]:
 *   att_h[y][c] = sigmoid(z(mean_x x) + z(max_x x)), att_w likewise over y,
 *   z = shared_conv: 1x1 (c/groups -> c/groups/16) + BatchNorm(eval, eps
 *   1e-5) + ReLU + 1x1 back, applied per channel group;
 *   out = x * ((x * att_h) * att_w), fp32 arithmetic, 16-bit out.
 * w1 [cr][cg], b1 [cr], bn4 [4][cr] = running_mean, running_var, weight,
 * bias; w2 [cg][cr], b2 [cg] (fp32; cg = c/groups, cr = cg/16).
 * FAC_ERR_SHAPE unless h, w <= 16, cg a multiple of 16, cg <= 256,
 * h*w*cg <= 16384 and (2h + 2w)*cg <= 8192 (the group's features and its
 * 2h + 2w pooled vectors are held in LDS).  FAC_ERR_ARG: a null pointer, a
 * dtype other than bf16 / fp16, n, h, w, c or groups <= 0, c % groups != 0. */
int fac_ggca(int dtype, const void* x, int n, int h, int w, int c, int groups, const float* w1, const float* b1,
             const float* bn4, const float* w2, const float* b2, void* out, void* stream);

/* GGCA with the caller's combine, for every GGCA site of the CViT variants
 * (ggca.hip).  x, the weights and att_h / att_w are fac_ggca's; with
 * g = (x * att_h) * att_w in fp32,
 *   op 0: out = x * g   (cvit_GGCA_ADD.py, ..._DEConv.py, ..._RepBn8.py)
 *   op 1: out = x + g   (cvit_GGCA_ADD_RepBn.py, ..._DEConv_RepBn{,3,4,5}.py)
 * rounded to 16 bits once.  The route depends on (h, w, c, groups) alone
 * (fac_ggca_apply_route: 1, 2, or 0 for a shape neither takes), so a crop's
 * output bits do not depend on n or on its place in the batch:
 *   1 LDS        shapes inside fac_ggca's limits; op 0 is bit-identical to
 *                fac_ggca.
 *   2 streaming  every other map with h, w <= 64, cg = c/groups a multiple
 *                of 16, cg <= 256 and c <= 2048 (cr = cg/16 may be 1):
 *                pooling (per-row and per-column mean and max), the shared
 *                MLP + sigmoid on the 2(h + w) pooled vectors of each group,
 *                element-wise apply.  No atomics, fixed reduction order.  x
 *                and out must be 16-byte aligned.  The partial results live
 *                in a library-owned fp32 workspace, one per (device, stream),
 *                of n * (2h + 2w*ceil(h/16) + h + w) * c floats, allocated
 *                the first time a stream needs that much and never moved
 *                afterwards, so later calls allocate nothing and can be
 *                captured into a graph.  Calls on one stream are ordered;
 *                calls on different streams use different workspaces.
 * FAC_ERR_ARG: a null or (route 2) misaligned pointer, a dtype other than
 * bf16 / fp16, an op other than 0 / 1, n, h, w, c or groups <= 0,
 * c % groups != 0.  FAC_ERR_SHAPE: a shape outside both routes.
 * FAC_ERR_OOM: the workspace could not be allocated, or would have to grow
 * while `stream` is capturing (run the shape once on it before capturing). */
int fac_ggca_apply_route(int h, int w, int c, int groups);
int fac_ggca_apply(int dtype, const void* x, int n, int h, int w, int c, int groups, const float* w1, const float* b1,
                   const float* bn4, const float* w2, const float* b2, int op, void* out, void* stream);

/* GGCA(x) itself, out = (x * att_h) * att_w rounded once, for the classes
 * that assign x = GGCA(x) (CViT-main/model/other/cvit_GGCA.py, cvit_GGCA4.py).
 * fac_ggca_apply's LDS route with no combine: its arguments, FAC_ERR_ARG as
 * there, FAC_ERR_SHAPE for a shape outside that route
 * (fac_ggca_apply_route(h, w, c, groups) != 1). */
int fac_ggca_scale(int dtype, const void* x, int n, int h, int w, int c, int groups, const float* w1, const float* b1,
                   const float* bn4, const float* w2, const float* b2, void* out, void* stream);

/* GCNet context block of CA_S3D_v3 — ContextBlock3d(c, ratio, pooling 'avg',
 * fusion ('channel_add',)), sx_exp_deepfakedetect-master/S3D/new_model/
 * context_block_3d.py:5-88 — on a 16-bit channels-last map x [n][s][c]
 * (s = T*H*W positions per clip):
 *   ctx[b][:]  = mean over s of x[b]                     (fp32 sum / s)
 *   h          = w0 ctx[b] + b0                          (p values)
 *   h          = LayerNorm over exactly those p values (biased variance,
 *                ln_eps, affine ln_w / ln_b), then min(max(h, 0), 6)
 *   term[b][:] = w3 h + b3                               (c values)
 *   out        = round_to_nearest_even_16(float(x) + term[b][c])
 * All of it fp32 between the 16-bit load and the one 16-bit conversion.
 * w0 [p][c] (channel_add_conv.0.weight), b0 [p], ln_w / ln_b [p], b3 [c];
 * w3t [p][c] is channel_add_conv.3.weight [c][p] TRANSPOSED (channel-minor,
 * so a wavefront reads consecutive channels).  out may be x.  term, if not
 * NULL, receives the fp32 [n][c] terms.  No atomics.
 * route: 1 per-clip (one launch, one workgroup per clip; the clip is held in
 * LDS when it fits), 2 split (partial sums over 64-row chunks, per-clip
 * reduce + MLP, vectorised apply: three launches), 0 picks one from (s, c)
 * alone (fac_context_route: per-clip for clips up to 256 KB).  Within one
 * route a clip's term and output do not depend on n or on its place in the
 * batch, and route 0 never switches with n, so the same holds for it; the
 * two routes add the pool in different orders and may differ in the last
 * bits of term.  scratch: fac_context_scratch_bytes(n, s, c) bytes of device
 * memory (0 for a bad shape); needed by the split route only, so it may be
 * NULL with route 1, or with route 0 when fac_context_route(s, c) is 1.
 * x and out must be 16-byte aligned.
 * FAC_ERR_SHAPE: c % 8 != 0, c > 4096, p < 1, p > 64, n < 1 or s < 1;
 * FAC_ERR_ARG: a null or misaligned pointer, a bad dtype or route. */
int fac_context_route(int s, int c);   /* 1 or 2: what route 0 takes; 0 for a bad shape */
size_t fac_context_scratch_bytes(int n, int s, int c);
int fac_context_add(int dtype, const void* x, int n, int s, int c, int p, const float* w0, const float* b0,
                    const float* ln_w, const float* ln_b, float ln_eps, const float* w3t, const float* b3,
                    void* out /* may == x */, float* term /* [n][c], may be NULL */, void* scratch,
                    int route /* 0 auto, 1 per-clip, 2 split */, void* stream);

/* The iFormer / MSCA blocks of msca_S3D (sx_exp_deepfakedetect-master/S3D/
 * new_model/iformer_3d.py, msca_3d.py, Conv3d.py) — msca.hip.  Activations
 * are 16-bit channels-last [n][t][h][w][ld]; every operand is a channel slice
 * [off, off + c) of rows of ld elements (ld, off, c multiples of 8, 16-byte
 * aligned base), so slices are read in place and results land in their slot
 * of a wider tensor.  fp32 between the 16-bit load and the one 16-bit
 * conversion; a clip's result does not depend on n.  Nothing is allocated or
 * synchronised; every launch goes to `stream`.
 * FAC_ERR_SHAPE: a bad n/t/h/w/c, k or kt; FAC_ERR_ARG: a null or misaligned
 * pointer, a slice outside its row, a bad dtype, act or op.
 *
 * fac_dwsep3d: DWSepConv3d(c, (kt,k,k), padding (kt/2,k/2,k/2)) — depthwise
 * (1,k,k) conv, then depthwise (kt,1,1) conv, zero padding, no bias — then
 *   v = min(max(acc * scale + shift, 0), 6)            (folded BN, ReLU6)
 *   act FAC_DWSEP_AFFINE2: v = v * scale2 + shift2     (fc_dw's own BN)
 *   act FAC_DWSEP_GELU:    v = v/2 (1 + erf(v/sqrt 2)) (the Mlp)
 * k in {3,5,7}, kt in {1,3}.  ws: fp32 TAP-MAJOR [k*k][c] (conv_s.weight
 * [c][1][k][k] transposed, so 8 channels of a tap are one vector); wt: fp32
 * [kt][c] (conv_t.weight transposed), NULL when kt == 1 (the host folds that
 * scale into ws).  Maps smaller than the window are fine.  out_f32: out is
 * fp32 [..][ldo] instead of 16-bit (tests: the value before the rounding). */
#define FAC_DWSEP_NONE 0
#define FAC_DWSEP_AFFINE2 1
#define FAC_DWSEP_GELU 2
typedef struct {
  int dtype;
  const void* in;
  int ldi, i_off;
  int n, t, h, w, c;
  int kt, k;
  const float* ws;
  const float* wt;
  const float* scale;
  const float* shift;
  int act;
  const float* scale2;
  const float* shift2;
  void* out;
  int ldo, o_off;
  int out_f32;
} fac_dwsep_desc;
int fac_dwsep3d(const fac_dwsep_desc* desc, void* stream);

/* MaxPool3d((kt,3,3), stride 1, padding (kt/2,1,1)) of in * scale + shift
 * (a BatchNorm applied on load: it does not commute with the max where a
 * scale is negative), kt in {1,3}; one 16-bit rounding of the max. */
int fac_bn_maxpool3d(int dtype, const void* in, int ldi, int i_off, int n, int t, int h, int w, int c, int kt,
                     const float* scale, const float* shift, void* out, int ldo, int o_off, void* stream);

/* Element-wise steps over rows x c: out = op(a[, b[, c3]]).  out may be a. */
#define FAC_EW_AFFINE 0    /* a * scale[c] + shift[c] */
#define FAC_EW_GELU 1      /* exact-erf GELU(a) */
#define FAC_EW_MUL 2       /* a * b */
#define FAC_EW_ADD 3       /* a + b */
#define FAC_EW_ADD_GELU 4  /* GELU(a + b) */
#define FAC_EW_CLAMP6 5    /* min(max(a, 0), 6) */
#define FAC_EW_ADD3 6      /* (a + b) + c3: the MSCA sum */
int fac_ew(int dtype, int op, const void* a, int lda, int a_off, const void* b, int ldb, int b_off, const void* c3,
           int ldc, int c_off, const float* scale, const float* shift, void* out, int ldo, int o_off, long long rows,
           int c, void* stream);

/* The CViT conv-stack kernels as layers (fac_cvit.h runs them inside its
 * fused forward; the CViT variants of the reference stack them differently —
 * the RepBn8 variant, SURVEY §8f-4, whose DEConv blocks fold into plain 3x3
 * convs, fac_fake_amd/repbn8.py).  Activations 16-bit NHWC.
 *
 * fac_conv3x3: Conv2d(3x3, stride 1, padding 1) + folded BN (+ ReLU if relu)
 * (+ MaxPool2d(2,2) if pool) — cvit.py:86-148 — on the halo-staged implicit
 * GEMM of conv.hip: in [n][h][h][cin] -> out [n][h'][h'][cout] (h' = h/2 with
 * pool); h in {112, 56, 28, 14} (224: cout 32, the unfused kernel), cin a
 * multiple of 32, cout a multiple of one of the resolution's blocks (64 at
 * 112; 128 or 64 at 56; 256, 192 or 128 at 28; 128, 192 or 64 at 14 — the
 * first of these, in the order given, that divides cout is used).  The 192
 * block at 14 has no fused pool: pool = 1 with such a cout (a multiple of 192
 * and not of 128) is FAC_ERR_SHAPE.  wpk: fac_conv3x3_pack of the folded fp32 weight
 * [cout][cin][3][3]; bias fp32 [cout]; zero256: 256 zero bytes of device
 * memory (the source of zero-padding loads).
 * fac_conv3x3_packed_elems: 16-bit elements of the packed weight (0: shape
 * not supported).  Packing runs on the host (host pointers). */
size_t fac_conv3x3_packed_elems(int h, int cin, int cout);
int fac_conv3x3_pack(int dtype, int h, int cin, int cout, const float* w, uint16_t* out);
int fac_conv3x3(int dtype, const void* in, const void* wpk, const float* bias, void* out, int n, int h, int cin,
                int cout, int pool, int relu, const void* zero256, void* stream);

/* The fused 224x224 block (stem224.hip): input normalisation, conv 3->32,
 * conv 32->32, conv 32->32 (each + folded BN + ReLU), MaxPool2d(2,2) ->
 * [n][112][112][32].  u8: uint8 NHWC crops [n][224][224][3] (x/255 and
 * Normalize fused); else normalised fp32 NCHW [n][3][224][224].  w1p:
 * fac_stem224_pack_conv1 of the folded [32][3][3][3] conv-1 weight (host ->
 * host, 32 x 64 16-bit); w2, w3: fac_conv3x3_pack with h = 224. */
int fac_stem224_pack_conv1(int dtype, const float* w, uint16_t* out);
int fac_stem224(int dtype, int u8, const void* in, const void* w1p, const float* b1, const void* w2, const float* b2,
                const void* w3, const float* b3, void* out, int n, void* stream);

/* A ResNet BasicBlock's second conv (CViT-main/ResKan/kan_resnet.py:57-63) in
 * one launch (resnet.hip): Conv2d(3x3, stride 1, padding 1, c -> c) + folded
 * bn2, + residual, then ReLU: out = max(conv(in) + bias + residual, 0).
 * in, residual, out: 16-bit channels-last [n][h][h][c]; fp32 accumulation,
 * the residual added in fp32, one rounding on the store.  (h, c) is one of a
 * ResNet-34's maps: (56, 64), (28, 128), (14, 256), (7, 512); at 7 the GEMM
 * rows run across crops (n*49), padding stays per crop.  wpk:
 * fac_conv3x3_res_pack of the folded fp32 weight [c][c][3][3] (host -> host,
 * fac_conv3x3_res_packed_elems 16-bit elements, 0 for an unsupported shape);
 * bias fp32 [c].  A crop's output does not depend on n.
 * FAC_ERR_ARG: a null pointer, a bad dtype, n <= 0; FAC_ERR_SHAPE: any other
 * (h, c), or n * 14 >= 2^31 (the launch grid). */
size_t fac_conv3x3_res_packed_elems(int h, int c);
int fac_conv3x3_res_pack(int dtype, int h, int c, const float* w, uint16_t* out);
int fac_conv3x3_res(int dtype, const void* in, const void* wpk, const float* bias, const void* residual, void* out,
                    int n, int h, int c, void* stream);

/* Mean over s of 16-bit x [n][s][c] -> fp32 y [n][c] (a global average pool
 * whose result is not rounded to 16 bits: the input of a KAN head).  fp32
 * sums over s in index order, no atomics: bitwise reproducible.  x 16-byte
 * aligned.  FAC_ERR_ARG: a null pointer, a bad dtype, n <= 0; FAC_ERR_SHAPE:
 * s < 1, c < 8 or c % 8 != 0. */
int fac_avgpool_f32(int dtype, const void* x, int n, int s, int c, float* y, void* stream);

/* InceptionDWConv2d -> BatchNorm2d (eval) -> ReLU (-> MaxPool2d(2,2) if pool)
 * of CViT-main/model/cvit_GGCA_ADD_DConv.py:157-177 in one launch
 * (idwconv.hip).  in [n][h][w][c] -> out [n][h'][w'][c] (h' = h/2, w' = w/2
 * with pool), 16-bit channels-last, 16-byte aligned.  With gc = c/8:
 *   channels [0, c - 3gc)   y = in
 *   the next gc             y = depthwise 3x3, padding 1     w_hw [gc][3][3]
 *   the next gc             y = depthwise 1x11 along w, padding 5   w_w [gc][11]
 *   the last gc             y = depthwise 11x1 along h, padding 5   w_h [gc][11]
 *   out = maxpool?(relu(scale[c] * y + shift[c]))
 * Taps, scale and shift are fp32 device arrays.  The taps are used as given
 * (not pre-multiplied by scale): y is an fp32 fma chain over the taps in index
 * order, taps outside the map are skipped (zero padding of the conv's input:
 * they contribute 0, not shift), then fma(scale, y, shift), ReLU, the window
 * max, and the only rounding, at the store.  The caller folds the conv bias
 * and the BatchNorm: scale = gamma / sqrt(var + eps), shift = beta - mean *
 * scale (+ bias * scale on the 3gc conv channels).  A crop's output does not
 * depend on n.
 * FAC_ERR_ARG: a null or misaligned pointer, a bad dtype, n <= 0;
 * FAC_ERR_SHAPE: c no multiple of 32 or outside 32..256, h or w outside
 * 1..224, odd h or w with pool. */
int fac_idwconv(int dtype, const void* in, void* out, int n, int h, int w, int c, const float* w_hw, const float* w_w,
                const float* w_h, const float* scale, const float* shift, int pool, void* stream);

/* WTConv2d(c, kernel_size 5, wt_levels 1) -> BatchNorm2d (eval) -> ReLU
 * (-> MaxPool2d(2,2) if pool) of
 * CViT-main/model/other/cvit_GGCA_ADD_WTConv.py:167-328 in one launch
 * (wtconv.hip).  in [n][h][w][c] -> out [n][h'][w'][c] (h' = h/2, w' = w/2
 * with pool), 16-bit channels-last, 16-byte aligned, h and w even.  Per
 * channel ch, cross-correlation as in F.conv2d, k = 0..3, i, j in {0, 1}:
 *   s_k[y][x]     = sum_ij dwt[ch][k][i][j] in[2y+i][2x+j]           (half resolution)
 *   t_k           = depthwise 5x5 of s_k with wtaps[ch][k], zero padding 2
 *                   at the half-resolution border
 *   u[2y+i][2x+j] = sum_k iwt[ch][k][i][j] t_k[y][x]
 *   b             = depthwise 5x5 of in with btaps[ch], zero padding 2
 *   out           = maxpool?(relu(scale[ch] * (u + b) + shift[ch]))
 * The operands are fp32 device arrays, 4-byte aligned, with the channel split
 * as ch = 4 * quad + e and e innermost, so that one wave's four channels are
 * one contiguous run:
 *   dwt, iwt  [c/4][4 k][4 = i*2+j][4 e]   the state_dict's wt_filter / iwt_filter [4c][1][2][2], row 4ch + k
 *   wtaps     [c/4][4 k][25 = dy*5+dx][4 e]  wavelet_convs.0.weight [4c][1][5][5] times wavelet_scale.0.weight
 *   btaps     [c/4][25][4 e]                 base_conv.weight [c][1][5][5] times base_scale.weight
 *   scale, shift [c]    scale = gamma / sqrt(var + eps), shift = beta - mean *
 *                       scale + base_scale * base_conv.bias * scale
 * Every sum is an fp32 fma chain from 0 in index order (ij, then the 25 taps
 * row-major, then k), then u + b, fma(scale, ., shift), ReLU, the window max
 * and the only rounding, at the store: the subbands and t_k stay fp32.  A
 * pixel outside the map enters as 0 (it contributes 0, never shift); for even
 * sides that is also the reference's zero padding of the subbands.  No
 * scratch, no atomics; a crop's output does not depend on n.
 * FAC_ERR_ARG: a null or misaligned pointer, a bad dtype, a pool flag other
 * than 0 or 1, n <= 0; FAC_ERR_SHAPE: c no multiple of 32 or outside 32..256,
 * h or w odd or outside 2..224. */
int fac_wtconv(int dtype, const void* in, void* out, int n, int h, int w, int c, const float* dwt, const float* wtaps,
               const float* iwt, const float* btaps, const float* scale, const float* shift, int pool, void* stream);

/* SMFA(x) or x + SMFA(x) of CViT-main/model/other/cvit_GGCA_SMFA.py:160-203
 * (smfa.hip) on a 16-bit channels-last map x [n][h][w][c] -> out [n][h][w][c],
 * for 8 <= h, w <= 15, where the block's adaptive max-pool is the per-channel
 * global max.  With t = linear_0(x), y = t[:, :c], xx = t[:, c:]:
 *   u    = alpha * (cw * max_p xx + cb) + belt * var_p xx    (unbiased variance)
 *   g    = GELU(w1 u + b1)                                    fp32, [n][c]
 *   hmap = GELU(wpw dw3x3(y) + bpw)     depthwise 3x3, zero padding, output j
 *                                       reads y channel j / 2, + dwb
 *   out  = [x +] wcat [xx * g | hmap] + bcat
 * fac_smfa_pack (host pointers, fp32 in) writes fac_smfa_packed_bytes(c) bytes:
 * w0 [2c][c], b0 [2c]; gate4 [4][c] = alpha, cw, cb, belt (cw, cb: dw_conv's
 * centre tap and bias); w1 [c][c], b1 [c]; dww [2c][9], dwb [2c]; wpw [2c][2c],
 * bpw [2c]; wcat [c][3c] = [linear_2.W | linear_2.W conv_1.W], bcat [c].  w0,
 * wpw and wcat become 16-bit MFMA operands, the rest stays fp32.  wpk is that
 * blob in device memory.  gate_out: an optional fp32 [n][c] copy of g.
 * scratch: fac_smfa_scratch_bytes(n, h, w, c) bytes (0 for a bad shape); the
 * call allocates nothing, runs four launches on `stream` and can be captured.
 * Rounding: t, the depthwise operand, hmap, the xx * g operand and the output
 * are rounded to 16 bits, the statistics are taken from the stored xx; every
 * sum is fp32 in a fixed order, so a crop's output does not depend on n.
 * FAC_ERR_ARG: a null (x, wpk, out, scratch) or misaligned (16 bytes) pointer,
 * n <= 0, a bad dtype; FAC_ERR_SHAPE: h or w outside 8..15, c no multiple of
 * 64 or above 256. */
size_t fac_smfa_scratch_bytes(int n, int h, int w, int c);
size_t fac_smfa_packed_bytes(int c);
int fac_smfa_pack(int dtype, int c, const float* w0, const float* b0, const float* gate4, const float* w1,
                  const float* b1, const float* dww, const float* dwb, const float* wpw, const float* bpw,
                  const float* wcat, const float* bcat, void* out);
int fac_smfa(int dtype, const void* x, int n, int h, int w, int c, const void* wpk, int residual, void* out,
             float* gate_out, void* scratch, void* stream);

/* BFM(x, x) of CViT-main/model/other/cvit_GGCA4_BFM5.py:162-272 (bfm.hip) on
 * a 16-bit channels-last map x [n][h][w][c] -> out [n][h][w][c]:
 *   out = scale * (ReLU(conv3(x) + b3) + ReLU(conv5(x) + b5) + ReLU(conv7(x) + b7))
 * three c -> c convs (3x3, 5x5, 7x7, zero padding 1, 2, 3), each ReLU'd before
 * the sum; with both inputs the same tensor the reference's TFAM fusion is
 * exactly scale = 4, whatever its weights.  One launch: one implicit GEMM over
 * the 7x7 window whose shifted input fragments feed the one, two or three
 * convs that have a tap at that offset, three fp32 accumulator sets, one
 * rounding to 16 bits at the store.  fac_bfm_pack (host pointers) takes the
 * reference's fp32 weights w3 [c][c][3][3], w5 [c][c][5][5], w7 [c][c][7][7]
 * and writes fac_bfm_packed_elems(c) = 83 c c 16-bit elements (0 for a bad c);
 * wpk is that array in device memory, bias3 fp32 [3][c] = b3, b5, b7 on the
 * device.  Every sum is fp32 in a fixed order and nothing is allocated, so a
 * crop's output does not depend on n and the call can be captured.
 * FAC_ERR_ARG: a null (x, wpk, bias3, out) or misaligned (16 bytes) pointer,
 * n <= 0, a bad dtype, out overlapping x (the kernel reads halos);
 * FAC_ERR_SHAPE: h or w outside 7..14, c not one of 64, 128, 256, 512. */
size_t fac_bfm_packed_elems(int c);
int fac_bfm_pack(int dtype, int c, const float* w3, const float* w5, const float* w7, uint16_t* out);
int fac_bfm(int dtype, const void* x, int n, int h, int w, int c, const void* wpk, const float* bias3, float scale,
            void* out, void* stream);

/* MDFA(c, c) of CViT-main/model/other/cvit_GGCA4_MDFA5.py:158-261 (mdfa.hip)
 * on a 16-bit channels-last map x [n][h][w][c] -> out [n][h][w][c]: a 1x1 and
 * three 3x3 conv branches with padding = dilation = 6, 12, 18, each with its
 * eval BatchNorm folded and a ReLU; a fifth branch g = ReLU(W5 mean_p x + b5)
 * per crop; cat = [b1 b2 b3 b4 g]; m_p = max(ReLU(w_t . mean_p cat),
 * sigmoid(w_s . cat_p)); out = ReLU(m_p (Wcat . cat_p^2) + bcat).  That is the
 * reference's max(tongdao(cat), kongjian(cat)) * cat through conv_cat, exactly,
 * because cat >= 0.  Taps that lie outside an h x w map for every pixel are
 * dropped when the launch is planned.
 * fac_mdfa_pack (host pointers, fp32 in, BatchNorm already folded) takes w1
 * [c][c], w2 w3 w4 [c][c][3][3] (dilation 6, 12, 18), bias4 [4][c], w5 [c][c],
 * b5 [c], wcat [c][5c], bcat [c], ws [5c] (kongjian), wt [5c] (tongdao) and
 * writes fac_mdfa_packed_bytes(c) bytes (0 for a bad c): w1..w4 and
 * wcat[:, :4c] become 16-bit MFMA operands, the rest stays fp32.  packed is
 * that blob in device memory.  scratch: fac_mdfa_scratch_bytes(n, h, w, c)
 * bytes (0 for a bad shape); the call allocates nothing, runs four launches on
 * `stream` and can be captured.
 * Rounding: the 16-bit input and weights; the branch sums, bias, ReLU, both
 * dots, the crop means, g, its share of conv_cat, the sigmoid and m_p are fp32
 * in a fixed order without atomics, so a crop's output does not depend on n;
 * cat^2 is rounded once to 16 bits as the conv_cat operand (fp16: clamped to
 * 65504, so no inf or NaN is produced); the output is rounded once.
 * FAC_ERR_ARG: a null (x, packed, out, scratch) or misaligned (16 bytes)
 * pointer, n <= 0, a bad dtype, out overlapping x; FAC_ERR_SHAPE: h or w
 * outside 7..14, c not one of 64, 128, 256, 512. */
size_t fac_mdfa_packed_bytes(int c);
size_t fac_mdfa_scratch_bytes(int n, int h, int w, int c);
int fac_mdfa_pack(int dtype, int c, const float* w1, const float* w2, const float* w3, const float* w4,
                  const float* bias4, const float* w5, const float* b5, const float* wcat, const float* bcat,
                  const float* ws, const float* wt, void* out);
int fac_mdfa(int dtype, const void* x, int n, int h, int w, int c, const void* packed, void* out, void* scratch,
             void* stream);

/* ScConv(c) -> affine(scale, shift) -> ReLU -> optional 2x2 max-pool of
 * CViT-main/model/other/cvit_GGCA_ADD_ScConv.py:311-353 (scconv.hip) on a 16-bit
 * channels-last map x [n][h][w][c] -> out [n][h][w][c], pooled [n][h/2][w/2][c]:
 * GroupNorm(4, c) statistics per crop, the hard gate that moves channels between
 * the two halves, the two 1x1 squeezes, GWC (3x3, 2 groups, bias) + PWC1 and
 * [PWC2; identity], and the softmax over the 2c per-crop channel means that
 * rescales both, the means taken from the linear sums of the squeezed map.
 * fac_scconv_pack (host pointers, fp32 in) takes gamma, beta [c] (the
 * GroupNorm's), kc [c] = gamma / sum(gamma), squeeze1, squeeze2 [c/4][c/2], gwc_w
 * [c][c/8][3][3], gwc_b [c], pwc1 [c][c/4], pwc2 [3c/4][c/4], scale, shift [c]
 * (the BatchNorm that follows, folded) and writes fac_scconv_packed_bytes(c)
 * bytes (0 for a bad c): the five conv weights become 16-bit MFMA operands, the
 * rest stays fp32.  packed is that blob in device memory.  scratch:
 * fac_scconv_scratch_bytes(n, h, w, c) bytes (0 for a bad shape); the call
 * allocates nothing, runs six launches on `stream` and can be captured.
 * stats_out: null, or device fp32 [n][4][2] that receives (mu_g, 1 / sqrt(var_g +
 * 1e-5)), the values the gate used.
 * Rounding to 16 bits: the input and the conv weights; the gated map as the
 * squeeze's operand; the squeezed map [u | l] at its store; the output.  All
 * sums are fp32 in a fixed order that depends on (h, w, c) alone, no atomics: a
 * crop's bits do not depend on n.  The gate is z > 0.
 * FAC_ERR_ARG: a null (x, packed, out, scratch) or misaligned (16 bytes)
 * pointer, n <= 0, a bad dtype or pool, out overlapping x; FAC_ERR_SHAPE: c not
 * one of 64, 128, 256, h or w outside 2..224 or odd with pool, n above 65535. */
size_t fac_scconv_packed_bytes(int c);
size_t fac_scconv_scratch_bytes(int n, int h, int w, int c);
int fac_scconv_pack(int dtype, int c, const float* gamma, const float* beta, const float* kc, const float* squeeze1,
                    const float* squeeze2, const float* gwc_w, const float* gwc_b, const float* pwc1,
                    const float* pwc2, const float* scale, const float* shift, void* out);
int fac_scconv(int dtype, const void* x, int n, int h, int w, int c, const void* packed, int pool, void* out,
               float* stats_out, void* scratch, void* stream);

/* ODConv2d(c, c, 3, padding 1) -> affine(scale, shift) -> optional ReLU ->
 * optional 2x2 max-pool of CViT-main/model/other/cvit_GGCA_ADD_ODConv.py:158-292
 * (odconv.hip; kernel_num 4, attention width 16, temperature 1, no conv bias) on
 * a 16-bit channels-last map x [n][h][w][c] -> out [n][h][w][c], pooled
 * [n][h/2][w/2][c].  Per crop: p = the channel means, hid = ReLU(bn_scale (fc p)
 * + bn_shift), ca = sigmoid(channel_fc hid + channel_b), fa = sigmoid(filter_fc
 * hid + filter_b), sa = sigmoid(spatial_fc hid + spatial_b), ka =
 * softmax(kernel_fc hid + kernel_b), and
 *   out[o] = act(fa[o] sum_tap sa[tap] sum_i (sum_k ka[k] W[k][o][i][tap]) ca[i] x[i, tap] * scale[o] + shift[o]):
 * the conv weights differ per crop.
 * fac_odconv_pack (host pointers, fp32 in) takes W [4][c][c][3][3], fc [16][c],
 * bn_scale, bn_shift [16] (the attention's BatchNorm, folded), channel_fc
 * [c][16], channel_b [c], filter_fc [c][16], filter_b [c], spatial_fc [9][16],
 * spatial_b [9], kernel_fc [4][16], kernel_b [4], scale, shift [c] (the BatchNorm
 * that follows, folded; 1 and 0 for a bare block) and writes
 * fac_odconv_packed_bytes(c) bytes (0 for a bad c); everything stays fp32 in
 * the blob, which is the same for both dtypes.  packed is that blob in device
 * memory.  scratch: fac_odconv_scratch_bytes(n, h, w, c) bytes (0 for a bad
 * shape), at most 48 MiB of aggregated weights plus n (ceil(h w / 512) c + 2 c +
 * 16) floats.  The call allocates nothing, runs 2 + 2 ceil(n / k) launches on
 * `stream` (k = the crops whose aggregated weights fit the 48 MiB: 682, 170, 42
 * for c = 64, 128, 256; fac_odconv_chunk(n, c) gives min(n, k), 0 for a bad n or
 * c) and can be captured.
 * relu: 1 ReLU, 0 identity.  att_out: null, or device fp32 [n][2c + 13] that
 * receives ca | fa | sa | ka as the conv used them.
 * Rounding to 16 bits: the input; the aggregated per-crop weight sa[tap] ca[i]
 * sum_k ka[k] W_k, once (the W_k themselves are never rounded); the output.  The
 * means, hid, the four attentions, fa, scale, shift, the aggregation and all
 * accumulation are fp32, every sum in a fixed order that depends on (h, w, c)
 * alone, no atomics: a crop's bits do not depend on n or on its position.
 * FAC_ERR_ARG: a null (x, packed, out, scratch) or misaligned (16 bytes; att_out
 * 4) pointer, n <= 0, a bad dtype, relu or pool, out overlapping x;
 * FAC_ERR_SHAPE: c not one of 64, 128, 256, h or w outside 2..224 or odd with
 * pool, n above 65535. */
size_t fac_odconv_packed_bytes(int c);
size_t fac_odconv_scratch_bytes(int n, int h, int w, int c);
int fac_odconv_chunk(int n, int c);
int fac_odconv_pack(int dtype, int c, const float* weight, const float* fc, const float* bn_scale, const float* bn_shift,
                    const float* channel_fc, const float* channel_b, const float* filter_fc, const float* filter_b,
                    const float* spatial_fc, const float* spatial_b, const float* kernel_fc, const float* kernel_b,
                    const float* scale, const float* shift, void* out);
int fac_odconv(int dtype, const void* x, int n, int h, int w, int c, const void* packed, int relu, int pool, void* out,
               float* att_out, void* scratch, void* stream);

/* Row-wise sigmoid of logits (the per-logit pred_sig of the heads). */
int fac_sigmoid(const float* x, float* y, int n, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FAC_OPS_H */
