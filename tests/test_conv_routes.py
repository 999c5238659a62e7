"""Which kernel family fac_conv_nd / fac_conv_nd_split / fac_conv_nd_dual /
fac_pool_nd pick for a descriptor, pinned without a GPU through
fac_conv_nd_route / fac_conv_nd_dual_route / fac_pool_nd_route (they walk the
dispatchers' own route tables and launch nothing).

The expected names were read off the dispatchers as they stood before the
route tables (csrc/ops.hip at commit d847aa6): the number beside each row is
the line of the branch that decides it there.  A GPU test cannot see a wrong
route: a descriptor that falls through to convnd_igemm still computes the
right values, only slower.
"""
import ctypes as C

import pytest

from fac_fake_amd import _lib
from fac_fake_amd.ops import (MAXPOOL3S1, MAXPOOL3S2, OUT_F32, PREPOOL3S2, RELU, RELU2, RESID, ConvDesc, PoolDesc)

INT_MAX = 2 ** 31 - 1
ARG, SHAPE = -1, -2
PTR = 64            # a dummy non-NULL pointer: the queries only test pointers for NULL
BNECK = RELU | RESID | RELU2
IG_OCC3, IG_SMALL, IG_BIG, IG = ("convnd_igemm:128x64:3", "convnd_igemm:64x64:3", "convnd_igemm:256x128:1",
                                "convnd_igemm:128x64:2")


@pytest.fixture(scope="module")
def lib(built_lib):
    return _lib.load()


def conv(cin, cout, dhw, k=(1, 1, 1), s=(1, 1, 1), p=(0, 0, 0), *, n=2, flags=RELU, ldo=None, c_off=0, ldr=None,
         r_off=0, **over):
    d = ConvDesc()
    d.dtype, d.inp, d.weight, d.bias, d.out = 0, PTR, PTR, PTR, PTR
    d.n, (d.d, d.h, d.w), d.cin, d.cout = n, dhw, cin, cout
    (d.kd, d.kh, d.kw), (d.sd, d.sh, d.sw), (d.pd, d.ph, d.pw) = k, s, p
    d.od, d.oh, d.ow = [(i + 2 * pp - kk) // ss + 1 for i, kk, ss, pp in zip(dhw, k, s, p)]
    d.k_pad = (k[0] * k[1] * k[2] * cin + 63) // 64 * 64
    d.ldo, d.c_off, d.flags = cout if ldo is None else ldo, c_off, flags
    if flags & RESID:
        d.residual, d.ldr, d.r_off = PTR, cout if ldr is None else ldr, r_off
    for key, v in over.items():
        setattr(d, key, v)
    return d


def pool(c, dhw, k, s, p, *, mode=0, n=2, ldo=None, c_off=0, **over):
    d = PoolDesc()
    d.dtype, d.inp, d.out, d.mode = 0, PTR, PTR, mode
    d.n, (d.d, d.h, d.w), d.c = n, dhw, c
    (d.kd, d.kh, d.kw), (d.sd, d.sh, d.sw), (d.pd, d.ph, d.pw) = k, s, p
    d.od, d.oh, d.ow = [(i + 2 * pp - kk) // ss + 1 for i, kk, ss, pp in zip(dhw, k, s, p)]
    d.ldo, d.c_off = c if ldo is None else ldo, c_off
    for key, v in over.items():
        setattr(d, key, v)
    return d


def conv_route(lib, d, split=(INT_MAX, INT_MAX)):
    st = C.c_int(99)
    name = lib.fac_conv_nd_route(C.byref(d) if d is not None else None, split[0], split[1], C.byref(st))
    return (name.decode() if name else None), st.value


def dual_route(lib, d, ds):
    st = C.c_int(99)
    name = lib.fac_conv_nd_dual_route(C.byref(d), C.byref(ds), C.byref(st))
    return (name.decode() if name else None), st.value


def pool_route(lib, d):
    st = C.c_int(99)
    name = lib.fac_pool_nd_route(C.byref(d) if d is not None else None, C.byref(st))
    return (name.decode() if name else None), st.value


# the models' layers ------------------------------------------------------
def s2d4(flags=RELU, side=115, **kw):          # the 16 -> 64 4x4 space-to-depth first conv (112 x 112 out)
    return conv(16, 64, (1, side, side), (1, 4, 4), n=4, flags=flags, **kw)


def base2(**kw):                                # S3D base.1 + base.2 at 56-wide
    kw.setdefault("flags", RELU | PREPOOL3S2)
    return conv(64, 64, (8, 56, 56), oh=28, ow=28, **kw)


def branch3(cin, cout, d, side, **kw):          # Mixed_* branch3: MaxPool3d(3,1,1) + 1x1x1
    kw.setdefault("flags", RELU | MAXPOOL3S1)
    return conv(cin, cout, (d, side, side), **kw)


def temporal(cin, cout, side=14, d=8, **kw):    # SepConv3d's (3,1,1) half
    return conv(cin, cout, (d, side, side), (3, 1, 1), p=(1, 0, 0), **kw)


def conv3(k, side, cout=None, **kw):            # a ResNet-50 bottleneck's conv3 + identity at K = k
    kw.setdefault("flags", BNECK)
    return conv(k, cout or 4 * k, (1, side, side), n=4, **kw)


def heads(cin, cout, **kw):                     # an Inception block's three merged 1x1x1 heads at 14 x 14
    return conv(cin, cout, (8, 14, 14), ldo=256, **kw)


CONV_ROWS = [
    # ---- every route once, on the models' own layers
    ("S3D base.2 at 56-wide", base2(), None, "maxpool2s_pw"),                                      # 4142
    ("ResNet conv1 + maxpool", s2d4(RELU | MAXPOOL3S2), None, "conv_s2d4_mp"),                     # 4231
    ("Mixed_3b branch3 at 14", branch3(192, 32, 8, 14, ldo=256, c_off=224), None, "maxpool3_pw"),  # 4245
    ("Mixed_4b branch3 at 7", branch3(480, 64, 4, 7, ldo=512, c_off=448), None, "maxpool3_pw"),    # 4245
    ("Mixed_5b branch3 at 3", branch3(832, 128, 2, 3, ldo=832, c_off=704), None, "maxpool3_pw"),   # 4245
    ("ResNet conv1 alone", s2d4(), None, "conv_s2d4"),                                             # 4292
    ("S3D base.0 spatial half", conv(16, 64, (16, 59, 59), (1, 4, 4)), None, "conv_s2d4"),         # 4292
    ("Mixed_3b heads, K 192", heads(192, 176), (64, 160), "pw_res"),                               # 4307
    ("Mixed_3c heads, K 256", heads(256, 288), (128, 256), "pw_res"),                              # 4307
    ("layer2 conv3 + identity", conv3(128, 28), None, "pw_res"),                                   # 4332
    ("layer3 conv3 + identity", conv3(256, 14), None, "pw_res"),                                   # 4332
    ("layer4 conv3 + identity", conv3(512, 7), None, "pw_res2"),                                   # 4361
    ("layer1 conv3 + identity", conv3(64, 56), None, "conv_pw"),                                   # 4380
    ("S3D base.2 alone", conv(64, 64, (8, 28, 28)), None, "conv_pw"),                              # 4380
    ("1x1 256 -> 64", conv(256, 64, (1, 56, 56)), None, "conv_pw"),                                # 4380
    ("(3,1,1) at cin 64", temporal(64, 64, 28), None, "conv_tk2"),                                 # 4433
    ("(3,1,1) at cin 128", temporal(128, 128), None, "conv_tk2"),                                  # 4433
    ("(3,1,1) at cin 192", temporal(192, 192, 28), None, "conv_tk2"),                              # 4433
    ("base.0's (7,1,1)/2", conv(64, 64, (16, 56, 56), (7, 1, 1), (2, 1, 1), (3, 0, 0)), None, "conv_tk2"),  # 4433
    ("(3,1,1) at cin 256", temporal(256, 256, 7), None, "conv_tk"),                                # 4472
    ("layer3 conv2, 3x3/2", conv(256, 256, (1, 28, 28), (1, 3, 3), (1, 2, 2), (0, 1, 1), n=4), None, "convnd_pt"),  # 4085
    ("7x7/2 first conv, unpacked", conv(8, 64, (1, 224, 224), (1, 7, 7), (1, 2, 2), (0, 3, 3), n=8), None, IG),  # 4107
    # ---- the nearest descriptor that must not take a route
    # conv_pw: cin 128 / 256 with cout % 128 == 0 is convnd_pt's (4379)
    ("1x1 128 -> 128", conv(128, 128, (1, 28, 28)), None, "convnd_pt"),                            # 4379, 4085
    ("1x1 256 -> 128", conv(256, 128, (1, 56, 56)), None, "convnd_pt"),                            # 4379, 4085
    # conv_pw: c_off / cout / fp32 output / residual stride; one K step is not convnd_pt's either (4054)
    ("conv_pw shape, c_off 4", conv(64, 64, (1, 56, 56), ldo=72, c_off=4), None, IG_OCC3),         # 4383, 4090
    # (over 8 frames such a 1x1x1 conv passes conv_tk's test, which asks for c_off % 4 only)
    ("conv_pw shape, c_off 4, 8 frames", conv(64, 64, (8, 28, 28), ldo=72, c_off=4), None, "conv_tk"),  # 4383, 4422, 4472
    ("conv_pw shape, cout 96", conv(64, 96, (8, 28, 28)), None, IG_OCC3),                          # 4383, 4090
    ("conv_pw shape, fp32 out", conv(64, 64, (8, 28, 28), flags=RELU | OUT_F32), None, IG_OCC3),   # 4383, 4090
    ("layer1 conv3, ldr 260", conv3(64, 56, ldr=260), None, IG_OCC3),                              # 4384, 4090
    # pw_res: residual stride, c_off; K 128 is two K steps: the 3-per-CU tile (4090)
    ("layer2 conv3, ldr 516", conv3(128, 28, ldr=516), None, IG_OCC3),                             # 4336, 4055, 4090
    ("layer2 conv3, c_off 4", conv3(128, 28, ldo=520, c_off=4), None, IG_OCC3),                    # 4336, 4054, 4090
    ("layer3 conv3, ldr 1028", conv3(256, 14, ldr=1028), None, IG_SMALL),                          # 4336, 4055, 4095
    ("layer2 conv3, cout 384", conv3(128, 28, cout=384), None, "convnd_pt"),                       # 4335, 4379, 4085
    ("layer4 conv3, cout 1920", conv3(512, 7, cout=1920), None, "convnd_pt"),                      # 4364, 4085
    ("layer4 conv3, r_off 4", conv3(512, 7, ldr=2056, r_off=4), None, IG_SMALL),                   # 4364, 4055, 4095
    # pw_res split heads: K 128 is not in its set, a split that is no multiple of 8 is rejected before
    ("heads at K 128", heads(128, 176), (64, 160), IG_OCC3),                                       # 4309, 4062, 4090
    ("heads at K 192, few rows", heads(192, 176, flags=0), (64, 160), "pw_res"),                   # 4307
    # conv_tk2 / conv_tk: od, cout, flags, cin
    ("(3,1,1) over 4 frames", temporal(128, 128, 7, d=4), None, "convnd_pt"),                      # 4422, 4085
    ("(3,1,1) 64 -> 96", temporal(64, 96), None, IG_SMALL),                                        # 4423, 4062, 4095
    ("(3,1,1) fp32 out", temporal(64, 64, flags=RELU | OUT_F32), None, IG_OCC3),                   # 4425, 4055, 4090
    ("(3,1,1) at cin 320", temporal(320, 64, 7), None, IG_SMALL),                                  # 4427 (db 0), 4062, 4095
    ("(5,1,1) at cin 64", conv(64, 64, (8, 14, 14), (5, 1, 1), p=(2, 0, 0)), None, "conv_tk"),     # 4433, 4472
    # conv_s2d4: its 8 x 28 boxes, a dense output
    ("4x4 conv, 104 wide", s2d4(side=107), None, IG_OCC3),                                         # 4222, 4090
    ("4x4 conv into a slot", s2d4(ldo=128), None, IG_OCC3),                                        # 4222, 4090
    # convnd_pt with a partial column block: from 32 row tiles of 256 on (4062)
    ("3x3 64 -> 192, 32 row tiles", conv(64, 192, (1, 64, 64), (1, 3, 3), p=(0, 1, 1)), None, "convnd_pt"),  # 4062
    ("3x3 64 -> 192, 31 row tiles", conv(64, 192, (1, 64, 124), (1, 3, 3), p=(0, 1, 1), n=1), None, IG_SMALL),  # 4062, 4095
    # convnd_igemm's tiles
    ("one K step", conv(8, 64, (8, 28, 28)), None, IG_OCC3),                                       # 4090
    ("two K steps", conv(128, 64, (8, 28, 28), flags=RELU | OUT_F32), None, IG_OCC3),              # 4090
    ("cout 64, three K steps", conv(16, 64, (1, 56, 56), (1, 3, 3), p=(0, 1, 1), n=16), None, IG_OCC3),  # 4090 (nd_occ3)
    ("cout 128, three K steps, 4 tiles", conv(16, 128, (1, 14, 14), (1, 3, 3), p=(0, 1, 1), n=1), None, IG_SMALL),  # 4095
    ("3x3 64 -> 512 fp32, 392 big tiles", conv(64, 512, (1, 56, 56), (1, 3, 3), p=(0, 1, 1), n=8,
                                               flags=RELU | OUT_F32), None, IG_BIG),               # 4055, 4099
    ("3x3 64 -> 128 fp32, 147 big tiles", conv(64, 128, (1, 56, 56), (1, 3, 3), p=(0, 1, 1), n=12,
                                               flags=RELU | OUT_F32), None, IG),                   # 4099, 4107
    ("3x3 16 -> 96", conv(16, 96, (1, 56, 56), (1, 3, 3), p=(0, 1, 1), n=16), None, IG),           # 4107
]


@pytest.mark.parametrize("what,d,split,want", CONV_ROWS, ids=[r[0] for r in CONV_ROWS])
def test_conv_route(lib, what, d, split, want):
    assert conv_route(lib, d, split or (INT_MAX, INT_MAX)) == (want, 0)


CONV_REJECTS = [
    ("null descriptor", None, None, ARG),                                                          # 4137
    ("null weight", s2d4(weight=None), None, ARG),                                                 # 4137
    ("dtype 2", conv3(128, 28, dtype=2), None, ARG),                                               # 4138
    ("cin 12", conv(12, 64, (1, 8, 8)), None, SHAPE),                                              # 4139
    # a flag route whose shape test fails does not fall through
    ("prepool on a 28-wide map", conv(64, 64, (8, 28, 28), flags=RELU | PREPOOL3S2, oh=14, ow=14), None, ARG),  # 4143
    ("prepool with relu2", base2(flags=RELU | RELU2 | PREPOOL3S2), None, ARG),                     # 4143
    ("prepool, c_off 4", base2(ldo=72, c_off=4), None, ARG),                                       # 4146
    ("conv + maxpool on a 1x1 conv", conv(64, 64, (1, 56, 56), flags=RELU | MAXPOOL3S2), None, ARG),  # 4232
    ("conv + maxpool without relu", s2d4(MAXPOOL3S2), None, ARG),                                  # 4232
    ("pool + 1x1 on a 28-wide map", branch3(192, 32, 8, 28), None, ARG),                           # 4249
    ("pool + 1x1, cout 48", branch3(192, 48, 8, 14), None, ARG),                                   # 4249
    ("pool + 1x1, c_off 4", branch3(192, 32, 8, 14, ldo=40, c_off=4), None, ARG),                  # 4249
    ("pool + 1x1 on split heads", branch3(192, 176, 8, 14, ldo=256), (64, 160), ARG),              # 4247
    # the general validation
    ("k_pad one step short", temporal(64, 64, k_pad=128), None, SHAPE),                            # 4172
    ("k_pad of another layout", conv(16, 64, (1, 14, 14), (1, 3, 3), p=(0, 1, 1), k_pad=144), None, SHAPE),  # 4172
    ("ceil-mode output dims", conv(64, 64, (1, 15, 15), s=(1, 2, 2), oh=9, ow=9), None, SHAPE),    # 4167
    ("output one row short", conv(64, 64, (1, 14, 14), (1, 3, 3), p=(0, 1, 1), oh=13), None, SHAPE),  # 4167
    ("ldo below c_off + cout", conv(64, 64, (8, 28, 28), ldo=96, c_off=64), None, SHAPE),          # 4173
    ("residual narrower than cout", conv3(128, 28, ldr=256), None, ARG),                           # 4174
    ("residual flag, no pointer", conv3(128, 28, residual=None), None, ARG),                       # 4174
    ("2^31 output positions", conv(8, 8, (2048, 1024, 1024), n=1), None, SHAPE),                   # 4176
    # fac_conv_nd_split's own argument checks
    ("split not a multiple of 8", heads(192, 176), (60, 160), ARG),                                # 4666
    ("split past cout", heads(192, 176), (64, 176), ARG),                                          # 4666
    ("split with a residual", heads(192, 176, flags=BNECK), (64, 160), ARG),                       # 4667
]


@pytest.mark.parametrize("what,d,split,want", CONV_REJECTS, ids=[r[0] for r in CONV_REJECTS])
def test_conv_route_rejects(lib, what, d, split, want):
    assert conv_route(lib, d, split or (INT_MAX, INT_MAX)) == (None, want)


def down(cin, cout, side, s):                   # a bottleneck's downsample conv over the block input
    return conv(cin, cout, (1, side, side), s=(1, s, s), n=4, flags=0)


def dual3(k, side, cout=None):                  # ... and its conv3 (+ ReLU, + ReLU after the sum)
    return conv3(k, side, cout, flags=RELU | RELU2)


DUAL_ROWS = [
    ("layer1 block 0", dual3(64, 56), down(64, 256, 56, 1), "pw_res", 0),                          # 4736
    ("layer2 block 0", dual3(128, 28), down(256, 512, 56, 2), "pw_dual2", 0),                      # 4753
    ("layer3 block 0", dual3(256, 14), down(512, 1024, 28, 2), "pw_dual2", 0),                     # 4753
    ("layer4 block 0", dual3(512, 7), down(1024, 2048, 14, 2), "convnd_pt", 0),                    # 4780
    # near misses
    ("layer1 pair, cout 128", dual3(64, 56, 128), down(64, 128, 56, 1), "convnd_pt", 0),           # 4736, 4780
    ("layer1 pair, strided downsample", dual3(64, 28), down(64, 256, 56, 2), "convnd_pt", 0),      # 4737, 4780
    ("layer2 pair, cout 384", dual3(128, 28, 384), down(256, 384, 56, 2), "convnd_pt", 0),         # 4753, 4780
    ("layer2 pair, downsample K 512", dual3(128, 28), down(512, 512, 56, 2), "convnd_pt", 0),      # 4753, 4780
    # rejected
    ("cout 192", dual3(64, 56, 192), down(64, 192, 56, 1), None, SHAPE),                           # 4729
    ("cin 32", dual3(32, 56, 256), down(64, 256, 56, 1), None, SHAPE),                             # 4677
    ("other output positions", dual3(128, 28), down(256, 512, 56, 1), None, SHAPE),                # 4728
    ("a residual flag", conv3(128, 28), down(256, 512, 56, 2), None, ARG),                         # 4725
    ("flags on the downsample", dual3(128, 28), conv(256, 512, (1, 56, 56), s=(1, 2, 2), n=4), None, ARG),  # 4725
]


@pytest.mark.parametrize("what,d,ds,want,status", DUAL_ROWS, ids=[r[0] for r in DUAL_ROWS])
def test_dual_route(lib, what, d, ds, want, status):
    assert dual_route(lib, d, ds) == (want, status)


def maxpool3(c, d, side, **kw):                 # S3D's MaxPool3d(3, 1, 1)
    return pool(c, (d, side, side), (3, 3, 3), (1, 1, 1), (1, 1, 1), **kw)


POOL_ROWS = [
    ("Mixed_3b branch3 pool", maxpool3(192, 8, 14), "maxpool3_lds14", 0),                          # 4853
    ("Mixed_4b branch3 pool", maxpool3(480, 4, 7), "maxpool3_roll", 0),                            # 4862
    ("Mixed_5b branch3 pool", maxpool3(832, 2, 3), "maxpool3_s1", 0),                              # 4873
    ("S3D base.1, (1,3,3)/(1,2,2)", pool(64, (8, 56, 56), (1, 3, 3), (1, 2, 2), (0, 1, 1)), "pool_max_win", 0),  # 4899
    ("S3D maxpool 3a, (3,3,3)/2", pool(192, (8, 28, 28), (3, 3, 3), (2, 2, 2), (1, 1, 1)), "pool_max_win", 0),   # 4900
    ("S3D maxpool 5a, (2,2,2)/2", pool(832, (4, 7, 7), (2, 2, 2), (2, 2, 2), (0, 0, 0)), "pool_max_win", 0),     # 4901
    ("S3D's average pool", pool(1024, (2, 3, 3), (2, 3, 3), (1, 1, 1), (0, 0, 0), mode=1), "pool_nd", 0),        # 4904
    # near misses
    ("3x3x3 pool at 14, 72 channels", maxpool3(72, 8, 14), "maxpool3_s1", 0),                      # 4853, 4873
    ("3x3x3 pool at 14 x 7", pool(192, (8, 14, 7), (3, 3, 3), (1, 1, 1), (1, 1, 1)), "maxpool3_roll", 0),  # 4853, 4862
    ("3x3x3 pool at 28", maxpool3(64, 8, 28), "maxpool3_s1", 0),                                   # 4873
    ("3x3x3 average at 14", maxpool3(192, 8, 14, mode=1), "pool_nd", 0),                           # 4851, 4891
    ("(1,2,2) window", pool(64, (8, 56, 56), (1, 2, 2), (1, 2, 2), (0, 0, 0)), "pool_nd", 0),      # 4899-4901
    ("ceil-mode (1,3,3)/(1,2,2)", pool(64, (8, 56, 56), (1, 3, 3), (1, 2, 2), (0, 0, 0), oh=28, ow=28), "pool_nd", 0),  # 4887
    # rejected
    ("null descriptor", None, None, ARG),                                                          # 4842
    ("null output", maxpool3(192, 8, 14, out=None), None, ARG),                                    # 4842
    ("12 channels", maxpool3(12, 8, 14), None, SHAPE),                                             # 4844
    ("mode 2", maxpool3(192, 8, 14, mode=2), None, SHAPE),                                         # 4844
    ("ldo below c_off + c", maxpool3(192, 8, 14, ldo=256, c_off=128), None, SHAPE),                # 4847
    ("c_off 4", maxpool3(192, 8, 14, ldo=256, c_off=4), None, SHAPE),                              # 4847
]


@pytest.mark.parametrize("what,d,want,status", POOL_ROWS, ids=[r[0] for r in POOL_ROWS])
def test_pool_route(lib, what, d, want, status):
    assert pool_route(lib, d) == (want, status)


@pytest.fixture
def knob(lib):
    """Sets a process-wide A/B knob and puts its default back afterwards.
    fac_set_option needs a context, so a device; the knobs it sets are the
    plain C++ setters of csrc/ops_common.hpp (fac::set_<name>(int)), called
    here by their mangled names."""
    defaults = {"pw_res": 1, "pool_roll": 1, "pool_lds14": 1, "pool_win": 1, "nd_pt_wide": 32, "nd_occ3": 4}
    touched = set()

    def setter(name, value):
        fn = getattr(lib, f"_ZN3fac{len(name) + 4}set_{name}Ei")
        fn.argtypes, fn.restype = [C.c_int], None
        fn(value)

    def set_(name, value):
        touched.add(name)
        setter(name, value)

    yield set_
    for name in touched:
        setter(name, defaults[name])


def test_knob_pw_res(lib, knob):
    """"pw_res" 0: pw_res, pw_res2 and pw_dual2 all off; 2: only pw_res2 and pw_dual2 off."""
    l1 = (dual3(64, 56), down(64, 256, 56, 1))
    l2 = (dual3(128, 28), down(256, 512, 56, 2))

    def routes():
        return [conv_route(lib, conv3(128, 28))[0], conv_route(lib, conv3(256, 14))[0],
                conv_route(lib, heads(192, 176), (64, 160))[0], conv_route(lib, conv3(512, 7))[0],
                dual_route(lib, *l1)[0], dual_route(lib, *l2)[0],
                conv_route(lib, conv3(64, 56))[0]]

    on = ["pw_res", "pw_res", "pw_res", "pw_res2", "pw_res", "pw_dual2", "conv_pw"]
    assert routes() == on
    knob("pw_res", 0)   # 4307, 4332, 4361, 4736, 4753 all fail; the split heads' 13 row tiles stay off convnd_pt (4062)
    assert routes() == ["convnd_pt", "convnd_pt", IG_SMALL, "convnd_pt", "convnd_pt", "convnd_pt", "conv_pw"]
    knob("pw_res", 2)   # 4361 and 4753 test == 1
    assert routes() == ["pw_res", "pw_res", "pw_res", "convnd_pt", "pw_res", "convnd_pt", "conv_pw"]
    knob("pw_res", 1)
    assert routes() == on


def test_knobs_pool(lib, knob):
    """"pool_lds14" 0 / "pool_roll" 0 send their maps to maxpool3_s1 (4853,
    4862), "pool_win" 0 the compile-time windows to pool_nd (4891); each
    leaves the other routes alone."""
    rows = [maxpool3(192, 8, 14), maxpool3(480, 4, 7), maxpool3(832, 2, 3),
            pool(64, (8, 56, 56), (1, 3, 3), (1, 2, 2), (0, 1, 1)),
            pool(1024, (2, 3, 3), (2, 3, 3), (1, 1, 1), (0, 0, 0), mode=1)]

    def routes():
        return [pool_route(lib, d)[0] for d in rows]

    on = ["maxpool3_lds14", "maxpool3_roll", "maxpool3_s1", "pool_max_win", "pool_nd"]
    assert routes() == on
    knob("pool_lds14", 0)
    assert routes() == ["maxpool3_s1"] + on[1:]
    knob("pool_lds14", 1)
    knob("pool_roll", 0)
    assert routes() == [on[0], "maxpool3_s1"] + on[2:]
    knob("pool_roll", 2)   # two frames per thread: still maxpool3_roll
    assert routes() == on
    knob("pool_roll", 1)
    knob("pool_win", 0)
    assert routes() == on[:3] + ["pool_nd", "pool_nd"]
    knob("pool_win", 1)
    assert routes() == on


def test_knobs_generic_conv(lib, knob):
    """"nd_pt_wide" moves convnd_pt's threshold for a partial column block
    (4062), "nd_occ3" the 3-per-CU tile's K-step bound at cout <= 64 (4090)."""
    wide31 = conv(64, 192, (1, 64, 124), (1, 3, 3), p=(0, 1, 1), n=1)
    wide32 = conv(64, 192, (1, 64, 64), (1, 3, 3), p=(0, 1, 1))
    narrow = conv(16, 64, (1, 56, 56), (1, 3, 3), p=(0, 1, 1), n=32)      # three K steps, 784 tiles
    assert [conv_route(lib, d)[0] for d in (wide31, wide32, narrow)] == [IG_SMALL, "convnd_pt", IG_OCC3]
    knob("nd_pt_wide", 31)
    assert [conv_route(lib, d)[0] for d in (wide31, wide32)] == ["convnd_pt", "convnd_pt"]
    knob("nd_pt_wide", 0)
    assert [conv_route(lib, d)[0] for d in (wide31, wide32)] == [IG_SMALL, IG_SMALL]
    knob("nd_pt_wide", 32)
    knob("nd_occ3", 0)
    assert conv_route(lib, narrow)[0] == IG
    knob("nd_occ3", 4)
    assert [conv_route(lib, d)[0] for d in (wide31, wide32, narrow)] == [IG_SMALL, "convnd_pt", IG_OCC3]
