"""Drop-in ``CViT`` for the reference's inference path, running on gfx950 HIP kernels.

Interface parity with ``CViT-main/model/cvit.py``:

* constructor ``CViT(image_size=224, patch_size=7, num_classes=2, channels=512,
  dim=1024, depth=6, heads=8, mlp_dim=2048)`` (cvit.py:81-82);
* ``state_dict()`` / ``load_state_dict()`` with the same 193 keys, shapes and
  order (checkpoints written by ``cvit_train.py:210`` load unchanged);
* ``forward(img, mask=None)`` on normalised fp32 NCHW ``[B,3,224,224]``
  returning fp32 logits ``[B,2]`` (cvit.py:167-179), including the
  reference's batch-slot ``pos_embedding`` rule (crop j of a call gets
  ``pos_embedding[j]``, cvit.py:174-175) and its ``B > 32`` RuntimeError;
  ``mask`` follows the reference's semantics exactly (``reference_mask_poisons``).

The parameters live in a tree of plain containers purely to expose the
reference's state_dict; the arithmetic never runs through them.  On the first
forward after (re)loading, the state_dict is handed to ``fac_load_weights``
(BN folding + 16-bit repacking in C++), and every forward is one call into
``libfac_cvit.so`` on the current torch stream.  There is no CPU fallback:
a CPU tensor or a missing library raises.

Extensions beyond the reference: ``pos_index=`` (explicit slot per crop, for
sharded / chunked calls), ``forward_u8()`` taking raw uint8 NHWC face crops
with the normalisation fused into conv1, and ``dtype`` ("fp16" or "bf16": the
16-bit MFMA operand type; accumulation is fp32 either way).  The default is
"fp16", the parity-grade mode (per-frame probabilities within the north
star's 1e-3 of the fp32 reference) at the same MFMA rate;
"bf16" -- which bench.py selects for the bf16 throughput metric -- moves
them by up to 4.0e-3 on config 2's 256 golden crops (measured, BENCH_r04 and r05;
the oracle's emulated bf16 rounding alone gives 5.3e-3 there,
tests/golden/bf16_envelope.json) and is an explicit opt-in.
"""
from __future__ import annotations

import threading

import ctypes
import math

import torch
from torch import nn

from . import _lib
from .weights import cvit_param_specs

SUPPORTED = dict(image_size=224, patch_size=7, num_classes=2, channels=512, dim=1024, depth=6, heads=8,
                 mlp_dim=2048)
MAX_SLOTS = 32  # pos_embedding has 32 rows (cvit.py:154)
_BUFFER_KINDS = ("rmean", "rvar", "nbt")


def reference_mask_poisons(mask, B: int, heads: int = 8, n_tokens: int = 2) -> bool:
    """The reference's attention mask (cvit.py:50-55; the same code in every
    CViT variant), evaluated on the host for the [B, heads, 2, 2] score shape:
    ``F.pad(mask.flatten(1), (1, 0), value=True)``, its outer product, and
    ``dots.masked_fill_(~mask, -inf)``.  Raises what the reference raises (the
    AssertionError for a wrong width; the broadcast RuntimeError, since the
    [B,2,2] mask lines up with dots' [heads,2,2] dims: only B in {1, heads}
    works).  Returns True when some score is masked: its token's score row
    is then all -inf, softmax gives NaN, and through ``attn @ v`` (0 * NaN)
    every crop's logits become NaN (checked against the reference module);
    False (all positions kept) leaves the forward exactly as with no mask."""
    m = torch.as_tensor(mask).to("cpu")
    m = torch.nn.functional.pad(m.flatten(1), (1, 0), value=True)
    assert m.shape[-1] == n_tokens, "mask has incorrect dimensions"
    m = m[:, None, :] * m[:, :, None]
    dots = torch.zeros(B, heads, n_tokens, n_tokens)
    dots.masked_fill_(~m, float("-inf"))
    return bool(torch.isinf(dots).any())


_SLOTS: dict = {}


def weight_versions(module: nn.Module) -> tuple:
    """(version counter, data pointer) of every parameter and buffer of a
    drop-in's fixed container tree: the weights are re-uploaded when an
    in-place update or a swapped tensor changes this.  The (module, name)
    slots are listed once; walking them costs ~40-70 us per call, against
    ~0.5 ms for the state_dict() this replaced (it ran on every forward, the
    reference's one-video call included).  The cached slots are rebuilt when
    the module tree changed since they were listed (a submodule replaced,
    added or removed, e.g. ``m.mlp_head[2] = nn.Linear(...)``): each module's
    children are compared by identity, ~10 us."""
    cache = module.__dict__.get("_wv_slots")
    if cache is not None:
        for kids, seen in cache[0]:
            if len(kids) != len(seen) or any(a is not b for a, b in zip(kids.values(), seen)):
                cache = None
                break
    if cache is None:
        mods = [m for _, m in module.named_modules()]
        tree = [(m._modules, tuple(m._modules.values())) for m in mods]
        slots = [(m._parameters, k) for m in mods for k in m._parameters] + \
                [(m._buffers, k) for m in mods for k in m._buffers]
        cache = module.__dict__["_wv_slots"] = (tree, slots)
    slots = cache[1]
    out = []
    for d, k in slots:
        t = d[k]
        out.append(t._version)
        out.append(t.data_ptr())
    return tuple(out)


def _default_slots(device) -> torch.Tensor:
    """int32 arange(32) on `device`, made once: the default slots 0..B-1 of a
    B <= 32 call (cvit.py:175) as a slice, with no per-call launch or copy."""
    device = torch.device(device)
    t = _SLOTS.get(device)
    if t is None:
        t = _SLOTS[device] = torch.arange(MAX_SLOTS, dtype=torch.int32, device=device)
    return t


class _Node(nn.Module):
    """Parameter container (keeps state_dict paths such as features.1.running_var)."""

    def forward(self, *a, **k):  # pragma: no cover - never called
        raise RuntimeError("parameter container")


def _init_tensor(shape, kind):
    if kind == "nbt":
        return torch.zeros((), dtype=torch.long)
    if kind in ("rmean", "beta", "cbias", "lbias"):
        return torch.zeros(shape)
    if kind in ("rvar", "gamma"):
        return torch.ones(shape)
    if kind == "emb":
        return torch.randn(shape)
    t = torch.empty(shape)
    fan_in = int(math.prod(shape[1:]))
    bound = 1.0 / math.sqrt(fan_in)
    return t.uniform_(-bound, bound)


class CViT(nn.Module):
    def __init__(self, image_size=224, patch_size=7, num_classes=2, channels=512, dim=1024, depth=6, heads=8,
                 mlp_dim=2048, *, dtype: str = "fp16"):
        super().__init__()
        assert image_size % patch_size == 0, "image dimensions must be divisible by the patch size"
        cfg = dict(image_size=image_size, patch_size=patch_size, num_classes=num_classes, channels=channels, dim=dim,
                   depth=depth, heads=heads, mlp_dim=mlp_dim)
        if cfg != SUPPORTED:
            raise NotImplementedError(f"the gfx950 CViT path implements the cvit_prediction.py configuration "
                                      f"{SUPPORTED}, got {cfg}")
        if dtype not in _lib.DTYPES:
            raise ValueError(f"dtype must be one of {list(_lib.DTYPES)}")
        self.patch_size = patch_size
        self.dtype_name = dtype
        for name, shape, kind in cvit_param_specs(dim=dim, depth=depth, mlp_dim=mlp_dim, num_classes=num_classes,
                                                  channels=channels, patch_size=patch_size):
            *path, leaf = name.split(".")
            mod = self
            for p in path:
                if p not in mod._modules:
                    mod.add_module(p, _Node())
                mod = mod._modules[p]
            t = _init_tensor(shape, kind)
            if kind in _BUFFER_KINDS:
                mod.register_buffer(leaf, t)
            else:
                mod.register_parameter(leaf, nn.Parameter(t))
        self._ctx = None
        self._ctx_device = None
        self._loaded_versions = None
        # one fac_ctx per model: its workspace and streams are shared by every
        # call.  The C ABI orders the forwards of one context on the device
        # (each waits for the previous one's last kernel, whatever stream
        # either ran on), and this lock serialises the host side of the calls
        # (the context's bookkeeping is not thread-safe), so threads may share
        # the model on different streams.
        self._lock = threading.RLock()
        self.eval()

    # ------------------------------------------------------------------ weights
    def _versions(self):
        return weight_versions(self)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        out = super().load_state_dict(state_dict, strict=strict, assign=assign)
        self._loaded_versions = None
        return out

    def _ensure_ctx(self, device: torch.device, verify: bool = True):
        """The device context, with the current weights uploaded.  verify =
        False (the forwards): weights already uploaded once are not
        re-checked here -- the caller launches first and then calls
        _weights_changed(), which hides the ~25-70 us walk of the parameter
        slots behind the GPU work of the reference's per-video call."""
        lib = _lib.load()
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if self._ctx is None or self._ctx_device != idx:
            self._release()
            h = ctypes.c_void_p()
            _lib.check(lib.fac_create(idx, _lib.DTYPES[self.dtype_name], ctypes.byref(h)), None, "fac_create")
            self._ctx, self._ctx_device, self._loaded_versions = h, idx, None
        if verify or self._loaded_versions is None:
            self._upload_if_changed(lib)
        return lib

    def _weights_changed(self) -> bool:
        """After a launch on the uploaded weights: re-upload if a parameter or
        buffer changed since (in place, or a swapped tensor); True if so, and
        the caller then runs the forward again (stream-ordered after the stale
        one, whose outputs it overwrites)."""
        if self._loaded_versions == self._versions():
            return False
        self._upload_if_changed(_lib.load())
        return True

    def _upload_if_changed(self, lib):
        v = self._versions()
        if self._loaded_versions != v:
            keep, descs = [], []
            for k, t in self.state_dict().items():
                if k.endswith("num_batches_tracked"):
                    continue
                h = t.detach().to("cpu", torch.float32).contiguous()
                keep.append(h)
                d = _lib.TensorDesc()
                d.name = k.encode()
                d.data = h.data_ptr()
                d.ndim = h.dim()
                for i, s in enumerate(h.shape):
                    d.shape[i] = s
                descs.append(d)
            arr = (_lib.TensorDesc * len(descs))(*descs)
            _lib.check(lib.fac_load_weights(self._ctx, ctypes.cast(arr, ctypes.c_void_p), len(descs)), self._ctx,
                       "fac_load_weights")
            self._loaded_versions = v

    def reserve(self, max_batch: int, device=None):
        """Pre-size the device workspace (call before CUDA-graph capture)."""
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        with self._lock:
            lib = self._ensure_ctx(dev)
            _lib.check(lib.fac_reserve(self._ctx, int(max_batch)), self._ctx, "fac_reserve")

    def set_stem_chunk(self, crops: int):
        if self._ctx is None:
            raise RuntimeError("no device context yet: call reserve() or forward() first")
        _lib.check(_lib.load().fac_set_stem_chunk(self._ctx, int(crops)), self._ctx, "fac_set_stem_chunk")

    def set_option(self, key: str, value: int):
        """fac_set_option knobs (include/fac_cvit.h): stem_chunk, fuse_stem224,
        gemm_{patch,qkv,out,ff1,ff2,head}, proj_splits."""
        if self._ctx is None:
            raise RuntimeError("no device context yet: call reserve() or forward() first")
        _lib.check(_lib.load().fac_set_option(self._ctx, key.encode(), int(value)), self._ctx, "fac_set_option")

    def debug_gemm(self, epi: int, a: torch.Tensor, w: torch.Tensor, bias, out: torch.Tensor, splits: int = 1,
                   variant: int = -1):
        """One encoder GEMM out = a . w^T through fac_debug_gemm (16-bit a [M,K], w [N,K])."""
        M, K = a.shape
        N = w.shape[0]
        lib = self._ensure_ctx(a.device)
        stream = torch.cuda.current_stream(a.device).cuda_stream
        _lib.check(lib.fac_debug_gemm(self._ctx, int(epi), a.data_ptr(), w.data_ptr(),
                                      bias.data_ptr() if bias is not None else None, out.data_ptr(),
                                      M, N, K, int(splits), int(variant), stream), self._ctx, "fac_debug_gemm")

    def _release(self):
        if self._ctx is not None:
            _lib.load().fac_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError("the gfx950 CViT path is inference-only (eval-mode BatchNorm is folded into the convs)")
        return super().train(False)

    # ------------------------------------------------------------------ forward
    @staticmethod
    def _pos_index(B: int, pos_index, device) -> torch.Tensor:
        if pos_index is None:
            if B > MAX_SLOTS:
                # what `x += self.pos_embedding[0:B]` raises in the reference (cvit.py:175)
                raise RuntimeError(f"The size of tensor a ({B}) must match the size of tensor b ({MAX_SLOTS}) "
                                   f"at non-singleton dimension 0")
            return _default_slots(device)[:B]
        p = torch.as_tensor(pos_index)
        if p.shape != (B,):
            raise ValueError(f"pos_index must have shape ({B},), got {tuple(p.shape)}")
        if p.numel() and (int(p.min()) < 0 or int(p.max()) >= MAX_SLOTS):
            raise IndexError(f"pos_index values must lie in [0, {MAX_SLOTS})")
        return p.to(device=device, dtype=torch.int32).contiguous()

    def _run(self, x, B, pos_index, u8: bool, want_probs: bool):
        with self._lock:
            return self._run_locked(x, B, pos_index, u8, want_probs)

    def _run_locked(self, x, B, pos_index, u8: bool, want_probs: bool):
        if not x.is_cuda:
            raise RuntimeError("CViT (gfx950 HIP path) needs its input on a GPU device; there is no CPU fallback")
        lib = self._ensure_ctx(x.device, verify=False)
        pidx = self._pos_index(B, pos_index, x.device)
        logits = torch.empty(B, 2, dtype=torch.float32, device=x.device)
        probs = torch.empty(B, 2, dtype=torch.float32, device=x.device) if want_probs else None
        if B == 0:  # an empty batch: empty outputs, as the reference's forward gives (the C ABI takes B >= 1)
            return logits, probs
        stream = torch.cuda.current_stream(x.device).cuda_stream
        fn = lib.fac_forward_nhwc_u8 if u8 else lib.fac_forward_nchw_f32
        args = (self._ctx, x.data_ptr(), B, pidx.data_ptr(), logits.data_ptr(),
                probs.data_ptr() if probs is not None else None, stream)
        _lib.check(fn(*args), self._ctx, fn.__name__)
        if self._weights_changed():
            _lib.check(fn(*args), self._ctx, fn.__name__)
        return logits, probs

    def forward(self, img: torch.Tensor, mask=None, pos_index=None) -> torch.Tensor:
        if img.dim() != 4 or tuple(img.shape[1:]) != (3, 224, 224):
            raise ValueError(f"expected img [B,3,224,224], got {tuple(img.shape)}")
        poison = mask is not None and reference_mask_poisons(mask, img.shape[0])
        x = img.to(torch.float32).contiguous()
        logits, _ = self._run(x, x.shape[0], pos_index, u8=False, want_probs=False)
        return logits.fill_(float("nan")) if poison else logits

    def forward_u8_pipelined(self, crops: torch.Tensor, pos_index, chunk: int = 256,
                             equal: bool = True) -> torch.Tensor:
        """forward_u8 over more crops than one batch: the crops go in
        ceil(n/chunk) chunks (equal ones, or with ``equal=False`` full chunks
        of ``chunk`` and the remainder last) through
        fac_forward_nhwc_u8_pipelined, so chunk k's encoder + head (on the
        context's tail stream) overlaps chunk k+1's conv stack; then the
        current stream waits for every chunk.  Logits are bit-identical to one
        forward_u8 call (a crop's logits do not depend on its batch)."""
        if crops.dtype != torch.uint8 or crops.dim() != 4 or tuple(crops.shape[1:]) != (224, 224, 3):
            raise ValueError(f"expected uint8 crops [B,224,224,3], got {crops.dtype} {tuple(crops.shape)}")
        if not crops.is_cuda:
            raise RuntimeError("CViT (gfx950 HIP path) needs its input on a GPU device; there is no CPU fallback")
        with self._lock:
            return self._pipelined_locked(crops.contiguous(), pos_index, chunk, equal)

    def _pipelined_locked(self, x, pos_index, chunk, equal):
        n = int(x.shape[0])
        lib = self._ensure_ctx(x.device)
        pidx = self._pos_index(n, pos_index, x.device)
        logits = torch.empty(n, 2, dtype=torch.float32, device=x.device)
        if n == 0:
            return logits
        k = -(-n // max(1, int(chunk)))
        step = -(-n // k) if equal else max(1, int(chunk))
        stream = torch.cuda.current_stream(x.device).cuda_stream
        for lo in range(0, n, step):
            hi = min(n, lo + step)
            _lib.check(lib.fac_forward_nhwc_u8_pipelined(self._ctx, x[lo:hi].data_ptr(), hi - lo,
                                                         pidx[lo:hi].data_ptr(), logits[lo:hi].data_ptr(), None,
                                                         None, stream), self._ctx, "fac_forward_nhwc_u8_pipelined")
        _lib.check(lib.fac_pipeline_join(self._ctx, 0, stream), self._ctx, "fac_pipeline_join")
        return logits

    # ------------------------------------------------------------------ Grad-CAM (fac_fake_amd/gradcam.py)
    def gradcam_features(self, x: torch.Tensor, u8: bool):
        """(A, feat): the last BatchNorm's output before ReLU and MaxPool (features[-3], 16-bit NHWC
        [B,14,14,512]) and the stem output the forward computes ([B,7,7,512], bit-identical to it)."""
        with self._lock:
            lib = self._ensure_ctx(x.device)
            B = x.shape[0]
            t16 = torch.float16 if self.dtype_name == "fp16" else torch.bfloat16
            a = torch.empty(B, 14, 14, 512, dtype=t16, device=x.device)
            feat = torch.empty(B, 7, 7, 512, dtype=t16, device=x.device)
            _lib.check(lib.fac_gradcam_features(self._ctx, x.data_ptr(), int(u8), B, a.data_ptr(), feat.data_ptr(),
                                                torch.cuda.current_stream(x.device).cuda_stream), self._ctx,
                       "fac_gradcam_features")
            return a, feat

    def gradcam_tail(self, feat: torch.Tensor, pos_index, target: torch.Tensor):
        """(logits [B,2], d logits[b][target[b]] / d feat as fp32 [B,7,7,512]); target int32 [B] on the
        device, -1 = the crop's argmax.  The logits are bit-identical to the forward's."""
        with self._lock:
            lib = self._ensure_ctx(feat.device)
            B = feat.shape[0]
            pidx = self._pos_index(B, pos_index, feat.device)
            logits = torch.empty(B, 2, dtype=torch.float32, device=feat.device)
            grad = torch.empty(B, 7, 7, 512, dtype=torch.float32, device=feat.device)
            _lib.check(lib.fac_gradcam_tail(self._ctx, feat.data_ptr(), B, pidx.data_ptr(), target.data_ptr(),
                                            logits.data_ptr(), grad.data_ptr(),
                                            torch.cuda.current_stream(feat.device).cuda_stream), self._ctx,
                       "fac_gradcam_tail")
            return logits, grad

    def forward_u8(self, crops: torch.Tensor, pos_index=None, return_probs: bool = False):
        """uint8 NHWC RGB face crops [B,224,224,3] -> logits (and per-logit sigmoids)."""
        if crops.dtype != torch.uint8 or crops.dim() != 4 or tuple(crops.shape[1:]) != (224, 224, 3):
            raise ValueError(f"expected uint8 crops [B,224,224,3], got {crops.dtype} {tuple(crops.shape)}")
        x = crops.contiguous()
        logits, probs = self._run(x, x.shape[0], pos_index, u8=True, want_probs=return_probs)
        return (logits, probs) if return_probs else logits
