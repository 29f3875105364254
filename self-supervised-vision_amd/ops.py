"""Tensor-level wrappers over the C ABI.  Activations are NHWC fp32 device tensors, filters are
[O,I,H,W] tensors in channels_last memory format (= OHWI in memory).  Every function only enqueues
kernels on the current HIP stream; torch provides allocation, nothing else."""
import ctypes as C
import math
import os

import torch

from . import _lib
from ._lib import ConvDesc, call, ptr, stream, workspace

BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def _empty(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


# HOW the GEMM-shaped launches multiply (include/ssv_hip.h: ssv_conv_desc.arithmetic; csrc/split_bf16.h).  "bf16x3" (default since round 6): every fp32 operand as three
# bf16 pieces, six exact piece products per fp32 product, fp32 accumulation on the bf16 matrix pipe - fp32 in, fp32 out, error against fp64 at or below the fp32-MFMA
# kernels' on every layer shape (tests/test_gpu_split.py).  "f32": v_mfma_f32_32x32x2_f32 on the fp32 operands, the arithmetic of rounds 1-5.
# SSV_ARITHMETIC=f32|bf16x3; bench.py reports both in one line.  Launches without a bf16-piece kernel (image stem, C % 32 != 0 forwards, the strided data
# gradient below 128 input channels and on every grouped bank) run on fp32 MFMA either way.  A grouped bank's forward, its stride-1 data gradient (the forward kernel
# on the transposed bank) and its weight gradient DO take the bf16-piece kernels (tests/test_gpu_grouped_forms.py, rule (c)).
ARITHMETIC = os.environ.get("SSV_ARITHMETIC", "bf16x3")
if ARITHMETIC not in ("bf16x3", "f32"):
    raise _lib.SsvError(f"SSV_ARITHMETIC must be bf16x3 or f32 (got {ARITHMETIC!r})")


class arithmetic:
    """``with ops.arithmetic("f32"): ...`` - the launches inside run on the named arithmetic (tests, bench.py's fp32-instruction leg)."""

    def __init__(self, name):
        if name not in ("bf16x3", "f32"):
            raise _lib.SsvError(f"arithmetic must be bf16x3 or f32 (got {name!r})")
        self.name = name

    def __enter__(self):
        global ARITHMETIC
        self.prev, ARITHMETIC = ARITHMETIC, self.name
        invalidate_weight_caches()
        return self

    def __exit__(self, *exc):
        global ARITHMETIC
        ARITHMETIC = self.prev
        invalidate_weight_caches()
        return False


def conv_desc(x_shape, w_shape, stride, pad, w=None):
    """``w``: the tensor the launch will be given as its weight operand (the filter, its transpose, a transformed filter) - in the bf16x3 arithmetic its pre-split
    planes ride in the descriptor (made once per weight, stream and step: `_planes`).  Launches whose operands are both activations (weight gradients) pass none."""
    n, h, w_, c = x_shape
    k, ci, r, s = w_shape
    if ci != c:
        raise _lib.SsvError(f"conv: input has {c} channels, filter expects {ci}")
    ho, wo = (h + 2 * pad - r) // stride + 1, (w_ + 2 * pad - s) // stride + 1
    d = ConvDesc(n, h, w_, c, k, r, s, stride, pad, ho, wo)
    if ARITHMETIC == "bf16x3":
        d.arithmetic = _lib.ARITH_BF16X3
        if w is not None and w.numel() % 8 == 0 and (c % 32 == 0 or k % 32 == 0):      # forward products contract over C, the strided data gradient over K
            d.w_planes = ptr(_planes(w))
    return d


def _ohwi(w):
    """The filter must be OHWI in memory: a channels_last [O,I,H,W] tensor (or any [O,I,1,1]/2-D matrix)."""
    if w.dim() == 2:
        if not w.is_contiguous():
            raise _lib.SsvError("linear weight must be contiguous")
        return w, (w.shape[0], w.shape[1], 1, 1)
    if not w.is_contiguous(memory_format=torch.channels_last):
        raise _lib.SsvError("conv filter must be in channels_last (OHWI) memory format")
    return w, tuple(w.shape)


# The conv kernels address every tensor through a buffer descriptor with a non-negative 32-bit byte offset, so one launch handles
# tensors below 2 GiB (check_desc in csrc/conv_mfma.hip).  Larger batches are split along N HERE: NHWC tensors are contiguous per
# sample, a chunk is a plain sub-range of every operand, and each chunk is its own launch on the same stream.
_MAX_ELEMS = (1 << 29) - (1 << 22)


def _batch_chunks(n, per_sample_elems, rows_per_sample=None):
    """[(n0, n1)] such that every chunk keeps all tensors below the per-launch limit.  ``rows_per_sample`` (output rows per sample):
    chunk rows are kept a multiple of 64 so that the 64-row statistics partials of the chunks concatenate to exactly the partials of
    the unsplit launch."""
    worst = max(per_sample_elems)
    if n * worst < _MAX_ELEMS:
        return [(0, n)]
    nc = (_MAX_ELEMS - 1) // worst
    if nc < 1:
        raise _lib.SsvError("a single sample exceeds the 2 GiB per-launch tensor limit of the convolution kernels")
    if rows_per_sample is not None:
        q = 64 // math.gcd(rows_per_sample, 64)
        if nc // q * q < 1:
            raise _lib.SsvError(f"the statistics epilogue needs chunks of a multiple of {q} samples ({rows_per_sample} output rows per sample) but only "
                                f"{nc} sample(s) fit below the 2 GiB per-launch tensor limit: run this layer without the fused statistics "
                                f"(SSV_NO_BN_STATS_FUSION=1) or with smaller images")
        nc = nc // q * q
    return [(s0, min(s0 + nc, n)) for s0 in range(0, n, nc)]


def _sub(t, n0, n1):
    return None if t is None else t[n0:n1]


def conv2d_fwd(x, w, stride=1, pad=0, bias=None, addend=None, groups=1):
    """``groups`` > 1: w is the DENSE block-diagonal bank of a grouped convolution (group_expand); every column tile then contracts over the
    channels of its own groups only."""
    _lib._dev(x, w, bias, addend)
    w, wshape = _ohwi(w)
    d = conv_desc(x.shape, wshape, stride, pad)
    y = _empty((d.N, d.Ho, d.Wo, d.K), x)
    for n0, n1 in _batch_chunks(d.N, (d.H * d.W * d.C, d.Ho * d.Wo * d.K)):
        dc = conv_desc((n1 - n0,) + tuple(x.shape[1:]), wshape, stride, pad, w=w)
        if groups > 1:
            call("ssv_conv2d_fwd_grouped", C.byref(dc), int(groups), ptr(x[n0:n1]), ptr(w), ptr(bias), ptr(_sub(addend, n0, n1)), ptr(y[n0:n1]), stream())
        else:
            call("ssv_conv2d_fwd", C.byref(dc), ptr(x[n0:n1]), ptr(w), ptr(bias), ptr(_sub(addend, n0, n1)), ptr(y[n0:n1]), stream())
    return y


def conv2d_fwd_stats(x, w, stride=1, pad=0, keep_v=False):
    """y = conv(x, w) plus the BatchNorm statistics partials of y from the same epilogue: (y, pmean, pm2[, rows per group]) with one partial
    per 64 output rows unless the third element says otherwise.  Returns None when the shape is outside the fused kernel's preconditions
    (C % 32, K % 4)."""
    _lib._dev(x, w)
    _, wshape = _ohwi(w)
    if (wshape[1] % 32 and wshape[1] != 4) or wshape[0] % 4:          # C == 4: the padded image stem
        return None
    d = conv_desc(x.shape, wshape, stride, pad)
    try:                     # huge samples with an odd row count: no 64-row-aligned chunk fits one launch - the caller runs the stand-alone statistics pass
        _batch_chunks(d.N, (d.H * d.W * d.C, d.Ho * d.Wo * d.K), rows_per_sample=d.Ho * d.Wo)
    except _lib.SsvError:
        return None
    y, part = conv2d_fwd_fused(x, w, stride, pad, in_affine=None, want_stats=True, keep_v=keep_v)
    return (y,) + tuple(part)


def conv2d_fwd_fused(x, w, stride=1, pad=0, in_affine=None, want_stats=True, keep_v=False):
    """y = conv(act(x), w) where act is the identity or, with ``in_affine = (scale, shift)``, relu(x * scale[c] + shift[c]) applied while
    the operand is staged (x is then the producer's RAW conv output: the activation itself is never written).  With ``want_stats``
    the epilogue also leaves the BatchNorm statistics partials of y: returns (y, (pmean, pm2[, rows per group]) | None).
    Stride-1 3x3 convolutions of the deep stages run through Winograd F(2x2, 3x3) (`use_winograd`); ``keep_v`` then leaves the transformed
    input on the result (``y._wino_v``) for `conv2d_wgrad`."""
    _lib._dev(x, w)
    w, wshape = _ohwi(w)
    d = conv_desc(x.shape, wshape, stride, pad)
    if use_winograd(wshape, stride, pad, x.shape, want_stats):
        y, part, v = wino_conv2d_fwd(x, w, in_affine=in_affine, want_stats=want_stats, keep_v=keep_v)
        if v is not None:
            y._wino_v = v                  # the transformed input: the weight gradient's operand (nn.conv hands it to conv2d_wgrad)
        return y, part
    if in_affine is None and not want_stats:
        return conv2d_fwd(x, w, stride, pad), None
    y = _empty((d.N, d.Ho, d.Wo, d.K), x)
    lib = _lib.load()
    groups = int(lib.ssv_conv2d_fwd_stats_groups(C.byref(d)))
    part = _empty((2, groups, d.K), x) if want_stats else None
    sc, sh = in_affine if in_affine is not None else (None, None)
    g0 = 0
    for n0, n1 in _batch_chunks(d.N, (d.H * d.W * d.C, d.Ho * d.Wo * d.K), rows_per_sample=d.Ho * d.Wo if want_stats else None):
        dc = conv_desc((n1 - n0,) + tuple(x.shape[1:]), wshape, stride, pad, w=w)
        gc = int(lib.ssv_conv2d_fwd_stats_groups(C.byref(dc)))
        call("ssv_conv2d_fwd_bnrelu_in_stats", C.byref(dc), ptr(x[n0:n1]), ptr(sc), ptr(sh), ptr(w), ptr(y[n0:n1]),
             ptr(part[0][g0:g0 + gc]) if want_stats else None, ptr(part[1][g0:g0 + gc]) if want_stats else None, stream())
        g0 += gc
    return y, (None if part is None else (part[0], part[1]))


def can_form_closing_sum(w_shape, stride, pad, groups=1):
    """Can this convolution form (and write) the closing activation of the previous residual unit while it stages its input?"""
    k, c, r, s_ = w_shape
    return groups == 1 and r == 1 and s_ == 1 and stride == 1 and pad == 0 and c % 32 == 0 and k % 4 == 0


def conv2d_fwd_sumin(x, res, scale, shift, res_affine, w, want_mask=True):
    """y = conv1x1(a, w) with a = relu(x * scale + shift + res) (``res_affine = (rscale, rshift)``: + res * rscale + rshift) formed while it is
    staged AND written out by the same kernel; the epilogue leaves the BatchNorm statistics partials of y.
    Returns (y, (pmean, pm2), a, mask | None) - a / mask bit-identical to `bn_apply(x, scale, shift, relu=True, residual=res, ...)`."""
    _lib._dev(x, res, w)
    w, wshape = _ohwi(w)
    d = conv_desc(x.shape, wshape, 1, 0)
    y = _empty((d.N, d.Ho, d.Wo, d.K), x)
    a = torch.empty_like(x)
    m, c = _rows(x)
    mask = torch.empty((m * c // 4,), dtype=torch.uint8, device=x.device) if want_mask else None
    lib = _lib.load()
    groups = int(lib.ssv_conv2d_fwd_stats_groups(C.byref(d)))
    part = _empty((2, groups, d.K), x)
    rs, rh = res_affine if res_affine is not None else (None, None)
    per = d.H * d.W * d.C
    g0 = 0
    for n0, n1 in _batch_chunks(d.N, (per, d.Ho * d.Wo * d.K), rows_per_sample=d.Ho * d.Wo):
        dc = conv_desc((n1 - n0,) + tuple(x.shape[1:]), wshape, 1, 0, w=w)
        gc = int(lib.ssv_conv2d_fwd_stats_groups(C.byref(dc)))
        call("ssv_conv2d_fwd_sumin_stats", C.byref(dc), ptr(x[n0:n1]), ptr(res[n0:n1]), ptr(scale), ptr(shift), ptr(rs), ptr(rh), ptr(w), ptr(y[n0:n1]),
             ptr(part[0][g0:g0 + gc]), ptr(part[1][g0:g0 + gc]), ptr(a[n0:n1]), None if mask is None else ptr(mask[n0 * per // 4:n1 * per // 4]), stream())
        g0 += gc
    return y, (part[0], part[1]), a, mask


def can_fuse_conv_input(cin, cout, groups=1):
    """Preconditions of the fused-input convolution kernels (forward and weight gradient)."""
    return groups == 1 and cin % 32 == 0 and cin <= 1024 and cout % 4 == 0


_WT_CACHE = {}          # (weight address, stream, shape, version) -> (storage kept alive, transposed filter): one transpose per weight, stream and step
_WINO_U = {}            # (weight address, stream, shape, transposed?, version) -> (storage kept alive, Winograd-transformed filter), same lifetime
_PLANES = {}            # (operand address, stream, elements, version) -> (storage kept alive, its three bf16 planes), same lifetime


def invalidate_weight_caches():
    """Called by everything that mutates a GEMM operand in place (the optimizers' step() and zero_grad(), the EMA of target
    networks, MemoryBank pushes, checkpoint loads): a cached transposed filter must never outlive the weights it was made from."""
    _WT_CACHE.clear()
    _WINO_U.clear()
    _PLANES.clear()


def _planes(w):
    """The three bf16 planes of a weight operand (ssv_split_planes): [3][numel] bf16 as an int16 tensor, cached per HIP stream like the transposed filters."""
    n = w.numel()
    key = (w.data_ptr(), stream(), n, w._version)       # torch-level in-place edits of the operand move its version; the library's own updates call invalidate_weight_caches()
    hit = _PLANES.get(key)
    if hit is not None:
        return hit[1]
    if n % 8:
        raise _lib.SsvError(f"_planes: operand of {n} elements (needs a multiple of 8)")
    pl = torch.empty((3, n), dtype=torch.int16, device=w.device)
    call("ssv_split_planes", n, ptr(w), ptr(pl), stream())
    _PLANES[key] = (w.untyped_storage(), pl)
    return pl


def drop_planes(t):
    """Forget the cached bf16 planes of every operand inside ``t``'s memory: for a GEMM operand that is not a weight (it changes in place, or it dies with
    the call that made it) - the cache would otherwise keep its planes and its storage alive until the next optimizer step."""
    lo, hi = t.data_ptr(), t.data_ptr() + t.element_size() * t.numel()
    for key in [k for k in _PLANES if lo <= k[0] < hi]:
        del _PLANES[key]


def _transposed_filter(w, wshape):
    """wt[c][R-1-r][S-1-s][k] = w[k][r][s][c].  Cached per HIP stream (the transpose is ordered on that stream) until the next
    zero_grad(); the entry keeps the weight's storage alive, so an address can never come back as a different tensor."""
    # w._version, as _planes: a torch-level in-place edit of the filter (w.mul_(), w.copy_(), a foreign optimizer) must miss; the library's own raw-pointer
    # updates call invalidate_weight_caches() (tests/test_gpu_wino_forms.py, test_cached_filters_follow_in_place_edits)
    key = (w.data_ptr(), stream(), wshape, w._version)
    hit = _WT_CACHE.get(key)
    if hit is not None:
        return hit[1]
    k, c, r, s_ = wshape
    wt = torch.empty((c, r, s_, k), dtype=torch.float32, device=w.device)
    call("ssv_filter_transpose", k, r, s_, c, ptr(w), ptr(wt), stream())
    _WT_CACHE[key] = (w.untyped_storage(), wt)
    return wt


class BnGateCtx:
    """What a convolution's data gradient needs to run the first half of the BatchNorm backward in its epilogue (include/ssv_hip.h,
    ssv_bn_gate): the BatchNorm's input x, its saved statistics, and the ReLU bit - byte mask or the forward's (scale, shift)."""
    __slots__ = ("x", "mean", "invstd", "mask", "scale", "shift", "x2", "mean2", "invstd2")

    def __init__(self, x, mean, invstd, mask=None, scale=None, shift=None, second=None):
        """``second = (x2, mean2, invstd2)``: the gated gradient is also the gradient w.r.t. the output of the projection shortcut's BatchNorm
        (input x2): the epilogue then reduces sum g * xhat2 as well (mask gates on stride-1 data gradients only; dropped otherwise)."""
        self.x, self.mean, self.invstd, self.mask, self.scale, self.shift = x, mean, invstd, mask, scale, shift
        self.x2, self.mean2, self.invstd2 = second if second is not None else (None, None, None)


class LazyGrad:
    """The gradient w.r.t. a convolution output x that sits behind a BatchNorm, NOT written to HBM: dx = A[c] * g + B[c] * (x - mean[c])
    + D[c] with g the (relu-gated) gradient w.r.t. the BatchNorm's output and coef = [A | mean | B | D] from `bn_bwd_coef`.  The producing
    convolution's weight and data gradient form it while they stage their dY operand (ssv_conv2d_wgrad_dyin / ssv_conv2d_fwd_dyin), so the
    element-wise pass of the BatchNorm backward does not run (1x1 / stride-1 convolutions: conv3 and the stride-1 projection shortcut of
    networks/resnet.py:66-75, the widest tensors of a residual unit)."""
    __slots__ = ("g", "x", "coef", "wino_vd")

    def __init__(self, g, x, coef):
        self.g, self.x, self.coef = g, x, coef
        self.wino_vd = None              # Winograd F(4x4) layers: the data gradient's transformed input, left by the weight gradient's pass over (g, x)

    @property
    def shape(self):
        return self.g.shape


class StridedGrad:
    """The data gradient of a 1x1 / stride-2 convolution (the projection shortcut of a stage entry, networks/resnet.py:131-135), COMPACT: ``t``
    [N, ceil(H/2), ceil(W/2), C] holds the gradient of the input pixels with even (h, w); every other pixel's is zero and is not stored.  The
    unit input's other contribution (conv1's data gradient) takes it as its addend (ssv_conv2d_fwd_*_s2add); `materialize` is the fallback."""
    __slots__ = ("t", "full_shape")

    def __init__(self, t, full_shape):
        self.t, self.full_shape = t, tuple(full_shape)

    @property
    def shape(self):
        return self.full_shape

    def materialize(self):
        full = fill_(torch.empty(self.full_shape, dtype=torch.float32, device=self.t.device), 0.0)
        full[:, ::2, ::2, :].copy_(self.t)            # rare path (a consumer that cannot take the compact form): torch's strided copy
        return full


def compact_s2_dgrad(dy, w, x_shape):
    """dx of a 1x1 / stride-2 / unpadded convolution on the subsampled grid: one dense GEMM, as a StridedGrad."""
    n, h, w_, c = x_shape
    ho, wo = dy.shape[1], dy.shape[2]
    if (ho, wo) != ((h + 1) // 2, (w_ + 1) // 2):
        raise _lib.SsvError("compact_s2_dgrad: output grid does not match a 1x1 / stride-2 convolution")
    return StridedGrad(conv2d_dgrad(dy, w, (n, ho, wo, c), 1, 0), x_shape)


def can_lazy_dy(w_shape, stride, pad):
    """Can the weight and data gradient of this convolution take their dY operand as a LazyGrad?"""
    k, c, r, s_ = w_shape
    return r == 1 and s_ == 1 and stride == 1 and pad == 0 and k % 32 == 0 and c % 4 == 0


def _dyin_struct(lg, n0, n1):
    return _lib.BnDyin(ptr(lg.x[n0:n1]), ptr(lg.coef))


def _gate_struct(gate, groups, channels, like, second=False):
    part = _empty((3 if second else 2, groups, channels), like)
    st = _lib.BnGate(ptr(gate.x), ptr(gate.scale), ptr(gate.shift), ptr(gate.mask), ptr(gate.mean), ptr(gate.invstd), ptr(part[0]), ptr(part[1]),
                     ptr(gate.x2) if second else None, ptr(gate.mean2) if second else None, ptr(gate.invstd2) if second else None, ptr(part[2]) if second else None)
    return st, part


def _gate_sub(gate, n0, n1):
    return BnGateCtx(gate.x[n0:n1], gate.mean, gate.invstd, mask=None if gate.mask is None else gate.mask[n0 * gate.x[0].numel() // 4:n1 * gate.x[0].numel() // 4],
                     scale=gate.scale, shift=gate.shift, second=None if gate.x2 is None else (gate.x2[n0:n1], gate.mean2, gate.invstd2))


def conv2d_dgrad(dy, w, x_shape, stride=1, pad=0, addend=None, out=None, gate=None, groups=1):
    """dx = conv_transpose(dy, w) (+ addend).  Stride-1 layers (every Linear, every 1x1 and 3x3 stride-1 convolution) are computed
    as the FORWARD convolution of dy with the transposed, 180-degree rotated filter: both GEMM operands are then k-contiguous
    rows for ds_read_b128, which the dgrad kernel (weights read in place, k-major) cannot have - measured 5-15 % faster.
    ``gate`` (BnGateCtx): dx is the gradient w.r.t. a BatchNorm + ReLU output and this call is its LAST contribution - the epilogue
    stores the relu-gated gradient and the partial sums of the BatchNorm backward; they come back as ``dx._gate_partials``
    (psum_g, psum_gx, groups).  Silently ungated when the shape is outside the gated kernels' preconditions.
    ``groups`` > 1: w is the dense block-diagonal bank of a grouped convolution (plain data gradient only: no gate, no formed-on-load operand)."""
    if groups > 1 and (gate is not None or isinstance(dy, LazyGrad) or isinstance(addend, StridedGrad)):
        raise _lib.SsvError("conv2d_dgrad: the grouped data gradient takes no gate / lazy operand")
    lazy = dy if isinstance(dy, LazyGrad) else None
    if lazy is not None:
        dy = lazy.g
    compact = addend if isinstance(addend, StridedGrad) else None
    if compact is not None:
        _, wsh = _ohwi(w)
        fits = (gate is not None and gate.mask is not None and stride == 1 and wsh[2] == 1 and wsh[3] == 1 and pad == 0 and wsh[1] >= 128
                and wsh[0] % 32 == 0 and wsh[1] % 4 == 0 and tuple(gate.x.shape) == tuple(x_shape) and dy[0].numel() * dy.shape[0] < _MAX_ELEMS
                and x_shape[0] * x_shape[1] * x_shape[2] * x_shape[3] < _MAX_ELEMS)
        if not fits:
            addend, compact = compact.materialize(), None
            out = addend
        else:
            addend, out = compact.t, None
    _lib._dev(dy, w, addend)
    w, wshape = _ohwi(w)
    k, c, r, s_ = wshape
    if lazy is not None and lazy.wino_vd is not None:            # a Winograd F(4x4) layer: the weight gradient's pass over (g, x) left this product's transformed input
        if not (addend is None and out is None and (gate is None or gate.x2 is None) and groups == 1):
            raise _lib.SsvError("conv2d_dgrad: a LazyGrad of a Winograd layer reached a data gradient with an addend / second gate target (nn.conv marks such layers only "
                                "behind a fused input chain, where neither exists)")
        return wino44_conv2d_dgrad(lazy, w, gate=gate)
    if lazy is not None and not can_lazy_dy(wshape, stride, pad):
        raise _lib.SsvError("conv2d_dgrad: a LazyGrad reached a convolution that cannot form it (the producer must check ops.can_lazy_dy)")
    dx = out if out is not None else _empty(tuple(x_shape), dy)
    dx.__dict__.pop("_gate_partials", None)            # an accumulated-into buffer never keeps the partial sums of its old content
    dx.__dict__.pop("_gate_partials_res", None)
    if gate is not None and (k % 32 or c % 4 or tuple(gate.x.shape) != tuple(dx.shape)):
        gate = None
    lib = _lib.load()
    n = dy.shape[0]
    if (lazy is None and addend is None and out is None and (gate is None or gate.x2 is None) and groups == 1
            and use_winograd((c, k, r, s_), stride, pad, dy.shape, False)):
        return wino_conv2d_dgrad(dy, w, gate=gate)
    chunks = _batch_chunks(n, (dy[0].numel(), dx[0].numel()))
    as_fwd = stride == 1 and r == s_ and r - 1 - pad >= 0 and k % 16 == 0 and c % 4 == 0
    if gate is not None and not as_fwd and stride > 8:
        gate = None
    wt = _transposed_filter(w, wshape) if as_fwd else None
    second = gate is not None and as_fwd and gate.x2 is not None and gate.mask is not None and tuple(gate.x2.shape) == tuple(dx.shape)
    parts = []
    for n0, n1 in chunks:
        dyc, dxc, adc = dy[n0:n1], dx[n0:n1], _sub(addend, n0, n1)
        if as_fwd:
            d = conv_desc(dyc.shape, (c, k, r, s_), 1, r - 1 - pad, w=wt)
            if (d.Ho, d.Wo) != (x_shape[1], x_shape[2]):
                raise _lib.SsvError("conv2d_dgrad: input shape does not match the stride-1 geometry")
            if compact is not None:         # one chunk (checked above); the compact stride-2 addend rides on the byte-mask gate epilogues
                h2, w2 = compact.t.shape[1], compact.t.shape[2]
                groups = int(lib.ssv_conv2d_fwd_gate_groups(C.byref(d)))
                st, part = _gate_struct(gate, groups, c, dy, second)
                parts.append(part)
                if lazy is not None:
                    dyin = _dyin_struct(lazy, n0, n1)
                    call("ssv_conv2d_fwd_dyin_s2add", C.byref(d), ptr(dyc), C.byref(dyin), ptr(wt), ptr(compact.t), h2, w2, ptr(dxc), C.byref(st), stream())
                else:
                    call("ssv_conv2d_fwd_gated_s2add", C.byref(d), ptr(dyc), ptr(wt), ptr(compact.t), h2, w2, ptr(dxc), C.byref(st), stream())
            elif lazy is not None:
                st = None
                if gate is not None:
                    groups = int(lib.ssv_conv2d_fwd_gate_groups(C.byref(d)))
                    st, part = _gate_struct(_gate_sub(gate, n0, n1), groups, c, dy, second)
                    parts.append(part)
                dyin = _dyin_struct(lazy, n0, n1)
                call("ssv_conv2d_fwd_dyin", C.byref(d), ptr(dyc), C.byref(dyin), ptr(wt), ptr(adc), ptr(dxc), None if st is None else C.byref(st), stream())
            elif gate is not None:
                groups = int(lib.ssv_conv2d_fwd_gate_groups(C.byref(d)))
                st, part = _gate_struct(_gate_sub(gate, n0, n1), groups, c, dy, second)
                call("ssv_conv2d_fwd_gated", C.byref(d), ptr(dyc), ptr(wt), ptr(adc), ptr(dxc), C.byref(st), stream())
                parts.append(part)
            elif groups > 1:          # the transposed bank is block-diagonal too (input and output channels of a group change places)
                call("ssv_conv2d_fwd_grouped", C.byref(d), int(groups), ptr(dyc), ptr(wt), None, ptr(adc), ptr(dxc), stream())
            else:
                call("ssv_conv2d_fwd", C.byref(d), ptr(dyc), ptr(wt), None, ptr(adc), ptr(dxc), stream())
        else:
            d = conv_desc(dxc.shape, wshape, stride, pad, w=w if groups == 1 else None)
            if gate is not None:
                groups = int(lib.ssv_conv2d_dgrad_gate_groups(C.byref(d)))
                st, part = _gate_struct(_gate_sub(gate, n0, n1), groups, c, dy)
                call("ssv_conv2d_dgrad_gated", C.byref(d), ptr(dyc), ptr(w), ptr(adc), ptr(dxc), C.byref(st), stream())
                parts.append(part)
            elif groups > 1:
                call("ssv_conv2d_dgrad_grouped", C.byref(d), int(groups), ptr(dyc), ptr(w), ptr(adc), ptr(dxc), stream())
            else:
                call("ssv_conv2d_dgrad", C.byref(d), ptr(dyc), ptr(w), ptr(adc), ptr(dxc), stream())
    if parts:
        part = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)      # partial SUMS: any grouping of the rows adds up the same
        dx._gate_partials = (part[0], part[1], part.shape[1])
        if part.shape[0] == 3:                 # the same g against the projection shortcut's BatchNorm input
            dx._gate_partials_res = (part[0], part[2], part.shape[1])
    return dx


FUSE_BIAS_GRAD = os.environ.get("SSV_NO_BIAS_GRAD_FUSION", "0") != "1"      # diagnostic switch: bias gradients by the stand-alone column-sum pass


def conv2d_wgrad(x, dy, w_like, dw, stride=1, pad=0, accumulate=True, in_affine=None, wino_v=None, groups=1, dbias=None, dgrad_follows=None):
    """dw (+)= wgrad.  ``dw`` has the memory layout of ``w_like`` (OHWI).  ``in_affine = (scale, shift)``: x is a raw conv output and
    the operand is relu(x * scale + shift), formed on load (the fused chain's never-materialised activation).  ``wino_v``: the transformed
    input the Winograd forward of this convolution kept - the weight gradient is then 16 batched GEMMs on it (x / in_affine are not read).
    ``groups`` > 1: ``dw`` is the dense block-diagonal layout of a grouped convolution's bank and ONLY its diagonal blocks are defined afterwards
    (what group_extract reads); tiles no group touches are skipped.
    ``dgrad_follows`` (Winograd F(4x4) layers): will a PLAIN data gradient of the same dy follow (no addend, no accumulation target)?  Then the dY transform also
    writes that product's transformed input (one pass over dy); False spares the extra 2.25x write when the data gradient will take another kernel; None = decide by
    the dispatch rule alone.
    ``dbias``: the layer's bias gradient, (+)= the column sums of dy - taken from the same pass over dy when the layer is a Linear / 1x1 / stride-1
    one (the weight-gradient workgroups of column tile 0 sum the rows they stage), by the stand-alone column-sum kernel otherwise."""
    if dbias is not None:
        _, wsh = _ohwi(w_like)
        fused = (FUSE_BIAS_GRAD and groups == 1 and wino_v is None and in_affine is None and not isinstance(dy, LazyGrad)
                 and wsh[2] == 1 and wsh[3] == 1 and stride == 1 and pad == 0 and wsh[0] % 4 == 0 and wsh[1] % 4 == 0)
        if isinstance(dy, LazyGrad):
            raise _lib.SsvError("conv2d_wgrad: a bias gradient needs the materialised output gradient (a biased convolution is never followed by a fused BatchNorm)")
        if not fused:
            colsum(dy, dbias, accumulate=accumulate)
            return conv2d_wgrad(x, dy, w_like, dw, stride, pad, accumulate, in_affine, wino_v, groups)
        _lib._dev(x, dy, dw, dbias)
        lib = _lib.load()
        for i, (n0, n1) in enumerate(_batch_chunks(x.shape[0], (x[0].numel(), dy[0].numel()))):
            d = conv_desc(x[n0:n1].shape, wsh, stride, pad)
            ws = workspace.get(lib.ssv_conv2d_wgrad_bias_workspace_bytes(C.byref(d)), x.device)
            call("ssv_conv2d_wgrad_bias", C.byref(d), ptr(x[n0:n1]), ptr(dy[n0:n1]), ptr(dw), ptr(dbias), int(accumulate or i > 0), ptr(ws), ws.numel(), stream())
        return dw
    if groups > 1:
        if isinstance(dy, LazyGrad) or in_affine is not None or wino_v is not None:
            raise _lib.SsvError("conv2d_wgrad: the grouped weight gradient takes plain operands")
        _lib._dev(x, dy, dw)
        _, wshape = _ohwi(w_like)
        lib = _lib.load()
        for i, (n0, n1) in enumerate(_batch_chunks(x.shape[0], (x[0].numel(), dy[0].numel()))):
            d = conv_desc(x[n0:n1].shape, wshape, stride, pad)
            ws = workspace.get(lib.ssv_conv2d_wgrad_grouped_workspace_bytes(C.byref(d), int(groups)), x.device)
            call("ssv_conv2d_wgrad_grouped", C.byref(d), int(groups), ptr(x[n0:n1]), ptr(dy[n0:n1]), ptr(dw), int(accumulate or i > 0), ptr(ws), ws.numel(), stream())
        return dw
    if wino_v is not None and (not isinstance(dy, LazyGrad) or (wino_v.shape[0] == 36 and WINOGRAD44_DY_BOTH)):
        return wino_conv2d_wgrad(wino_v, dy, w_like, dw, accumulate=accumulate, dgrad_follows=dgrad_follows)
    lazy = dy if isinstance(dy, LazyGrad) else None
    if lazy is not None:
        dy = lazy.g
    _lib._dev(x, dy, dw)
    _, wshape = _ohwi(w_like)
    if lazy is not None and not can_lazy_dy(wshape, stride, pad):
        raise _lib.SsvError("conv2d_wgrad: a LazyGrad reached a convolution that cannot form it (the producer must check ops.can_lazy_dy)")
    lib = _lib.load()
    sc, sh = in_affine if in_affine is not None else (None, None)
    for i, (n0, n1) in enumerate(_batch_chunks(x.shape[0], (x[0].numel(), dy[0].numel()))):
        xc, dyc = x[n0:n1], dy[n0:n1]
        d = conv_desc(xc.shape, wshape, stride, pad)
        ws = workspace.get(lib.ssv_conv2d_wgrad_workspace_bytes(C.byref(d)), x.device)
        if lazy is not None:
            dyin = _dyin_struct(lazy, n0, n1)
            call("ssv_conv2d_wgrad_dyin", C.byref(d), ptr(xc), ptr(sc), ptr(sh), ptr(dyc), C.byref(dyin), ptr(dw), int(accumulate or i > 0), ptr(ws), ws.numel(), stream())
            continue
        call("ssv_conv2d_wgrad_bnrelu_in", C.byref(d), ptr(xc), ptr(sc), ptr(sh), ptr(dyc), ptr(dw), int(accumulate or i > 0), ptr(ws), ws.numel(), stream())
    return dw


def _rows(x):
    c = x.shape[-1]
    return x.numel() // c, c


def _rows_per_group(partials):
    """Statistics partials are (pmean, pm2) over groups of 64 output rows (the GEMM epilogues) or (pmean, pm2, rows per group) (the Winograd
    output transform on odd maps: one image per group)."""
    return int(partials[2]) if len(partials) > 2 else 64


def bn_train_fwd(x, gamma, beta, running_mean, running_var, nbt, relu=False, residual=None,
                 eps=BN_EPS, momentum=BN_MOMENTUM, want_mask=False, skip_mask=False, partials=None):
    """Returns (y, mean, invstd[, relu_mask]).  relu_mask: uint8, one byte per four channels, for the backward.
    ``partials`` = (pmean, pm2) from conv2d_fwd_stats: the statistics pass over x is skipped."""
    _lib._dev(x, gamma, beta, residual)
    m, c = _rows(x)
    y = torch.empty_like(x)
    mean, invstd = _empty((c,), x), _empty((c,), x)
    mask = torch.empty((m * c // 4,), dtype=torch.uint8, device=x.device) if (want_mask and relu and not skip_mask) else None
    ws = workspace.get(_lib.load().ssv_bn_workspace_bytes(m, c), x.device)
    if partials is not None:
        call("ssv_bn_train_fwd_partials", m, c, ptr(x), ptr(partials[0]), ptr(partials[1]), _rows_per_group(partials), ptr(gamma), ptr(beta), ptr(residual), int(relu), eps, momentum,
             ptr(running_mean), ptr(running_var), ptr(nbt), ptr(y), ptr(mask), ptr(mean), ptr(invstd), ptr(ws), ws.numel(), stream())
        return (y, mean, invstd, mask) if want_mask else (y, mean, invstd)
    call("ssv_bn_train_fwd", m, c, ptr(x), ptr(gamma), ptr(beta), ptr(residual), int(relu), eps, momentum,
         ptr(running_mean), ptr(running_var), ptr(nbt), ptr(y), ptr(mask), ptr(mean), ptr(invstd), ptr(ws), ws.numel(), stream())
    return (y, mean, invstd, mask) if want_mask else (y, mean, invstd)


def bn_stats_finalize(x_shape_rows, c, partials, gamma, beta, running_mean, running_var, nbt, eps=BN_EPS, momentum=BN_MOMENTUM):
    """Statistics partials of a conv output -> (mean, invstd, scale, shift) + running statistics: BatchNorm without its apply pass."""
    m = int(x_shape_rows)
    dev = gamma.device
    stats = torch.empty((4, c), dtype=torch.float32, device=dev)            # mean | invstd | scale | shift
    ws = workspace.get(_lib.load().ssv_bn_workspace_bytes(m, c), dev)
    call("ssv_bn_stats_finalize", m, c, ptr(partials[0]), ptr(partials[1]), _rows_per_group(partials), ptr(gamma), ptr(beta), eps, momentum,
         ptr(running_mean), ptr(running_var), ptr(nbt), ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(stats[3]), ptr(ws), ws.numel(), stream())
    return stats[0], stats[1], stats[2], stats[3]


def bn_apply(x, scale, shift, relu=False, residual=None, res_affine=None, want_mask=False):
    """y = relu?(x * scale + shift (+ residual | + residual * res_scale + res_shift)); returns (y, mask | None)."""
    _lib._dev(x, scale, shift, residual)
    m, c = _rows(x)
    y = torch.empty_like(x)
    mask = torch.empty((m * c // 4,), dtype=torch.uint8, device=x.device) if (want_mask and relu) else None
    rs, rh = res_affine if res_affine is not None else (None, None)
    call("ssv_bn_apply", m, c, ptr(x), ptr(scale), ptr(shift), ptr(residual), ptr(rs), ptr(rh), int(relu), ptr(y), ptr(mask), stream())
    return y, mask


def bn_relu_bwd_affine(dy, x, gamma, mean, invstd, scale, shift, dgamma, dbeta, accumulate=True):
    """Backward of a BatchNorm + ReLU whose output was never materialised: the gate is x * scale + shift > 0."""
    _lib._dev(dy, x)
    m, c = _rows(x)
    dx = torch.empty_like(x)
    ws = workspace.get(_lib.load().ssv_bn_workspace_bytes(m, c), x.device)
    call("ssv_bn_relu_bwd_affine", m, c, ptr(dy), ptr(x), ptr(gamma), ptr(mean), ptr(invstd), ptr(scale), ptr(shift), ptr(dx),
         ptr(dgamma), ptr(dbeta), int(accumulate), ptr(ws), ws.numel(), stream())
    return dx


def bn_bwd_from_partials(g, x, gamma, mean, invstd, partials, dgamma, dbeta, accumulate=True):
    """Second half of the BatchNorm backward behind a gated convolution (g already relu-gated, partial sums given)."""
    _lib._dev(g, x)
    m, c = _rows(x)
    dx = torch.empty_like(x)
    ws = workspace.get(_lib.load().ssv_bn_workspace_bytes(m, c), x.device)
    call("ssv_bn_bwd_from_partials", m, c, ptr(g), ptr(x), ptr(gamma), ptr(mean), ptr(invstd), ptr(partials[0]), ptr(partials[1]), int(partials[2]),
         ptr(dx), ptr(dgamma), ptr(dbeta), int(accumulate), ptr(ws), ws.numel(), stream())
    return dx


def bn_bwd_coef(x, gamma, mean, invstd, partials, dgamma, dbeta, accumulate=True):
    """The merge of `bn_bwd_from_partials` without its element-wise pass: dgamma / dbeta and the [4, C] coefficients of a LazyGrad."""
    _lib._dev(x, gamma)
    m, c = _rows(x)
    coef = torch.empty((4, c), dtype=torch.float32, device=x.device)
    ws = workspace.get(_lib.load().ssv_bn_workspace_bytes(m, c), x.device)
    call("ssv_bn_bwd_coef", m, c, ptr(gamma), ptr(mean), ptr(invstd), ptr(partials[0]), ptr(partials[1]), int(partials[2]),
         ptr(coef), ptr(dgamma), ptr(dbeta), int(accumulate), ptr(ws), ws.numel(), stream())
    return coef


def bn_train_bwd(dy, y, x, gamma, mean, invstd, relu, dgamma, dbeta, want_dres=False, accumulate=True, relu_mask=None):
    _lib._dev(dy, y, x)
    m, c = _rows(x)
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_dres else None
    ws = workspace.get(_lib.load().ssv_bn_workspace_bytes(m, c), x.device)
    call("ssv_bn_train_bwd", m, c, ptr(dy), ptr(y), ptr(relu_mask), ptr(x), ptr(gamma), ptr(mean), ptr(invstd), int(relu),
         ptr(dx), ptr(dres), ptr(dgamma), ptr(dbeta), int(accumulate), ptr(ws), ws.numel(), stream())
    return dx, dres


def colsum(x, out, accumulate=True):
    m, c = _rows(x)
    ws = workspace.get(_lib.load().ssv_bn_workspace_bytes(m, c), x.device)
    call("ssv_colsum", m, c, ptr(x), ptr(out), int(accumulate), ptr(ws), ws.numel(), stream())
    return out


def bn_relu_maxpool_fwd(y, scale, shift, keep_xmax=False):
    """maxpool3x3s2(relu(y * scale + shift)) of a raw conv output [N,H,W,C] in one pass: returns (pooled, argmax slots[, xmax]).
    ``keep_xmax``: also the raw conv output at every window's arg-max pixel - what lets the backward reduce at the pooled resolution."""
    _lib._dev(y, scale, shift)
    n, h, w, c = y.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = _empty((n, ho, wo, c), y)
    am = torch.empty((n, ho, wo, c), dtype=torch.uint8, device=y.device)
    xmax = _empty((n, ho, wo, c), y) if keep_xmax else None
    call("ssv_bn_relu_maxpool_fwd", n, h, w, c, ptr(y), ptr(scale), ptr(shift), ptr(out), ptr(am), ptr(xmax), stream())
    return (out, am, xmax) if keep_xmax else (out, am)


def bn_relu_maxpool_bwd(dpool, am, y, gamma, mean, invstd, scale, shift, dgamma, dbeta, accumulate=True, xmax=None):
    """Gradient w.r.t. the raw conv output y through maxpool, ReLU and BatchNorm, plus dgamma / dbeta.  ``xmax`` (from the forward): the
    reduction pass runs over the pooled positions instead of the full-resolution map (equal to rounding)."""
    _lib._dev(dpool, am, y, xmax)
    n, h, w, c = y.shape
    dy = torch.empty_like(y)
    ws = workspace.get(_lib.load().ssv_bn_workspace_bytes(n * h * w, c), y.device)
    call("ssv_bn_relu_maxpool_bwd", n, h, w, c, ptr(dpool), ptr(am), ptr(y), ptr(xmax), ptr(gamma), ptr(mean), ptr(invstd), ptr(scale), ptr(shift),
         ptr(dy), ptr(dgamma), ptr(dbeta), int(accumulate), ptr(ws), ws.numel(), stream())
    return dy


def maxpool_fwd(x):
    n, h, w, c = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    y = _empty((n, ho, wo, c), x)
    am = torch.empty((n, ho, wo, c), dtype=torch.uint8, device=x.device)
    call("ssv_maxpool3x3s2_fwd", n, h, w, c, ptr(x), ptr(y), ptr(am), stream())
    return y, am


def maxpool_bwd(dy, am, x_shape):
    n, h, w, c = x_shape
    dx = _empty(tuple(x_shape), dy)
    call("ssv_maxpool3x3s2_bwd", n, h, w, c, ptr(dy), ptr(am), ptr(dx), stream())
    return dx


def gap_fwd(x):
    n, h, w, c = x.shape
    y = _empty((n, c), x)
    call("ssv_gap_fwd", n, h * w, c, ptr(x), ptr(y), stream())
    return y


def gap_bwd(dy, x_shape):
    n, h, w, c = x_shape
    dx = _empty(tuple(x_shape), dy)
    call("ssv_gap_bwd", n, h * w, c, ptr(dy), ptr(dx), stream())
    return dx


def nchw_to_nhwc(x):
    """[N,C,H,W] (any strides) -> contiguous NHWC.  A channels_last input already IS NHWC in memory."""
    _lib._dev(x)
    n, c, h, w = x.shape
    if x.is_contiguous(memory_format=torch.channels_last) and c > 1:
        return x.permute(0, 2, 3, 1)
    if not x.is_contiguous():
        raise _lib.SsvError("image batch must be contiguous NCHW or channels_last")
    y = _empty((n, h, w, c), x)
    call("ssv_nchw_to_nhwc", n, c, h, w, ptr(x), ptr(y), stream())
    return y


def l2norm_fwd(z, normalize=True, ldo=None, eps=1e-12, out=None):
    _lib._dev(z)
    rows, d = z.shape
    ldo = d if ldo is None else ldo
    zhat = out if out is not None else _empty((rows, ldo), z)
    inv = _empty((rows,), z)
    call("ssv_l2norm_fwd", rows, d, ptr(z), int(normalize), eps, ptr(zhat), ldo, ptr(inv), stream())
    return zhat, inv


def l2norm_bwd(zhat, inv, dzhat, d, normalize=True):
    rows = zhat.shape[0]
    dz = _empty((rows, d), zhat)
    call("ssv_l2norm_bwd", rows, d, ptr(zhat), zhat.shape[1], ptr(inv), ptr(dzhat), dzhat.shape[1], int(normalize), ptr(dz), stream())
    return dz


def ema_(dst_flat, src_flat, momentum):
    """dst = momentum * dst + (1 - momentum) * src[:len(dst)]: the target arena mirrors a PREFIX of the online arena (same offsets;
    BYOL's online network has the predictor behind it)."""
    _lib._dev(dst_flat, src_flat)
    if dst_flat.numel() > src_flat.numel():
        raise _lib.SsvError("ema_: the source arena is shorter than the target")
    invalidate_weight_caches()
    call("ssv_ema", dst_flat.numel(), ptr(dst_flat), ptr(src_flat), float(momentum), stream())
    return dst_flat


def scale_(x, factor_dev):
    call("ssv_scale", x.numel(), ptr(x), ptr(factor_dev), stream())
    return x


def fill_(x, value):
    call("ssv_fill", x.numel(), ptr(x), float(value), stream())
    return x


def add_(dst, src):
    call("ssv_add", dst.numel(), ptr(dst), ptr(src), stream())
    return dst


def ntxent_splits(nglob, b):
    """Column splits of the NT-Xent row kernels at this shape: the library's choice (ssv_ntxent_default_splits), or SSV_NTXENT_SPLITS
    (diagnostic switch: 1 = the unsplit kernels)."""
    forced = os.environ.get("SSV_NTXENT_SPLITS")
    if forced:
        return max(1, min(int(forced), (2 * nglob + 31) // 32, 64))
    return int(_lib.load().ssv_ntxent_default_splits(nglob, b))


def _ntxent_ws(zall, b, splits):
    if splits <= 1:
        return None, 0
    nbytes = int(_lib.load().ssv_ntxent_split_workspace_bytes(b, zall.shape[1], splits))
    return workspace.get(nbytes, zall.device), nbytes


def ntxent_fwd(zall, nglob, b, seg0, inv_temp, splits=None):
    """Row log-sum-exp and positive logit of this rank's 2*b rows against the gathered [2*nglob, ld] matrix."""
    _lib._dev(zall)
    lse = _empty((2 * b,), zall)
    pos = _empty((2 * b,), zall)
    splits = ntxent_splits(nglob, b) if splits is None else splits
    ws, nbytes = _ntxent_ws(zall, b, splits)
    call("ssv_ntxent_fwd_split", nglob, b, seg0, zall.shape[1], ptr(zall), float(inv_temp), ptr(lse), ptr(pos), splits, ptr(ws), nbytes, stream())
    return lse, pos


def ntxent_gram_fwd(gram, nglob, b, seg0, inv_temp):
    """(lse, pos) of this rank's 2*b rows from the materialised Gram block [2*b, lds] (wide embeddings)."""
    _lib._dev(gram)
    lse, pos = _empty((2 * b,), gram), _empty((2 * b,), gram)
    call("ssv_ntxent_gram_fwd", nglob, b, seg0, gram.shape[1], ptr(gram), float(inv_temp), ptr(lse), ptr(pos), stream())
    return lse, pos


def ntxent_gram_weights(gram, lse_all, nglob, b, seg0, inv_temp, gscale):
    """In place: the Gram block becomes the weight matrix W' whose product with Z_all is dZ."""
    _lib._dev(gram, lse_all)
    call("ssv_ntxent_gram_weights", nglob, b, seg0, gram.shape[1], ptr(gram), ptr(lse_all), float(inv_temp), float(gscale), stream())
    return gram


def ntxent_loss(lse, pos, scale):
    loss = torch.empty((), dtype=torch.float32, device=lse.device)
    call("ssv_ntxent_loss", lse.numel(), ptr(lse), ptr(pos), float(scale), ptr(loss), stream())
    return loss


def ntxent_bwd(zall, lse_all, nglob, b, seg0, inv_temp, gscale, splits=None):
    _lib._dev(zall, lse_all)
    dz = _empty((2 * b, zall.shape[1]), zall)
    splits = ntxent_splits(nglob, b) if splits is None else splits
    ws, nbytes = _ntxent_ws(zall, b, splits)
    call("ssv_ntxent_bwd_split", nglob, b, seg0, zall.shape[1], ptr(zall), ptr(lse_all), float(inv_temp), float(gscale), ptr(dz),
         splits, ptr(ws), nbytes, stream())
    return dz


def mse_pair(o1, o2, t1, t2, scale):
    """loss = scale * (|o1 - t2|^2 + |o2 - t1|^2) summed over all elements; returns (loss 0-d, dloss/do1, dloss/do2)."""
    _lib._dev(o1, o2, t1, t2)
    n = o1.numel()
    do1, do2 = torch.empty_like(o1), torch.empty_like(o2)
    loss = torch.empty((), dtype=torch.float32, device=o1.device)
    ws = _lib.workspace.get(_lib.load().ssv_reduce_workspace_bytes(n), o1.device)
    call("ssv_mse_pair_fwd_bwd", n, ptr(o1), ptr(o2), ptr(t1), ptr(t2), float(scale), ptr(loss), ptr(do1), ptr(do2), ptr(ws), ws.numel(), stream())
    return loss, do1, do2


def barlow_cgrad(craw, inv_b, lmbda):
    """C = craw * inv_b; loss = sum_ii (C-1)^2 + lmbda * sum_{i!=j} C^2; returns (loss 0-d, G = dloss/dcraw [D,D])."""
    _lib._dev(craw)
    d = craw.shape[0]
    g = torch.empty_like(craw)
    loss = torch.empty((), dtype=torch.float32, device=craw.device)
    ws = _lib.workspace.get(_lib.load().ssv_reduce_workspace_bytes(d * d), craw.device)
    call("ssv_barlow_cgrad", d, ptr(craw), float(inv_b), float(lmbda), ptr(loss), ptr(g), ptr(ws), ws.numel(), stream())
    return loss, g


# ------------------------------------------------------------------------------------------- VICReg (csrc/vicreg.hip)
def _vicreg_ws(b, d, like):
    nbytes = int(_lib.load().ssv_vicreg_workspace_bytes(b, d))
    if nbytes == 0:
        raise _lib.SsvError(f"VICReg: need B >= 2 and D a multiple of 32 in [32, {_lib.VICREG_MAX_D}] (got B={b} D={d})")
    return workspace.get(nbytes, like.device)


def vicreg_prep(x, y, sim_coeff, std_coeff, cov_coeff, eps):
    """x, y [B, D] -> (xc [2, B, D] centred, s [2, D] = sqrt(unbiased variance + eps), e [2, B, D] the sim and std terms of (dx, dy),
    parts [2] the weighted sim and std terms of the loss)."""
    _lib._dev(x, y)
    if x.dim() != 2 or x.shape != y.shape or not (x.is_contiguous() and y.is_contiguous()):
        raise _lib.SsvError(f"vicreg_prep expects two dense [B, D] matrices, got {tuple(x.shape)} and {tuple(y.shape)}")
    b, d = x.shape
    ws = _vicreg_ws(b, d, x)
    xc, s, e, parts = _empty((2, b, d), x), _empty((2, d), x), _empty((2, b, d), x), _empty((2,), x)
    call("ssv_vicreg_prep", b, d, ptr(x), ptr(y), float(sim_coeff), float(std_coeff), float(cov_coeff), float(eps),
         ptr(xc), ptr(s), ptr(e), ptr(parts), ptr(ws), ws.numel(), stream())
    return xc, s, e, parts


def vicreg_cgrad(craw, b, cov_coeff, parts):
    """craw [2, D, D] = xc^T xc per view is OVERWRITTEN by G = 4 cov_coeff / (D (B-1)^2) craw with a zero diagonal; returns (loss [4] = total and the
    weighted sim, std, cov terms, G)."""
    _lib._dev(craw, parts)
    if craw.dim() != 3 or craw.shape[0] != 2 or craw.shape[1] != craw.shape[2] or not craw.is_contiguous():
        raise _lib.SsvError(f"vicreg_cgrad expects a dense [2, D, D] block, got {tuple(craw.shape)}")
    d = craw.shape[1]
    ws = _vicreg_ws(b, d, craw)
    loss = _empty((4,), craw)
    drop_planes(craw)          # craw becomes a GEMM operand after it changed in place: planes split from it before are stale
    call("ssv_vicreg_cgrad", b, d, ptr(craw), float(cov_coeff), ptr(parts), ptr(loss), ptr(ws), ws.numel(), stream())
    return loss, craw


def _arith_code():
    """ARITHMETIC as the C ABI's code, for the entry points that take it as an argument (the searches and k-means)"""
    return _lib.ARITH_BF16X3 if ARITHMETIC == "bf16x3" else _lib.ARITH_F32_MFMA


def knn_label_agreement(z, labels, k):
    """Number of (query, neighbour) pairs with equal labels among each row's k nearest neighbours by inner product
    (best hit dropped), as a python int.  z [n,d] fp32 device, labels [n] int32 device."""
    _lib._dev(z, labels)
    n, d = z.shape
    if d % 4:
        z = torch.nn.functional.pad(z, (0, 4 - d % 4))
        d = z.shape[1]
    z = z.contiguous()
    count = torch.empty((1,), dtype=torch.int64, device=z.device)
    arith = _arith_code()
    ws = torch.empty(_lib.load().ssv_knn_workspace_bytes_arith(n, d, arith), dtype=torch.uint8, device=z.device)    # up to ~1 GB: not kept in the training scratch
    call("ssv_knn_label_agreement_arith", n, d, ptr(z), ptr(labels), int(k), ptr(count), arith, ptr(ws), ws.numel(), stream())
    return int(count.item())


# ------------------------------------------------------------------------------------------- k-means / cluster accuracy (csrc/kmeans.hip)
def _kmeans_operands(who, x, centroids):
    """Checks shared by the two k-means calls; returns (x, centroids, n, d, k, dp) with dp the column count the kernels see (d rounded up to 4)."""
    _lib._dev(x, centroids)
    if x.dim() != 2 or centroids.dim() != 2 or x.dtype != torch.float32 or centroids.dtype != torch.float32:
        raise _lib.SsvError(f"{who}: fp32 matrices x [n, d] and centroids [k, d] expected (got {tuple(x.shape)} {x.dtype}, {tuple(centroids.shape)} {centroids.dtype})")
    if not x.is_contiguous() or not centroids.is_contiguous():
        raise _lib.SsvError(f"{who}: x and centroids must be contiguous")
    (n, d), (k, dc) = x.shape, centroids.shape
    if dc != d:
        raise _lib.SsvError(f"{who}: x has {d} columns, the centroids {dc}")
    if not 1 <= k <= n:
        raise _lib.SsvError(f"{who}: need 1 <= k <= n (got k = {k}, n = {n})")
    if k > _lib.KMEANS_MAX_K or d > _lib.KMEANS_MAX_D or d < 1:
        raise _lib.SsvError(f"{who}: k <= {_lib.KMEANS_MAX_K} and 1 <= d <= {_lib.KMEANS_MAX_D} (got k = {k}, d = {d})")
    return n, d, k, (d + 3) // 4 * 4


def _pad4(t, dp):
    return t if t.shape[1] == dp else torch.nn.functional.pad(t, (0, dp - t.shape[1]))        # zero columns: exact


def kmeans_prep(x, centroids):
    """The buffer ssv_kmeans_assign / _update keep 1/2 |c|^2 and the centroids' bf16 planes in (caller-owned: it lives from an update to the next assignment)."""
    n, d, k, dp = _kmeans_operands("kmeans_prep", x, centroids)
    return torch.empty(_lib.load().ssv_kmeans_prep_bytes(dp, k), dtype=torch.uint8, device=x.device)


def kmeans_assign(x, centroids, prep=None, prep_ready=False):
    """labels [n] int32 = argmax_j (x . c_j - 1/2 |c_j|^2) (exact ties to the lowest j), dist [n] = squared distance to that centroid, counts [k] int32,
    objective (0-d) = sum dist.  x [n, d], centroids [k, d]: contiguous fp32 device matrices; any d (columns are padded with zeros to a multiple of 4 here).
    ``prep`` (kmeans_prep) with ``prep_ready``: the centroid-side operands kmeans_update left for exactly these centroids - they are not made again."""
    n, d, k, dp = _kmeans_operands("kmeans_assign", x, centroids)
    xp, cp = _pad4(x, dp), _pad4(centroids, dp)
    lib = _lib.load()
    if prep is None:
        prep, prep_ready = torch.empty(lib.ssv_kmeans_prep_bytes(dp, k), dtype=torch.uint8, device=x.device), False
    labels = torch.empty(n, dtype=torch.int32, device=x.device)
    dist = torch.empty(n, dtype=torch.float32, device=x.device)
    counts = torch.empty(k, dtype=torch.int32, device=x.device)
    objective = torch.empty((), dtype=torch.float32, device=x.device)
    arith = _arith_code()
    ws = workspace.get(lib.ssv_kmeans_workspace_bytes(n, dp, k, arith), x.device)
    call("ssv_kmeans_assign", n, dp, k, ptr(xp), ptr(cp), ptr(prep), int(bool(prep_ready)), ptr(labels), ptr(dist), ptr(counts), ptr(objective), arith,
         ptr(ws), ws.numel(), stream())
    return labels, dist, counts, objective


def kmeans_update(x, labels, counts, centroids, prep=None):
    """In place: centroids[j] = mean of the rows of x labelled j (fixed summation order); counts[j] == 0 keeps centroids[j].  ``prep``: left ready for the next
    kmeans_assign of these centroids."""
    n, d, k, dp = _kmeans_operands("kmeans_update", x, centroids)
    _lib._dev(labels, counts)
    if labels.dtype != torch.int32 or counts.dtype != torch.int32 or labels.shape != (n,) or counts.shape != (k,) or not (labels.is_contiguous() and counts.is_contiguous()):
        raise _lib.SsvError(f"kmeans_update: contiguous int32 labels [{n}] and counts [{k}] expected")
    xp, cp = _pad4(x, dp), _pad4(centroids, dp)
    lib = _lib.load()
    arith = _arith_code()
    ws = workspace.get(lib.ssv_kmeans_workspace_bytes(n, dp, k, arith), x.device)
    call("ssv_kmeans_update", n, dp, k, ptr(xp), ptr(labels), ptr(counts), ptr(cp), ptr(prep), arith, ptr(ws), ws.numel(), stream())
    if cp is not centroids:
        centroids.copy_(cp[:, :d])
    invalidate_weight_caches()          # the centroids are a GEMM operand (the unfused assignment's filter bank) and changed in place
    return centroids


def cluster_votes(pred, targets, pred_k, targets_k):
    """votes [pred_k, targets_k] int64: rows with pred == p and targets == t (the table hungarian_match counts on the host).  A label outside its range
    raises SsvError (it is not counted; the device flag is read here - one synchronisation, this is an evaluation)."""
    _lib._dev(pred, targets)
    n = pred.numel()
    if pred.dtype != torch.int32 or targets.dtype != torch.int32 or pred.dim() != 1 or targets.shape != pred.shape or not (pred.is_contiguous() and targets.is_contiguous()):
        raise _lib.SsvError("cluster_votes: contiguous int32 vectors pred [n] and targets [n] expected")
    votes = torch.empty((int(pred_k), int(targets_k)), dtype=torch.int64, device=pred.device)
    flag = torch.empty(1, dtype=torch.int32, device=pred.device)
    call("ssv_cluster_votes", n, ptr(pred), ptr(targets), int(pred_k), int(targets_k), ptr(votes), ptr(flag), stream())
    if int(flag.item()) != 0:
        raise _lib.SsvError(f"cluster_votes: a label lies outside [0, {int(pred_k)}) x [0, {int(targets_k)})")
    return votes


# ------------------------------------------------------------------------------------------- weighted kNN classifier (csrc/knnclassify.hip)
def knn_search(queries, bank, k, chunk_rows=0, part_cols=0):
    """(sim [m, k] fp32, idx [m, k] int32): for every row of queries [m, d] the k rows of bank [n, d] with the largest inner product, sorted - similarity
    descending, exact ties to the lower index, a NaN below every number.  Contiguous fp32 device matrices of any d (columns are padded with zeros to a multiple
    of 4 here: exact); 1 <= k <= min(n, 1024).  ``chunk_rows`` / ``part_cols``: query rows and bank rows of one block of the product (0: the library's choice)."""
    _lib._dev(queries, bank)
    if queries.dim() != 2 or bank.dim() != 2 or queries.dtype != torch.float32 or bank.dtype != torch.float32:
        raise _lib.SsvError(f"knn_search: fp32 matrices queries [m, d] and bank [n, d] expected (got {tuple(queries.shape)} {queries.dtype}, {tuple(bank.shape)} {bank.dtype})")
    if not queries.is_contiguous() or not bank.is_contiguous():
        raise _lib.SsvError("knn_search: queries and bank must be contiguous")
    (m, d), (n, db), k = queries.shape, bank.shape, int(k)
    if db != d or d < 1 or d > _lib.KNN_MAX_D:
        raise _lib.SsvError(f"knn_search: queries have {d} columns, the bank {db}; 1 <= d <= {_lib.KNN_MAX_D}")
    if m < 1 or not 1 <= k <= min(n, _lib.KNN_MAX_K):
        raise _lib.SsvError(f"knn_search: need m >= 1 and 1 <= k <= min(n, {_lib.KNN_MAX_K}) (got m = {m}, n = {n}, k = {k})")
    dp = (d + 3) // 4 * 4
    qp, bp = _pad4(queries, dp), _pad4(bank, dp)
    arith = _arith_code()
    need = _lib.load().ssv_knn_search_workspace_bytes(m, n, dp, k, arith, int(chunk_rows), int(part_cols))
    ws = workspace.get(max(need, 16), queries.device)                   # need == 0: a partition the library refuses - the call below says why
    sim = torch.empty((m, k), dtype=torch.float32, device=queries.device)
    idx = torch.empty((m, k), dtype=torch.int32, device=queries.device)
    call("ssv_knn_search", m, n, dp, k, ptr(qp), ptr(bp), ptr(sim), ptr(idx), arith, int(chunk_rows), int(part_cols), ptr(ws), ws.numel(), stream())
    return sim, idx


def knn_vote(sim, idx, bank_labels, num_classes, temperature, topn=1, return_scores=False):
    """pred [m, topn] int32: per row of (sim, idx) [m, k] (what knn_search returns) the ``topn`` classes by score descending, ties to the lower class, with
    score[c] = sum over the neighbours labelled c of exp((sim - sim[:, 0]) / temperature), summed in rank order.  ``return_scores``: (pred, scores [m, C] fp32).
    bank_labels [n] int32.  An index outside the bank or a label outside [0, num_classes) raises SsvError (it is not counted; the device flag is read here -
    one synchronisation, this is an evaluation)."""
    _lib._dev(sim, idx, bank_labels)
    if sim.dim() != 2 or sim.dtype != torch.float32 or idx.dtype != torch.int32 or idx.shape != sim.shape or not (sim.is_contiguous() and idx.is_contiguous()):
        raise _lib.SsvError("knn_vote: contiguous sim [m, k] fp32 and idx [m, k] int32 expected")
    if bank_labels.dim() != 1 or bank_labels.dtype != torch.int32 or not bank_labels.is_contiguous():
        raise _lib.SsvError("knn_vote: a contiguous int32 vector bank_labels [n] expected")
    (m, k), n, c, topn = sim.shape, bank_labels.numel(), int(num_classes), int(topn)
    if not (float(temperature) > 0.0 and math.isfinite(1.0 / float(temperature))):
        raise _lib.SsvError(f"knn_vote: the temperature must be positive and finite (got {temperature})")
    if m < 1 or not 1 <= k <= _lib.KNN_MAX_K or n < 1 or not 1 <= c <= _lib.KNN_MAX_CLASSES or not 1 <= topn <= min(c, _lib.KNN_MAX_TOPN):
        raise _lib.SsvError(f"knn_vote: need m >= 1, 1 <= k <= {_lib.KNN_MAX_K}, n >= 1, 1 <= num_classes <= {_lib.KNN_MAX_CLASSES}, 1 <= topn <= min(num_classes, "
                            f"{_lib.KNN_MAX_TOPN}) (got m = {m}, k = {k}, n = {n}, num_classes = {c}, topn = {topn})")
    pred = torch.empty((m, topn), dtype=torch.int32, device=sim.device)
    scores = torch.empty((m, c), dtype=torch.float32, device=sim.device) if return_scores else None
    flag = torch.empty(1, dtype=torch.int32, device=sim.device)
    call("ssv_knn_vote", m, k, n, c, topn, ptr(sim), ptr(idx), ptr(bank_labels), 1.0 / float(temperature), ptr(pred), ptr(scores), ptr(flag), stream())
    if int(flag.item()) != 0:
        raise _lib.SsvError(f"knn_vote: a neighbour index lies outside [0, {n}) or a bank label outside [0, {c})")
    return (pred, scores) if return_scores else pred


# ------------------------------------------------------------------------------------------- NNCLR's pieces: the nearest-neighbour lookup (csrc/nnlookup.hip), the cross-entropy
def nn_lookup_slice_rows(n):
    """Bank rows one workgroup of the fused lookup folds before its partial result leaves for the workspace (include/ssv_hip.h: ssv_nn_lookup, `arithmetic`):
    rows [s * L, (s + 1) * L) form slice s."""
    n = int(n)
    if not 1 <= n < 1 << 31:
        raise _lib.SsvError(f"nn_lookup_slice_rows: need 1 <= n < 2^31 (got {n})")
    slices = -(-n // _lib.NN_LOOKUP_SLICE)
    return _lib.NN_LOOKUP_SLICE * -(-slices // _lib.NN_LOOKUP_MAX_SLICES)


def softmax_ce(logits, labels, classes=None, want_grad=True):
    """(stats [2], dlogits or None) of a dense logit matrix [N, ld] whose first ``classes`` columns are valid (default all) against int32 labels [N]: stats[0] = the
    mean cross-entropy, stats[1] = the fraction of rows whose arg-max is the label, dlogits [N, ld] = d(mean loss) / dlogits with zeros in the pad columns
    (ssv_softmax_ce_fwd_bwd, the linear probe's kernel)."""
    _lib._dev(logits, labels)
    if logits.dim() != 2 or logits.dtype != torch.float32 or not logits.is_contiguous() or labels.dtype != torch.int32 or labels.shape != (logits.shape[0],) or not labels.is_contiguous():
        raise _lib.SsvError("softmax_ce: a contiguous fp32 matrix logits [N, ld] and contiguous int32 labels [N] expected")
    n, ld = logits.shape
    c = ld if classes is None else int(classes)
    if not 1 <= c <= ld:
        raise _lib.SsvError(f"softmax_ce: need 1 <= classes <= {ld} columns (got {c})")
    stats = _empty((2,), logits)
    dlog = torch.empty_like(logits) if want_grad else None
    ws = workspace.get(_lib.load().ssv_softmax_ce_workspace_bytes(n), logits.device)
    call("ssv_softmax_ce_fwd_bwd", n, c, ld, ptr(logits), ptr(labels), ptr(stats), ptr(dlog), ptr(ws), ws.numel(), stream())
    return stats, dlog


def nn_lookup(queries, bank, n=None, out_scale=1.0, want_rows=True):
    """(nn [m, d] fp32 or None, idx [m] int32, sim [m] fp32): for every row of queries [m, d] the row j < n of bank [>= n, d] with the largest inner product - exact
    ties to the lowest j, a NaN score never wins - as idx, its score as sim, and out_scale * bank[idx] as nn (``want_rows``).  ``n``: the rows of the bank that
    are searched (default all; a MemoryBank's pad rows stay outside).  Contiguous fp32 device matrices, d % 4 == 0, m <= 8192.  Only enqueues: no host
    synchronisation, capturable in a step graph."""
    _lib._dev(queries, bank)
    if queries.dim() != 2 or bank.dim() != 2 or queries.dtype != torch.float32 or bank.dtype != torch.float32:
        raise _lib.SsvError(f"nn_lookup: fp32 matrices queries [m, d] and bank [rows, d] expected (got {tuple(queries.shape)} {queries.dtype}, {tuple(bank.shape)} {bank.dtype})")
    if not queries.is_contiguous() or not bank.is_contiguous():
        raise _lib.SsvError("nn_lookup: queries and bank must be contiguous")
    (m, d), (rows, db) = queries.shape, bank.shape
    n = rows if n is None else int(n)
    if db != d or d < 4 or d % 4 or d > _lib.KNN_MAX_D:
        raise _lib.SsvError(f"nn_lookup: queries have {d} columns, the bank {db}; d % 4 == 0 and 4 <= d <= {_lib.KNN_MAX_D}")
    if not 1 <= m <= _lib.NN_LOOKUP_MAX_M or not 1 <= n <= rows:
        raise _lib.SsvError(f"nn_lookup: need 1 <= m <= {_lib.NN_LOOKUP_MAX_M} and 1 <= n <= the bank's {rows} rows (got m = {m}, n = {n})")
    if not math.isfinite(float(out_scale)):
        raise _lib.SsvError(f"nn_lookup: out_scale must be finite (got {out_scale})")
    arith = _arith_code()
    ws = workspace.get(max(_lib.load().ssv_nn_lookup_workspace_bytes(m, n, d, arith), 16), queries.device)
    nn = torch.empty((m, d), dtype=torch.float32, device=queries.device) if want_rows else None
    idx = torch.empty(m, dtype=torch.int32, device=queries.device)
    sim = torch.empty(m, dtype=torch.float32, device=queries.device)
    call("ssv_nn_lookup", m, n, d, ptr(queries), ptr(bank), float(out_scale), ptr(nn), ptr(idx), ptr(sim), arith, ptr(ws), ws.numel(), stream())
    return nn, idx, sim


# ------------------------------------------------------------------------------------------- W-MSE's pieces: the batched whitening and the permutation (csrc/whiten.hip)
def _whiten_check(who, x, rows):
    _lib._dev(x, rows)
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous() or rows.dim() != 2 or rows.dtype != torch.int32 or not rows.is_contiguous():
        raise _lib.SsvError(f"{who}: a contiguous fp32 matrix x [n_rows, d] and contiguous int32 rows [blocks, w] expected (got {tuple(x.shape)} {x.dtype}, {tuple(rows.shape)} {rows.dtype})")
    (n_rows, d), (blocks, w) = x.shape, rows.shape
    if d < 4 or d % 4 or d > _lib.WHITEN_MAX_D or not d < w <= _lib.WHITEN_MAX_W or blocks < 1:
        raise _lib.SsvError(f"{who}: need d % 4 == 0, 4 <= d <= {_lib.WHITEN_MAX_D}, d < w <= {_lib.WHITEN_MAX_W} and at least one block (got d = {d}, w = {w}, blocks = {blocks})")
    return n_rows, d, blocks, w


def whiten_fwd(x, rows, eps=0.0):
    """(y [blocks * w, d], mean [blocks, d], winv [blocks, d, d], info int32 [blocks]): every block rows[b] of w row indices into x [n_rows, d] is centred and whitened by
    the inverse Cholesky factor of (1 - eps) cov + eps I (include/ssv_hip.h: ssv_whiten_fwd).  info[b] = 0, j + 1 for a failed pivot j, -1 for an index out of range
    (the block's outputs are NaN then).  Only enqueues: no host synchronisation, capturable in a step graph."""
    n_rows, d, blocks, w = _whiten_check("whiten_fwd", x, rows)
    if not 0.0 <= float(eps) < 1.0:
        raise _lib.SsvError(f"whiten_fwd: need 0 <= eps < 1 (got {eps})")
    y = _empty((blocks * w, d), x)
    mean = _empty((blocks, d), x)
    winv = _empty((blocks, d, d), x)
    info = torch.empty(blocks, dtype=torch.int32, device=x.device)
    ws = workspace.get(_lib.load().ssv_whiten_workspace_bytes(blocks, w, d), x.device)
    call("ssv_whiten_fwd", blocks, w, d, n_rows, ptr(x), ptr(rows), float(eps), ptr(y), ptr(mean), ptr(winv), ptr(info), ptr(ws), ws.numel(), stream())
    return y, mean, winv, info


def whiten_bwd(x, rows, eps, mean, winv, dy, dx=None):
    """dx [n_rows, d]: the gradient of whiten_fwd's y with respect to x given dy [blocks * w, d]; the rows the blocks name are written, the others keep what ``dx``
    held (zeros when it is allocated here).  The indices of one call must be distinct."""
    n_rows, d, blocks, w = _whiten_check("whiten_bwd", x, rows)
    _lib._dev(mean, winv, dy)
    if tuple(mean.shape) != (blocks, d) or tuple(winv.shape) != (blocks, d, d) or tuple(dy.shape) != (blocks * w, d) or not (mean.is_contiguous() and winv.is_contiguous() and dy.is_contiguous()):
        raise _lib.SsvError(f"whiten_bwd: contiguous mean [{blocks}, {d}], winv [{blocks}, {d}, {d}] and dy [{blocks * w}, {d}] expected")
    if dx is None:
        dx = torch.zeros_like(x) if blocks * w < n_rows else torch.empty_like(x)
    ws = workspace.get(_lib.load().ssv_whiten_workspace_bytes(blocks, w, d), x.device)
    call("ssv_whiten_bwd", blocks, w, d, n_rows, ptr(x), ptr(rows), float(eps), ptr(mean), ptr(winv), ptr(dy), ptr(dx), ptr(ws), ws.numel(), stream())
    return dx


def wmse_perm(n, views, iters, seed, step=0, step_dev=None, device=None):
    """int32 [iters, views, n]: per iteration a permutation of 0 .. n - 1 (positions sorted by their Philox draw keyed by (seed, step, iteration)), view v offset
    by v * n.  ``step_dev`` (an int64 device tensor of one element) replaces ``step`` and is advanced by one behind the launch."""
    device = step_dev.device if step_dev is not None else device
    if step_dev is not None and (step_dev.dtype != torch.int64 or step_dev.numel() != 1):
        raise _lib.SsvError("wmse_perm: step_dev must be an int64 tensor of one element")
    perm = torch.empty((int(iters), int(views), int(n)), dtype=torch.int32, device=device)
    _lib._dev(perm)
    call("ssv_wmse_perm", int(n), int(views), int(iters), int(seed), int(step), ptr(step_dev), ptr(perm), stream())
    return perm


# ------------------------------------------------------------------------------------------- PCL's piece: the fused ProtoNCE loss (csrc/protonce.hip)
def proto_nce_route(d):
    """"fused" or "unfused": the route ssv_proto_nce takes at width d under the current arithmetic (include/ssv_hip.h: ssv_proto_nce, `arithmetic`); the benchmark
    (tools/bench_pcl.py) found no shape at which the fused route loses, so nothing else enters the choice"""
    return "fused" if ARITHMETIC == "bf16x3" and d % 32 == 0 and d <= _lib.PROTO_NCE_FUSED_MAX_D else "unfused"


def proto_nce(q, protos, inv_phi, labels, seg_end):
    """(loss 0-d, lse [segs, m], dq [m, d], flag int32 [1]) of the ProtoNCE term: q [m, d] against the prototypes protos [ktot, d], cut by the python ints
    ``seg_end`` into segments (one clustering each), with scores (q . c_j) * inv_phi[j] and labels [segs, m] int32 naming every query's prototype INSIDE each
    segment: loss = 1 / segs * sum_s mean_i (lse[s, i] - s_iy), dq = d loss / dq (include/ssv_hip.h: ssv_proto_nce).  flag: bit 0 a label outside its segment,
    bit 1 an inv_phi that is not finite and positive - left on the device for the caller to read when it chooses.  Contiguous device tensors, d % 4 == 0,
    m <= 8192, at most 8 segments.  Only enqueues: no host synchronisation, capturable in a step graph."""
    _lib._dev(q, protos, inv_phi, labels)
    if q.dim() != 2 or protos.dim() != 2 or q.dtype != torch.float32 or protos.dtype != torch.float32 or inv_phi.dtype != torch.float32 or labels.dtype != torch.int32:
        raise _lib.SsvError(f"proto_nce: fp32 q [m, d], protos [ktot, d], inv_phi [ktot] and int32 labels [segs, m] expected (got {tuple(q.shape)} {q.dtype}, "
                            f"{tuple(protos.shape)} {protos.dtype}, {tuple(inv_phi.shape)} {inv_phi.dtype}, {tuple(labels.shape)} {labels.dtype})")
    if not (q.is_contiguous() and protos.is_contiguous() and inv_phi.is_contiguous() and labels.is_contiguous()):
        raise _lib.SsvError("proto_nce: q, protos, inv_phi and labels must be contiguous")
    ends = [int(e) for e in seg_end]
    (m, d), (rows, dc), segs = q.shape, protos.shape, len(ends)
    if not 1 <= segs <= _lib.PROTO_NCE_MAX_SEGS or any(b <= a for a, b in zip([0] + ends, ends)) or ends[-1] > rows:
        raise _lib.SsvError(f"proto_nce: seg_end must hold 1 to {_lib.PROTO_NCE_MAX_SEGS} strictly increasing positive row counts within the {rows} prototypes (got {ends})")
    ktot = ends[-1]
    if dc != d or d < 4 or d % 4 or d > _lib.KNN_MAX_D or not 1 <= m <= _lib.PROTO_NCE_MAX_M:
        raise _lib.SsvError(f"proto_nce: q has {d} columns, the prototypes {dc}; d % 4 == 0, 4 <= d <= {_lib.KNN_MAX_D} and 1 <= m <= {_lib.PROTO_NCE_MAX_M} (got m = {m})")
    if inv_phi.dim() != 1 or inv_phi.numel() < ktot or tuple(labels.shape) != (segs, m):
        raise _lib.SsvError(f"proto_nce: inv_phi [>= {ktot}] and labels [{segs}, {m}] expected (got {tuple(inv_phi.shape)}, {tuple(labels.shape)})")
    arith = _arith_code()
    ws = workspace.get(max(_lib.load().ssv_proto_nce_workspace_bytes(m, ktot, d, segs, arith), 16), q.device)
    loss = torch.empty((1,), dtype=torch.float32, device=q.device)
    lse = torch.empty((segs, m), dtype=torch.float32, device=q.device)
    dq = torch.empty((m, d), dtype=torch.float32, device=q.device)
    flag = torch.empty(1, dtype=torch.int32, device=q.device)
    call("ssv_proto_nce", m, d, segs, (C.c_int64 * segs)(*ends), ptr(q), ptr(protos), ptr(inv_phi), ptr(labels), ptr(loss), ptr(lse), ptr(dq), ptr(flag), arith,
         ptr(ws), ws.numel(), stream())
    return loss.view(()), lse, dq, flag


def check_proto_nce_flag(flag):
    """Reads the flag of a proto_nce call (one host synchronisation) and raises SsvError for what it reports."""
    bits = 0 if flag is None else int(flag.item())
    if bits & 1:
        raise _lib.SsvError("proto_nce: a label lies outside its segment of prototypes")
    if bits & 2:
        raise _lib.SsvError("proto_nce: an inverse concentration is not finite and positive")


# ------------------------------------------------------------------------------------------- DenseCL's pieces: the dense matching and the queue InfoNCE (csrc/densecl.hip)
def dense_match(f1, f2, eps=1e-12):
    """(idx int32 [b, s], sim [b, s]) of two backbone feature maps f1, f2 [b, ..., c] (NHWC maps, or [b, s, c] rows): for every cell of f1 the cell of f2 of the same
    image with the largest f1 . f2 / max(|f2|, eps), lowest cell among equal scores, as the row n * s + j of the [b * s, d] key grid, and the cosine of the pair
    (include/ssv_hip.h: ssv_dense_match).  At most 256 cells per image, c % 4 == 0.  Only enqueues: no host synchronisation, capturable in a step graph."""
    _lib._dev(f1, f2)
    if f1.dim() < 3 or f1.shape != f2.shape or f1.dtype != torch.float32 or f2.dtype != torch.float32 or not (f1.is_contiguous() and f2.is_contiguous()):
        raise _lib.SsvError(f"dense_match: two contiguous fp32 maps of one shape [b, ..., c] expected (got {tuple(f1.shape)} {f1.dtype}, {tuple(f2.shape)} {f2.dtype})")
    b, c = f1.shape[0], f1.shape[-1]
    s = f1.numel() // max(b * c, 1)
    if b < 1 or not 1 <= s <= _lib.DENSE_MATCH_MAX_S or c < 4 or c % 4 or c > _lib.DENSE_MATCH_MAX_C:
        raise _lib.SsvError(f"dense_match: need 1 <= cells <= {_lib.DENSE_MATCH_MAX_S}, c % 4 == 0 and 4 <= c <= {_lib.DENSE_MATCH_MAX_C} (got b = {b}, cells = {s}, c = {c})")
    idx = torch.empty((b, s), dtype=torch.int32, device=f1.device)
    sim = _empty((b, s), f1)
    call("ssv_dense_match", b, s, c, ptr(f1), ptr(f2), float(eps), ptr(idx), ptr(sim), _arith_code(), stream())
    return idx, sim


def queue_nce_route(d):
    """"fused" or "unfused": the route ssv_queue_nce takes at width d under the current arithmetic (include/ssv_hip.h: ssv_queue_nce, `arithmetic`)"""
    return "fused" if ARITHMETIC == "bf16x3" and d % 32 == 0 and d <= _lib.QUEUE_NCE_FUSED_MAX_D else "unfused"


def queue_nce(q, keys, pos, bank, K, inv_temp):
    """(loss 0-d, lse [m], dq [m, d], flag int32 [1]) of InfoNCE against a queue with one gathered positive per query: q [m, d] (normalised by the caller), the
    positive of query i is keys[pos[i]] (keys [mk, d], pos int32 [m]), the negatives are the first ``K`` rows of bank [>= K, d], every score times ``inv_temp``
    (include/ssv_hip.h: ssv_queue_nce).  flag bit 0: a pos outside [0, mk) - left on the device for the caller to read when it chooses.  Contiguous device
    tensors, d % 4 == 0, m <= 131072.  Only enqueues: no host synchronisation, capturable in a step graph."""
    _lib._dev(q, keys, pos, bank)
    if (q.dim() != 2 or keys.dim() != 2 or bank.dim() != 2 or pos.dim() != 1 or q.dtype != torch.float32 or keys.dtype != torch.float32
            or bank.dtype != torch.float32 or pos.dtype != torch.int32):
        raise _lib.SsvError(f"queue_nce: fp32 q [m, d], keys [mk, d], bank [>= K, d] and int32 pos [m] expected (got {tuple(q.shape)} {q.dtype}, {tuple(keys.shape)} "
                            f"{keys.dtype}, {tuple(bank.shape)} {bank.dtype}, {tuple(pos.shape)} {pos.dtype})")
    if not (q.is_contiguous() and keys.is_contiguous() and pos.is_contiguous() and bank.is_contiguous()):
        raise _lib.SsvError("queue_nce: q, keys, pos and bank must be contiguous")
    (m, d), (mk, dk), (rows, db), K = q.shape, keys.shape, bank.shape, int(K)
    if dk != d or db != d or d < 4 or d % 4 or d > _lib.KNN_MAX_D or not 1 <= m <= _lib.QUEUE_NCE_MAX_M or mk < 1 or pos.shape[0] != m:
        raise _lib.SsvError(f"queue_nce: q, keys and bank must share d columns, d % 4 == 0, 4 <= d <= {_lib.KNN_MAX_D}, 1 <= m <= {_lib.QUEUE_NCE_MAX_M}, pos [m] "
                            f"(got q {tuple(q.shape)}, keys {tuple(keys.shape)}, bank {tuple(bank.shape)}, pos {tuple(pos.shape)})")
    if not 1 <= K <= rows:
        raise _lib.SsvError(f"queue_nce: K must lie in [1, {rows} rows of the bank] (got {K})")
    if not (float(inv_temp) > 0.0 and float(inv_temp) < float("inf")):
        raise _lib.SsvError(f"queue_nce: inv_temp must be finite and positive (got {inv_temp})")
    arith = _arith_code()
    ws = workspace.get(max(_lib.load().ssv_queue_nce_workspace_bytes(m, K, d, arith), 16), q.device)
    loss = torch.empty((1,), dtype=torch.float32, device=q.device)
    lse = torch.empty((m,), dtype=torch.float32, device=q.device)
    dq = torch.empty((m, d), dtype=torch.float32, device=q.device)
    flag = torch.empty(1, dtype=torch.int32, device=q.device)
    call("ssv_queue_nce", m, d, K, mk, ptr(q), ptr(keys), ptr(pos), ptr(bank), float(inv_temp), ptr(loss), ptr(lse), ptr(dq), ptr(flag), arith, ptr(ws), ws.numel(),
         stream())
    return loss.view(()), lse, dq, flag


def check_queue_nce_flag(flag):
    """Reads the flag of a queue_nce call (one host synchronisation) and raises SsvError for what it reports."""
    bits = 0 if flag is None else int(flag.item())
    if bits & 1:
        raise _lib.SsvError("queue_nce: a positive's index lies outside the key grid")


# ------------------------------------------------------------------------------------------- ViT / DINO pieces
LN_EPS = 1e-5
ATTENTION_BF16X3 = True      # the attention forward's two products in the bf16x3 arithmetic when ops.ARITHMETIC says so (the backward stays on the fp32 instruction)


def layernorm_fwd(x, gamma, beta, addend=None, eps=LN_EPS):
    """y = LayerNorm(x) * gamma + beta (+ addend) over the last axis of a dense [M, C] matrix; returns (y, mean, invstd)."""
    _lib._dev(x, gamma, beta, addend)
    m, c = _rows(x)
    y = torch.empty_like(x)
    mean, invstd = _empty((m,), x), _empty((m,), x)
    call("ssv_layernorm_fwd", m, c, ptr(x), ptr(gamma), ptr(beta), ptr(addend), float(eps), ptr(y), ptr(mean), ptr(invstd), stream())
    return y, mean, invstd


def layernorm_bwd(dy, x, gamma, mean, invstd, dgamma, dbeta, dx_addend=None, accumulate=True):
    _lib._dev(dy, x, dx_addend)
    m, c = _rows(x)
    dx = dx_addend if dx_addend is not None else torch.empty_like(x)      # in-place accumulate into the addend when given
    ws = workspace.get(_lib.load().ssv_layernorm_workspace_bytes(m, c), x.device)
    call("ssv_layernorm_bwd", m, c, ptr(dy), ptr(x), ptr(gamma), ptr(mean), ptr(invstd), ptr(dx_addend), ptr(dx), ptr(dgamma), ptr(dbeta),
         int(accumulate), ptr(ws), ws.numel(), stream())
    return dx


def gelu_fwd(x):
    _lib._dev(x)
    y = torch.empty_like(x)
    call("ssv_gelu_fwd", x.numel(), ptr(x), ptr(y), stream())
    return y


def gelu_bwd(x, dy):
    _lib._dev(x, dy)
    dx = torch.empty_like(x)
    call("ssv_gelu_bwd", x.numel(), ptr(x), ptr(dy), ptr(dx), stream())
    return dx


def _ld(t):
    if t.dim() != 2 or t.stride(1) != 1:
        raise _lib.SsvError("attention operands must be [M, heads*dh] matrices with unit column stride")
    return t.stride(0)


def attention_fwd(q, k, v, batch, tokens, heads):
    """softmax(q k^T / sqrt(dh)) v per (image, head); q/k/v: [batch*tokens, heads*dh] (may be column slices of one matrix)."""
    _lib._dev(q, k, v)
    hid = q.shape[1]
    dh = hid // heads
    if not (_ld(q) == _ld(k) == _ld(v)):
        raise _lib.SsvError("attention: q, k, v must share one row stride")
    o = torch.empty((batch * tokens, hid), dtype=torch.float32, device=q.device)
    lse = torch.empty((batch, heads, tokens), dtype=torch.float32, device=q.device)
    call("ssv_attention_fwd_arith", batch, tokens, heads, dh, ptr(q), ptr(k), ptr(v), _ld(q), dh ** -0.5, ptr(o), hid, ptr(lse),
         _lib.ARITH_BF16X3 if (ARITHMETIC == "bf16x3" and ATTENTION_BF16X3) else _lib.ARITH_F32_MFMA, stream())
    return o, lse


def attention_bwd(q, k, v, o, dout, lse, batch, tokens, heads, out=None):
    """Returns (dq, dk, dv); with ``out`` = a [M, 3*hidden] matrix they are its three column blocks."""
    _lib._dev(q, k, v, o, dout, lse)
    hid = q.shape[1]
    dh = hid // heads
    if out is None:
        dq, dk, dv = (torch.empty((batch * tokens, hid), dtype=torch.float32, device=q.device) for _ in range(3))
    else:
        dq, dk, dv = out[:, :hid], out[:, hid:2 * hid], out[:, 2 * hid:]
    delta = torch.empty_like(lse)
    call("ssv_attention_bwd", batch, tokens, heads, dh, ptr(q), ptr(k), ptr(v), _ld(q), dh ** -0.5, ptr(o), ptr(dout), _ld(o), ptr(lse),
         ptr(delta), ptr(dq), ptr(dk), ptr(dv), _ld(dq), stream())
    return dq, dk, dv


def vit_embed_fwd(img_nhwc, cls, pos, patch):
    """[B,H,W,3] image -> token matrix [B*T, 3*patch^2 + E] (cls row first, positional embedding concatenated)."""
    _lib._dev(img_nhwc, cls, pos)
    b, h, w, _ = img_nhwc.shape
    e = pos.shape[1]
    t = (h // patch) * (w // patch) + 1
    if t > pos.shape[0]:
        raise _lib.SsvError(f"vit_embed: {t} tokens but only {pos.shape[0]} positional embeddings")
    tok = torch.empty((b * t, 3 * patch * patch + e), dtype=torch.float32, device=img_nhwc.device)
    call("ssv_vit_embed_fwd", b, h, w, patch, e, ptr(img_nhwc), ptr(cls), ptr(pos), ptr(tok), stream())
    return tok, t


def vit_embed_bwd(dtok, batch, tokens, p3, e, dcls, dpos, accumulate=True):
    _lib._dev(dtok, dcls, dpos)
    call("ssv_vit_embed_bwd", batch, tokens, p3, e, ptr(dtok), ptr(dcls), ptr(dpos), int(accumulate), stream())


def weightnorm_fwd(g, v):
    _lib._dev(g, v)
    w = torch.empty_like(v)
    inv = _empty((v.shape[0],), v)
    call("ssv_weightnorm_fwd", v.shape[0], v.shape[1], ptr(g), ptr(v), ptr(w), ptr(inv), stream())
    return w, inv


def weightnorm_bwd(dw, g, v, inv, dg, dv, accumulate=True):
    _lib._dev(dw, g, v, inv, dg, dv)
    call("ssv_weightnorm_bwd", v.shape[0], v.shape[1], ptr(dw), ptr(g), ptr(v), ptr(inv), ptr(dg), ptr(dv), int(accumulate), stream())


def dino_loss(teacher, student, center, temp_s, temp_t, weight, loss, accumulate):
    """teacher [bs,2,K], student [bs,V,K] (dense), center [K]; loss (0-d device tensor) (+)= weighted loss; returns dstudent."""
    _lib._dev(teacher, student, center, loss)
    bs, v, k = student.shape
    if tuple(teacher.shape) != (bs, 2, k) or center.numel() != k:
        raise _lib.SsvError(f"dino_loss: teacher {tuple(teacher.shape)} / center {tuple(center.shape)} do not match student {tuple(student.shape)}")
    d = torch.empty_like(student)
    ws = workspace.get(_lib.load().ssv_dino_loss_workspace_bytes(bs, v, k), student.device)
    call("ssv_dino_loss", bs, v, k, ptr(teacher), ptr(student), ptr(center), float(temp_s), float(temp_t), float(weight), ptr(loss),
         int(accumulate), ptr(d), ptr(ws), ws.numel(), stream())
    return d


def dino_center_update(center, t1, t2, momentum):
    _lib._dev(center, t1, t2)
    k = center.numel()
    call("ssv_dino_center_update", k, t1.numel() // k, ptr(t1), 0 if t2 is None else t2.numel() // k, ptr(t2), float(momentum), ptr(center), stream())
    return center


def multicrop_params(batch, hs, ws_, ncrop, view_base, scale, seed, step, sample_ids=None, sample0=0, device=None):
    boxes = torch.empty((batch, ncrop, 4), dtype=torch.int32, device=device if sample_ids is None else sample_ids.device)
    call("ssv_multicrop_params", batch, hs, ws_, ncrop, view_base, float(scale[0]), float(scale[1]), int(seed), int(step), ptr(sample_ids),
         int(sample0), ptr(boxes), stream())
    return boxes


def multicrop(views_nhwc, boxes, size):
    """views [B,Hs,Ws,3] float, boxes [B,ncrop,4] int32 -> [B,ncrop,Ho,Wo,3] (crop + bicubic resize)."""
    _lib._dev(views_nhwc, boxes)
    b, hs, ws_, _ = views_nhwc.shape
    ncrop = boxes.shape[1]
    out = torch.empty((b, ncrop, size[0], size[1], 3), dtype=torch.float32, device=views_nhwc.device)
    call("ssv_multicrop", b, hs, ws_, ptr(views_nhwc), ncrop, ptr(boxes), size[0], size[1], ptr(out), stream())
    return out


# ------------------------------------------------------------------------------------------- sibling algorithms' losses
def negdot_pair(o1, o2, t1, t2, scale):
    """loss = -scale * (sum o1*t2 + sum o2*t1); returns (loss 0-d, dloss/do1, dloss/do2)."""
    _lib._dev(o1, o2, t1, t2)
    n = o1.numel()
    do1, do2 = torch.empty_like(o1), torch.empty_like(o2)
    loss = torch.empty((), dtype=torch.float32, device=o1.device)
    ws = workspace.get(_lib.load().ssv_reduce_workspace_bytes(n), o1.device)
    call("ssv_negdot_pair_fwd_bwd", n, ptr(o1), ptr(o2), ptr(t1), ptr(t2), float(scale), ptr(loss), ptr(do1), ptr(do2), ptr(ws), ws.numel(), stream())
    return loss, do1, do2


def relic_kl(zi, zj, zo, inv_temp, alpha):
    """ReLIC invariance term on dense [N,D] matrices; returns (alpha * kl as a 0-d tensor, dzi, dzj, dzo)."""
    _lib._dev(zi, zj, zo)
    n, d = zi.shape
    loss = torch.empty((), dtype=torch.float32, device=zi.device)
    dzi, dzj, dzo = torch.empty_like(zi), torch.empty_like(zj), torch.empty_like(zo)
    ws = workspace.get(_lib.load().ssv_relic_kl_workspace_bytes(n), zi.device)
    call("ssv_relic_kl_fwd_bwd", n, d, ptr(zi), ptr(zj), ptr(zo), float(inv_temp), float(alpha), ptr(loss), 0, ptr(dzi), ptr(dzj), ptr(dzo),
         ptr(ws), ws.numel(), stream())
    return loss, dzi, dzj, dzo


def moco_loss(q, k, neg, queue_size, inv_temp):
    """q, k [N,D] (already normalised if the loss normalises), neg [N, ldk] = q bank^T; neg is overwritten by dloss/dneg.
    Returns (loss 0-d, dq_init [N,D])."""
    _lib._dev(q, k, neg)
    n, d = q.shape
    loss = torch.empty((), dtype=torch.float32, device=q.device)
    dq = torch.empty_like(q)
    ws = workspace.get(n * 8, q.device)
    call("ssv_moco_loss_fwd_bwd", n, d, int(queue_size), neg.shape[1], ptr(q), ptr(k), ptr(neg), float(inv_temp), ptr(loss), ptr(dq), ptr(ws), ws.numel(), stream())
    return loss, dq


def queue_push(bank, queue_size, pointer, keys, eps=1e-12):
    """bank[(pointer + i) % queue_size] = normalize(keys[i]); returns the new pointer."""
    _lib._dev(bank, keys)
    invalidate_weight_caches()                        # the bank is a GEMM operand whose transposed image may be cached
    call("ssv_queue_push", int(queue_size), bank.shape[1], ptr(bank), int(pointer), keys.shape[0], ptr(keys), float(eps), stream())
    return (pointer + keys.shape[0]) % queue_size


def queue_push_counted(bank, queue_size, pointer_dev, keys, eps=1e-12):
    """queue_push with the pointer in device memory (an int32 tensor of one element, advanced by the call): what a replayed step needs."""
    _lib._dev(bank, keys, pointer_dev)
    invalidate_weight_caches()
    call("ssv_queue_push_counted", int(queue_size), bank.shape[1], ptr(bank), ptr(pointer_dev), keys.shape[0], ptr(keys), float(eps), stream())


# K splits of the PIRL loss kernel: None = the library's choice (ssv_pirl_default_splits), an integer forces it (diagnostic switch, set from Python: 1 = every row
# block sweeps all negatives in one workgroup, 64 = the most the kernel takes; the library clamps it to the number of 32-negative tiles)
PIRL_SPLITS = None


def pirl_splits():
    return 0 if PIRL_SPLITS is None else max(1, min(int(PIRL_SPLITS), 64))


def pirl_loss(bank, pos_index, neg_index, img_features, patch_features, normalize, inv_temp, loss_weight, splits=None):
    """PirlLoss forward + backward against the device bank [N, D], read by index (int64 [B] positives, int64 [K] negatives).
    Returns (loss 0-d, d img_features, d patch_features, flag): flag is a one-element int32 tensor, non-zero when an index fell outside [0, N) -
    check_pirl_flag turns it into an error."""
    _lib._dev(bank, pos_index, neg_index, img_features, patch_features)
    if pos_index.dtype != torch.int64 or neg_index.dtype != torch.int64:
        raise _lib.SsvError("pirl_loss: indices must be int64")
    b, d = img_features.shape
    if patch_features.shape != img_features.shape or bank.dim() != 2 or bank.shape[1] != d or pos_index.numel() != b or not bank.is_contiguous():
        raise _lib.SsvError(f"pirl_loss: features {tuple(img_features.shape)} / {tuple(patch_features.shape)}, bank {tuple(bank.shape)}, {pos_index.numel()} positives do not fit together")
    splits = pirl_splits() if splits is None else int(splits)
    loss = torch.empty((), dtype=torch.float32, device=bank.device)
    dimg, dpatch = torch.empty_like(img_features), torch.empty_like(patch_features)
    ws = workspace.get(_lib.load().ssv_pirl_loss_workspace_bytes(b, 64), bank.device)
    call("ssv_pirl_loss_fwd_bwd", bank.shape[0], d, b, neg_index.numel(), ptr(bank), ptr(pos_index), ptr(neg_index), ptr(img_features), ptr(patch_features),
         int(bool(normalize)), float(inv_temp), float(loss_weight), splits, ptr(loss), ptr(dimg), ptr(dpatch), ptr(ws), ws.numel(), stream())
    return loss, dimg, dpatch, ws[:4].view(torch.int32).clone()         # the workspace is reused by the next call: the flag word leaves it now


def check_pirl_flag(flag):
    if int(flag.item()) != 0:
        raise _lib.SsvError("pirl_loss: a positive or negative index lies outside the memory bank (the entry was left out of the loss)")


def bank_momentum_update(bank, index, z, momentum, eps=1e-12):
    """bank[index[i]] = momentum * bank[index[i]] + (1 - momentum) * z[i] / max(|z[i]|, eps); the indices of one call are distinct."""
    _lib._dev(bank, index, z)
    if index.dtype != torch.int64 or z.shape != (index.numel(), bank.shape[1]) or not (bank.is_contiguous() and z.is_contiguous()):
        raise _lib.SsvError(f"bank_momentum_update: int64 [n] indices and dense [n, {bank.shape[1]}] features expected")
    call("ssv_bank_momentum_update", bank.shape[0], bank.shape[1], ptr(bank), index.numel(), ptr(index), ptr(z), float(momentum), float(eps), stream())
    return bank


def patch_split(x, patch):
    """[B,C,H,W] (NCHW or channels_last) -> [P,B,C,patch,patch], every patch[p] a channels_last batch of its own (what the encoders take without a copy);
    p = xi * (H / patch) + yi - the reference's loop order (models/pirl.py:67-71)."""
    nhwc = nchw_to_nhwc(x)
    b, h, w, c = nhwc.shape
    if h % patch or w % patch:
        raise _lib.SsvError(f"patch_split: {patch} does not divide {h} x {w}")
    out = _empty(((h // patch) * (w // patch), b, patch, patch, c), nhwc)
    call("ssv_patch_split", b, h, w, c, int(patch), ptr(nhwc), ptr(out), stream())
    return out.permute(0, 1, 4, 2, 3)


def linear_gelu_fwd(x, w, bias, keep_h=True):
    """(h, gelu(h)) with h = x w^T + bias, both written by one GEMM epilogue.  x [M, C] dense, w [K, C].  ``keep_h`` False (a forward without
    a backward): only gelu(h) is written and h comes back as None."""
    _lib._dev(x, w, bias)
    m, c = x.shape
    w, wshape = _ohwi(w)
    d = conv_desc((m, 1, 1, c), wshape, 1, 0, w=w)
    act = _empty((m, wshape[0]), x)
    h = torch.empty_like(act) if keep_h else None
    call("ssv_linear_gelu_fwd", C.byref(d), ptr(x), ptr(w), ptr(bias), ptr(h), ptr(act), stream())
    return h, act


LINEAR_GELUGRAD_ON_FWD = os.environ.get("SSV_NO_GELUGRAD_FWD_KERNEL", "0") != "1"     # diagnostic switch: fc2's data gradient on the dgrad kernel
GELU_DACT_IN_FWD = os.environ.get("SSV_NO_GELU_DACT", "0") != "1"      # diagnostic switch: the forward keeps the pre-activation and the backward epilogue evaluates gelu' (rounds 1-3)


def can_gelu_dact(w1_shape, w2_shape):
    """fc1 [inter, din] / fc2 [dout, inter] shapes for which the forward can write gelu'(h) and the backward multiply by it on the forward kernel."""
    inter, dout = w1_shape[0], w2_shape[0]
    return GELU_DACT_IN_FWD and LINEAR_GELUGRAD_ON_FWD and dout % 32 == 0 and inter % 4 == 0 and inter >= 128


def linear_gelu_fwd_dact(x, w, bias):
    """(gelu'(h), gelu(h)) with h = x w^T + bias, both written by one GEMM epilogue: the derivative is taken where the cdf is at hand."""
    _lib._dev(x, w, bias)
    m, c = x.shape
    w, wshape = _ohwi(w)
    d = conv_desc((m, 1, 1, c), wshape, 1, 0, w=w)
    act = _empty((m, wshape[0]), x)
    dact = torch.empty_like(act)
    call("ssv_linear_gelu_fwd_dact", C.byref(d), ptr(x), ptr(w), ptr(bias), ptr(dact), ptr(act), stream())
    return dact, act


def linear_dgrad_mul(dy, w, dact, addend=None, out=None):
    """dh = (dy w) * dact (+ addend) with dact = gelu'(h) from linear_gelu_fwd_dact: the forward kernel on the transposed weights."""
    _lib._dev(dy, w, dact, addend)
    m = dy.shape[0]
    w, wshape = _ohwi(w)
    k, c = wshape[0], wshape[1]
    dh = out if out is not None else torch.empty_like(dact)
    wt = _transposed_filter(w, wshape)
    dt = conv_desc((m, 1, 1, k), (c, k, 1, 1), 1, 0, w=wt)
    call("ssv_linear_fwd_mulgrad", C.byref(dt), ptr(dy), ptr(wt), ptr(dact), ptr(addend), ptr(dh), stream())
    return dh


def linear_dgrad_gelu(dy, w, h, addend=None, out=None):
    """dh = (dy w) * gelu'(h) (+ addend): the backward of `gelu(h) -> Linear(w)` down to the pre-activation, in the dgrad epilogue."""
    _lib._dev(dy, w, h, addend)
    m = dy.shape[0]
    w, wshape = _ohwi(w)
    d = conv_desc((m, 1, 1, wshape[1]), wshape, 1, 0)
    dh = out if out is not None else torch.empty_like(h)
    k, c = wshape[0], wshape[1]
    if LINEAR_GELUGRAD_ON_FWD and k % 32 == 0 and c % 4 == 0 and c >= 128:
        # forward kernel on the transposed weights (cached per step like every stride-1 data gradient's): both operands k-contiguous rows
        wt = _transposed_filter(w, wshape)
        dt = conv_desc((m, 1, 1, k), (c, k, 1, 1), 1, 0, w=wt)
        call("ssv_linear_fwd_gelugrad", C.byref(dt), ptr(dy), ptr(wt), ptr(h), ptr(addend), ptr(dh), stream())
        return dh
    call("ssv_conv2d_dgrad_gelu", C.byref(d), ptr(dy), ptr(w), ptr(h), ptr(addend), ptr(dh), stream())
    return dh


def group_expand(wg, groups):
    """Grouped filter bank [K, C/groups, R, S] (OHWI memory) -> dense block-diagonal [K, C, R, S] (OHWI memory)."""
    _lib._dev(wg)
    wg, (k, cg, r, s_) = _ohwi(wg)
    wd = torch.empty((k, cg * groups, r, s_), dtype=torch.float32, device=wg.device).contiguous(memory_format=torch.channels_last)
    call("ssv_group_expand", k, r, s_, cg, groups, ptr(wg), ptr(wd), stream())
    return wd


def group_extract(dwd, dwg, groups, accumulate=True):
    """dwg (+)= the block-diagonal part of the dense weight gradient dwd."""
    _lib._dev(dwd, dwg)
    _, (k, cg, r, s_) = _ohwi(dwg)
    call("ssv_group_extract", k, r, s_, cg, groups, ptr(dwd), ptr(dwg), int(accumulate), stream())
    return dwg


def pad_channels(t, channels):
    """Zero-pad the LAST axis of a dense tensor to `channels` (e.g. an NHWC image batch or an OHWI filter from 3 to 4 channels)."""
    _lib._dev(t)
    cin = t.shape[-1]
    out = torch.empty(t.shape[:-1] + (channels,), dtype=torch.float32, device=t.device)
    call("ssv_pad_channels", t.numel() // cin, cin, channels, ptr(t), ptr(out), 0, stream())
    return out


def unpad_channels(t, out, accumulate=True):
    """out (+)= the first out.shape[-1] channels of t (both dense, channel axis last)."""
    _lib._dev(t, out)
    call("ssv_pad_channels", t.numel() // t.shape[-1], t.shape[-1], out.shape[-1], ptr(t), ptr(out), int(accumulate), stream())
    return out


# ------------------------------------------------------------------------------------------- Winograd F(2x2, 3x3) and F(4x4, 3x3)
class _WinoForm:
    """What the drivers of the two forms differ in: the transformed-domain positions, the names (the note's tag, the library's symbols: formed once, the drivers
    run in the launch-bound regime) and whether ssv_<prefix>groups takes the statistics flag (F(4x4) groups by row of tiles or by image, F(2x2) always by 16 tiles)."""

    def __init__(self, tag, prefix, positions, groups_takes_stats):
        self.positions, self.groups_takes_stats = positions, groups_takes_stats
        self.note_fwd, self.note_dgrad, self.note_wgrad = tag + "_fwd", tag + "_dgrad", tag + "_wgrad"
        self.sym_tiles, self.sym_groups, self.sym_rows_per_group = prefix + "tiles", prefix + "groups", prefix + "stats_rows_per_group"
        self.filter_transform, self.filter_grad = prefix + "filter_transform", prefix + "filter_grad"
        self.input_transform, self.output_transform = prefix + "input_transform", prefix + "output_transform"

    def tiles(self, n, h, w_):
        return int(getattr(_lib.load(), self.sym_tiles)(n, h, w_))

    def groups(self, n, h, w_, stats):
        fn = getattr(_lib.load(), self.sym_groups)
        return int(fn(n, h, w_, int(stats)) if self.groups_takes_stats else fn(n, h, w_))


_F22, _F44 = _WinoForm("wino22", "ssv_wino_", 16, False), _WinoForm("wino44", "ssv_wino44_", 36, True)


def _wino_filter(w, wshape, transposed=False, form=_F22):
    """U = G g G^T of the filter [K][3][3][C] (16 or 36 positions) - or, ``transposed``, of the rotated filter with the channel roles swapped (data gradient)."""
    key = (w.data_ptr(), stream(), wshape, transposed, form.positions, w._version)      # the version as _transposed_filter: an edited filter must miss
    hit = _WINO_U.get(key)
    if hit is not None:
        return hit[1]
    k, c, _, _ = wshape
    src, kk, cc = (w, k, c) if not transposed else (_transposed_filter(w, wshape), c, k)
    u = torch.empty((form.positions, kk, cc), dtype=torch.float32, device=w.device)
    call(form.filter_transform, kk, cc, ptr(src), ptr(u), stream())
    _WINO_U[key] = (w.untyped_storage(), u)
    return u


WINOGRAD = os.environ.get("SSV_NO_WINOGRAD", "0") != "1"          # diagnostic switch: every 3x3 convolution on the direct implicit-GEMM kernels
# Measured at bs 512 (tools/probe_winograd.py, profiles/r03_probe_winograd.txt): 14x14 x 256 channels forward 1.50x, data gradient 1.62x, weight
# gradient 1.97x; 7x7 x 512: 1.76 / 1.73 / 1.72; 28x28 x 128: 1.13 / 1.10 / 1.54; 56x56 x 64: 0.79 / 0.71 (the transforms move 9x the tensors
# and that layer is HBM-heavy already) - so: at least 128 channels on both sides.
WINOGRAD_MIN_CHANNELS = int(os.environ.get("SSV_WINOGRAD_MIN_CHANNELS", "128"))
# Round 5: that verdict was F(2x2)'s.  With all three products on F(4x4) (2.25x instead of 4x transformed tensors, no second transformed input, one pass over dY) the
# 64-channel 3x3 layers of layer1 (56x56) win too: same-box A/B 215.9 -> 210.7 ms per step (profiles/r05_probe_wino64_step_ab.txt).  Narrower layers than
# WINOGRAD_MIN_CHANNELS therefore take Winograd from this width on - but only where F(4x4) is what runs (`_use_wino44`), never F(2x2).
# Round 6: on the bf16x3 arithmetic the direct product is 1.4x cheaper and the verdict flips back - the three 64-channel layers on the direct kernels: +0.5 % images/s
# and 707 -> 654 GB of HBM traffic per step (same box, alternating, profiles/r06_probe_wino_floor_traffic.txt; the 128-channel layers direct as well: 625 GB but
# -1.7 %).  Default therefore by arithmetic: 128 on bf16x3, 64 on fp32 MFMA; SSV_WINOGRAD44_MIN_CHANNELS=<n> overrides both.
WINOGRAD44_MIN_CHANNELS = int(os.environ["SSV_WINOGRAD44_MIN_CHANNELS"]) if os.environ.get("SSV_WINOGRAD44_MIN_CHANNELS") else None


def _wino44_min_channels():
    return WINOGRAD44_MIN_CHANNELS if WINOGRAD44_MIN_CHANNELS is not None else (128 if ARITHMETIC == "bf16x3" else 64)


WINOGRAD_MIN_TILES = int(os.environ.get("SSV_WINOGRAD_MIN_TILES", "256"))     # below that the three launches cost more than they save


def _lanes_ok(ch):
    return ch % 32 == 0 and ((ch // 4 <= 256 and 256 % (ch // 4) == 0) or (ch // 4) % 256 == 0)


def use_winograd(wshape, stride, pad, x_shape, want_stats):
    """Does this convolution run through F(2x2, 3x3)?  3x3 / stride 1 / padding 1, channel counts the transforms' lane mapping takes, enough
    tiles, every operand slice below the per-launch limit, and - when the statistics epilogue is wanted - a map that partitions evenly."""
    k, c, r, s_ = wshape
    if not (WINOGRAD and r == 3 and s_ == 3 and stride == 1 and pad == 1 and _lanes_ok(c) and _lanes_ok(k)):
        return False
    n, h, w_ = x_shape[0], x_shape[1], x_shape[2]
    if min(c, k) < WINOGRAD_MIN_CHANNELS:          # narrow layers: only where every product runs F(4x4) (forward / data / weight gradient share the 0.75 ratio rule)
        # (the forward's own ratio too: a narrow layer admitted on the data gradient's ratio alone would run its forward on F(2x2) when SSV_WINOGRAD44_FWD_RATIO is lowered)
        if not (min(c, k) >= _wino44_min_channels() and WINOGRAD44_WGRAD
                and _use_wino44(n, h, w_, c, k, min(WINOGRAD44_MAX_RATIO_FWD_NO_V2, WINOGRAD44_MAX_RATIO_DGRAD))):
            return False
    t = n * ((h + 1) // 2) * ((w_ + 1) // 2)
    if t < WINOGRAD_MIN_TILES or t * max(c, k) >= _MAX_ELEMS:
        return False
    return not want_stats or int(_lib.load().ssv_wino_stats_rows_per_group(n, h, w_)) > 0


# F(4x4, 3x3) for the forward and the data gradient of the Winograd layers (csrc/winograd44.hip; the weight gradient stays on F(2x2), whose operand the F(4x4) input
# transform leaves beside its own).  SSV_WINOGRAD44=0|1 overrides the shipped default.
WINOGRAD44 = os.environ.get("SSV_WINOGRAD44", "1") == "1"
# Which product takes F(4x4): by the transformed-domain work it leaves, 36 positions x tiles of 4 against 16 x tiles of 2 (0.5625 on maps that tile evenly - 28x28 -
# and on 7x7, where both tilings cover 8; 0.735 on 14x14, which F(2x2) tiles exactly and F(4x4) covers with 16).  The forward pays for writing both transformed
# inputs (its own and the weight gradient's), so it switches only when the work halves; the data gradient already wins at 0.735 (tools/probe/wino44_stages.py,
# profiles/r04_probe_wino44_stages.txt: 14x14 forward 1.07x, data gradient 1.28x; go / no-go bar 1.25x).
WINOGRAD44_MAX_RATIO_FWD, WINOGRAD44_MAX_RATIO_DGRAD = 0.6, 0.75
# Round 5: with the weight gradient on F(4x4) too (WINOGRAD44_WGRAD) the forward no longer writes the second, F(2x2) transformed input - its input transform drops from
# 0.209 to 0.133 ms on 14x14 x 256 - and the weight gradient it feeds is 0.485 instead of 0.548 ms: the forward then switches at the data gradient's ratio
# (14x14: 0.70 -> 0.57 ms forward; profiles/r05_probe_winograd44_wgrad.txt, r04_probe_wino44_stages.txt).
WINOGRAD44_MAX_RATIO_FWD_NO_V2 = float(os.environ.get("SSV_WINOGRAD44_FWD_RATIO", "0.75"))
# ... and only up to the contraction length the numerics bar was measured for: the transformed-domain sums run over the channels and F(4x4)'s error grows with
# their count like any fp32 sum, but from a 3x higher base - 128 / 256 / 512 channels: 2.97x / 2.84x / 2.85x the direct kernel's error against fp64 (bar: 3x),
# 1024 channels (wide_resnet's layer4): 3.8x.  Wider layers stay on F(2x2).
WINOGRAD44_MAX_CHANNELS = 512
# ... and only for launches with enough tiles: 36 small GEMMs of a few row tiles each buy nothing over 16 (B = 64: 7x7 x 512, 256 tiles: 0.109 vs 0.116 ms) while
# the larger rounding error stays - small batches keep F(2x2)
WINOGRAD44_MIN_TILES = int(os.environ.get("SSV_WINOGRAD44_MIN_TILES", "1024"))
# The weight gradient of a layer whose FORWARD ran F(4x4) takes F(4x4) too (round 5): its operand is the V the forward's input transform wrote anyway (no second,
# F(2x2) transformed input), 36 products over a quarter of the tiles, a 2.25x dY transform.  Error against fp64 1.1 - 1.6e-6 relative (bar 2e-6: a weight gradient's
# error never crosses a ReLU gate).  SSV_WINOGRAD44_WGRAD=0: those layers keep the F(2x2) operand and weight gradient (round 4's selection).
WINOGRAD44_WGRAD = os.environ.get("SSV_WINOGRAD44_WGRAD", "1") == "1"
# ... with BLOCKED accumulation of its 36 transformed-domain sums: fp32 chains of at most this many tiles, the chunks folded in fp64 (ssv_gemm_batched_wgrad_blocked);
# 0 = the plain split (diagnostic: how the error grows with the chain length)
WINOGRAD44_WGRAD_CHUNK = int(os.environ.get("SSV_WINOGRAD44_WGRAD_CHUNK", "512"))
# ... or / and inside the kernel: the MFMA accumulators flushed into a second register set every 128 tiles (0 = off)
WINOGRAD44_WGRAD_FLUSH = int(os.environ.get("SSV_WINOGRAD44_WGRAD_FLUSH", "128"))
WINOGRAD44_WGRAD_FLUSH_BF16X3 = 0
# The backward of such a layer reads its output gradient ONCE: the weight gradient's dY transform also writes the data gradient's transformed input
# (ssv_wino44_dy_transform_both; the data gradient that follows picks it up), and behind a fused input chain the output gradient is never written at all - the
# BatchNorm backward hands over (g, x, coefficients) as a LazyGrad and the transform forms it on load (`wino44_lazy_dy_ok`).  SSV_WINOGRAD44_DY_BOTH=0: separate passes.
WINOGRAD44_DY_BOTH = os.environ.get("SSV_WINOGRAD44_DY_BOTH", "1") == "1"


def wino44_lazy_dy_ok(y, w_shape, x_shape):
    """May the BatchNorm behind this convolution output hand its backward over as a LazyGrad?  Only when forward, data gradient and weight gradient all run F(4x4):
    the output carries F(4x4)'s own transformed input (the weight gradient will take the (g, x) operand) and the data gradient's dispatch rule holds for dy's shape
    (= the output's: 3x3 / stride 1 / padding 1)."""
    v = getattr(y, "_wino_v", None)
    k, c, _, _ = w_shape
    return (WINOGRAD44_DY_BOTH and WINOGRAD44_WGRAD and v is not None and v.shape[0] == 36
            and _use_wino44(y.shape[0], y.shape[1], y.shape[2], c, k, WINOGRAD44_MAX_RATIO_DGRAD))


# Which Winograd form each product took (launch counts by name), recorded while DISPATCH is a dict: bench.py's parity gate prints it so that the line
# shows the gate ran the kernel selection of the timed batch-512 step (`large_batch_dispatch`)
DISPATCH = None


def _note(kind):
    if DISPATCH is not None:
        DISPATCH[kind] = DISPATCH.get(kind, 0) + 1


class large_batch_dispatch:
    """Run a SMALL batch through the kernel selection of a large one: the tile-count floors of the two Winograd forms are lifted, so every 3x3 product
    that takes F(4x4) / F(2x2) at batch 512 takes it here too (the ratio / channel rules are batch-independent).  Test and gate plumbing only."""

    def __enter__(self):
        global WINOGRAD_MIN_TILES, WINOGRAD44_MIN_TILES, DISPATCH
        self.prev = (WINOGRAD_MIN_TILES, WINOGRAD44_MIN_TILES, DISPATCH)
        WINOGRAD_MIN_TILES, WINOGRAD44_MIN_TILES, DISPATCH = 0, 0, {}
        self.log = DISPATCH
        return self

    def __exit__(self, *exc):
        global WINOGRAD_MIN_TILES, WINOGRAD44_MIN_TILES, DISPATCH
        WINOGRAD_MIN_TILES, WINOGRAD44_MIN_TILES, DISPATCH = self.prev
        return False


class graph_dispatch:
    """The kernel selection for a step that is being captured into a HIP graph (graph.StepGraph) on SMALL images: without a per-launch host cost the Winograd forms
    pay from far fewer tiles and from 64 channels - their 16 / 36 batched products put 16 / 36 times the workgroups of the direct kernel on maps whose direct
    launch fills a fraction of the chip (resnet18 at 32 x 32, batch 64: layer4's 3x3 is 32 workgroups walking 144 k-tiles each).  Measured through the graph,
    ms per step at batch 64 / 512 (profiles/r05_cifar_wino_floors.txt): default floors 6.79 / 9.47, these 5.17 / 9.31; launched kernel by kernel the same
    selection is SLOWER (10.6 vs 9.2 at batch 64: more launches) - hence only under capture."""
    CHANNELS, TILES, TILES44 = 64, 64, 256

    def __enter__(self):
        global WINOGRAD_MIN_CHANNELS, WINOGRAD_MIN_TILES, WINOGRAD44_MIN_TILES
        self.prev = (WINOGRAD_MIN_CHANNELS, WINOGRAD_MIN_TILES, WINOGRAD44_MIN_TILES)
        WINOGRAD_MIN_CHANNELS, WINOGRAD_MIN_TILES, WINOGRAD44_MIN_TILES = (min(self.prev[0], self.CHANNELS), min(self.prev[1], self.TILES), min(self.prev[2], self.TILES44))
        return self

    def __exit__(self, *exc):
        global WINOGRAD_MIN_CHANNELS, WINOGRAD_MIN_TILES, WINOGRAD44_MIN_TILES
        WINOGRAD_MIN_CHANNELS, WINOGRAD_MIN_TILES, WINOGRAD44_MIN_TILES = self.prev
        return False


def _wino44_ratio(h, w_):
    return (36.0 * ((h + 3) // 4) * ((w_ + 3) // 4)) / (16.0 * ((h + 1) // 2) * ((w_ + 1) // 2))


def _use_wino44(n, h, w_, c, k, max_ratio):
    return (WINOGRAD44 and max(c, k) <= WINOGRAD44_MAX_CHANNELS and _wino44_ratio(h, w_) <= max_ratio
            and n * ((h + 3) // 4) * ((w_ + 3) // 4) >= WINOGRAD44_MIN_TILES)


def _gemm_batched(nb, t, c, k, a, u, m):
    """m[b] = a[b] . u[b]^T for the nb transformed-domain positions (a [nb][t][c], u [nb][k][c], m [nb][t][k]); in the bf16x3 arithmetic on the planes of u."""
    if ARITHMETIC == "bf16x3" and c % 32 == 0 and k % 4 == 0:
        _note("gemm_batched_bf16x3")
        call("ssv_gemm_batched_split", nb, t, c, k, ptr(a), ptr(_planes(u)), ptr(m), None, None, stream())
    else:
        call("ssv_gemm_batched", nb, t, c, k, ptr(a), ptr(u), ptr(m), stream())


def _gemm_batched_wgrad(nb, t, c, k, v, dm, du, chunk=0, flush=0):
    """du[b] = dm[b]^T . v[b] over the t tiles; ``chunk`` / ``flush``: blocked accumulation (ssv_gemm_batched_wgrad_blocked)."""
    lib = _lib.load()
    if ARITHMETIC == "bf16x3" and c % 4 == 0 and k % 4 == 0:
        _note("gemm_batched_wgrad_bf16x3")
        ws = workspace.get(lib.ssv_gemm_batched_wgrad_blocked_workspace_bytes(nb, t, c, k, chunk), v.device)
        call("ssv_gemm_batched_wgrad_split", nb, t, c, k, ptr(v), ptr(dm), ptr(du), chunk, flush, ptr(ws), ws.numel(), stream())
    elif chunk > 0 or flush > 0:
        ws = workspace.get(lib.ssv_gemm_batched_wgrad_blocked_workspace_bytes(nb, t, c, k, chunk), v.device)
        call("ssv_gemm_batched_wgrad_blocked", nb, t, c, k, ptr(v), ptr(dm), ptr(du), chunk, flush, ptr(ws), ws.numel(), stream())
    else:
        ws = workspace.get(lib.ssv_gemm_batched_wgrad_workspace_bytes(nb, t, c, k), v.device)
        call("ssv_gemm_batched_wgrad", nb, t, c, k, ptr(v), ptr(dm), ptr(du), ptr(ws), ws.numel(), stream())


def _wino_fwd(f, x, w, in_affine, want_stats, keep_v):
    _note(f.note_fwd)
    _lib._dev(x, w)
    w, wshape = _ohwi(w)
    n, h, w_, c = x.shape
    k = wshape[0]
    lib = _lib.load()
    t = f.tiles(n, h, w_)
    u = _wino_filter(w, wshape, form=f)
    sc, sh = in_affine if in_affine is not None else (None, None)
    v = torch.empty((f.positions, t, c), dtype=torch.float32, device=x.device)
    v2 = None              # without its own weight gradient (round 4's selection) F(4x4)'s input transform also leaves the F(2x2) transformed input: that one is then kept
    if f is _F44 and keep_v and not WINOGRAD44_WGRAD:
        v2 = torch.empty((16, _F22.tiles(n, h, w_), c), dtype=torch.float32, device=x.device)
    second = (ptr(v2),) if f is _F44 else ()
    call(f.input_transform, n, h, w_, c, ptr(x), ptr(sc), ptr(sh), ptr(v), *second, stream())
    m = torch.empty((f.positions, t, k), dtype=torch.float32, device=x.device)
    _gemm_batched(f.positions, t, c, k, v, u, m)
    y = _empty((n, h, w_, k), x)
    part = _empty((2, f.groups(n, h, w_, True), k), x) if want_stats else None
    call(f.output_transform, n, h, w_, k, ptr(m), ptr(y), None if part is None else ptr(part[0]), None if part is None else ptr(part[1]), None, stream())
    rpg = int(getattr(lib, f.sym_rows_per_group)(n, h, w_)) if want_stats else 0
    return y, (None if part is None else (part[0], part[1], rpg)), ((v if v2 is None else v2) if keep_v else None)


def _wino_dgrad(f, dy, w, gate):
    _note(f.note_dgrad)
    vd = None
    if f is _F44:          # the transformed input the weight gradient's one pass over dy already wrote (`wino44_conv2d_wgrad`)
        if isinstance(dy, LazyGrad):
            vd, dy.wino_vd, dy = dy.wino_vd, None, dy.g
            if vd is None:
                raise _lib.SsvError("wino44_conv2d_dgrad: a LazyGrad without the transformed input the weight gradient leaves")
        else:
            vd = dy.__dict__.pop("_wino44_vd", None)
    _lib._dev(dy, w)
    w, wshape = _ohwi(w)
    n, h, w_, k = dy.shape
    c = wshape[1]
    t = f.tiles(n, h, w_)
    u = _wino_filter(w, wshape, transposed=True, form=f)          # [16 | 36][C][K]
    if vd is not None and tuple(vd.shape) == (f.positions, t, k):
        v = vd
    else:
        v = torch.empty((f.positions, t, k), dtype=torch.float32, device=dy.device)
        call(f.input_transform, n, h, w_, k, ptr(dy), None, None, ptr(v), *((None,) if f is _F44 else ()), stream())
    m = torch.empty((f.positions, t, c), dtype=torch.float32, device=dy.device)
    _gemm_batched(f.positions, t, k, c, v, u, m)
    dx = _empty((n, h, w_, c), dy)
    if gate is not None:
        groups = f.groups(n, h, w_, False)
        st, part = _gate_struct(gate, groups, c, dy)
        call(f.output_transform, n, h, w_, c, ptr(m), ptr(dx), None, None, C.byref(st), stream())
        dx._gate_partials = (part[0], part[1], groups)
    else:
        call(f.output_transform, n, h, w_, c, ptr(m), ptr(dx), None, None, None, stream())
    return dx


def _wino_wgrad(f, v, dy, w_like, dw, accumulate, dgrad_follows):
    """The skeleton both forms share: dM = A dY A^T, the batched products dU_p = dM_p^T V_p over the tiles, dw (+)= G^T dU G."""
    _note(f.note_wgrad)
    lazy = dy if isinstance(dy, LazyGrad) else None
    g = lazy.g if lazy is not None else dy
    _lib._dev(v, g, dw)
    _, wshape = _ohwi(w_like)
    n, h, w_, k = dy.shape
    c = wshape[1]
    t = f.tiles(n, h, w_)
    if f is _F22:
        dm = torch.empty((16, t, k), dtype=torch.float32, device=g.device)
        call("ssv_wino_dy_transform", n, h, w_, k, ptr(g), ptr(dm), stream())
        flush = chunk = 0
    else:
        if tuple(v.shape) != (36, t, c):
            raise _lib.SsvError(f"wino44_conv2d_wgrad: transformed input {tuple(v.shape)} does not belong to a {n}x{h}x{w_}x{c} activation")
        dm = torch.empty((36, t, k), dtype=torch.float32, device=g.device)
        # the data gradient of the same layer follows (nn.conv: weight gradient first): when it will run F(4x4) too, its transformed input comes out of this pass
        both = WINOGRAD44_DY_BOTH and (lazy is not None or (dgrad_follows is not False and _use_wino44(n, h, w_, c, k, WINOGRAD44_MAX_RATIO_DGRAD)))
        if lazy is not None and not both:
            raise _lib.SsvError("wino44_conv2d_wgrad: a LazyGrad needs the one-pass transform (ops.WINOGRAD44_DY_BOTH was switched off after the forward marked this layer)")
        if both:
            vd = torch.empty((36, t, k), dtype=torch.float32, device=g.device)
            dyin = _dyin_struct(lazy, 0, n) if lazy is not None else None
            _note("wino44_dy_both_formed_on_load" if lazy is not None else "wino44_dy_both")
            call("ssv_wino44_dy_transform_both", n, h, w_, k, ptr(g), None if dyin is None else C.byref(dyin), ptr(vd), ptr(dm), stream())
            if lazy is not None:
                lazy.wino_vd = vd
            else:
                dy._wino44_vd = vd
        else:
            call("ssv_wino44_dy_transform", n, h, w_, k, ptr(g), ptr(dm), stream())
        # the bf16 instruction folds 32 products per accumulator rounding (the fp32 one: 2), so a chain's rounding error is that of one 16x shorter: the register-level
        # flush is not needed for the 2e-6 bar (tests/test_gpu_winograd44.py measures it), the chunked fp64 fold stays
        chunk, flush = WINOGRAD44_WGRAD_CHUNK, (WINOGRAD44_WGRAD_FLUSH_BF16X3 if ARITHMETIC == "bf16x3" else WINOGRAD44_WGRAD_FLUSH)
    du = torch.empty((f.positions, k, c), dtype=torch.float32, device=g.device)
    _gemm_batched_wgrad(f.positions, t, c, k, v, dm, du, chunk, flush)
    call(f.filter_grad, k, c, ptr(du), ptr(dw), int(accumulate), stream())
    return dw


def wino_conv2d_fwd(x, w, in_affine=None, want_stats=False, keep_v=False):
    """y = conv3x3(act(x), w) (stride 1, padding 1) through F(2x2, 3x3).  Returns (y, (pmean, pm2) | None, V | None): the statistics
    partials are one per 16 tiles = 64 output rows (needs even H, W); V is the transformed input, kept for the weight gradient."""
    if _use_wino44(x.shape[0], x.shape[1], x.shape[2], x.shape[3], w.shape[0], WINOGRAD44_MAX_RATIO_FWD_NO_V2 if WINOGRAD44_WGRAD else WINOGRAD44_MAX_RATIO_FWD):
        return wino44_conv2d_fwd(x, w, in_affine, want_stats, keep_v)
    return _wino_fwd(_F22, x, w, in_affine, want_stats, keep_v)


def wino44_conv2d_fwd(x, w, in_affine=None, want_stats=False, keep_v=False):
    """wino_conv2d_fwd through F(4x4, 3x3): 36 transformed-domain GEMMs over a quarter of the tiles.  ``keep_v``: the weight gradient's operand comes back as
    the third result - the transformed input V [36][T][C] itself (WINOGRAD44_WGRAD: the weight gradient runs F(4x4) too), or the F(2x2) transformed input
    [16][T2][C] the input transform then also leaves (wino_conv2d_wgrad tells them apart by the leading dimension).  Statistics partials: one per row of
    tiles (H % 4 == 0) or per image."""
    return _wino_fwd(_F44, x, w, in_affine, want_stats, keep_v)


def wino_conv2d_dgrad(dy, w, gate=None):
    """dx = conv3x3 data gradient (stride 1, padding 1) through F(2x2, 3x3) on the transposed, rotated filter; ``gate`` (BnGateCtx without
    a second target): dx is gated and its partial sums come back as ``dx._gate_partials`` like conv2d_dgrad's."""
    if _use_wino44(dy.shape[0], dy.shape[1], dy.shape[2], w.shape[1], dy.shape[3], WINOGRAD44_MAX_RATIO_DGRAD):
        return wino44_conv2d_dgrad(dy, w, gate)
    return _wino_dgrad(_F22, dy, w, gate)


def wino44_conv2d_dgrad(dy, w, gate=None):
    """wino_conv2d_dgrad through F(4x4, 3x3); the gate's partial sums come one per row of tiles.  ``dy`` may be the LazyGrad / tensor whose transformed input
    the weight gradient's pass already wrote (`wino44_conv2d_wgrad`): the input transform is then skipped."""
    return _wino_dgrad(_F44, dy, w, gate)


def wino_conv2d_wgrad(v, dy, w_like, dw, accumulate=True, dgrad_follows=None):
    """dw (+)= weight gradient of the 3x3 convolution whose transformed input V was kept by wino_conv2d_fwd ([16][T2][C]: F(2x2); [36][T][C]: F(4x4))."""
    if v.shape[0] == 36:
        return wino44_conv2d_wgrad(v, dy, w_like, dw, accumulate, dgrad_follows=dgrad_follows)
    return _wino_wgrad(_F22, v, dy, w_like, dw, accumulate, dgrad_follows)


def wino44_conv2d_wgrad(v, dy, w_like, dw, accumulate=True, dgrad_follows=None):
    """wino_conv2d_wgrad through F(4x4, 3x3): dM = A dY A^T, 36 products dU_p = dM_p^T V_p over the tiles, dw (+)= G^T dU G."""
    return _wino_wgrad(_F44, v, dy, w_like, dw, accumulate, dgrad_follows)


# ------------------------------------------------------------------------------------------- the 3-channel image stem, row-taps form
def can_row_stem(w_shape):
    k, c, r, s_ = w_shape
    return c == 3 and 3 * s_ <= 24 and s_ <= 8 and k % 4 == 0


def stem_weight_rows(w):
    """[K,3,R,S] filter (OHWI memory) -> [K*R][24]: its rows of 3 S floats, (s, c) order, zero-padded to 24."""
    w, (k, c, r, s_) = _ohwi(w)
    rows = w.permute(0, 2, 3, 1).reshape(k * r, s_ * c)
    return rows if s_ * c == 24 else pad_channels(rows, 24)          # 8 taps fill the 24 floats: nothing to pad (ssv_pad_channels refuses cin == cout)


def stem_conv_fwd(x, wrows, w_shape, stride, pad, want_stats=False):
    """y = conv(x, w) for a 3-channel NHWC image batch, x UNPADDED: returns (y, (pmean, pm2) | None)."""
    _lib._dev(x, wrows)
    d = conv_desc(x.shape, w_shape, stride, pad)
    y = _empty((d.N, d.Ho, d.Wo, d.K), x)
    lib = _lib.load()
    # statistics partials: one per 64 output pixels, or per whole output rows on the rows-in-LDS kernel (the same for every chunk: it depends on the map, not the batch)
    rpg = int(lib.ssv_stem_conv_fwd_stats_rows_per_group(C.byref(d)))
    m = d.N * d.Ho * d.Wo
    part = _empty((2, -(-m // rpg), d.K), x) if want_stats else None
    g0 = 0
    for n0, n1 in _batch_chunks(d.N, (d.H * d.W * d.C, d.Ho * d.Wo * d.K), rows_per_sample=d.Ho * d.Wo if want_stats else None):
        dc = conv_desc((n1 - n0,) + tuple(x.shape[1:]), w_shape, stride, pad)
        if int(lib.ssv_stem_conv_fwd_stats_rows_per_group(C.byref(dc))) != rpg:
            raise _lib.SsvError("ssv_stem_conv_fwd: statistics group size changed between batch chunks")
        gc = -(-(n1 - n0) * d.Ho * d.Wo // rpg)
        call("ssv_stem_conv_fwd", C.byref(dc), ptr(x[n0:n1]), ptr(wrows), ptr(y[n0:n1]),
             ptr(part[0][g0:g0 + gc]) if want_stats else None, ptr(part[1][g0:g0 + gc]) if want_stats else None, stream())
        g0 += gc
    if part is None:
        return y, None
    return y, ((part[0], part[1]) if rpg == 64 else (part[0], part[1], rpg))


def stem_conv_wgrad(x, dy, w_shape, stride, pad):
    """Weight gradient in the row-taps layout: [K*R][24] (columns >= 3 S are zero)."""
    _lib._dev(x, dy)
    k, c, r, s_ = w_shape
    lib = _lib.load()
    out = None
    for n0, n1 in _batch_chunks(x.shape[0], (x[0].numel(), dy[0].numel())):
        d = conv_desc(x[n0:n1].shape, w_shape, stride, pad)
        ws = workspace.get(lib.ssv_stem_conv_wgrad_workspace_bytes(C.byref(d)), x.device)
        dwr = torch.empty((k * r, 24), dtype=torch.float32, device=x.device)
        call("ssv_stem_conv_wgrad", C.byref(d), ptr(x[n0:n1]), ptr(dy[n0:n1]), ptr(dwr), ptr(ws), ws.numel(), stream())
        out = dwr if out is None else add_(out, dwr)
    return out
