"""Thin tensor-level wrappers over the C ABI (include/subgc_hip.h).

Every function takes torch tensors that already live on the MI355X, hands their raw device
pointers to libsubgc_hip.so on torch's CURRENT stream and returns torch tensors.  No autograd
here (see functions.py) and no fallback: CPU tensors raise.
"""
from __future__ import annotations

import gc
import math

import torch

from ._lib import SubgcError, call, call_beam_att, call_consensus, call_criterion, call_decode_b16, call_decode_rules, call_gcn_agg, call_neighbours, call_selfcritical, lib
from . import _scoring

RELU, ACCUM = 1, 2
FLOPS = {"on": False, "gemm": 0.0, "gemm_bytes": 0.0, "gemm_calls": 0}


# torch.cuda.current_stream() builds a Stream object through three layers of Python (~6 us; ~190 calls per train step = 1.2 ms
# of the host's 7.5); the raw-handle getters behind it cost a fraction of a microsecond.  Same value, public path as fallback.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream_of(idx):
    return _raw_stream(idx) if _raw_stream is not None else torch.cuda.current_stream(idx).cuda_stream


def _stream():
    if _raw_stream is not None and _raw_device is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


GRAD_WRITES = [0]          # moved by every gradient writer that goes through raw pointers (functions._direct, the decoder backwards)
_WS = {}
WS_MBYTES = 160


def ensure_workspace(device=None, mbytes=None):
    """The split-K scratch of the CURRENT stream of `device`: one buffer per (device, stream), handed to every GEMM call as
    its `workspace, ws_bytes` arguments (the C ABI keeps no global scratch), so concurrent streams never share partial planes.
    Buffers live for the life of the process: captured hipGraphs bake their addresses in."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (idx, _stream_of(idx))
    buf = _WS.get(key)
    if buf is None:
        if torch.cuda.is_current_stream_capturing():
            raise SubgcError("no split-K workspace for the capturing stream: capture through ops.graph_capture(), which brings its own")
        buf = _WS[key] = torch.empty((mbytes or WS_MBYTES) << 20, dtype=torch.uint8, device=torch.device("cuda", idx))
    return buf


_WS_RAW = {}


def _ws(t):
    """(pointer, bytes) of the current stream's workspace on t's device -- the two `workspace, ws_bytes` call arguments."""
    idx = t.device.index
    key = (idx, _stream_of(idx))
    raw = _WS_RAW.get(key)
    if raw is None:
        buf = ensure_workspace(t.device)
        raw = _WS_RAW[key] = (buf.data_ptr(), buf.numel())
    return raw


_CAPTURE_STREAMS = {}
class graph_capture:
    """`with ops.graph_capture(graph, device): ...` = torch.cuda.graph on a dedicated capture stream of that device whose
    split-K workspace was allocated EAGERLY (outside any graph's private pool), so the addresses a captured GEMM bakes in stay
    valid for every later capture and replay.  All graphs captured through this class on one device share that one workspace:
    they must not be REPLAYED concurrently on different streams (the decode paths replay them one after the other on the current
    stream); a caller that wants concurrent replays captures on its own stream with its own `ensure_workspace`."""

    def __init__(self, graph, device):
        dev = torch.device(device)
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        st = _CAPTURE_STREAMS.get(idx)
        if st is None:
            st = _CAPTURE_STREAMS[idx] = torch.cuda.Stream(device=idx)
            with torch.cuda.stream(st):
                ensure_workspace(torch.device("cuda", idx))
        self.ctx = torch.cuda.graph(graph, stream=st)

    def __enter__(self):
        # The cyclic garbage collector must not run INSIDE a capture: a dead cycle that owns an older CUDAGraph (a dropped model's
        # graph cache) frees its private pool when collected, hipFree is illegal while a stream of the process captures
        # (capture_error_mode "global") and the error surfaces in a destructor, i.e. as abort().  torch.cuda.graph stopped
        # collecting on entry (torch.compiler.config.force_cudagraph_gc), so: collect now, keep the collector off until the end.
        self._gc_was_on = gc.isenabled()
        gc.collect()
        gc.disable()
        try:
            return self.ctx.__enter__()
        except BaseException:
            if self._gc_was_on:
                gc.enable()
            raise

    def __exit__(self, *exc):
        try:
            return self.ctx.__exit__(*exc)
        finally:
            if self._gc_was_on:
                gc.enable()


GEMM_MODES = {"f32": 1 << 4, "bf16x3": 2 << 4, "bf16": 3 << 4}       # SUBGC_GEMM_MODE_* bits of the per-call flags


class gemm_mode:
    """`with ops.gemm_mode("bf16x3"): ...` -- arithmetic of the 128x128-tile forms of the fp32-OPERAND GEMM, passed with every
    call (SUBGC_GEMM_MODE_*): "f32" (default), "bf16x3" (fp32 operands split exactly into three bf16 planes, six MFMA terms:
    fp32-grade) or "bf16" (fp32 operands rounded to bf16 in the staging path).  Storage stays fp32 in all three; the
    bf16-STORAGE path of BASELINE configs 3 / 5 is `model.bf16_storage` + bf16 tensors through `gemm` (subgc_gemm_bf16)."""

    current = "f32"

    def __init__(self, mode):
        if mode not in GEMM_MODES:
            raise SubgcError(f"unknown GEMM mode {mode!r}")
        self.mode = mode

    def __enter__(self):
        self.prev = gemm_mode.current
        gemm_mode.current = self.mode

    def __exit__(self, *exc):
        gemm_mode.current = self.prev


def set_gemm_mode(mode):
    if mode not in GEMM_MODES:
        raise SubgcError(f"unknown GEMM mode {mode!r}")
    gemm_mode.current = mode


class debug_bounds:
    """`with ops.debug_bounds(): ...` -- the library's debug bounds mode (subgc_debug_bounds): every entry point that consumes an index
    tensor it did not produce (rel_ind, gpn_obj_ind, node lists, word ids, criterion targets, class ids) validates it on the device before
    its kernels run and raises SubgcError naming the tensor, the first bad position and its value -- the way the reference fails on a bad
    loader tensor (IndexError; the asserts of gpn.py:117-118).  One launch + one stream synchronisation per checked tensor: debugging only."""

    def __init__(self, on=True):
        self.on = bool(on)

    def __enter__(self):
        self.prev = lib().subgc_debug_bounds(int(self.on))
        return self

    def __exit__(self, *exc):
        lib().subgc_debug_bounds(int(self.prev))


_DET = [False]         # mirror of subgc_deterministic as set through this module: the `_ws` wrappers hand over scratch only while it is on


def set_deterministic(on):
    """Switch the library's deterministic mode (subgc_deterministic) on or off for the whole process; returns the previous setting."""
    prev = bool(lib().subgc_deterministic(int(bool(on))))
    _DET[0] = bool(on)
    return prev


def _det_ws(t):
    """`workspace, ws_bytes` of the `_ws` siblings: the current stream's scratch in deterministic mode; (NULL, 0) otherwise, where the
    siblings launch their originals (no per-stream workspace is allocated for them, e.g. on the reducer's side stream)."""
    return _ws(t) if _DET[0] else (None, 0)


class deterministic:
    """`with ops.deterministic(): ...` -- the library's deterministic mode (subgc_deterministic): every reduction of the training step sums
    in an order fixed by the shape alone (inverted-index gather sums, slab partials with ordered finish passes; no float atomics), so two
    runs from the same weights, batches and seeds give the same bits.  Process-wide, read when a call is enqueued; the previous setting
    is restored on exit."""

    def __init__(self, on=True):
        self.on = bool(on)

    def __enter__(self):
        self.prev = lib().subgc_deterministic(int(self.on))
        _DET[0] = self.on
        return self

    def __exit__(self, *exc):
        lib().subgc_deterministic(int(self.prev))
        _DET[0] = bool(self.prev)


class gemm_tune:
    """Measurement-script switches of the GEMM dispatch, handed over per call in `flags` (the library keeps no tunable state):
    `with ops.gemm_tune(no_splitk=True, no_skinny=True): ...` for subgc_gemm_f32, `tile=128|256|"p8"`, `no_p8`, `splits=n` for subgc_gemm_bf16."""

    f32_bits = 0
    b16_bits = 0

    TILE_BITS = {0: 0, 128: 64, 256: 128, "p8": 1 << 13}                      # SUBGC_GEMM_TILE128 / TILE256 / TILE_P8

    def __init__(self, no_splitk=False, no_skinny=False, tile=0, no_p8=False, splits=0):
        self.f32 = (64 if no_splitk else 0) | (128 if no_skinny else 0)      # SUBGC_GEMM_NO_SPLITK | SUBGC_GEMM_NO_SKINNY
        self.b16 = self.TILE_BITS[tile] | ((1 << 14) if no_p8 else 0) | ((splits & 15) << 8)    # ... | SUBGC_GEMM_NO_P8 | SUBGC_GEMM_SPLITS(n)

    def __enter__(self):
        self.prev = (gemm_tune.f32_bits, gemm_tune.b16_bits)
        gemm_tune.f32_bits, gemm_tune.b16_bits = self.f32, self.b16

    def __exit__(self, *exc):
        gemm_tune.f32_bits, gemm_tune.b16_bits = self.prev


BF16 = torch.bfloat16


def is_b16(t):
    return t is not None and t.dtype == BF16


def empty_b16(rows, cols, device, zero=False):
    """[rows, cols] bf16 view whose leading dimension is padded to a multiple of 8 elements (16-byte row segments for the GEMM)."""
    pad = (cols + 7) // 8 * 8
    if zero:                                                  # bf16 zero is the all-zero bit pattern: fill the fp32 view
        buf = fill_(torch.empty(max(rows * pad // 2, 1), device=device, dtype=torch.float32), 0.0).view(BF16)[: rows * pad].view(rows, pad)
    else:
        buf = torch.empty(rows, pad, device=device, dtype=BF16)
    return buf[:, :cols] if pad != cols else buf


def act_buffer(shape, device, bf16, zero=False):
    """A buffer that only GEMMs consume: bf16 (last dim must be a multiple of 8 so that every [.., cols] slice keeps 16-byte
    rows) or fp32."""
    if not bf16:
        return zeros(*shape, device=device) if zero else torch.empty(*shape, device=device, dtype=torch.float32)
    n = 1
    for d in shape:
        n *= d
    if shape[-1] % 8:
        raise SubgcError(f"bf16 activation buffers need a last dimension that is a multiple of 8, got {tuple(shape)}")
    if zero:
        return fill_(torch.empty(max(n // 2, 1), device=device, dtype=torch.float32), 0.0).view(BF16)[:n].view(*shape)
    return torch.empty(*shape, device=device, dtype=BF16)


# Row pitch of the activation / weight-snapshot buffers the decoder allocates for its recurrent GEMMs, in elements (0 = unpadded).
# bf16: a K-contiguous operand tile is 32 elements = 64 bytes per row; with R = 1000 the natural pitches (2000 / 4000 / 6000 bytes) put
# half of those segments across two 128-byte lines, i.e. twice the L2 requests per LDS-DMA tile (tools/gemm_bf16_bench.py --pad 64:
# 1280 x 4000 x 2000 52 -> 40 us).  Every kernel that writes these buffers takes a leading dimension, so the pad is free.
PITCH = {"bf16": 64, "f32": 0}


def pitch_of(cols, bf16):
    q = PITCH["bf16" if bf16 else "f32"]
    return (cols + q - 1) // q * q if q else cols


def act_padded(shape, device, bf16, zero_rows=0):
    """`act_buffer` with the last dimension's pitch rounded up to PITCH (a [..., cols] view of a [..., pitch] buffer); the first
    `zero_rows` rows (of the flattened leading dimensions) are zeroed, pad columns included."""
    *lead, cols = shape
    ldp = pitch_of(cols, bf16)
    if bf16 and cols % 8:
        raise SubgcError(f"bf16 activation buffers need a last dimension that is a multiple of 8, got {tuple(shape)}")
    base = torch.empty(*lead, ldp, device=device, dtype=BF16 if bf16 else torch.float32)
    if zero_rows:
        z = base.view(-1, ldp)[:zero_rows]
        fill_(z.view(torch.float32) if bf16 else z, 0.0)
    return base[..., :cols] if ldp != cols else base


def flat_rows(t3):
    """[T, S, C] (unit inner stride, stride(0) == S * stride(1)) -> the [T * S, C] view with the same row pitch."""
    T, S, C = t3.shape
    if t3.stride(2) != 1 or (T > 1 and t3.stride(0) != S * t3.stride(1)):
        raise SubgcError(f"flat_rows: not a row-pitched [T, S, C] view: {tuple(t3.shape)} / {t3.stride()}")
    return torch.as_strided(t3, (T * S, C), (t3.stride(1), 1), t3.storage_offset())


def cast_bf16(x, out=None, m_dev=None):
    """bf16 copy of a 2-D fp32 view (subgc_cast_f32_bf16); the destination's columns are padded with zeros to a multiple of 8
    (a K-contiguous GEMM operand needs K % 8 == 0).  Returns the [rows, cols_pad] bf16 tensor."""
    rows, cols = x.shape
    pad = (cols + 7) // 8 * 8
    if out is None:
        out = torch.empty(rows, pad, device=x.device, dtype=BF16)
    call("subgc_cast_f32_bf16", _ptr(x, torch.float32), ld(x), _ptr(out, BF16), ld(out), rows, cols, out.size(1), _ptr(m_dev, torch.int32), _stream())
    return out


def as_b16(x, m_dev=None):
    """The GEMM-operand form of a 2-D activation: itself when already bf16, else a bf16 copy ([rows, cols] view, padded ld)."""
    if is_b16(x):
        return x
    y = cast_bf16(x, m_dev=m_dev)
    return y[:, : x.size(1)] if y.size(1) != x.size(1) else y


def transpose_bf16(x, out=None):
    """out[c, r] = bf16(x[r, c]) (subgc_transpose_f32_bf16): the W^T snapshots; rows of `out` padded to a multiple of 8 elements."""
    rows, cols = x.shape
    if out is None:
        out = torch.zeros(cols, (rows + 7) // 8 * 8, device=x.device, dtype=BF16)[:, :rows]
    call("subgc_transpose_f32_bf16", _ptr(x, torch.float32), ld(x), _ptr(out, BF16), ld(out), rows, cols, _stream())
    return out


def _ptr(t, dtype=None):
    if t is None:
        return None
    if not t.is_cuda:
        raise SubgcError("subgc ops need device tensors (the HIP path has no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise SubgcError(f"expected {dtype}, got {t.dtype}")
    return t.data_ptr()


def ld(t):
    """Leading dimension of a 2-D row-major view with unit inner stride."""
    if t.dim() != 2 or (t.size(1) > 1 and t.stride(1) != 1):
        raise SubgcError(f"need a 2-D tensor with unit inner stride, got {tuple(t.shape)} / {t.stride()}")
    if t.size(0) > 1 and t.stride(0) < t.size(1):
        raise SubgcError(f"overlapping rows: shape {tuple(t.shape)} stride {t.stride()}")
    return max(t.stride(0), t.size(1))


def gemm(a, b, out, *, ta=False, tb=False, bias=None, add=None, keep=None, keep_scale=1.0, relu=False,
         accum=False, a_rows=None, c_rows=None, m_dev=None, out16=None):
    """out = epilogue(op(a) @ op(b));  a, b, out are 2-D row-major views (any leading dim).
    fp32 a, b -> subgc_gemm_f32 (arithmetic = the current `gemm_mode`); bf16 a, b -> subgc_gemm_bf16: `out` may then be fp32 or
    bf16 and `out16` an additional bf16 destination of the same result (for consumers that are GEMMs themselves)."""
    if is_b16(a) or is_b16(b):
        return _gemm_b16(a, b, out, ta, tb, bias, add, keep, keep_scale, relu, accum, a_rows, c_rows, m_dev, out16)
    if out16 is not None:
        raise SubgcError("out16 needs bf16 operands")
    M = a.size(1) if ta else a.size(0)
    K = a.size(0) if ta else a.size(1)
    N = b.size(0) if tb else b.size(1)
    Kb = b.size(1) if tb else b.size(0)
    if a_rows is not None:
        M = a_rows.numel()
    if K != Kb or (c_rows is None and out.size(0) < M) or out.size(1) != N:
        raise SubgcError(f"gemm shape mismatch: op(a)=[{M},{K}] op(b)=[{Kb},{N}] out={tuple(out.shape)}")
    if FLOPS["on"]:                      # bench.py's untimed accounting step: exact, ragged-aware algorithmic FLOPs
        r = int(m_dev.item()) if m_dev is not None else None
        me, ke = (M, min(K, r)) if (ta and r is not None) else ((min(M, r) if r is not None else M), K)
        FLOPS["gemm"] += 2.0 * me * N * ke
        # algorithmic HBM bytes of the same call: each operand read once, the result written once (+ read when accumulated into)
        FLOPS["gemm_bytes"] += 4.0 * (me * ke + ke * N + me * N * (2 if (accum or add is not None) else 1))
        FLOPS["gemm_calls"] += 1
    call("subgc_gemm_f32", int(ta), int(tb), M, N, K, _ptr(a, torch.float32), ld(a), _ptr(b, torch.float32), ld(b),
         _ptr(out, torch.float32), ld(out), _ptr(bias), _ptr(add), ld(add) if add is not None else 0,
         _ptr(keep, torch.uint8), float(keep_scale), (RELU if relu else 0) | (ACCUM if accum else 0) | GEMM_MODES[gemm_mode.current] | gemm_tune.f32_bits,
         _ptr(a_rows, torch.int32), _ptr(c_rows, torch.int32), _ptr(m_dev, torch.int32), *_ws(a), _stream())
    return out


def _gemm_b16(a, b, out, ta, tb, bias, add, keep, keep_scale, relu, accum, a_rows, c_rows, m_dev, out16):
    if not (is_b16(a) and is_b16(b)):
        raise SubgcError(f"bf16 GEMM needs both operands in bf16, got {a.dtype} / {b.dtype}")
    if a_rows is not None or c_rows is not None:
        raise SubgcError("the bf16 GEMM has no gathered / scattered row forms")
    M = a.size(1) if ta else a.size(0)
    K = a.size(0) if ta else a.size(1)
    N = b.size(0) if tb else b.size(1)
    Kb = b.size(1) if tb else b.size(0)
    if K != Kb or out.size(0) < M or out.size(1) != N:
        raise SubgcError(f"gemm shape mismatch: op(a)=[{M},{K}] op(b)=[{Kb},{N}] out={tuple(out.shape)}")
    c32, c16 = (None, out) if is_b16(out) else (out, out16)
    if c16 is not None and (c16.size(0) < M or c16.size(1) != N or not is_b16(c16)):
        raise SubgcError("out16 must be a bf16 [M, N] view")
    if FLOPS["on"]:
        r = int(m_dev.item()) if m_dev is not None else None
        me, ke = (M, min(K, r)) if (ta and r is not None) else ((min(M, r) if r is not None else M), K)
        FLOPS["gemm"] += 2.0 * me * N * ke
        FLOPS["gemm_bytes"] += 2.0 * (me * ke + ke * N) + me * N * ((4.0 * (2 if (accum or add is not None) else 1) if c32 is not None else 0.0)
                                                                   + (2.0 if c16 is not None else 0.0))
        FLOPS["gemm_calls"] += 1
    call("subgc_gemm_bf16", int(ta), int(tb), M, N, K, _ptr(a, BF16), ld(a), _ptr(b, BF16), ld(b), _ptr(c32, torch.float32),
         ld(c32) if c32 is not None else 0, _ptr(c16, BF16), ld(c16) if c16 is not None else 0, _ptr(bias, torch.float32), _ptr(add, torch.float32),
         ld(add) if add is not None else 0, _ptr(keep, torch.uint8), float(keep_scale), (RELU if relu else 0) | (ACCUM if accum else 0) | gemm_tune.b16_bits,
         _ptr(m_dev, torch.int32), *_ws(a), _stream())
    return out


PAIR_LAUNCHES = True      # the two same-shape products of a GCN unit pair in one launch (subgc_gemm_bf16_pair); False: two subgc_gemm_bf16 calls


def gemm_pair(a1, a2, b1, b2, out1, out2, *, ta=False, tb=False, bias1=None, bias2=None, relu=False, accum=False):
    """out_i = epilogue(op(a_i) @ op(b_i)) for two problems of the same shape in ONE launch (subgc_gemm_bf16_pair / subgc_gemm_f32_pair);
    shapes, leading dimensions or storage types that differ run as two `gemm` calls."""
    b16 = is_b16(a1)
    same = (PAIR_LAUNCHES and all(is_b16(t) == b16 for t in (a2, b1, b2)) and a1.shape == a2.shape and b1.shape == b2.shape and out1.shape == out2.shape
            and out1.dtype == out2.dtype and ld(a1) == ld(a2) and ld(b1) == ld(b2) and ld(out1) == ld(out2) and (bias1 is None) == (bias2 is None)
            and (b16 or (not relu and out1.dtype == torch.float32 and a1.dtype == torch.float32 and b1.dtype == torch.float32)))
    if not same:
        gemm(a1, b1, out1, ta=ta, tb=tb, bias=bias1, relu=relu, accum=accum)
        gemm(a2, b2, out2, ta=ta, tb=tb, bias=bias2, relu=relu, accum=accum)
        return out1, out2
    M = a1.size(1) if ta else a1.size(0)
    K = a1.size(0) if ta else a1.size(1)
    N = b1.size(0) if tb else b1.size(1)
    if K != (b1.size(1) if tb else b1.size(0)) or out1.size(0) < M or out1.size(1) != N:
        raise SubgcError(f"gemm_pair shape mismatch: op(a)=[{M},{K}] op(b)=[..,{N}] out={tuple(out1.shape)}")
    o16 = is_b16(out1)
    if FLOPS["on"]:
        esz = 2.0 if b16 else 4.0
        FLOPS["gemm"] += 4.0 * M * N * K
        FLOPS["gemm_bytes"] += 2.0 * (esz * (M * K + K * N) + M * N * (2.0 if o16 else 4.0 * (2 if accum else 1)))
        FLOPS["gemm_calls"] += 1
    if not b16:
        call("subgc_gemm_f32_pair", int(ta), int(tb), M, N, K, _ptr(a1, torch.float32), _ptr(a2, torch.float32), ld(a1), _ptr(b1, torch.float32),
             _ptr(b2, torch.float32), ld(b1), _ptr(out1, torch.float32), _ptr(out2, torch.float32), ld(out1), _ptr(bias1, torch.float32),
             _ptr(bias2, torch.float32), (ACCUM if accum else 0) | GEMM_MODES[gemm_mode.current] | gemm_tune.f32_bits, *_ws(a1), _stream())
        return out1, out2
    call("subgc_gemm_bf16_pair", int(ta), int(tb), M, N, K, _ptr(a1, BF16), _ptr(a2, BF16), ld(a1), _ptr(b1, BF16), _ptr(b2, BF16), ld(b1),
         None if o16 else _ptr(out1, torch.float32), None if o16 else _ptr(out2, torch.float32), 0 if o16 else ld(out1),
         _ptr(out1, BF16) if o16 else None, _ptr(out2, BF16) if o16 else None, ld(out1) if o16 else 0, _ptr(bias1, torch.float32), _ptr(bias2, torch.float32),
         (RELU if relu else 0) | (ACCUM if accum else 0) | gemm_tune.b16_bits, *_ws(a1), _stream())
    return out1, out2


def wgrad(dy, x, dW, db, accum=False, db_accum=False, m_dev=None):
    """Weight AND bias gradient of one linear layer in one call: dW (+)= dy^T x, db (+)= column sums of dy (subgc_gemm_f32_wgrad /
    subgc_gemm_bf16_wgrad: the workgroups of dW's tile column 0 add up the dy tiles they stage anyway -- no second read of dy, no
    column-sum launches).  dy [rows, M], x [rows, N] (both fp32 or both bf16), dW fp32 [M, N], db fp32 [M]; m_dev bounds the rows."""
    K, M = dy.shape
    N = x.size(1)
    if x.size(0) != K or dW.size(0) != M or dW.size(1) != N or db.numel() != M or not db.is_contiguous():
        raise SubgcError(f"wgrad shape mismatch: dy={tuple(dy.shape)} x={tuple(x.shape)} dW={tuple(dW.shape)} db={tuple(db.shape)}")
    b16 = is_b16(dy)
    if b16 != is_b16(x):
        raise SubgcError(f"wgrad needs both operands in one storage type, got {dy.dtype} / {x.dtype}")
    if FLOPS["on"]:
        ke = min(K, int(m_dev.item())) if m_dev is not None else K
        FLOPS["gemm"] += 2.0 * M * N * ke
        FLOPS["gemm_bytes"] += (2.0 if b16 else 4.0) * (M * ke + ke * N) + 4.0 * M * N * (2 if accum else 1)
        FLOPS["gemm_calls"] += 1
    if b16:
        call("subgc_gemm_bf16_wgrad", M, N, K, _ptr(dy, BF16), ld(dy), _ptr(x, BF16), ld(x), _ptr(dW, torch.float32), ld(dW), _ptr(db, torch.float32),
             (ACCUM if accum else 0) | gemm_tune.b16_bits, int(db_accum), _ptr(m_dev, torch.int32), *_ws(dy), _stream())
    else:
        call("subgc_gemm_f32_wgrad", M, N, K, _ptr(dy, torch.float32), ld(dy), _ptr(x, torch.float32), ld(x), _ptr(dW, torch.float32), ld(dW),
             _ptr(db, torch.float32), (ACCUM if accum else 0) | GEMM_MODES[gemm_mode.current] | gemm_tune.f32_bits, int(db_accum),
             _ptr(m_dev, torch.int32), *_ws(dy), _stream())
    return dW, db


def colsum_set(xs, outs, accumulate=False):
    """Column sums of several matrices: bf16 ones of one shape and leading dimension go three at a time through subgc_colsum_bf16_set (two
    launches per group instead of two per matrix); everything else through `colsum`."""
    groups = {}
    for x, o in zip(xs, outs):
        key = (tuple(x.shape), ld(x)) if (is_b16(x) and PAIR_LAUNCHES) else id(x)
        groups.setdefault(key, []).append((x, o))
    for key, items in groups.items():
        while items:
            chunk, items = items[:3], items[3:]
            if len(chunk) == 1 or not isinstance(key, tuple):
                for x, o in chunk:
                    colsum(x, out=o, accumulate=accumulate)
                continue
            x0 = chunk[0][0]
            px = [_ptr(x, BF16) for x, _ in chunk] + [None] * (3 - len(chunk))
            po = [_ptr(o, torch.float32) for _, o in chunk] + [None] * (3 - len(chunk))
            call("subgc_colsum_bf16_set", len(chunk), px[0], px[1], px[2], ld(x0), x0.size(0), x0.size(1), po[0], po[1], po[2], int(accumulate), *_ws(x0), _stream())


def colsum(x, out=None, accumulate=False, m_dev=None):
    out = torch.empty(x.size(1), device=x.device, dtype=torch.float32) if out is None else out
    if is_b16(x):
        call("subgc_colsum_bf16", _ptr(x, BF16), ld(x), x.size(0), x.size(1), _ptr(out, torch.float32), int(accumulate),
             _ptr(m_dev, torch.int32), *_ws(x), _stream())
        return out
    call("subgc_colsum_f32", _ptr(x, torch.float32), ld(x), x.size(0), x.size(1), _ptr(out), int(accumulate),
         _ptr(m_dev, torch.int32), *_ws(x), _stream())
    return out


def row_argmax(x, skip=0, want_val=False, i32=False):
    rows, cols = x.shape
    if i32:                              # class ids that index an embedding table: int32 rows for gather_rows / scatter_add_rows
        idx = torch.empty(rows, device=x.device, dtype=torch.int32)
        call("subgc_row_argmax_i32", _ptr(x, torch.float32), ld(x), rows, cols, skip, _ptr(idx), _stream())
        return idx
    idx = torch.empty(rows, device=x.device, dtype=torch.int64)
    val = torch.empty(rows, device=x.device, dtype=torch.float32) if want_val else None
    call("subgc_row_argmax_f32", _ptr(x, torch.float32), ld(x), rows, cols, skip, _ptr(idx), _ptr(val), _stream())
    return (idx, val) if want_val else idx


def csr_build(rel_ind, N):
    B, K, _ = rel_ind.shape
    rel_ind = rel_ind.contiguous()
    ptr = torch.empty(2, B, N + 1, device=rel_ind.device, dtype=torch.int32)
    edges = torch.empty(2, B, K, device=rel_ind.device, dtype=torch.int32)
    call("subgc_csr_build", _ptr(rel_ind, torch.int64), B, K, N, _ptr(ptr), _ptr(edges), _stream())
    return ptr, edges


def gcn_nodes_fwd(F0, F1, ptr, edges, skip, B, N, K, L, want_act=True):
    out = torch.empty(B, N, L, device=F0.device, dtype=torch.float32)
    act = torch.empty(B, N, L, device=F0.device, dtype=torch.uint8) if want_act else None
    call("subgc_gcn_nodes_fwd", _ptr(F0), _ptr(F1), _ptr(ptr), _ptr(edges), _ptr(skip), _ptr(out), _ptr(act), B, N, K, L, _stream())
    return out, act


def gcn_nodes_bwd(dX, act, rel_ind, ptr, B, N, K, L, bf16=False):
    dF0 = torch.empty(B, K, L, device=dX.device, dtype=BF16 if bf16 else torch.float32)
    dF1 = torch.empty_like(dF0)
    call("subgc_gcn_nodes_bwd", _ptr(dX), _ptr(act), _ptr(rel_ind), _ptr(ptr), _ptr(dF0), _ptr(dF1), int(bf16), B, N, K, L, _stream())
    return dF0, dF1


# Collection units WITHOUT BatchNorm whose targets are fewer than their sources (nodes <- relations: 37 against 65 rows per image) apply the
# 0/1 map to the 1024-wide source rows first and run fc_lft / fc_rgt per role on the target rows (functions.GcnAggFirstFn):
# (A X) W^T in place of A (X W^T).  False: the launches of the paired units + gcn_nodes_fwd, exactly as before.
GCN_AGGREGATE_FIRST = True


def gcn_agg_fwd(X, ptr, edges, B, N, K, L):
    """-> (Xagg0, Xagg1 [B*N, L], s0, s1 [B*N]): per role 0.5 * (sum of the node's relation rows) / (cnt + 1e-7) and the bias scale
    0.5 * cnt / (cnt + 1e-7) of the row (subgc_gcn_agg_fwd)."""
    A0, A1 = (torch.empty(B * N, L, device=X.device, dtype=torch.float32) for _ in range(2))
    s0, s1 = (torch.empty(B * N, device=X.device, dtype=torch.float32) for _ in range(2))
    call_gcn_agg("subgc_gcn_agg_fwd", _ptr(X, torch.float32), _ptr(ptr, torch.int32), _ptr(edges, torch.int32), _ptr(A0), _ptr(A1), _ptr(s0), _ptr(s1),
                 B, N, K, L, _stream())
    return A0, A1, s0, s1


def gcn_agg_bwd(dA0, dA1, rel_ind, ptr, B, N, K, L, out=None):
    """d(source) [B*K, L] of gcn_agg_fwd: a gather of one subject and one object row per relation; `out` given: added to it."""
    dX = out if out is not None else torch.empty(B * K, L, device=dA0.device, dtype=torch.float32)
    call_gcn_agg("subgc_gcn_agg_bwd", _ptr(dA0, torch.float32), _ptr(dA1, torch.float32), _ptr(rel_ind, torch.int64), _ptr(ptr, torch.int32),
                 _ptr(dX, torch.float32), int(out is not None), B, N, K, L, _stream())
    return dX


def gcn_agg_relu_bwd(dy, y0, y1):
    """-> (dy where y0 > 0, dy where y1 > 0): the ReLU masks of the two roles from the stored outputs, one launch."""
    dz0, dz1 = torch.empty_like(y0), torch.empty_like(y1)
    call_gcn_agg("subgc_gcn_agg_relu_bwd", _ptr(dy, torch.float32), _ptr(y0, torch.float32), _ptr(y1, torch.float32), _ptr(dz0), _ptr(dz1), dy.numel(), _stream())
    return dz0, dz1


def gemm_rowbias(a, b, out, *, ta=False, tb=False, bias=None, bias_scale=None, relu=False, accum=False):
    """`gemm` on fp32 operands with the bias of row m entering as bias_scale[m] * bias (subgc_gemm_f32_rowbias; bias_scale None = the
    plain bias): A (X W^T + 1 b^T) = (A X) W^T + rowsum(A) b^T."""
    M = a.size(1) if ta else a.size(0)
    K = a.size(0) if ta else a.size(1)
    N = b.size(0) if tb else b.size(1)
    if K != (b.size(1) if tb else b.size(0)) or out.size(0) < M or out.size(1) != N or (bias_scale is not None and bias_scale.numel() != M):
        raise SubgcError(f"gemm_rowbias shape mismatch: op(a)=[{M},{K}] op(b)=[..,{N}] out={tuple(out.shape)}")
    if FLOPS["on"]:
        FLOPS["gemm"] += 2.0 * M * N * K
        FLOPS["gemm_bytes"] += 4.0 * (M * K + K * N + M * N * (2 if accum else 1))
        FLOPS["gemm_calls"] += 1
    call_gcn_agg("subgc_gemm_f32_rowbias", int(ta), int(tb), M, N, K, _ptr(a, torch.float32), ld(a), _ptr(b, torch.float32), ld(b),
                 _ptr(out, torch.float32), ld(out), _ptr(bias, torch.float32), _ptr(bias_scale, torch.float32),
                 (RELU if relu else 0) | (ACCUM if accum else 0) | GEMM_MODES[gemm_mode.current] | gemm_tune.f32_bits, *_ws(a), _stream())
    return out


def gemm_pair_rowbias(a1, a2, b1, b2, out1, out2, *, tb=False, bias1=None, bias2=None, scale1=None, scale2=None, relu=False):
    """`gemm_pair` on fp32 operands with per-row bias scales and an optional ReLU (subgc_gemm_f32_pair_rowbias); operands that do not form
    a pair (or PAIR_LAUNCHES off) run as two `gemm_rowbias` calls."""
    same = (PAIR_LAUNCHES and a1.shape == a2.shape and b1.shape == b2.shape and out1.shape == out2.shape and ld(a1) == ld(a2) and ld(b1) == ld(b2)
            and ld(out1) == ld(out2) and (bias1 is None) == (bias2 is None) and (scale1 is None) == (scale2 is None))
    if not same:
        gemm_rowbias(a1, b1, out1, tb=tb, bias=bias1, bias_scale=scale1, relu=relu)
        gemm_rowbias(a2, b2, out2, tb=tb, bias=bias2, bias_scale=scale2, relu=relu)
        return out1, out2
    M, K = a1.shape
    N = b1.size(0) if tb else b1.size(1)
    if K != (b1.size(1) if tb else b1.size(0)) or out1.size(0) < M or out1.size(1) != N or (scale1 is not None and scale1.numel() != M):
        raise SubgcError(f"gemm_pair_rowbias shape mismatch: a=[{M},{K}] op(b)=[..,{N}] out={tuple(out1.shape)}")
    if FLOPS["on"]:
        FLOPS["gemm"] += 4.0 * M * N * K
        FLOPS["gemm_bytes"] += 2.0 * 4.0 * (M * K + K * N + M * N)
        FLOPS["gemm_calls"] += 1
    call_gcn_agg("subgc_gemm_f32_pair_rowbias", 0, int(tb), M, N, K, _ptr(a1, torch.float32), _ptr(a2, torch.float32), ld(a1), _ptr(b1, torch.float32),
                 _ptr(b2, torch.float32), ld(b1), _ptr(out1, torch.float32), _ptr(out2, torch.float32), ld(out1), _ptr(bias1, torch.float32),
                 _ptr(bias2, torch.float32), _ptr(scale1, torch.float32), _ptr(scale2, torch.float32),
                 (RELU if relu else 0) | GEMM_MODES[gemm_mode.current] | gemm_tune.f32_bits, *_ws(a1), _stream())
    return out1, out2


def colsum_rows(xs, ws, outs, accumulate=False):
    """outs[q][c] (+)= sum_i ws[q][i] * xs[q][i, c] for one or two fp32 matrices of one shape and leading dimension (subgc_colsum_rows_f32:
    slabs of rows, added in slab order -- no atomics).  The slab partials live in the registered GEMM workspace."""
    x0 = xs[0]
    M, N = x0.shape
    n = len(xs)
    if n not in (1, 2) or any(x.shape != x0.shape or ld(x) != ld(x0) for x in xs) or any(w.numel() != M for w in ws) or any(o.numel() != N for o in outs):
        raise SubgcError("colsum_rows: one or two matrices of one shape, one weight per row, one output per column")
    px = [_ptr(x, torch.float32) for x in xs] + [None] * (2 - n)
    pw = [_ptr(w, torch.float32) for w in ws] + [None] * (2 - n)
    po = [_ptr(o, torch.float32) for o in outs] + [None] * (2 - n)
    call_gcn_agg("subgc_colsum_rows_f32", n, px[0], px[1], ld(x0), M, N, pw[0], pw[1], po[0], po[1], int(accumulate), *_ws(x0), _stream())


def gcn_edges_fwd(F2, F3, rel_ind, skip, B, N, K, L):
    out = torch.empty(B, K, L, device=F2.device, dtype=torch.float32)
    call("subgc_gcn_edges_fwd", _ptr(F2), _ptr(F3), _ptr(rel_ind), _ptr(skip), _ptr(out), B, N, K, L, _stream())
    return out


def gcn_edges_bwd(dP, F2, F3, ptr, edges, B, N, K, L):
    dF2 = torch.empty(B, N, L, device=dP.device, dtype=torch.float32)
    dF3 = torch.empty_like(dF2)
    call("subgc_gcn_edges_bwd", _ptr(dP), _ptr(F2), _ptr(F3), _ptr(ptr), _ptr(edges), _ptr(dF2), _ptr(dF3), B, N, K, L, _stream())
    return dF2, dF3


def bn_fwd(x, gamma, beta, running_mean, running_var, training, momentum=0.1, eps=1e-5):
    M, C = x.shape
    y = torch.empty_like(x)
    sm = torch.empty(C, device=x.device, dtype=torch.float32) if training else None
    sr = torch.empty(C, device=x.device, dtype=torch.float32) if training else None
    call("subgc_bn_fwd", _ptr(x), _ptr(y), M, C, _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var),
         _ptr(sm), _ptr(sr), int(training), float(momentum), float(eps), *_ws(x), _stream())
    return y, sm, sr


def bn_bwd(dy, x, gamma, sm, sr):
    M, C = x.shape
    dx = torch.empty_like(x)
    dg = torch.empty(C, device=x.device, dtype=torch.float32)
    db = torch.empty_like(dg)
    call("subgc_bn_bwd", _ptr(dy), _ptr(x), _ptr(gamma), _ptr(sm), _ptr(sr), _ptr(dx), _ptr(dg), _ptr(db), M, C, *_ws(x), _stream())
    return dx, dg, db


def bn_stats(x, gamma, beta, running_mean, running_var, training, momentum=0.1, eps=1e-5):
    """Batch statistics of the raw unit output x [M, C] (fp32 or bf16) -> (aff [3, C] = mean | gamma * rstd | beta, rstd [C]); the
    consumer kernels normalise on load (subgc_bn_stats).  Eval mode: aff from the running statistics."""
    M, C = x.shape
    aff = torch.empty(3, C, device=x.device, dtype=torch.float32)
    rstd = torch.empty(C, device=x.device, dtype=torch.float32)
    if x.stride(0) != C or x.stride(1) != 1:
        raise SubgcError("bn_stats: contiguous rows needed")
    call("subgc_bn_stats", _ptr(x), int(is_b16(x)), M, C, _ptr(gamma, torch.float32), _ptr(beta, torch.float32), _ptr(running_mean, torch.float32),
         _ptr(running_var, torch.float32), _ptr(aff), _ptr(rstd), int(training), float(momentum), float(eps), *_ws(x), _stream())
    return aff, rstd


def bn_stats_pair(x0, x1, gamma0, beta0, rm0, rv0, gamma1, beta1, rm1, rv1, training, momentum=0.1, eps=1e-5):
    """`bn_stats` for the two units a fused aggregation consumes (same shape and storage type, training mode) in two launches instead of
    four (subgc_bn_stats_pair) -> ((aff0, rstd0), (aff1, rstd1))."""
    if (not training or not PAIR_LAUNCHES or x0.shape != x1.shape or x0.dtype != x1.dtype or rm0 is None or rm1 is None):
        return bn_stats(x0, gamma0, beta0, rm0, rv0, training, momentum, eps), bn_stats(x1, gamma1, beta1, rm1, rv1, training, momentum, eps)
    M, C = x0.shape
    if x0.stride(0) != C or x0.stride(1) != 1 or x1.stride(0) != C or x1.stride(1) != 1:
        raise SubgcError("bn_stats_pair: contiguous rows needed")
    aff0, aff1 = torch.empty(3, C, device=x0.device, dtype=torch.float32), torch.empty(3, C, device=x0.device, dtype=torch.float32)
    rstd0, rstd1 = torch.empty(C, device=x0.device, dtype=torch.float32), torch.empty(C, device=x0.device, dtype=torch.float32)
    f32 = torch.float32
    call("subgc_bn_stats_pair", _ptr(x0), _ptr(x1), int(is_b16(x0)), M, C, _ptr(gamma0, f32), _ptr(gamma1, f32), _ptr(beta0, f32), _ptr(beta1, f32),
         _ptr(rm0, f32), _ptr(rm1, f32), _ptr(rv0, f32), _ptr(rv1, f32), _ptr(aff0), _ptr(aff1), _ptr(rstd0), _ptr(rstd1), float(momentum), float(eps),
         *_ws(x0), _stream())
    return (aff0, rstd0), (aff1, rstd1)


def bn_bwd_fused_pair(dy0, dy1, x0, x1, gamma0, gamma1, aff0, aff1, rstd0, rstd1, dg0, dg1, db0, db1, accumulate):
    """`bn_bwd_fused` for both units in two launches instead of four (subgc_bn_bwd_fused_pair) -> (dx0, dx1)."""
    M, C = x0.shape
    dx0, dx1 = torch.empty_like(x0), torch.empty_like(x1)
    f32 = torch.float32
    call("subgc_bn_bwd_fused_pair", _ptr(dy0, f32), _ptr(dy1, f32), _ptr(x0), _ptr(x1), int(is_b16(x0)), M, C, _ptr(gamma0, f32), _ptr(gamma1, f32),
         _ptr(aff0, f32), _ptr(aff1, f32), _ptr(rstd0, f32), _ptr(rstd1, f32), _ptr(dx0), _ptr(dx1), int(is_b16(dx0)), _ptr(dg0, f32), _ptr(dg1, f32),
         _ptr(db0, f32), _ptr(db1, f32), int(accumulate), *_ws(x0), _stream())
    return dx0, dx1


def bn_bwd_fused(dy, x, gamma, aff, rstd, dgamma, dbeta, accumulate):
    """-> d(x) in x's storage type; dgamma / dbeta [C] written (or added to)."""
    M, C = x.shape
    dx = torch.empty_like(x)
    call("subgc_bn_bwd_fused", _ptr(dy, torch.float32), _ptr(x), int(is_b16(x)), M, C, _ptr(gamma, torch.float32), _ptr(aff, torch.float32),
         _ptr(rstd, torch.float32), _ptr(dx), int(is_b16(dx)), _ptr(dgamma, torch.float32), _ptr(dbeta, torch.float32), int(accumulate), *_ws(x), _stream())
    return dx


def gcn_nodes_fwd_bn(F0, F1, aff0, aff1, ptr, edges, skip, B, N, K, L, want16=False):
    out = torch.empty(B, N, L, device=F0.device, dtype=torch.float32)
    out16 = torch.empty(B, N, L, device=F0.device, dtype=BF16) if want16 else None
    act = torch.empty(B, N, L, device=F0.device, dtype=torch.uint8)
    call("subgc_gcn_nodes_fwd_bn", _ptr(F0), _ptr(F1), int(is_b16(F0)), _ptr(aff0, torch.float32), _ptr(aff1, torch.float32), _ptr(ptr), _ptr(edges),
         _ptr(skip, torch.float32), _ptr(out), _ptr(out16), _ptr(act), B, N, K, L, _stream())
    return out, out16, act


def gcn_edges_fwd_bn(F2, F3, aff2, aff3, rel_ind, skip, B, N, K, L, want16=False):
    out = torch.empty(B, K, L, device=F2.device, dtype=torch.float32)
    out16 = torch.empty(B, K, L, device=F2.device, dtype=BF16) if want16 else None
    call("subgc_gcn_edges_fwd_bn", _ptr(F2), _ptr(F3), int(is_b16(F2)), _ptr(aff2, torch.float32), _ptr(aff3, torch.float32), _ptr(rel_ind, torch.int64),
         _ptr(skip, torch.float32), _ptr(out), _ptr(out16), B, N, K, L, _stream())
    return out, out16


def gcn_edges_bwd_bn(dP, F2, F3, aff2, aff3, ptr, edges, B, N, K, L, bf16=False):
    dF2 = torch.empty(B, N, L, device=dP.device, dtype=BF16 if bf16 else torch.float32)
    dF3 = torch.empty_like(dF2)
    call("subgc_gcn_edges_bwd_bn", _ptr(dP, torch.float32), _ptr(F2), _ptr(F3), int(is_b16(F2)), _ptr(aff2, torch.float32), _ptr(aff3, torch.float32),
         _ptr(ptr), _ptr(edges), _ptr(dF2), _ptr(dF3), int(bf16), B, N, K, L, _stream())
    return dF2, dF3


def _pool_account(denom, G, L, fwd):
    if FLOPS["on"]:                      # untimed accounting step: the valid node rows of every sub-graph, not the padded N
        rows = float(denom[:G].cpu().sum())                  # host-side sum: the accounting step launches nothing of its own
        # fwd: read the member rows, write [max | mean] (+ arg-max);  bwd: read d[max | mean] + arg-max, read-modify-write the member rows
        FLOPS["pool_bytes"] = FLOPS.get("pool_bytes", 0.0) + 4.0 * ((rows * L + 3.0 * G * L) if fwd else (3.0 * G * L + 2.0 * rows * L))


def pool_fwd(X, idx, idx_stride, w, w_g, w_i, denom, img, G, N, L, want_argmax=True, out=None):
    _pool_account(denom, G, L, True)
    out = torch.empty(G, 2 * L, device=X.device, dtype=torch.float32) if out is None else out
    am = torch.empty(G, L, device=X.device, dtype=torch.int32) if want_argmax else None
    call("subgc_subgraph_pool_fwd", _ptr(X), _ptr(idx, torch.int64), idx_stride, _ptr(w, torch.float32), w_g, w_i,
         _ptr(denom, torch.float32), _ptr(img, torch.int32), _ptr(out), _ptr(am), G, N, L, _stream())
    return out, am


def pool_bwd(dout, idx, idx_stride, w, w_g, w_i, denom, img, am, dX, G, N, L):
    _pool_account(denom, G, L, False)
    call("subgc_subgraph_pool_bwd_ws", _ptr(dout), _ptr(idx, torch.int64), idx_stride, _ptr(w), w_g, w_i, _ptr(denom),
         _ptr(img, torch.int32), _ptr(am, torch.int32), _ptr(dX), G, N, L, dX.size(0), *_det_ws(dX), _stream())
    return dX


def gpn_score_fwd(hid, keep, scale, w2, b2, want_loss=True, out=None):
    G, H = hid.shape
    score = torch.empty(G, 1, device=hid.device, dtype=torch.float32) if out is None else out
    loss = torch.empty((), device=hid.device, dtype=torch.float32) if want_loss else None
    call("subgc_gpn_score_fwd", _ptr(hid), _ptr(keep, torch.uint8), float(scale), _ptr(w2), _ptr(b2), _ptr(score), _ptr(loss), G, H, _stream())
    return score, loss


def gpn_score_bwd(hid, keep, scale, w2, score, dloss):
    G, H = hid.shape
    dhid = torch.empty_like(hid)
    dw2 = torch.empty(1, H, device=hid.device, dtype=torch.float32)
    db2 = torch.empty(1, device=hid.device, dtype=torch.float32)
    call("subgc_gpn_score_bwd_ws", _ptr(hid), _ptr(keep, torch.uint8), float(scale), _ptr(w2), _ptr(score), _ptr(dloss), _ptr(dhid),
         _ptr(dw2), _ptr(db2), G, H, *_det_ws(hid), _stream())
    return dhid, dw2, db2


NMS_WORDS = 4


def subgraph_nms(score, idx, lens, thres, max_keep):
    """-> (keep[int64, M] buffer, n_keep int32[1]) both on device; caller syncs to read n_keep."""
    M, N = idx.shape
    keep = torch.empty(max(M, 1), device=score.device, dtype=torch.int64)
    n_keep = torch.zeros(1, device=score.device, dtype=torch.int32)
    scratch = torch.empty(max(M, 1) * (NMS_WORDS * 8 + 8), device=score.device, dtype=torch.uint8)
    call("subgc_subgraph_nms", _ptr(score, torch.float32), _ptr(idx, torch.int64), idx.stride(0), _ptr(lens, torch.int32), M, N,
         float(thres), int(max_keep), _ptr(keep), _ptr(n_keep), _ptr(scratch), scratch.numel(), _stream())
    return keep, n_keep


def subgraph_nms_batched(score, idx, lens, sizes, thres, max_keep, offsets=None, keep=None):
    """NMS of several images in ONE launch.  `sizes`: candidates per image (python ints, consecutive segments of score/idx/lens).
    `offsets` (device int32 [images + 1], optional): the segment offsets when the caller already has them on the device
    (subgc_gpn_test_prep writes them); `keep`: destination (int64, >= total elements).
    -> (keep int64 [total] with image b's kept indices (relative to its segment) at its segment start, n_keep int32 [images])."""
    total, N = idx.shape
    dev = score.device
    offs = [0]
    for n in sizes:
        offs.append(offs[-1] + int(n))
    if offsets is None:
        offsets = upload(offs, torch.int32, dev)                                  # one small upload
    keep = torch.empty(max(total, 1), device=dev, dtype=torch.int64) if keep is None else keep
    n_keep = zero_(torch.empty(len(sizes), device=dev, dtype=torch.int32))
    scratch = torch.empty(max(total, 1) * (NMS_WORDS * 8 + 8), device=dev, dtype=torch.uint8)
    call("subgc_subgraph_nms_batched", _ptr(score, torch.float32), _ptr(idx, torch.int64), idx.stride(0), _ptr(lens, torch.int32),
         _ptr(offsets, torch.int32), len(sizes), total, max(sizes) if sizes else 0, N, float(thres), int(max_keep), _ptr(keep, torch.int64), _ptr(n_keep),
         _ptr(scratch), scratch.numel(), _stream())
    return keep, n_keep, offs


def stack_first(groups):
    """groups: lists of per-image tensors (same shape / dtype within a list, 4- or 8-byte dtypes, contiguous).  -> one stacked tensor
    per list holding block [0] of every image ([I, *shape[1:]]), built by subgc_gather_blocks from ONE uploaded address table."""
    dev = groups[0][0].device
    ptrs, alive = [], []
    for ts in groups:
        for t in ts:
            t = t if t.is_contiguous() else t.contiguous()
            alive.append(t)
            ptrs.append(t.data_ptr())
    table = upload(ptrs, torch.int64, dev)
    outs, o = [], 0
    for ts in groups:
        I, t0 = len(ts), ts[0]
        words = t0[0].numel() * t0.element_size() // 4
        out = torch.empty((I,) + tuple(t0.shape[1:]), device=dev, dtype=t0.dtype)
        call("subgc_gather_blocks", _ptr(table[o:o + I], torch.int64), I, words, out.data_ptr(), _stream())
        outs.append(out)
        o += I
    return outs


def decode_batch_finish(seq, seqlp, bounds):
    """The per-image early break of a batched decode (subgc_decode_batch_finish): zeroes seqlp beyond each image's break step in
    place; `bounds`: python list of row bounds per image.  -> int32 [images, 2] on the device: (break step, stopped at all)."""
    dev = seq.device
    b = upload(bounds, torch.int32, dev)                                            # one small upload
    out = torch.empty(len(bounds) - 1, 2, device=dev, dtype=torch.int32)
    if not (seq.is_contiguous() and seqlp.is_contiguous()):
        raise SubgcError("decode_batch_finish: contiguous seq / seqlp")
    call("subgc_decode_batch_finish", _ptr(seq, torch.int64), _ptr(seqlp, torch.float32), _ptr(b, torch.int32), len(bounds) - 1, seq.size(1), _ptr(out),
         _stream())
    return out


_PINNED = {}


def upload(values, dtype, device):
    """A small host list -> device tensor through a PINNED staging buffer and an asynchronous copy on the current stream.  (A pageable
    `torch.tensor(...).to(device)` makes the host wait until the stream has drained -- in the one-image decode that is the whole previous
    image's token loop.)  Two staging buffers per (device, dtype) alternate; every caller reads something back from the device
    (survivor counts, finished beams) before it comes here a third time; an event per buffer makes that a guarantee."""
    n = len(values)
    key = (str(device), dtype)
    ring = _PINNED.get(key)
    if ring is None or ring[0][0][0].numel() < n:
        for _, busy in (ring[0] if ring is not None else ()):     # growing: the old staging buffers may still be the source of a copy in flight
            if busy is not None:
                busy.synchronize()
        cap = max(256, 1 << (max(n, 1) - 1).bit_length())
        ring = _PINNED[key] = [[[torch.empty(cap, dtype=dtype).pin_memory(), None] for _ in range(2)], 0]
    slots, turn = ring
    ring[1] = turn ^ 1
    buf, busy = slots[turn]
    if busy is not None:
        busy.synchronize()                                     # the copy that last read this staging buffer (long done in every caller's flow)
    stage = buf[:n]
    stage.copy_(torch.tensor(values, dtype=dtype))
    out = stage.to(device, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    slots[turn][1] = ev
    return out


def nms_compact(keep_all, n_keep, offsets32, images, total):
    """-> (keep int64 [total], glob int64 [total]): the NMS survivors in image order (subgc_nms_compact)."""
    dev = keep_all.device
    keep = torch.empty(total, device=dev, dtype=torch.int64)
    glob = torch.empty(total, device=dev, dtype=torch.int64)
    call("subgc_nms_compact", _ptr(keep_all, torch.int64), _ptr(n_keep, torch.int32), _ptr(offsets32, torch.int32), int(images), int(total),
         _ptr(keep), _ptr(glob), _stream())
    return keep, glob


def gpn_test_prep(items, N, device, out=None):
    """The sGPN test branch's input views for a list of images in ONE launch (subgc_gpn_test_prep; gpn.py:84-96 reads counterpart 0
    of the loader's five copies).  items: (row, gpn_obj_ind [5,2,M,N], att_masks [5,2,M,N], gpn_pool_mtx [5,2,M,N,N]) per image.
    One small upload (the segment offsets and the three tensor addresses per image); no torch op touches the loader tensors.
    `out`: namespace with idx / lens capacity buffers to write into (the one-image decode's static buffers).
    -> (idx int64 [G,N], w [G,N], denom fp32 [G], lens int32 [G], img int32 [G], offsets32 int32 [images+1], sizes, keepalive)"""
    sizes = [int(g.size(1) * g.size(2)) for _, g, _, _ in items]
    offs = [0]
    for n in sizes:
        offs.append(offs[-1] + n)
    G, I = offs[-1], len(items)
    alive, words = [], list(offs)
    for row, g, a, p_ in items:
        g, a, p_ = (t if t.is_contiguous() else t.contiguous() for t in (g, a, p_))
        if g.dtype != torch.int64 or a.dtype != torch.float32 or p_.dtype != torch.float32:
            raise SubgcError("gpn_test_prep: gpn_obj_ind int64, att_masks / gpn_pool_mtx fp32")
        alive += [g, a, p_]
        words += [g.data_ptr(), p_.data_ptr(), a.data_ptr(), int(row)]
    table = upload(words, torch.int64, device)                                      # the one upload of the selection phase (pinned, asynchronous)
    e = lambda *sh, dt=torch.float32: torch.empty(*sh, device=device, dtype=dt)
    idx = out.idx[:G] if out is not None else e(max(G, 0), N, dt=torch.int64)
    lens = out.lens[:G] if out is not None else e(G, dt=torch.int32)
    w, denom, img, o32 = e(G, N), e(G), e(G, dt=torch.int32), e(I + 1, dt=torch.int32)
    call("subgc_gpn_test_prep", _ptr(table, torch.int64), I, G, N, _ptr(idx, torch.int64), _ptr(w), _ptr(denom), _ptr(lens, torch.int32), _ptr(img, torch.int32),
         _ptr(o32, torch.int32), _stream())
    return idx, w, denom, lens, img, o32, sizes, (alive, table)


def _words(t):
    """A contiguous tensor of a 4- or 8-byte dtype as its [rows, 4-byte words] float32 view (bit-level row operations)."""
    if not t.is_contiguous() or t.element_size() not in (4, 8):
        raise SubgcError(f"need a contiguous 4- or 8-byte tensor, got {t.dtype} {tuple(t.shape)} / {t.stride()}")
    t2 = t.view(t.size(0), -1) if t.dim() >= 1 and t.numel() else t.reshape(max(t.size(0) if t.dim() else 1, 0), -1)
    return t2.view(torch.float32) if t2.dtype != torch.float32 else t2


def zero_(t):
    """t[...] = 0 for a contiguous tensor of any 4- or 8-byte dtype (all-zero bits; subgc_fill_f32 on the word view)."""
    if t.numel():
        fill_(_words(t.view(-1, 1) if t.dim() == 1 else t), 0.0)
    return t


def copy_(dst, src):
    """Bit copy between contiguous tensors of one dtype and shape (subgc_copy2d_f32 on the word views)."""
    if dst.dtype != src.dtype or dst.shape != src.shape:
        raise SubgcError(f"copy_: {src.dtype} {tuple(src.shape)} -> {dst.dtype} {tuple(dst.shape)}")
    if src.numel():
        a, b = _words(src.view(1, -1)), _words(dst.view(1, -1))
        call("subgc_copy2d_f32", _ptr(a), a.size(1), _ptr(b), b.size(1), 1, a.size(1), 0, _stream())
    return dst


def take_rows(pairs, rows):
    """dst[m] = src[rows[m]] for up to four (src, dst) pairs of any 4- / 8-byte dtype in ONE launch, `rows` int64 on the device
    (subgc_gather_rows_multi_i64): 1-D tensors count as one-column rows."""
    if not 1 <= len(pairs) <= 4:
        raise SubgcError("take_rows takes 1..4 (src, dst) pairs")
    M = rows.numel()
    args = []
    for src, dst in list(pairs) + [(None, None)] * (4 - len(pairs)):
        if src is None:
            args += [None, 0, None, 0, 0]
            continue
        a = _words(src.view(-1, 1) if src.dim() == 1 else src)
        b = _words(dst.view(-1, 1) if dst.dim() == 1 else dst)
        if a.size(1) != b.size(1) or b.size(0) < M:
            raise SubgcError("take_rows: row widths differ or the destination is too short")
        args += [_ptr(a), a.stride(0), _ptr(b), b.stride(0), a.size(1)]
    call("subgc_gather_rows_multi_i64", len(pairs), *args, _ptr(rows, torch.int64), M, _stream())


def pack_rows(lens, idx, img, S, N, off=None):
    dev = lens.device
    off = torch.empty(S, device=dev, dtype=torch.int32) if off is None else off
    total = torch.empty(1, device=dev, dtype=torch.int32)
    src = torch.empty(S * N, device=dev, dtype=torch.int32)
    sent = torch.empty(S * N, device=dev, dtype=torch.int32)
    call("subgc_pack_rows", _ptr(lens, torch.int32), _ptr(idx, torch.int64), idx.stride(0), _ptr(img, torch.int32), S, N,
         _ptr(off), _ptr(total), _ptr(src), _ptr(sent), _stream())
    return off, total, src, sent


def embed_fwd(table, tok, tok_stride, keep, scale, out):
    """out [n, E] fp32 or bf16 (contiguous rows)."""
    n, E = out.shape
    call("subgc_embed_fwd", _ptr(table), _ptr(tok, torch.int64), tok_stride, _ptr(keep, torch.uint8), float(scale), _ptr(out), n, E,
         table.size(0), int(is_b16(out)), _stream())
    return out


def token_rows(table, tok, out, tok_stride=1):
    """out[r] = table[tok[r]] (int64 tokens): the decode-time lookup into a per-token table (subgc_token_rows_f32)."""
    call("subgc_token_rows_f32", _ptr(table, torch.float32), ld(table), _ptr(tok, torch.int64), tok_stride, _ptr(out, torch.float32), ld(out),
         out.size(0), out.size(1), table.size(0), _stream())
    return out


def lstm_gate_perm(R, device):
    """Row order of the permuted gate matrix subgc_lstm_step_skinny reads: row 16*b + 4*g + u <- gate g of unit 4*b + u."""
    p = torch.arange(4 * R, device=device)
    return (p % 16 // 4) * R + (p // 16) * 4 + p % 4


def lstm_step_skinny(x, w_perm, c_prev, c, hs, b0=None, b1=None, add1=None, tok=None, add2=None):
    """One LSTMCell step for <= 16 rows, GEMM + cell update in one launch (subgc_lstm_step_skinny).  `hs`: up to three 2-D
    views that receive h (none may alias x)."""
    S, K = x.shape
    R = c.size(1)
    hs = list(hs) + [None] * (3 - len(hs))
    hp = []
    for h_ in hs:
        hp += [_ptr(h_, torch.float32), ld(h_) if h_ is not None else 0]
    call("subgc_lstm_step_skinny", _ptr(x, torch.float32), ld(x), _ptr(w_perm), ld(w_perm), K, S, R,
         _ptr(add1, torch.float32), ld(add1) if add1 is not None else 0, _ptr(tok, torch.int64), add1.size(0) if tok is not None else 0,
         _ptr(add2, torch.float32), ld(add2) if add2 is not None else 0, _ptr(b0, torch.float32), _ptr(b1, torch.float32),
         _ptr(c_prev, torch.float32), _ptr(c, torch.float32), *hp, int(is_b16(w_perm)), _stream())


def gemm_skinny_wb16(x, W16, out, bias=None, relu=False):
    """out = act(x W16^T + bias) for <= 16 fp32 rows against a bf16-STORED weight matrix, fp32 accumulation (subgc_gemm_skinny_wb16:
    the h2att and logit products of a bf16 decode step)."""
    M, K = x.shape
    call("subgc_gemm_skinny_wb16", _ptr(x, torch.float32), ld(x), _ptr(W16, BF16), ld(W16), _ptr(out, torch.float32), ld(out),
         _ptr(bias, torch.float32), M, W16.size(0), K, int(relu), _stream())
    return out


PICK_BEST_ELEMS = 16 * 8 * 16       # uint64 slots of one `best` buffer of the fused greedy pick (subgc_hip.h)


def skinny_dual(x1, W1, out1, x2, W2, out2, bias1=None, bias2=None, unperm1_R=0, unperm2_R=0, best=None, lse_part=None):
    """Two weight-streaming products of <= 16 rows in one launch (subgc_skinny_dual): out1 = x1 W1^T (+ bias1) -- or, with `best`, the fused
    arg-max / log-sum-exp partials (packed arg-max by 64-bit atomicMax into `best`, per-workgroup (max, sum exp) into `lse_part`) instead of (or beside) out1 -- and out2 = x2 W2^T (+ bias2).  unperm*_R: W's rows are
    in the permuted LSTM gate order, the result is written gate-major."""
    S = x1.size(0)
    b16 = is_b16(W1)
    if is_b16(W2) != b16:
        raise SubgcError("skinny_dual: both weight matrices fp32 or both bf16")
    call("subgc_skinny_dual", S, _ptr(x1, torch.float32), ld(x1), _ptr(W1), ld(W1), _ptr(bias1, torch.float32), W1.size(0), x1.size(1),
         _ptr(out1, torch.float32), ld(out1) if out1 is not None else 0, int(unperm1_R), _ptr(best, torch.int64), _ptr(lse_part, torch.float32),
         _ptr(x2, torch.float32), ld(x2), _ptr(W2), ld(W2), _ptr(bias2, torch.float32), W2.size(0), x2.size(1), _ptr(out2, torch.float32), ld(out2),
         int(unperm2_R), int(b16), _stream())


def lstm_cell_pick(pre, c_prev, c, hs, b0, b1, table, add2, tok=None, pick=None, best_reset=None):
    """The attention LSTM's cell of a greedy decode step from gate-major pre-activations (subgc_lstm_cell_pick).  `pick` = (best_prev,
    unf_in, unf_out, seq, t_prev, count_out, prev_count), or None with `tok` [S] int64 (step 0)."""
    S, R = c.shape
    hs = list(hs) + [None] * (3 - len(hs))
    hp = []
    for h_ in hs:
        hp += [_ptr(h_, torch.float32), ld(h_) if h_ is not None else 0]
    if pick is not None:
        best_prev, unf_in, unf_out, seq, t_prev, count_out, prev_count = pick
        pk = [_ptr(best_prev, torch.int64), _ptr(unf_in, torch.int32), _ptr(unf_out, torch.int32), _ptr(seq, torch.int64), seq.size(1), int(t_prev),
              _ptr(count_out, torch.int32), _ptr(prev_count, torch.int32), _ptr(best_reset, torch.int64)]
    else:
        pk = [None, None, None, None, 0, 0, None, None, None]
    call("subgc_lstm_cell_pick", _ptr(pre, torch.float32), ld(pre), S, R, _ptr(table, torch.float32), ld(table), _ptr(tok, torch.int64), table.size(0),
         _ptr(add2, torch.float32), ld(add2) if add2 is not None else 0, _ptr(b0, torch.float32), _ptr(b1, torch.float32), _ptr(c_prev, torch.float32),
         _ptr(c, torch.float32), *hp, *pk, _stream())


def pick_file(best_prev, unf_in, unf_out, seq, t_prev, count_out, prev_count):
    call("subgc_pick_file", _ptr(best_prev, torch.int64), _ptr(unf_in, torch.int32), _ptr(unf_out, torch.int32), _ptr(seq, torch.int64), seq.size(0),
         seq.size(1), int(t_prev), _ptr(count_out, torch.int32), _ptr(prev_count, torch.int32), _stream())


def pick_lse_finish(lse_part, V, counts, seqlp):
    S, T = seqlp.shape
    call("subgc_pick_lse_finish", _ptr(lse_part, torch.float32), int(V), S, T, _ptr(counts, torch.int32), _ptr(seqlp, torch.float32), _stream())


def embed_bwd(table, tok, tok_stride, keep, scale, dout, dtable):
    n, E = dout.shape
    call("subgc_embed_bwd_ws", _ptr(table), _ptr(tok, torch.int64), tok_stride, _ptr(keep, torch.uint8), float(scale), _ptr(dout),
         _ptr(dtable), n, E, table.size(0), *_det_ws(dout), _stream())
    return dtable


def _same_storage(*ts):
    """1 when the (non-None) h destinations are bf16, 0 when fp32; mixing is an error."""
    kinds = {is_b16(t) for t in ts if t is not None}
    if len(kinds) > 1:
        raise SubgcError("the h destinations of one LSTM call must all be fp32 or all be bf16")
    return int(kinds.pop()) if kinds else 0


def lstm_fwd(g0, g1, g2, b0, b1, c_prev, c, h, h2, keep, scale, hdrop, gates, S, R, rows_h=0, rows_h2=0):
    L = lambda t: ld(t) if t is not None else 0
    call("subgc_lstm_fwd", _ptr(g0), L(g0), _ptr(g1), L(g1), _ptr(g2), L(g2), _ptr(b0), _ptr(b1), _ptr(c_prev), _ptr(c),
         _ptr(h), L(h), _ptr(h2), L(h2), _ptr(keep, torch.uint8), float(scale), _ptr(hdrop), L(hdrop), _ptr(gates), S, R, int(rows_h),
         int(rows_h2), _same_storage(h, h2, hdrop), _stream())


def lstm_fwd_gemm(x, w, pre, g1, g2, b0, b1, c_prev, c, h, h2, keep, scale, hdrop, gates, S, R, rows_h=0, rows_h2=0):
    """gemm(x, w^T) + lstm_fwd with the split-K reduce folded into the cell kernel (subgc_lstm_fwd_gemm); `pre` [S, 4R] is scratch.
    x, w both fp32 or both bf16; h / h2 / hdrop all fp32 or all bf16."""
    L = lambda t: ld(t) if t is not None else 0
    K = x.size(1)
    xb = int(is_b16(x))
    if is_b16(w) != bool(xb):
        raise SubgcError("lstm_fwd_gemm: x and w must have the same storage type")
    if FLOPS["on"]:                      # same accounting as ops.gemm: the product is the same launch family
        eb = 2.0 if xb else 4.0
        FLOPS["gemm"] += 2.0 * S * 4 * R * K
        FLOPS["gemm_bytes"] += eb * (S * K + K * 4 * R) + 4.0 * S * 4 * R
        FLOPS["gemm_calls"] += 1
    call("subgc_lstm_fwd_gemm", _ptr(x), ld(x), _ptr(w), ld(w), K, _ptr(pre, torch.float32), ld(pre),
         _ptr(g1), L(g1), _ptr(g2), L(g2), _ptr(b0), _ptr(b1), _ptr(c_prev), _ptr(c), _ptr(h), L(h), _ptr(h2), L(h2),
         _ptr(keep, torch.uint8), float(scale), _ptr(hdrop), L(hdrop), _ptr(gates), S, R, int(rows_h), int(rows_h2),
         xb | (_same_storage(h, h2, hdrop) << 1), GEMM_MODES[gemm_mode.current], *_ws(x), _stream())


def gemm_planes(a, b, planes, *, ta=False, tb=False):
    """op(a) @ op(b) left as n fp32 partial planes planes[q][M][N] whose sum is the product (subgc_gemm_*_planes: the split-K forms
    without their reduce pass; n = 1 when the dispatch does not split).  `planes`: a flat fp32 buffer of >= 8*M*N elements.
    -> (n, M * N)"""
    import ctypes
    M = a.size(1) if ta else a.size(0)
    K = a.size(0) if ta else a.size(1)
    N = b.size(0) if tb else b.size(1)
    if K != (b.size(1) if tb else b.size(0)):
        raise SubgcError("gemm_planes: shape mismatch")
    n = ctypes.c_int(0)
    if FLOPS["on"]:
        eb = 2.0 if is_b16(a) else 4.0
        FLOPS["gemm"] += 2.0 * M * N * K
        FLOPS["gemm_bytes"] += eb * (M * K + K * N) + 4.0 * M * N
        FLOPS["gemm_calls"] += 1
    if is_b16(a) or is_b16(b):
        if not (is_b16(a) and is_b16(b)):
            raise SubgcError("gemm_planes: both operands bf16 or both fp32")
        call("subgc_gemm_bf16_planes", int(ta), int(tb), M, N, K, _ptr(a, BF16), ld(a), _ptr(b, BF16), ld(b), _ptr(planes, torch.float32), planes.numel() * 4,
             ctypes.byref(n), _stream())
    else:
        call("subgc_gemm_f32_planes", int(ta), int(tb), M, N, K, _ptr(a, torch.float32), ld(a), _ptr(b, torch.float32), ld(b), _ptr(planes, torch.float32),
             planes.numel() * 4, ctypes.byref(n), GEMM_MODES[gemm_mode.current] | gemm_tune.f32_bits, _stream())
    return n.value, M * N


RECURRENCE_IN_C = True        # the train decoder's T-step loops as one C call per direction (subgc_recurrence_fwd / _bwd); False = step by step from Python
# The state entering step 0 of the train decoder is zero (init_hidden) and nothing reads its gradient: step 0 then forms no product
# against it (SubgcRecurrence.zero_state and the same launches in the Python loops), and the weight gradients whose x operand is a
# previous state contract over the rows after step 0 only.  False = every step issues the same launches.
ZERO_STATE_SKIP = True
_RECUR_T = None


class Recurrence:
    """Argument block of subgc_recurrence_fwd / subgc_recurrence_bwd (include/subgc_hip.h: SubgcRecurrence, mirrored from the header).
    Tensors go in as device pointers, python int lists (`m`, `row0`, `hout_off`, `dhout_off`) as host arrays owned by this object,
    everything else by value; fields not given stay 0 / NULL."""

    HOST = {"m": "c_int32", "row0": "c_int64", "hout_off": "c_int64", "dhout_off": "c_int64"}

    def __init__(self, **fields):
        import ctypes
        global _RECUR_T
        if _RECUR_T is None:
            from ._lib import lib, parse_struct
            _RECUR_T = parse_struct("SubgcRecurrence")
            if ctypes.sizeof(_RECUR_T) != int(lib().subgc_recurrence_sizeof()):
                raise SubgcError("SubgcRecurrence: the ctypes mirror and the library disagree about the struct layout")
        self.st = _RECUR_T()
        self._alive = []
        self.host = {}                                                  # the python lists behind the host-array fields (m, row0, ...)
        self.set(**fields)

    def set(self, **fields):
        import ctypes
        exp = _recurrence_field_types()
        for k, v in fields.items():
            if v is None:
                setattr(self.st, k, 0)                                  # NULL pointer / zero
            elif torch.is_tensor(v):
                if not v.is_cuda:
                    raise SubgcError(f"recurrence: {k} must be a device tensor")
                want = exp.get(k)
                if want is None:
                    raise SubgcError(f"recurrence: {k} is not a pointer field of SubgcRecurrence")
                if want != "any" and v.dtype != want:
                    raise SubgcError(f"recurrence: {k} is declared {want} in subgc_hip.h, got {v.dtype}")
                if want == "any" and v.dtype not in (torch.float32, torch.bfloat16, torch.uint16, torch.int16):
                    raise SubgcError(f"recurrence: {k} must be fp32 or bf16 storage, got {v.dtype}")
                if v.dim() >= 2 and v.stride(-1) != 1:
                    raise SubgcError(f"recurrence: {k} needs unit inner stride (shape {tuple(v.shape)}, stride {v.stride()})")
                if v.dim() <= 1 and not v.is_contiguous():
                    raise SubgcError(f"recurrence: {k} must be contiguous")
                setattr(self.st, k, v.data_ptr())
            elif k in self.HOST:
                arr = (getattr(ctypes, self.HOST[k]) * max(len(v), 1))(*[int(x) for x in v])
                self._alive.append(arr)
                self.host[k] = [int(x) for x in v]
                setattr(self.st, k, ctypes.addressof(arr))
                if k in ("m", "row0"):
                    setattr(self.st, "n_" + k, len(v))                  # the library checks >= T + 1 (it reads m[T] / row0[T])
            else:
                setattr(self.st, k, v)
        return self


_RECUR_TYPES = None


def _recurrence_field_types():
    """field -> expected torch dtype of every POINTER member of SubgcRecurrence, read from the header (`const float*` -> float32,
    `const int32_t*` -> int32, `const uint8_t*` -> uint8, `void*` -> "any": fp32 or bf16 storage by the `bf16` flags)."""
    global _RECUR_TYPES
    if _RECUR_TYPES is None:
        import re
        from ._lib import HEADER
        src = open(HEADER).read()
        src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
        body = re.search(r"typedef\s+struct\s+SubgcRecurrence\s*\{(.*?)\}\s*SubgcRecurrence\s*;", src, flags=re.S).group(1)
        table = {"float": torch.float32, "int32_t": torch.int32, "int64_t": torch.int64, "uint8_t": torch.uint8, "uint16_t": "any", "void": "any"}
        out = {}
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if "*" in decl:
                ty = decl.split("*")[0].replace("const", "").strip()
                out[decl.split("*")[-1].strip()] = table[ty]
        _RECUR_TYPES = out
    return _RECUR_TYPES


def recurrence_fwd(rec, like):
    import ctypes
    call("subgc_recurrence_fwd", ctypes.addressof(rec.st), *_ws(like), _stream())


def recurrence_bwd(rec):
    import ctypes
    call("subgc_recurrence_bwd", ctypes.addressof(rec.st), _stream())



def recurrence_ok():
    """The C loops apply unless a measurement mode needs the per-call Python wrappers (FLOP accounting, GEMM dispatch switches)."""
    return RECURRENCE_IN_C and not FLOPS["on"] and gemm_tune.f32_bits == 0


def lstm_bwd_planes(gates, c_prev, c, srcs, dh_drop, keep, scale, dc, dpre, dc_prev, S, R):
    """lstm_bwd whose d(h) sources are column windows of split-K plane stacks: srcs = up to three (planes, N, col0, n, stride, rows)
    -- `planes` the flat buffer gemm_planes filled ([n][rows][N]), the window starts at column col0; n = 0 entries are skipped."""
    args = []
    srcs = [x for x in srcs if x is not None and x[3] > 0]
    for k in range(3):
        if k < len(srcs):
            buf, N, col0, n, stride, rows = srcs[k]
            args += [buf.data_ptr() + 4 * col0, N, n, stride, rows]
        else:
            args += [None, 0, 0, 0, 0]
    L = lambda t: ld(t) if t is not None else 0
    call("subgc_lstm_bwd_planes", _ptr(gates), _ptr(c_prev), _ptr(c), *args, _ptr(dh_drop), L(dh_drop), _ptr(keep, torch.uint8), float(scale), _ptr(dc),
         _ptr(dpre), _ptr(dc_prev), S, R, int(is_b16(dpre)), _stream())


def lstm_bwd(gates, c_prev, c, dh_a, dh_b, dh_drop, keep, scale, dc, dpre, dc_prev, S, R):
    """dpre [S, 4R] contiguous rows, fp32 or bf16 (the gate gradients only feed GEMMs and bias sums)."""
    L = lambda t: ld(t) if t is not None else 0
    call("subgc_lstm_bwd", _ptr(gates), _ptr(c_prev), _ptr(c), _ptr(dh_a), L(dh_a), _ptr(dh_b), L(dh_b), _ptr(dh_drop), L(dh_drop),
         _ptr(keep, torch.uint8), float(scale), _ptr(dc), _ptr(dpre), _ptr(dc_prev), S, R, int(is_b16(dpre)), _stream())


def _attn_account(lens, S, A, R, passes):
    if FLOPS["on"]:                      # untimed accounting step: algorithmic bytes of the ragged attention sets
        FLOPS["attn_bytes"] = FLOPS.get("attn_bytes", 0.0) + 4.0 * float(lens[:S].cpu().sum()) * (A + R) * passes


def _uv_b16(u, v, A, R):
    """1 when the node features u [rows, A] / v [rows, R] are the bf16 tensors of compute_dtype = bf16 (both, contiguous rows)."""
    b = is_b16(u)
    if b != is_b16(v):
        raise SubgcError("attention: u and v must have the same storage type")
    if b and (ld(u) != A or ld(v) != R):
        raise SubgcError("attention: bf16 node features must have contiguous rows")
    return int(b)


def attn_fwd(u, v, ah, w_a, b_a, off, lens, ctx, alpha, S, A, R, q=None):
    """`q` = (planes, n, stride, bias): the query rows are the n split-K partial planes `gemm_planes` left in `planes` (+ bias); the
    summed rows are written to `ah` (subgc_attn_fwd_q)."""
    _attn_account(lens, S, A, R, 1)      # read u and v rows once
    if q is not None:
        planes, n, stride, bias = q
        call("subgc_attn_fwd_q", _ptr(u), _ptr(v), _ptr(planes, torch.float32), int(n), int(stride), _ptr(bias, torch.float32), _ptr(ah, torch.float32),
             _ptr(w_a), _ptr(b_a), _ptr(off, torch.int32), _ptr(lens, torch.int32), _ptr(ctx), ld(ctx), _ptr(alpha), alpha.size(1) if alpha is not None else 0,
             S, A, R, int(is_b16(ctx)) | (_uv_b16(u, v, A, R) << 1), _stream())
        return
    call("subgc_attn_fwd", _ptr(u), _ptr(v), _ptr(ah), _ptr(w_a), _ptr(b_a), _ptr(off, torch.int32), _ptr(lens, torch.int32),
         _ptr(ctx), ld(ctx), _ptr(alpha), alpha.size(1) if alpha is not None else 0, S, A, R, int(is_b16(ctx)) | (_uv_b16(u, v, A, R) << 1), _stream())


def _dctx_args(dctx):
    """d(ctx) as (pointer, ld, planes, plane stride): a 2-D view, or a window (planes, N, col0, n, stride, rows) of a plane stack."""
    if isinstance(dctx, tuple):
        buf, N, col0, n, stride, _rows = dctx
        return buf.data_ptr() + 4 * col0, N, n, stride
    return _ptr(dctx, torch.float32), ld(dctx), 1, 0


def attn_bwd(u, v, ah, w_a, off, lens, alpha, dctx, dah, du, dv, dw_a, db_a, S, A, R, dctx_keep=None, de_keep=None):
    """dv None: d(v) is deferred to one `attn_dv_accum` after the time loop; `dctx_keep` [S, R] then receives this step's d(ctx) rows.
    `de_keep` [S, n] (then du is not touched): d(u) is deferred likewise to one `attn_du_accum`.
    `dctx`: a 2-D view or a plane-stack window (see _dctx_args): the split-K planes of the data-gradient GEMM are summed on load."""
    _attn_account(lens, S, A, R, 3 if dv is not None else 2)      # read u, v; read-modify-write du (and dv)
    dp, dl, dn, ds = _dctx_args(dctx)
    if de_keep is not None:
        if de_keep.stride(0) != alpha.size(1) or alpha.stride(0) != alpha.size(1):
            raise SubgcError("attn_bwd: de_keep rows must have alpha's pitch")
        call("subgc_attn_bwd_planes_de", _ptr(u), _ptr(v), _ptr(ah), _ptr(w_a), _ptr(off, torch.int32), _ptr(lens, torch.int32), _ptr(alpha),
             alpha.size(1), dp, dl, dn, ds, _ptr(dah), _ptr(de_keep, torch.float32), _ptr(dv), _ptr(dw_a), _ptr(db_a), S, A, R,
             int(is_b16(dah)) | (_uv_b16(u, v, A, R) << 1), _ptr(dctx_keep, torch.float32), ld(dctx_keep) if dctx_keep is not None else 0, _stream())
        return
    call("subgc_attn_bwd_planes", _ptr(u), _ptr(v), _ptr(ah), _ptr(w_a), _ptr(off, torch.int32), _ptr(lens, torch.int32), _ptr(alpha),
         alpha.size(1), dp, dl, dn, ds, _ptr(dah), _ptr(du), _ptr(dv), _ptr(dw_a), _ptr(db_a), S, A, R,
         int(is_b16(dah)) | (_uv_b16(u, v, A, R) << 1), _ptr(dctx_keep, torch.float32), ld(dctx_keep) if dctx_keep is not None else 0, _stream())


def attn_dv_accum(alpha, dctx, step_off, T, off, lens, dv, S, R):
    """d(v) of all time steps in one pass (subgc_attn_dv_accum): alpha [rows, n], dctx [rows, R] hold step t's live sentences as
    rows step_off[t] .. step_off[t+1]-1; dv [sum lens, R] is overwritten."""
    call("subgc_attn_dv_accum", _ptr(alpha, torch.float32), alpha.size(1), _ptr(dctx, torch.float32), ld(dctx), _ptr(step_off, torch.int32), int(T),
         _ptr(off, torch.int32), _ptr(lens, torch.int32), _ptr(dv, torch.float32), S, R, _stream())


def attn_du_accum(u, ah, de, step_off, T, off, lens, w_a, du, S, A):
    """d(u) of all time steps in one pass (subgc_attn_du_accum): ah [rows, A] (the query rows the forward saved), de [rows, n] hold step
    t's live sentences as rows step_off[t] .. step_off[t+1]-1; du [sum lens, A] is overwritten."""
    call("subgc_attn_du_accum", _ptr(u), int(is_b16(u)), _ptr(ah, torch.float32), _ptr(de, torch.float32), de.size(1), _ptr(step_off, torch.int32), int(T),
         _ptr(off, torch.int32), _ptr(lens, torch.int32), _ptr(w_a, torch.float32), _ptr(du, torch.float32), S, A, _stream())


def attn_fwd_group(u, v, ah, w_a, b_a, rows, lens, m, B, g, Nn, ctx, alpha, A, R, q=None):
    """Attention step over per-image shared sets (subgc_attn_fwd_group): ah / ctx / alpha hold the step's rows.  `q`: see attn_fwd."""
    _attn_account_group(B, Nn, A, R, 1)
    if q is not None:
        planes, n, stride, bias = q
        call("subgc_attn_fwd_group_q", _ptr(u), _ptr(v), _ptr(planes, torch.float32), int(n), int(stride), _ptr(bias, torch.float32), _ptr(ah, torch.float32),
             _ptr(w_a), _ptr(b_a), _ptr(rows, torch.int32), _ptr(lens, torch.int32), int(m), B, g, Nn, _ptr(ctx), ld(ctx), _ptr(alpha),
             alpha.size(1) if alpha is not None else 0, A, R, int(is_b16(ctx)) | (_uv_b16(u, v, A, R) << 1), _stream())
        return
    call("subgc_attn_fwd_group", _ptr(u), _ptr(v), _ptr(ah, torch.float32), _ptr(w_a), _ptr(b_a), _ptr(rows, torch.int32), _ptr(lens, torch.int32), int(m),
         B, g, Nn, _ptr(ctx), ld(ctx), _ptr(alpha), alpha.size(1) if alpha is not None else 0, A, R, int(is_b16(ctx)) | (_uv_b16(u, v, A, R) << 1), _stream())


def attn_bwd_group(u, v, ah, w_a, rows, lens, m, B, g, Nn, alpha, dctx, dah, du, dw_a, db_a, A, R, dctx_keep):
    _attn_account_group(B, Nn, A, R, 2)
    dp, dl, dn, ds = _dctx_args(dctx)
    call("subgc_attn_bwd_group", _ptr(u), _ptr(v), _ptr(ah, torch.float32), _ptr(w_a), _ptr(rows, torch.int32), _ptr(lens, torch.int32), int(m), B, g, Nn,
         _ptr(alpha, torch.float32), alpha.size(1), dp, dl, _ptr(dah), _ptr(du, torch.float32), _ptr(dw_a), _ptr(db_a), A, R,
         int(is_b16(dah)) | (_uv_b16(u, v, A, R) << 1), _ptr(dctx_keep, torch.float32), ld(dctx_keep) if dctx_keep is not None else 0, dn, ds,
         du.size(0) if du.dim() == 3 else 1, du.stride(0) if du.dim() == 3 else 0, _stream())


def attn_group_du_planes(g):
    from ._lib import lib
    return int(lib().subgc_attn_group_du_planes(int(g)))


def attn_dv_accum_group(alpha, dctx, step_off, T, rows, B, g, Nn, dv, R):
    call("subgc_attn_dv_accum_group", _ptr(alpha, torch.float32), alpha.size(1), _ptr(dctx, torch.float32), ld(dctx), _ptr(step_off, torch.int32), int(T),
         _ptr(rows, torch.int32), B, g, Nn, _ptr(dv, torch.float32), R, _stream())


def _attn_account_group(B, Nn, A, R, passes):
    if FLOPS["on"]:                      # shared sets: every node row of u / v (and d(u)) moves once per image and step
        FLOPS["attn_bytes"] = FLOPS.get("attn_bytes", 0.0) + 4.0 * B * Nn * (A + R) * passes


def log_softmax_rows_(x, active=None):
    rows, V = x.shape
    call("subgc_log_softmax_rows", _ptr(x), ld(x), rows, V, _ptr(active, torch.int32), _stream())
    return x


def log_softmax_rows_bwd(logp, dout, dlogits, active=None):
    rows, V = logp.shape
    call("subgc_log_softmax_rows_bwd", _ptr(logp), _ptr(dout), _ptr(dlogits), ld(logp), rows, V, _ptr(active, torch.int32),
         int(is_b16(dlogits)), _stream())
    return dlogits


def row_lse(x):
    """lse[r] = logsumexp(x[r, :]) without touching x (subgc_row_lse_f32)."""
    rows, V = x.shape
    lse = torch.empty(rows, device=x.device, dtype=torch.float32)
    call("subgc_row_lse_f32", _ptr(x, torch.float32), ld(x), rows, V, _ptr(lse), _stream())
    return lse


def masked_nll_fwd(logp, target, mask, den=None, lse=None):
    """logp [S,T,V] contiguous; target/mask are [S,T] views (unit inner stride) of the label tensors.  `den` (device scalar):
    the denominator to use instead of the mask sum of the rows given.  `lse` [S*T]: logp holds raw logits (row_lse)."""
    S, T, V = logp.shape
    loss = torch.empty((), device=logp.device, dtype=torch.float32)
    scratch = torch.empty(2, device=logp.device, dtype=torch.float32)
    call("subgc_masked_nll_fwd", _ptr(logp), _ptr(target, torch.int64), target.stride(0), _ptr(mask, torch.float32), mask.stride(0),
         _ptr(loss), _ptr(scratch), S, T, V, _ptr(den, torch.float32), _ptr(lse, torch.float32), _stream())
    return loss, scratch


def live_plan(labels, mask_t):
    """Row plan of the packed decoder (subgc_live_plan) -> (perm32, perm64, inv32, plan int32 [2T+1] = counts[T] | offs[T+1], den)."""
    S, T = mask_t.shape
    dev = mask_t.device
    perm32 = torch.empty(S, device=dev, dtype=torch.int32)
    inv32 = torch.empty(S, device=dev, dtype=torch.int32)
    perm64 = torch.empty(S, device=dev, dtype=torch.int64)
    plan = torch.empty(2 * T + 1, device=dev, dtype=torch.int32)
    den = torch.empty(1, device=dev, dtype=torch.float32)
    if mask_t.stride(1) != 1 or labels.stride(1) != 1:
        raise SubgcError("live_plan: labels / mask need unit inner stride")
    call("subgc_live_plan", _ptr(labels, torch.int64), labels.stride(0), _ptr(mask_t, torch.float32), mask_t.stride(0), S, T, _ptr(perm32),
         _ptr(perm64), _ptr(inv32), _ptr(plan), plan.data_ptr() + 4 * T, _ptr(den), _stream())
    return perm32, perm64, inv32, plan, den


def packed_rows(labels, target, mask_t, perm32, offs, lens, idx, img):
    """-> (labels_p [S, cols], tok_flat [T*S], tgt_p [T*S, 1], msk_p [T*S, 1], lens_p, idx_p, img_p) in the plan's packed order."""
    S, T = mask_t.shape
    N = idx.size(1)
    dev = labels.device
    cols = labels.size(1)
    labels_p = torch.empty(S, cols, device=dev, dtype=torch.int64)
    tok = torch.empty(T * S, device=dev, dtype=torch.int64)
    tgt = torch.empty(T * S, 1, device=dev, dtype=torch.int64)
    msk = torch.empty(T * S, 1, device=dev, dtype=torch.float32)
    lens_p = torch.empty(S, device=dev, dtype=torch.int32)
    idx_p = torch.empty(S, N, device=dev, dtype=torch.int64)
    img_p = torch.empty(S, device=dev, dtype=torch.int32)
    if idx.stride(1) != 1 or target.stride(1) != 1 or mask_t.stride(1) != 1 or labels.stride(1) != 1:
        raise SubgcError("packed_rows: unit inner strides needed")
    call("subgc_packed_rows", _ptr(labels, torch.int64), labels.stride(0), _ptr(target, torch.int64), target.stride(0), _ptr(mask_t, torch.float32),
         mask_t.stride(0), _ptr(perm32, torch.int32), _ptr(offs, torch.int32), S, T, _ptr(labels_p), cols, _ptr(tok), _ptr(tgt), _ptr(msk),
         _ptr(lens, torch.int32), _ptr(idx, torch.int64), idx.stride(0), _ptr(img, torch.int32), N, _ptr(lens_p), _ptr(idx_p), _ptr(img_p), _stream())
    return labels_p, tok, tgt, msk, lens_p, idx_p, img_p


def gpn_prep(gpn_obj_ind, gpn_pool_mtx, att_masks, spi):
    """gpn.py:43-52 views as flat [G = 2*b5*hb] arrays (pos half, then neg half): idx int64 [G,N], w [G,N], denom [G], img int32 [G]."""
    b5, _, hb, N = gpn_obj_ind.shape
    dev = gpn_obj_ind.device
    G = 2 * b5 * hb
    gpn_obj_ind, gpn_pool_mtx, att_masks = gpn_obj_ind.contiguous(), gpn_pool_mtx.contiguous(), att_masks.contiguous()
    idx = torch.empty(G, N, device=dev, dtype=torch.int64)
    w = torch.empty(G, N, device=dev, dtype=torch.float32)
    denom = torch.empty(G, device=dev, dtype=torch.float32)
    img = torch.empty(G, device=dev, dtype=torch.int32)
    call("subgc_gpn_prep", _ptr(gpn_obj_ind, torch.int64), _ptr(gpn_pool_mtx, torch.float32), _ptr(att_masks, torch.float32), b5, hb, N, int(spi),
         _ptr(idx), _ptr(w), _ptr(denom), _ptr(img), _stream())
    return idx, w, denom, img


def gpn_select(score, gpn_obj_ind, att_masks, read_out, spi):
    """gpn.py:63-78 -> (sel_idx int64 [b5,N], lens int32 [b5], ro_sel [b5, W], img_s int32 [b5]): the best positive sub-graph of every
    sentence and the sentence's image."""
    b5, _, hb, N = gpn_obj_ind.shape
    dev = score.device
    W = read_out.size(1)
    sel_idx = torch.empty(b5, N, device=dev, dtype=torch.int64)
    lens = torch.empty(b5, device=dev, dtype=torch.int32)
    ro_sel = torch.empty(b5, W, device=dev, dtype=torch.float32)
    img_s = torch.empty(b5, device=dev, dtype=torch.int32)
    call("subgc_gpn_select", _ptr(score, torch.float32), _ptr(gpn_obj_ind.contiguous(), torch.int64), _ptr(att_masks.contiguous(), torch.float32),
         _ptr(read_out, torch.float32), b5, hb, N, W, _ptr(sel_idx), _ptr(lens), _ptr(ro_sel), None, int(spi), _ptr(img_s), _stream())
    return sel_idx, lens, ro_sel, img_s


def class_sum(x, cls, C):
    """-> [C, L]: sum of the rows of x [M, L] per class id (int32 cls [M]).  <= 64 classes: per-slab LDS accumulation + a column
    sum over the slabs (no atomics, fixed order); more classes: scatter-add with fp32 atomics (a few rows per class)."""
    M, L = x.shape
    if C <= 64:
        slabs = max(1, min(128, M // 64))
        part = torch.empty(slabs, C * L, device=x.device, dtype=torch.float32)
        call("subgc_class_partials", _ptr(x, torch.float32), ld(x), _ptr(cls, torch.int32), M, L, C, slabs, _ptr(part), _stream())
        return colsum(part).view(C, L)
    return scatter_add_rows(x, cls, zeros(C, L, device=x.device))


def add_n(ts):
    """Fresh tensor = sum of 2..4 same-shaped contiguous fp32 tensors (one launch)."""
    ts = [t.contiguous() for t in ts]
    out = torch.empty_like(ts[0])
    while len(ts) > 4:
        call("subgc_add_n_f32", _ptr(out), _ptr(ts[0], torch.float32), _ptr(ts[1], torch.float32), _ptr(ts[2], torch.float32), _ptr(ts[3], torch.float32),
             out.numel(), _stream())
        ts = [out] + ts[4:]
    ts = ts + [None] * (4 - len(ts))
    call("subgc_add_n_f32", _ptr(out), _ptr(ts[0], torch.float32), _ptr(ts[1], torch.float32), _ptr(ts[2], torch.float32), _ptr(ts[3], torch.float32),
         out.numel(), _stream())
    return out


def fill2d_(x, value):
    call("subgc_fill2d_f32", _ptr(x, torch.float32), ld(x), x.size(0), x.size(1), float(value), _stream())
    return x


def row_count(x):
    lens = torch.empty(x.size(0), device=x.device, dtype=torch.int32)
    call("subgc_row_count_f32", _ptr(x, torch.float32), ld(x), x.size(0), x.size(1), _ptr(lens), _stream())
    return lens


def masked_nll_bwd(target, mask, scratch, dloss, S, T, V):
    dlogp = torch.empty(S, T, V, device=mask.device, dtype=torch.float32)
    call("subgc_masked_nll_bwd", _ptr(target, torch.int64), target.stride(0), _ptr(mask), mask.stride(0), _ptr(scratch), _ptr(dloss),
         _ptr(dlogp), S, T, V, _stream())
    return dlogp


def nll_logsoftmax_bwd(logp, target, mask, scratch, dloss, dlogits, active, S, T, V, lse=None):
    call("subgc_nll_logsoftmax_bwd", _ptr(logp), _ptr(target, torch.int64), target.stride(0), _ptr(mask), mask.stride(0), _ptr(scratch),
         _ptr(dloss), _ptr(dlogits), ld(dlogits), S, T, V, _ptr(active, torch.int32), int(is_b16(dlogits)), _ptr(lse, torch.float32), _stream())
    return dlogits


# ---- label-smoothed language loss (include/subgc_criterion_hip.h; misc/utils.py:126-156)
def check_smoothing(smoothing):
    """-> float(smoothing); a value outside [0, 1] (NaN included) is refused here as the library refuses it, with the number in the text."""
    s = float(smoothing)
    if not 0.0 <= s <= 1.0:
        raise SubgcError(f"label smoothing {s!r} is outside [0, 1]")
    return s


def row_lse_sum(x, raw=True):
    """One read of x [rows, V] (subgc_row_lse_sum_f32).  raw: x holds logits -> (lse [rows], slp [rows] = sum_c (x - lse));
    else x holds log-probabilities -> (None, slp = sum_c x)."""
    rows, V = x.shape
    lse = torch.empty(rows, device=x.device, dtype=torch.float32) if raw else None
    slp = torch.empty(rows, device=x.device, dtype=torch.float32)
    call_criterion("subgc_row_lse_sum_f32", _ptr(x, torch.float32), ld(x), rows, V, _ptr(lse), _ptr(slp), _stream())
    return lse, slp


def smoothed_nll_fwd(logp, target, mask, slp, smoothing, den=None, lse=None):
    """LabelSmoothing's loss; arguments as masked_nll_fwd plus `slp` [S*T] (row_lse_sum) and `smoothing`.  `den`: the denominator over
    rows not given, which are taken as the reference's zero rows.  -> (loss, scratch {num, den})."""
    S, T, V = logp.shape
    loss = torch.empty((), device=logp.device, dtype=torch.float32)
    scratch = torch.empty(2, device=logp.device, dtype=torch.float32)
    call_criterion("subgc_smoothed_nll_fwd", _ptr(logp, torch.float32), _ptr(target, torch.int64), target.stride(0), _ptr(mask, torch.float32),
                   mask.stride(0), _ptr(slp, torch.float32), check_smoothing(smoothing), _ptr(loss), _ptr(scratch), S, T, V,
                   _ptr(den, torch.float32), _ptr(lse, torch.float32), _stream())
    return loss, scratch


def smoothed_nll_bwd(target, mask, scratch, dloss, smoothing, S, T, V):
    dlogp = torch.empty(S, T, V, device=mask.device, dtype=torch.float32)          # every element is written
    call_criterion("subgc_smoothed_nll_bwd", _ptr(target, torch.int64), target.stride(0), _ptr(mask, torch.float32), mask.stride(0),
                   _ptr(scratch), _ptr(dloss), check_smoothing(smoothing), _ptr(dlogp), S, T, V, _stream())
    return dlogp


def smoothed_logsoftmax_bwd(logp, target, mask, scratch, dloss, smoothing, dlogits, active, S, T, V, lse=None):
    call_criterion("subgc_smoothed_logsoftmax_bwd", _ptr(logp, torch.float32), _ptr(target, torch.int64), target.stride(0), _ptr(mask, torch.float32),
                   mask.stride(0), _ptr(scratch), _ptr(dloss), check_smoothing(smoothing), _ptr(dlogits), ld(dlogits), S, T, V,
                   _ptr(active, torch.int32), int(is_b16(dlogits)), _ptr(lse, torch.float32), _stream())
    return dlogits


# ---- self-critical sequence training (include/subgc_selfcritical_hip.h; misc/utils.py:89-109)
def check_reward_weights(cider_weight, bleu_weight):
    """-> (float, float); a weight that is not finite is refused here as the library refuses it, with the numbers in the text."""
    wc, wb = float(cider_weight), float(bleu_weight)
    if not (math.isfinite(wc) and math.isfinite(wb)):
        raise SubgcError(f"self-critical reward: the reward weights (cider {wc!r}, bleu {wb!r}) must be finite")
    return wc, wb


def sc_pick(logits, n_sample, temp, u, t, seq, seqlp, next_tok, unfinished, n_unf, prev_count=None, raw=False):
    """One rollout step (subgc_sc_pick): rows [0, n_sample) draw from softmax(logits / temp) with u[r], the others take the first arg-max
    exactly as decode_pick(k = 0) does; the bookkeeping is decode_pick's."""
    n, V = logits.shape
    call_selfcritical("subgc_sc_pick", _ptr(logits, torch.float32), ld(logits), n, int(n_sample), V, float(temp), _ptr(u, torch.float32), int(t),
                      _ptr(seq, torch.int64), _ptr(seqlp, torch.float32), seq.size(1), _ptr(next_tok, torch.int64),
                      _ptr(unfinished, torch.int32), _ptr(n_unf, torch.int32), _ptr(prev_count, torch.int32), int(raw), _stream())


def sc_prepare(seq2, V, eos_id=0, want_replay=True, want_rows=True):
    """Rollout tokens seq2 [2S, T] int64 (sampled half first) -> (labels [S, T+2], mask [S, T+1], score_rows [2S, T+1]) in one launch
    (subgc_sc_prepare); an output not wanted is None."""
    if seq2.dim() != 2 or seq2.size(0) % 2 or seq2.size(0) == 0 or not seq2.is_contiguous():
        raise SubgcError(f"sc_prepare: contiguous rollout tokens [2 S, T], got {tuple(seq2.shape)}")
    S, T = seq2.size(0) // 2, seq2.size(1)
    dev = seq2.device
    labels = torch.empty(S, T + 2, device=dev, dtype=torch.int64) if want_replay else None
    mask = torch.empty(S, T + 1, device=dev, dtype=torch.float32) if want_replay else None
    rows = torch.empty(2 * S, T + 1, device=dev, dtype=torch.int64) if want_rows else None
    call_selfcritical("subgc_sc_prepare", _ptr(seq2, torch.int64), S, T, int(V), int(eos_id), _ptr(labels), _ptr(mask), _ptr(rows), _stream())
    return labels, mask, rows


def sc_reward(row_d, S, T1, cider_weight, bleu_weight):
    """fp64 row records of subgc_accuracy_rows for 2S rows -> (reward [S, T1] fp32, mean_reward [] fp32, scores [2S] fp64)."""
    wc, wb = check_reward_weights(cider_weight, bleu_weight)
    dev = row_d.device
    reward = torch.empty(S, T1, device=dev, dtype=torch.float32)
    mean = torch.empty((), device=dev, dtype=torch.float32)
    scores = torch.empty(2 * S, device=dev, dtype=torch.float64)
    call_selfcritical("subgc_sc_reward", _ptr(row_d, torch.float64), ld(row_d), int(S), int(T1), wc, wb, _ptr(reward), _ptr(mean), _ptr(scores),
                      _stream())
    return reward, mean, scores


def reward_nll_fwd(inp, seq, reward, gpn_loss=None):
    """RewardCriterion.forward on gathered log-probabilities [S, T] (all contiguous) -> (loss, scratch {num, den})."""
    S, T = inp.shape
    loss = torch.empty((), device=inp.device, dtype=torch.float32)
    scratch = torch.empty(2, device=inp.device, dtype=torch.float32)
    call_selfcritical("subgc_reward_nll_fwd", _ptr(inp, torch.float32), _ptr(seq, torch.int64), _ptr(reward, torch.float32),
                      _ptr(gpn_loss, torch.float32), _ptr(loss), _ptr(scratch), S, T, _stream())
    return loss, scratch


def reward_nll_bwd(seq, reward, gpn_loss, scratch, dloss):
    S, T = seq.shape
    dinput = torch.empty(S, T, device=seq.device, dtype=torch.float32)           # every element is written
    dgpn = torch.empty(S, device=seq.device, dtype=torch.float32) if gpn_loss is not None else None
    call_selfcritical("subgc_reward_nll_bwd", _ptr(seq, torch.int64), _ptr(reward, torch.float32), _ptr(gpn_loss, torch.float32), _ptr(scratch),
                      _ptr(dloss), _ptr(dinput), _ptr(dgpn), S, T, _stream())
    return dinput, dgpn


def reward_logits_fwd(logp, target, mask, reward, den=None, lse=None):
    """RewardCriterion fused on the decoder's rows: masked_nll_fwd's arguments plus `reward` ([S, T] view) -> (loss, scratch {num, den})."""
    S, T, V = logp.shape
    loss = torch.empty((), device=logp.device, dtype=torch.float32)
    scratch = torch.empty(2, device=logp.device, dtype=torch.float32)
    call_selfcritical("subgc_reward_logits_fwd", _ptr(logp, torch.float32), _ptr(target, torch.int64), target.stride(0), _ptr(mask, torch.float32),
                      mask.stride(0), _ptr(reward, torch.float32), reward.stride(0), _ptr(loss), _ptr(scratch), S, T, V,
                      _ptr(den, torch.float32), _ptr(lse, torch.float32), _stream())
    return loss, scratch


def reward_logsoftmax_bwd(logp, target, mask, reward, scratch, dloss, dlogits, active, S, T, V, lse=None):
    call_selfcritical("subgc_reward_logsoftmax_bwd", _ptr(logp, torch.float32), _ptr(target, torch.int64), target.stride(0),
                      _ptr(mask, torch.float32), mask.stride(0), _ptr(reward, torch.float32), reward.stride(0), _ptr(scratch), _ptr(dloss),
                      _ptr(dlogits), ld(dlogits), S, T, V, _ptr(active, torch.int32), int(is_b16(dlogits)), _ptr(lse, torch.float32), _stream())
    return dlogits


class Criterion:
    """The criterion fused on the decoder's rows, chosen once per decoder forward: RewardCriterion when `reward` ([S, T] view; the packed
    decoder puts its packed rows there) is given, else LabelSmoothing when smoothing > 0, else LanguageModelCriterion."""

    def __init__(self, smoothing=0.0, reward=None):
        self.smoothing, self.reward = smoothing, reward

    def row_pass(self, x, raw):                  # -> (lse, slp) for fwd, either may be None; raw: x holds logits, and every criterion needs lse
        if self.smoothing > 0 and (raw or self.reward is None):
            return row_lse_sum(x, raw=raw)
        return (row_lse(x) if raw else None), None

    def fwd(self, logp, target, mask, slp, den=None, lse=None):
        if self.reward is not None:
            return reward_logits_fwd(logp, target, mask, self.reward, den=den, lse=lse)
        if self.smoothing > 0:
            return smoothed_nll_fwd(logp, target, mask, slp, self.smoothing, den=den, lse=lse)
        return masked_nll_fwd(logp, target, mask, den=den, lse=lse)

    def bwd(self, logp, target, mask, scratch, dloss, dlogits, active, S, T, V, lse=None):
        if self.reward is not None:
            return reward_logsoftmax_bwd(logp, target, mask, self.reward, scratch, dloss, dlogits, active, S, T, V, lse=lse)
        if self.smoothing > 0:
            return smoothed_logsoftmax_bwd(logp, target, mask, scratch, dloss, self.smoothing, dlogits, active, S, T, V, lse=lse)
        return nll_logsoftmax_bwd(logp, target, mask, scratch, dloss, dlogits, active, S, T, V, lse=lse)


def step_active(labels, T):
    S = labels.size(0)
    active = torch.empty(S * T, device=labels.device, dtype=torch.int32)
    call("subgc_step_active", _ptr(labels, torch.int64), labels.stride(0), S, T, _ptr(active), _stream())
    return active


def decode_pick(logp, k, temp, u, t, seq, seqlp, next_tok, unfinished, n_unf, prev_count=None, raw=False, top_p=1.0):
    """Greedy (k == 0) / top-k token choice.  k <= 8 without a nucleus cut runs subgc_decode_pick; a larger k or top_p < 1 runs the
    radix-select kernel subgc_decode_sample."""
    n, V = logp.shape
    if k > 8 or top_p != 1.0:
        return decode_sample(logp, k, top_p, temp, u, t, seq, seqlp, next_tok, unfinished, n_unf, prev_count, raw)
    call("subgc_decode_pick", _ptr(logp), ld(logp), n, V, int(k), float(temp), _ptr(u), int(t), _ptr(seq, torch.int64), _ptr(seqlp),
         seq.size(1), _ptr(next_tok, torch.int64), _ptr(unfinished, torch.int32), _ptr(n_unf, torch.int32), _ptr(prev_count, torch.int32), int(raw), _stream())


def decode_sample(logits, k, top_p, temp, u, t, seq, seqlp, next_tok, unfinished, n_unf, prev_count=None, raw=False):
    """Top-k / nucleus token choice for any 1 <= k <= V (subgc_decode_sample; see include/subgc_hip.h for the order and cut rules)."""
    n, V = logits.shape
    call("subgc_decode_sample", _ptr(logits), ld(logits), n, V, int(k), float(top_p), float(temp), _ptr(u), int(t), _ptr(seq, torch.int64),
         _ptr(seqlp), seq.size(1), _ptr(next_tok, torch.int64), _ptr(unfinished, torch.int32), _ptr(n_unf, torch.int32),
         _ptr(prev_count, torch.int32), int(raw), _stream())


def decode_rules(logits, seq, t, flags, trigram_pen, bad_ids=None, stats=None, prev_count=None):
    """The decode rules of step t, in place on the fp32 logits rows [n, V] (subgc_decode_rules; include/subgc_decode_rules_hip.h): the
    rows become their log-softmax with block_trigrams / suppress_unk / decoding_constraint / block_bad_endings (`flags`) applied from
    the history seq[:, :t].  `bad_ids`: device int32 ids; `stats`: int32 [n, 4] counters or None.  The pick then runs with raw=False."""
    n, V = logits.shape
    if seq.dim() != 2 or seq.size(0) != n or not seq.is_contiguous():
        raise SubgcError(f"decode_rules: seq must be a contiguous [n, T] tensor with n = {n} rows, got {tuple(seq.shape)}")
    if stats is not None and (tuple(stats.shape) != (n, 4) or not stats.is_contiguous()):
        raise SubgcError(f"decode_rules: stats must be a contiguous [{n}, 4] tensor, got {tuple(stats.shape)}")
    call_decode_rules("subgc_decode_rules", _ptr(logits, torch.float32), ld(logits), n, V, _ptr(seq, torch.int64), seq.size(1), int(t), int(flags),
                      float(trigram_pen), _ptr(bad_ids, torch.int32), 0 if bad_ids is None else bad_ids.numel(), _ptr(stats, torch.int32),
                      _ptr(prev_count, torch.int32), _stream())
    return logits


def row_topk(x, k, vals, idx, log_softmax=True):
    """vals/idx[r, :k] = the k largest of row r (value desc, index asc); raw logits -> log-probs when log_softmax."""
    call("subgc_row_topk_f32", _ptr(x), ld(x), x.size(0), x.size(1), int(k), int(log_softmax), _ptr(vals), _ptr(idx, torch.int32), _stream())
    return vals, idx


def beam_step(tv, ti, st, tok, src, t, T, G, bd, kk, unk, constraint, lam):
    """One (diverse) beam-search step of every sub-graph on the device (subgc_beam_step).  `st`: the tables of beam.DeviceTables."""
    n = st.sums.size(0)
    call("subgc_beam_step", _ptr(tv, torch.float32), _ptr(ti, torch.int32), _ptr(st.seq, torch.int32), _ptr(st.lps, torch.float32),
         _ptr(st.sums, torch.float32), _ptr(st.done_cnt, torch.int32), _ptr(st.done_seq, torch.int32), _ptr(st.done_lps, torch.float32),
         _ptr(st.done_p, torch.float32), _ptr(st.done_len, torch.int32), _ptr(tok, torch.int64), _ptr(src, torch.int32), n, int(t), int(T),
         int(G), int(bd), int(kk), int(unk), int(bool(constraint)), float(lam), st.cap, _stream())


BEAM_ATT_MAX_N = 4096          # SUBGC_BEAM_ATT_MAX_N


def beam_step_anc(tv, ti, st, tok, src, t, T, G, bd, kk, unk, constraint, lam):
    """`beam_step` that also records every beam's ancestry in st.anc / st.done_anc (subgc_beam_step_anc, subgc_beam_att_hip.h)."""
    n = st.sums.size(0)
    if st.anc is None or st.done_anc is None:
        raise SubgcError("beam_step_anc: the tables were built without ancestry (DeviceTables(..., return_att=True))")
    call_beam_att("subgc_beam_step_anc", _ptr(tv, torch.float32), _ptr(ti, torch.int32), _ptr(st.seq, torch.int32), _ptr(st.lps, torch.float32),
                  _ptr(st.sums, torch.float32), _ptr(st.done_cnt, torch.int32), _ptr(st.done_seq, torch.int32), _ptr(st.done_lps, torch.float32),
                  _ptr(st.done_p, torch.float32), _ptr(st.done_len, torch.int32), _ptr(st.anc, torch.int32), _ptr(st.done_anc, torch.int32),
                  _ptr(tok, torch.int64), _ptr(src, torch.int32), n, int(t), int(T), int(G), int(bd), int(kk), int(unk), int(bool(constraint)),
                  float(lam), st.cap, _stream())


def beam_att_gather(al_step, st, pick, n, G, bd, T, out):
    """out [T + 1, n, N] <- the attention rows of the finished beam pick[s] = (group, slot) of every sub-graph, zero rows behind its length
    (subgc_beam_att_gather).  al_step [steps, n * G * bd, N] contiguous; pick int32 [n, 2] on the device, range-checked by the caller
    (beam.check_picks)."""
    steps, rows, N = al_step.shape
    if not al_step.is_contiguous() or out.dim() != 3 or out.size(0) != T + 1 or out.size(1) != n or out.size(2) != N or out.stride(2) != 1:
        raise SubgcError(f"beam_att_gather: contiguous step buffer and out [T + 1, n, N], got {tuple(al_step.shape)} and {tuple(out.shape)}")
    if N > BEAM_ATT_MAX_N:
        raise SubgcError(f"beam_att_gather: {N} attention columns; the limit is {BEAM_ATT_MAX_N}")
    if pick.numel() != 2 * n:
        raise SubgcError(f"beam_att_gather: one (group, slot) pick per sub-graph, got {pick.numel()} numbers for {n}")
    call_beam_att("subgc_beam_att_gather", _ptr(al_step, torch.float32), al_step.stride(0), steps, rows, N, _ptr(st.done_anc, torch.int32),
                  _ptr(st.done_len, torch.int32), _ptr(pick, torch.int32), int(n), int(G), int(bd), st.cap, int(T), _ptr(out, torch.float32),
                  out.stride(0), out.stride(1), _stream())
    return out


def uniform(shape, seed, offset, device):
    out = torch.empty(shape, device=device, dtype=torch.float32)
    call("subgc_uniform_f32", _ptr(out), out.numel(), int(seed), int(offset), _stream())
    return out


def multinomial_rows_(logits, u, sel_u, prob, tok):
    """tok[r] <- draw from softmax(logits[r]) where sel_u[r] < prob (in place; `tok` may be a strided column of int64)."""
    rows, V = logits.shape
    call("subgc_multinomial_rows", _ptr(logits, torch.float32), ld(logits), rows, V, _ptr(u, torch.float32), _ptr(sel_u, torch.float32),
         float(prob), _ptr(tok, torch.int64), tok.stride(0) if tok.dim() else 1, _stream())
    return tok


def packed_time_sum(src, offsets, T, S, dst):
    """dst[s] = sum over live steps t of src[offsets[t] + s] (packed decoder; offsets int32 [T+1] on the device)."""
    call("subgc_packed_time_sum", _ptr(src), _ptr(offsets, torch.int32), int(T), int(S), src.size(1), _ptr(dst, torch.float32),
         int(is_b16(src)), _stream())
    return dst


def rank_desc(score):
    """(sorted scores, order): stable descending sort of a 1-D fp32 score vector (eval_utils.py:106)."""
    score = score.contiguous()
    order = torch.empty(score.numel(), device=score.device, dtype=torch.int64)
    srt = torch.empty_like(score)
    call("subgc_rank_desc_f32", _ptr(score, torch.float32), score.numel(), _ptr(order), _ptr(srt), _stream())
    return srt, order


def eval_collect(score, keep, seq, bounds, identity=False, AL=None, idx=None, pick=None, consensus=None, diversity=None, accuracy=None,
                 grounding=None):
    """The eval loop's per-image work for a whole decode batch: see `eval_glue.eval_collect`, which this forwards to."""
    from .eval_glue import eval_collect as run
    return run(score, keep, seq, bounds, identity, AL, idx, pick, consensus, diversity, accuracy, grounding)


def consensus_cook(tok, ukeys, ulogdf, ref_len, woff=None, max_words=0, row_len=None, bad=None):
    """subgc_consensus_cook: sentences -> sorted (n-gram key, tf-idf weight) lists, norms and bigram lengths (precook + counts2vec,
    cider_scorer_compute_sentence.py:15-30,188-212).  tok: int32 / int64; CSR over `woff` (int32 [S + 1], at most `max_words` words per
    sentence) or token rows [S, T] (words before the first 0, at most row_len[s], minus trailing `bad` words).
    -> (keys int64 bit patterns, wts fp64, cnt int32 [S], blen int32 [S], norm fp64 [S, 4]); sentence s owns keys / wts [4 * first word ...)."""
    p_tok = _ptr(tok)
    if tok.dtype not in (torch.int32, torch.int64) or not tok.is_contiguous():
        raise SubgcError(f"consensus_cook: contiguous int32 / int64 tokens, got {tok.dtype}")
    if woff is not None:
        S, T = woff.numel() - 1, 0
    else:
        S, T = tok.shape
    dev = tok.device
    keys = torch.empty(max(4 * tok.numel(), 1), device=dev, dtype=torch.int64)
    wts = torch.empty(max(4 * tok.numel(), 1), device=dev, dtype=torch.float64)
    cnt = torch.empty(max(S, 1), device=dev, dtype=torch.int32)
    blen = torch.empty(max(S, 1), device=dev, dtype=torch.int32)
    norm = torch.empty(max(S, 1), 4, device=dev, dtype=torch.float64)
    call("subgc_consensus_cook", p_tok, int(tok.dtype == torch.int64), _ptr(woff, torch.int32), int(T), _ptr(row_len, torch.int32),
         _ptr(bad, torch.uint8), 0 if bad is None else bad.numel(), int(S), int(max_words), _ptr(ukeys, torch.int64), _ptr(ulogdf, torch.float64),
         ukeys.numel(), float(ref_len), _ptr(keys), _ptr(wts), _ptr(cnt), _ptr(blen), _ptr(norm), _stream())
    return keys, wts, cnt, blen, norm


def consensus_score(cand, T, seg, I, max_cand, top_k, nn, k, cap_off, n_img, n_caps, nwoff, corpus, gauss, m, max_caps, sim, pair_out=None):
    """subgc_consensus_score: sim[row] = sum of the m largest CIDEr pair scores of candidate `row` against its image's neighbour captions
    (consensus_reranking.py:155-169).  cand / corpus: the tuples consensus_cook returned (rows of width T / CSR over nwoff); nn int32 [I, >= k]."""
    ck, cw, cc, cl, cn = cand
    nk, nw, nc, nl, nno = corpus
    call("subgc_consensus_score", _ptr(ck, torch.int64), _ptr(cw, torch.float64), _ptr(cc, torch.int32), _ptr(cl, torch.int32), _ptr(cn, torch.float64),
         int(T), _ptr(seg, torch.int32), int(I), int(max_cand), int(top_k), _ptr(nn, torch.int32), nn.stride(0) if nn.dim() == 2 else nn.numel(), int(k),
         _ptr(cap_off, torch.int32), int(n_img), int(n_caps), _ptr(nwoff, torch.int32), _ptr(nk, torch.int64), _ptr(nw, torch.float64),
         _ptr(nc, torch.int32), _ptr(nl, torch.int32), _ptr(nno, torch.float64), _ptr(gauss, torch.float64), gauss.numel(), int(m), int(max_caps),
         _ptr(sim, torch.float64), _ptr(pair_out, torch.float64), 0 if pair_out is None else pair_out.stride(0), _stream())
    return sim


def consensus_rank(sim, seg, I, top_k, order, first=None):
    """subgc_consensus_rank: per image the stable descending order of the fp64 sums (ties: lower candidate index first) and its head."""
    call("subgc_consensus_rank", _ptr(sim, torch.float64), _ptr(seg, torch.int32), int(I), int(top_k), _ptr(order, torch.int32),
         _ptr(first, torch.int32), _stream())
    return order


def consensus_bleu_cook(tok, woff=None, max_words=0, row_len=None, bad=None):
    """subgc_consensus_bleu_cook (include/subgc_consensus_hip.h): sentences -> their distinct n-grams of orders 1 .. 4 in ascending key
    order with an int32 count each (the Counters of bleu_score_util.py:33-34, all orders at once).  tok and the sentence arguments are
    consensus_cook's.  -> (keys int64 bit patterns, counts int32, cnt int32 [S], wlen int32 [S]: the words of each sentence); sentence s
    owns keys / counts [4 * first word ...)."""
    p_tok = _ptr(tok)
    if tok.dtype not in (torch.int32, torch.int64) or not tok.is_contiguous():
        raise SubgcError(f"consensus_bleu_cook: contiguous int32 / int64 tokens, got {tok.dtype}")
    if woff is not None:
        S, T = woff.numel() - 1, 0
    else:
        S, T = tok.shape
    dev = tok.device
    keys = torch.empty(max(4 * tok.numel(), 1), device=dev, dtype=torch.int64)
    counts = torch.empty(max(4 * tok.numel(), 1), device=dev, dtype=torch.int32)
    cnt = torch.empty(max(S, 1), device=dev, dtype=torch.int32)
    wlen = torch.empty(max(S, 1), device=dev, dtype=torch.int32)
    call_consensus("subgc_consensus_bleu_cook", p_tok, int(tok.dtype == torch.int64), _ptr(woff, torch.int32), int(T), _ptr(row_len, torch.int32),
                   _ptr(bad, torch.uint8), 0 if bad is None else bad.numel(), int(S), int(max_words), _ptr(keys), _ptr(counts), _ptr(cnt),
                   _ptr(wlen), _stream())
    return keys, counts, cnt, wlen


def consensus_bleu_score(cand, T, seg, I, max_cand, top_k, nn, k, cap_off, n_img, n_caps, nwoff, corpus, n, fpr, m, max_caps, sim, pair_out=None):
    """subgc_consensus_bleu_score: sim[row] = sum of the m largest sentence-level BLEU F-scores (bleu_score_util.py:15-61) of candidate
    `row` against its image's neighbour captions (consensus_reranking.py:155-169).  cand / corpus: the tuples consensus_bleu_cook
    returned (rows of width T / CSR over nwoff); nn int32 [I, >= k]; n the n-gram order, fpr the F-score's precision weight."""
    ck, cc, cn, cl = cand
    nk, nc, nn_, nl = corpus
    call_consensus("subgc_consensus_bleu_score", _ptr(ck, torch.int64), _ptr(cc, torch.int32), _ptr(cn, torch.int32), _ptr(cl, torch.int32), int(T),
                   _ptr(seg, torch.int32), int(I), int(max_cand), int(top_k), _ptr(nn, torch.int32), nn.stride(0) if nn.dim() == 2 else nn.numel(),
                   int(k), _ptr(cap_off, torch.int32), int(n_img), int(n_caps), _ptr(nwoff, torch.int32), _ptr(nk, torch.int64),
                   _ptr(nc, torch.int32), _ptr(nn_, torch.int32), _ptr(nl, torch.int32), int(n), float(fpr), int(m), int(max_caps),
                   _ptr(sim, torch.float64), _ptr(pair_out, torch.float64), 0 if pair_out is None else pair_out.stride(0), _stream())
    return sim


NN_MAX_K = 1024         # subgc_nn_select_f64: entries of one list


def nn_dist(q, x, dist):
    """subgc_nn_dist_f64 (include/subgc_neighbours_hip.h): dist[i, j] = the euclidean distance of query row i and train row j in fp64 by
    cdist's own sequential sum (consensus_reranking.py:105,113).  q [Q, D], x [N, D], dist [Q, >= N]: fp64 views with unit inner stride."""
    for name, t in (("q", q), ("x", x), ("dist", dist)):
        if t.dtype != torch.float64:
            raise SubgcError(f"nn_dist: {name} is {t.dtype}; the distances are float64 like the reference's")
    if q.size(1) != x.size(1) or dist.size(0) != q.size(0) or dist.size(1) < x.size(0):
        raise SubgcError(f"nn_dist: q {tuple(q.shape)}, x {tuple(x.shape)}, dist {tuple(dist.shape)} do not fit together")
    call_neighbours("subgc_nn_dist_f64", _ptr(q), ld(q), q.size(0), _ptr(x), ld(x), x.size(0), q.size(1), _ptr(dist), ld(dist), _stream())
    return dist


def nn_select(dist, N, k, idx, val=None):
    """subgc_nn_select_f64: idx[i, :k] (int32) / val[i, :k] (fp64) = the k smallest of dist[i, :N] in ascending (distance, index) order
    (np.argsort(...)[:, :num_NNimg], consensus_reranking.py:108,114; equal distances: lower index first; NaN last).  idx / val: contiguous [Q, k]."""
    Q = dist.size(0)
    for name, t, dt in (("idx", idx, torch.int32), ("val", val, torch.float64)):
        if t is not None and (t.dtype != dt or not t.is_contiguous() or tuple(t.shape) != (Q, int(k))):
            raise SubgcError(f"nn_select: {name} must be a contiguous {dt} [{Q}, {k}] tensor, got {t.dtype} {tuple(t.shape)}")
    call_neighbours("subgc_nn_select_f64", _ptr(dist, torch.float64), ld(dist), Q, int(N), int(k), _ptr(idx), _ptr(val), _stream())
    return idx, val


DIV_COLS = 8            # SUBGC_DIV_SEL: the integer columns in front of a set's selection (drawn, distinct, selected, words, unigrams, bigrams, novel, valid)
DIV_WANT = {1: 1, 2: 2, 3: 2, 4: 4}       # metric of diversity_score.py -> SUBGC_DIV_WANT_DRAW / _WORDS / _BLEU


def _div_tok(who, tok):
    t64, T = _scoring.token_rows(who, tok)
    return _ptr(tok), t64, T


def diversity_select(score, seg, I, rows, set_img, set_off, draw, n_sets, n_draw, max_draw, n_best, out_i):
    """subgc_diversity_select: per set the best n_best rows of its draw by score (later in the draw first among equal scores) into
    out_i [n_sets, >= DIV_COLS + n_best] (diversity_score.py:63-65)."""
    call("subgc_diversity_select", _ptr(score, torch.float32), _ptr(seg, torch.int32), int(I), int(rows), _ptr(set_img, torch.int32),
         _ptr(set_off, torch.int32), _ptr(draw, torch.int32), int(n_sets), int(n_draw), int(max_draw), int(n_best), _ptr(out_i, torch.int32),
         out_i.stride(0), _stream())
    return out_i


def diversity_distinct(tok, bad, seg, I, set_img, set_off, set_flags, draw, n_sets, n_draw, max_draw, out_i):
    """subgc_diversity_distinct: drawn and distinct captions of every whole draw (diversity_score.py:154-160)."""
    p_tok, t64, T = _div_tok("diversity_distinct", tok)
    call("subgc_diversity_distinct", p_tok, t64, T, _ptr(bad, torch.uint8), 0 if bad is None else bad.numel(), _ptr(seg, torch.int32), int(I),
         tok.size(0), _ptr(set_img, torch.int32), _ptr(set_off, torch.int32), _ptr(set_flags, torch.int32), _ptr(draw, torch.int32), int(n_sets),
         int(n_draw), int(max_draw), _ptr(out_i, torch.int32), out_i.stride(0), _stream())
    return out_i


def diversity_best(tok, bad, seg, I, set_img, set_flags, n_sets, n_best, nv_off, nv_tok, nv_n, out_i, out_d):
    """subgc_diversity_best: word / unigram / bigram / novel counts and the sentence BLEU-4 values of the rows diversity_select left in
    out_i (diversity_score.py:67-79, 96-108, 143-145); out_d fp64 [n_sets, >= n_best + 1]."""
    p_tok, t64, T = _div_tok("diversity_best", tok)
    call("subgc_diversity_best", p_tok, t64, T, _ptr(bad, torch.uint8), 0 if bad is None else bad.numel(), _ptr(seg, torch.int32), int(I),
         tok.size(0), _ptr(set_img, torch.int32), _ptr(set_flags, torch.int32), int(n_sets), int(n_best), _ptr(nv_off, torch.int32),
         _ptr(nv_tok, torch.int32), int(nv_n), _ptr(out_i, torch.int32), out_i.stride(0), _ptr(out_d, torch.float64), out_d.stride(0), _stream())
    return out_i, out_d


def dropout_mask(shape, p, seed, offset, device):
    keep = torch.empty(shape, device=device, dtype=torch.uint8)
    call("subgc_dropout_mask", _ptr(keep), keep.numel(), float(p), int(seed), int(offset), _stream())
    return keep


def fill_(x, value):
    call("subgc_fill_f32", _ptr(x, torch.float32), x.numel(), float(value), _stream())
    return x


def zeros(*shape, device):
    return fill_(torch.empty(*shape, device=device, dtype=torch.float32), 0.0)


def copy2d(x, y, accumulate=False):
    if is_b16(x):
        if accumulate or not is_b16(y):
            raise SubgcError("copy2d: bf16 rows are copied to bf16 rows only")
        call("subgc_copy2d_b16", _ptr(x, BF16), ld(x), _ptr(y, BF16), ld(y), x.size(0), x.size(1), _stream())
        return y
    call("subgc_copy2d_f32", _ptr(x), ld(x), _ptr(y), ld(y), x.size(0), x.size(1), int(accumulate), _stream())
    return y


def relu_bwd(dy, y, scale=1.0, out=None, bf16=False):
    """dz = dy * scale * [y > 0] (contiguous); `bf16`: dz is written bf16 (it only feeds the two gradient GEMMs)."""
    if out is None:
        out = torch.empty(y.shape, device=y.device, dtype=BF16 if bf16 else torch.float32)
    if not (y.is_contiguous() and dy.is_contiguous() and out.is_contiguous()):
        raise SubgcError("relu_bwd works on contiguous tensors")
    call("subgc_relu_bwd", _ptr(dy, torch.float32), _ptr(y), float(scale), _ptr(out), y.numel(), int(is_b16(out)) | (int(is_b16(y)) << 1), _stream())
    return out


def gather_rows(src, rows, dst, m_dev=None):
    """dst fp32 or bf16."""
    call("subgc_gather_rows", _ptr(src, torch.float32), ld(src), _ptr(rows, torch.int32), _ptr(dst), ld(dst), dst.size(0), dst.size(1),
         _ptr(m_dev, torch.int32), int(is_b16(dst)), _stream())
    return dst


def gather_rows_words(src, rows):
    """out[m] = src[rows[m]] as a bit copy for a contiguous tensor of any 4- or 8-byte dtype ([R] or [R, ...]; rows int32 [M]):
    subgc_gather_rows on the 4-byte word views, which moves words and does no arithmetic on them."""
    out = torch.empty((rows.numel(),) + tuple(src.shape[1:]), device=src.device, dtype=src.dtype)
    if out.numel():
        gather_rows(_words(src.view(-1, 1) if src.dim() == 1 else src), rows, _words(out.view(-1, 1) if out.dim() == 1 else out))
    return out


def gather_rows_keep(src, rows, keep, scale, dst, m_dev=None):
    """dst[m] = src[rows[m]] * keep[m] * scale (keep: uint8 [M, L] or None); src / dst fp32 or bf16."""
    call("subgc_gather_rows_keep", _ptr(src), ld(src), _ptr(rows, torch.int32), _ptr(keep, torch.uint8), ld(keep) if keep is not None else 0, float(scale),
         _ptr(dst), ld(dst), dst.size(0), dst.size(1), _ptr(m_dev, torch.int32), int(is_b16(dst)) | (int(is_b16(src)) << 1), _stream())
    return dst


def gather_rows_multi(pairs, rows):
    """dst[m] = src[rows[m]] for up to four (src, dst) pairs of 2-D views in one launch (subgc_gather_rows_multi)."""
    if not 1 <= len(pairs) <= 4:
        raise SubgcError("gather_rows_multi takes 1..4 (src, dst) pairs")
    args = []
    for src, dst in list(pairs) + [(None, None)] * (4 - len(pairs)):
        args += [_ptr(src, torch.float32), ld(src) if src is not None else 0, _ptr(dst, torch.float32), ld(dst) if dst is not None else 0,
                 dst.size(1) if dst is not None else 0]
    call("subgc_gather_rows_multi", len(pairs), *args, _ptr(rows, torch.int32), pairs[0][1].size(0), _stream())


def decode_cell_b16(g0, c_prev, c, hs, b0=None, b1=None, table=None, tok=None, g2=None):
    """One LSTM cell of the bf16-batched decode step (subgc_decode_cell_b16): pre = g0 + table[tok] + g2 + b0 + b1 in fp32, c fp32,
    h rounded once to bf16 into the 1..3 views `hs` (each [S, R] bf16 with its own pitch)."""
    S, R = c.shape
    hs = list(hs)
    if not 1 <= len(hs) <= 3:
        raise SubgcError(f"decode_cell_b16 writes h to 1..3 destinations, got {len(hs)}")
    if (table is None) != (tok is None):
        raise SubgcError("decode_cell_b16: the x->gates table and the tokens come together")
    if g0.size(0) < S or g0.size(1) != 4 * R or any(h_.size(0) < S or h_.size(1) != R for h_ in hs):
        raise SubgcError(f"decode_cell_b16 shape mismatch: g0 {tuple(g0.shape)}, c {tuple(c.shape)}, h {[tuple(h_.shape) for h_ in hs]}")
    if not (c.is_contiguous() and (c_prev is None or (c_prev.is_contiguous() and c_prev.shape == c.shape))):
        raise SubgcError("decode_cell_b16: c and c_prev are contiguous [S, R]")
    hp = []
    for h_ in hs + [None] * (3 - len(hs)):
        hp += [_ptr(h_, BF16), ld(h_) if h_ is not None else 0]
    call_decode_b16("subgc_decode_cell_b16", _ptr(g0, torch.float32), ld(g0), _ptr(table, torch.float32), ld(table) if table is not None else 0,
                    _ptr(tok, torch.int64), tok.stride(0) if tok is not None else 0, table.size(0) if table is not None else 0,
                    _ptr(g2, torch.float32), ld(g2) if g2 is not None else 0, _ptr(b0, torch.float32), _ptr(b1, torch.float32),
                    _ptr(c_prev, torch.float32), _ptr(c, torch.float32), *hp, len(hs), S, R, _stream())


def decode_fork_b16(b16_pairs, f32_pairs, src):
    """dst[m] = src_t[src[m]] for the two bf16 and the two fp32 (source, destination) pairs of the bf16-batched decode state in one launch
    (subgc_decode_fork_b16); `src` int32 [S] on the device, no destination may overlap a source."""
    if len(b16_pairs) != 2 or len(f32_pairs) != 2:
        raise SubgcError("decode_fork_b16 moves two bf16 and two fp32 tensors")
    S = src.numel()
    args = []
    for (a, b), dt in [(p, BF16) for p in b16_pairs] + [(p, torch.float32) for p in f32_pairs]:
        if a.shape != b.shape or a.size(0) != S:
            raise SubgcError(f"decode_fork_b16: {tuple(a.shape)} -> {tuple(b.shape)} with {S} rows")
        args += [_ptr(a, dt), ld(a), _ptr(b, dt), ld(b), a.size(1)]
    call_decode_b16("subgc_decode_fork_b16", *args, _ptr(src, torch.int32), S, _stream())


def scatter_add_rows(src, rows, dX, m_dev=None):
    call("subgc_scatter_add_rows_ws", _ptr(src), ld(src), _ptr(rows, torch.int32), _ptr(dX), ld(dX), src.size(0), src.size(1),
         _ptr(m_dev, torch.int32), dX.size(0), *_det_ws(src), _stream())
    return dX


def sumsq(g, out):
    call("subgc_sumsq_f32_ws", _ptr(g), g.numel(), _ptr(out), *_det_ws(g), _stream())
    return out


OPTIM_RULES = {"adam": 0, "adamw": 1, "sgd": 2, "rmsprop": 3, "adagrad": 4}      # SUBGC_OPTIM_* of the header


def clip_optim_step(rule, p, g, s1, s2, live, sumsq_t, max_norm, grad_scale, lr, h0, h1, eps, wd, step, nesterov=False, first=False,
                    p_bf16=None, zero_grad=False):
    """subgc_clip_optim_step(_zero): global-norm clip + one `rule` update over the flat bucket.  `live`: int64 device tensor of
    [lo, hi) element ranges (flattened lo0, hi0, lo1, ...) of the parameters that are updated, or None for all of them."""
    if live is not None and (live.dtype != torch.int64 or live.numel() % 2 or not live.is_contiguous()):
        raise SubgcError("clip_optim_step: live must be a contiguous int64 tensor of [lo, hi) pairs")
    if any(t is not None and (t.numel() < p.numel() or not t.is_contiguous()) for t in (p, g, s1, s2, p_bf16)):
        raise SubgcError("clip_optim_step: p, g, the states and the snapshot must be contiguous with p.numel() elements")
    call("subgc_clip_optim_step_zero" if zero_grad else "subgc_clip_optim_step", OPTIM_RULES[rule], _ptr(p), _ptr(g), _ptr(s1), _ptr(s2),
         p.numel(), _ptr(live), 0 if live is None else live.numel() // 2, _ptr(sumsq_t), float(max_norm), float(grad_scale), float(lr),
         float(h0), float(h1), float(eps), float(wd), int(step), (1 if nesterov else 0) | (2 if first else 0), _ptr(p_bf16, BF16), _stream())
