"""Marshalling between torch tensors and the C ABI: what every ``pulse_*`` wrapper (ops.py, kernels.py, MotionLib.query, PdSim) is built from.

A wrapper validates with ``check`` / ``ptr``, fills an argument struct through a ``Filler`` and enqueues with ``launch`` (or, on a hot path,
with the entry bound once by ``entry``).  Nothing here allocates outputs except ``step_outputs``.
"""
import ctypes

import torch

from . import _lib

_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream():
    """The current torch stream of the current device as a hipStream_t.  Called once per kernel launch: the raw accessor is ~20x cheaper than
    building a torch.cuda.Stream object (8 us under a profiler, a tenth of the rollout's host time)."""
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_entries = {}


def entry(name):
    """The C-ABI function ``name``, looked up in the library once (the library is loaded on the first call, never at import)."""
    fn = _entries.get(name)
    if fn is None:
        fn = _entries[name] = getattr(_lib.load(), name)
    return fn


def launch(name, *args, st=None):
    """Enqueue entry ``name`` with ``args`` on stream ``st`` (default: the current one); a failure is reported under the same name."""
    status = entry(name)(*args, stream() if st is None else st)
    if status:
        _lib.check(status, name)


def check(t, name, dtype=torch.float32, unit_stride=False, not_gpu=ValueError):
    """``t`` if it is a GPU tensor of ``dtype`` (bool passes for uint8), optionally with unit inner stride: a raw pointer of another dtype /
    device / layout would be silently re-interpreted by the kernel (e.g. uint8 dones read as int64).  ``not_gpu``: the class raised for a
    tensor that is not on the GPU, the one thing ops (ValueError) and kernels (TypeError) answer differently."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise not_gpu(f"{name}: expected a CUDA tensor, got one on {t.device}: tensors must live on the GPU (pulse_amd has no CPU path)")
    if t.dtype != dtype and not (dtype == torch.uint8 and t.dtype == torch.bool):
        raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if unit_stride and t.numel() > 0 and t.stride(-1) != 1:
        raise ValueError(f"{name}: innermost stride must be 1, got strides {tuple(t.stride())}")
    return t


def ptr(t, name=None, dtype=torch.float32, off=0, unit_stride=False, not_gpu=ValueError):
    """Device address of the optional tensor ``t`` (None for None) plus ``off`` elements of ``dtype``.  With a ``name`` the tensor is
    validated first (``check``); without one the caller vouches for a buffer it validated or allocated itself."""
    if t is None:
        return None
    if name is not None:
        check(t, name, dtype, unit_stride, not_gpu)
    return t.data_ptr() + off * dtype.itemsize if off else t.data_ptr()


def b16(t, what, off=0):
    """Device address (plus ``off`` elements) of an int16 GPU tensor, the storage of bf16 bit patterns; ``what`` names it in the error
    ("ppo_loss: dmu16")."""
    if t.dtype != torch.int16 or not t.is_cuda:
        raise TypeError(f"{what} must be an int16 (bf16 bit pattern) CUDA tensor")
    return t.data_ptr() + 2 * off


def mask_u8(m):
    """A bool mask as uint8 (a view: same memory, in-place edits stay visible to a replayed launch); anything else unchanged."""
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def rows2d(t, name, rows, cols, not_gpu=ValueError):
    """(pointer, row pitch) of a (rows, >= cols) float32 GPU view with unit column stride."""
    check(t, name, not_gpu=not_gpu)
    if t.dim() != 2 or t.shape[0] != rows or t.shape[1] < cols or (t.numel() > 0 and (t.stride(1) != 1 or (rows > 1 and t.stride(0) < cols))):
        raise ValueError(f"{name}: expected a ({rows}, >= {cols}) view with unit column stride, got shape {tuple(t.shape)} strides {tuple(t.stride())}")
    return t.data_ptr(), (t.stride(0) if rows > 1 else max(cols, t.shape[1]))


class Filler:
    """Fills the pointer fields of one launch's argument struct.  ``keep`` holds every tensor the struct points at (temporaries live until
    the wrapper returns -- or as long as a cached struct does); ``copied`` names the arguments that had to be converted into a temporary:
    a struct pointing at a private copy never sees later in-place edits of the caller's tensor, so such a launch must not be cached."""

    def __init__(self, not_gpu=ValueError):
        self.keep, self.copied, self.not_gpu = [], [], not_gpu

    def check(self, t, name, dtype=torch.float32):
        return check(t, name, dtype, not_gpu=self.not_gpu)

    def __call__(self, t, name, dtype=torch.float32, shape=None):
        """Pointer of the optional tensor ``t`` made contiguous (of ``shape``, when given)."""
        if t is None:
            return None
        c = check(t, name, dtype, not_gpu=self.not_gpu)
        if not c.is_contiguous():
            c = c.contiguous()
            self.copied.append(name)
        if shape is not None and tuple(c.shape) != shape:
            raise ValueError(f"{name}: expected shape {shape}, got {tuple(c.shape)}")
        self.keep.append(c)
        return c.data_ptr()

    def ids32(self, ids, name, device):
        """(pointer, count) of an id list as int32 on ``device``.  A Python list is copied silently (its VALUES identify the launch); a tensor
        that had to be converted counts as copied."""
        if isinstance(ids, torch.Tensor):
            t = ids.to(device=device, dtype=torch.int32).contiguous()
            if t.data_ptr() != ids.data_ptr():
                self.copied.append(name)
        else:
            t = torch.tensor(list(ids), dtype=torch.int32, device=device)
        self.keep.append(t)
        return t.data_ptr(), t.numel()


def select_envs(a, fill, env_ids, env_mask):
    """The env selection every ``*_args`` struct with these fields shares: an int64 id list and / or a bool / uint8 mask."""
    if env_ids is not None:
        a.env_ids, a.num_ids = fill(env_ids, "env_ids", torch.int64), env_ids.numel()
    if env_mask is not None:
        a.env_mask = fill(mask_u8(env_mask), "env_mask", torch.uint8)


def step_outputs(a, fill, out, n, device, *, reward, resets, raw_width, rew=None, rew_raw=None, reset=None, terminate=None):
    """The step wrappers' output blocks: the reward pair (``rew`` (N,), ``rew_raw`` (N, raw_width) float32) when ``reward``, the reset pair
    (``reset`` / ``terminate`` (N,) int64) when ``resets``; each allocated when not supplied, validated when it is, written into the struct
    and into ``out``."""
    if reward:
        rew = torch.empty(n, dtype=torch.float32, device=device) if rew is None else fill.check(rew, "rew")
        rew_raw = torch.empty(n, raw_width, dtype=torch.float32, device=device) if rew_raw is None else fill.check(rew_raw, "rew_raw")
        if not (rew.is_contiguous() and rew_raw.is_contiguous() and rew_raw.shape[-1] == raw_width):
            raise ValueError(f"rew / rew_raw must be contiguous, rew_raw (N, {raw_width})")
        a.rew, a.rew_raw = rew.data_ptr(), rew_raw.data_ptr()
        out["rew"], out["rew_raw"] = rew, rew_raw
    if resets:
        reset = torch.empty(n, dtype=torch.int64, device=device) if reset is None else fill.check(reset, "reset", torch.int64)
        terminate = torch.empty(n, dtype=torch.int64, device=device) if terminate is None else fill.check(terminate, "terminate", torch.int64)
        a.reset, a.terminate = reset.data_ptr(), terminate.data_ptr()
        out["reset"], out["terminate"] = reset, terminate
