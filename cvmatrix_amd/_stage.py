"""The front door of everything that runs on the batched training matrices (ridge.py, pcr.py, pls.py,
predict.py): the argument rules they share and the one way a call into the library is made.  A fitter is its own
argument rules + its output allocations + one ``launch`` (+ its ``check=True`` read-back)."""

from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _lib


def dtype_code(dtype) -> int:
    """The C ABI's element type of a torch dtype (float64, else float32: callers refuse anything else first)."""
    return _lib.CVM_F64 if dtype == torch.float64 else _lib.CVM_F32


def training_pair(who: str, XTX, XTY, *, y_optional: bool = False):
    """``(XTX, XTY, F, K, M)``, checked and contiguous: ``XTX`` (F,K,K) and ``XTY`` (F,K,M) device tensors of one
    dtype (float64 or float32) on one device; a single (K,K) with (K,M) or (K,) is taken as F = 1.
    ``y_optional``: ``XTY`` may be None (M = 0)."""
    no_y = y_optional and XTY is None
    if not (isinstance(XTX, torch.Tensor) and XTX.is_cuda and (no_y or (isinstance(XTY, torch.Tensor) and XTY.is_cuda))):
        raise TypeError(f"{who} takes device tensors (the batched training matrices).")
    if XTX.dim() == 2:
        XTX = XTX.unsqueeze(0)
        if not no_y:
            XTY = XTY.unsqueeze(0) if XTY.dim() == 2 else XTY.reshape(1, -1, 1)
    if XTX.dim() != 3 or XTX.shape[1] != XTX.shape[2]:
        raise ValueError("XTX must be (F,K,K)." if no_y else "XTX must be (F,K,K) and XTY (F,K,M).")
    if not no_y:
        if XTY.dim() != 3 or XTY.shape[:2] != XTX.shape[:2]:
            raise ValueError("XTX must be (F,K,K) and XTY (F,K,M).")
        if XTX.dtype != XTY.dtype:
            raise ValueError("XTX and XTY must both be float64 or both float32.")
        if XTX.device != XTY.device:
            raise ValueError("XTX and XTY must be on one device.")
        XTY = XTY.contiguous()
    if XTX.dtype not in (torch.float64, torch.float32):
        raise ValueError("XTX and XTY must both be float64 or both float32.")
    F, K = XTX.shape[:2]
    return XTX.contiguous(), XTY, F, K, (0 if no_y else XTY.shape[2])


def check_fit_dims(who_text: str, K: int, M: int, max_k: int, max_m: int) -> None:
    """1 <= K <= max_k variables, 1 <= M <= max_m responses; ``who_text`` opens the message ("The device ridge")."""
    if not 1 <= K <= max_k:
        raise ValueError(f"{who_text} takes 1 <= K <= {max_k}.")
    if not 1 <= M <= max_m:
        raise ValueError(f"{who_text} takes 1 to {max_m} responses.")


def check_tolerance(name: str, value) -> float:
    """None or a value <= 0: 0.0 (the library's default); otherwise a float below 1."""
    if value is None:
        return 0.0
    tol = float(value)
    if math.isnan(tol) or tol >= 1.0:
        raise ValueError(f"{name} must be below 1, got {value!r}.")
    return max(tol, 0.0)


def check_grid(name: str, values, limit: int, *, low_open: bool, high=None, scalar_ok: bool = False) -> np.ndarray:
    """A grid of penalties as a contiguous 1-D float64 array: 1 to ``limit`` values (``scalar_ok``: or a scalar),
    each finite and > 0 (``low_open``) or >= 0; with ``high``, each in [0, high] instead."""
    v = np.asarray(values, dtype=np.float64)
    if scalar_ok and v.ndim == 0:
        v = v.reshape(1)
    if v.ndim != 1:
        raise ValueError(f"{name} must be {'a scalar or ' if scalar_ok else ''}one-dimensional, got shape {v.shape}.")
    if not 1 <= v.size <= limit:
        raise ValueError(f"{name} must hold 1 to {limit} values, got {v.size}.")
    one = name.rstrip("s")                        # "every lambda" of "lambdas"
    low_ok = v > 0 if low_open else v >= 0        # (NaN fails every comparison)
    if high is not None:
        if not np.all(low_ok & (v <= high)):
            raise ValueError(f"every {one} must lie in {'(' if low_open else '['}0, {high}].")
    elif not np.all(np.isfinite(v) & low_ok):
        raise ValueError(f"every {one} must be finite and {'>' if low_open else '>='} 0.")
    return np.ascontiguousarray(v)


def check_count(name: str, value, top: int, what: str) -> int:
    """``value`` as an int: an integer (no bool) with 1 <= value <= top; ``what`` is how the message writes the
    upper bound ("K = 7")."""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 1 <= value <= top:
        raise ValueError(f"{name} must be an integer with 1 <= {name} <= {what}, got {value!r}.")
    return int(value)


def launch(what: str, dev, call, ws_bytes: int = 0, *, one: int = 0, limit: Optional[int] = None) -> None:
    """One call into the library on ``dev``'s current stream: ``call(ws_ptr, ws_bytes, stream) -> rc``, raised as
    ``RuntimeError`` unless CVM_OK.  The workspace lives until the stream has passed the call.  ``limit``: at
    most that many bytes, but never less than ``one`` problem needs (the library then runs fewer at once)."""
    if limit is not None:
        ws_bytes = min(ws_bytes, max(one, limit))
    ws_bytes = int(ws_bytes)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
        _lib.check(call(_lib.ptr(ws), ws_bytes, stream.cuda_stream), what)
        if ws is not None:
            ws.record_stream(stream)


def stat_tensor(name, t, F, width, dtype, dev):
    """One statistics tensor as the kernels read it: None, or F x width contiguous elements.  ``F`` None: one
    model, shape (width,); else (F, width), or (F, 1, width) as the fold stage returns it.  The shape is checked,
    not the element count alone: a (width, F) tensor would be read as (F, width) and predict wrongly in silence."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"the {name} must be a device tensor or None.")
    shapes = ((width,),) if F is None else ((F, width), (F, 1, width))
    if t.dtype != dtype or t.device != dev or tuple(t.shape) not in shapes:
        raise ValueError(f"the {name} does not belong to these folds / this model ({tuple(t.shape)} {t.dtype} on "
                         f"{t.device}; wanted {' or '.join(str(x) for x in shapes)} {dtype} on {dev}).")
    return t.contiguous()


def stat_tensors(stats, F, K, M, dtype, dev):
    """``(muX, sdX, muY, sdY)``, each through ``stat_tensor``."""
    if len(stats) != 4:
        raise ValueError("stats must be (muX, sdX, muY, sdY).")
    return tuple(stat_tensor(name, t, F, width, dtype, dev) for name, t, width in zip(
        ("mean of X", "std of X", "mean of Y", "std of Y"), stats, (K, K, M, M)))


def model_batch(who: str, cvm, folds, stats, B):
    """What ``cv_predict`` and ``pls_validation_sse`` both ask of (model, folds, statistics, coefficients): a
    fitted ``CVMatrix`` that keeps float32 / float64 device results, ``B`` (F, A, K, M) of the model's dtype on
    its device with F and K the batch's and the model's, the four statistics as ``stat_tensor`` takes them.
    Returns (the FoldBatch, ``B`` contiguous, the four statistics contiguous or None, the longest fold -- from
    the batch's own host offsets, never a caller's estimate: the kernels cut every fold into that many row
    chunks)."""
    if cvm.X is None:
        raise ValueError(f"{who} needs a fitted CVMatrix.")
    if cvm.output != "torch" or cvm._out_cast:
        raise ValueError(f"{who} takes device results of a float32 / float64 model "
                         "(output='torch', no cast of the results).")
    if not isinstance(B, torch.Tensor) or B.dim() != 4:
        raise ValueError("B must be (F, A, K, M).")
    batch = cvm.prepare_folds(folds)
    F, _, K, M = B.shape
    if K != cvm.K or F != batch.n_folds:
        raise ValueError("B does not belong to these folds / this model.")
    # one element type and one device for everything the kernel reads: it reinterprets X, the statistics and B
    # at B's element size
    dev = cvm.X.device
    if B.dtype != cvm.X.dtype or B.device != dev or B.dtype not in (torch.float64, torch.float32):
        raise ValueError(f"B is {B.dtype} on {B.device}, the model {cvm.X.dtype} on {dev}: {who} takes the "
                         "coefficients of THIS model's training matrices.")
    return batch, B.contiguous(), stat_tensors(stats, F, K, M, B.dtype, dev), int(batch.sizes.max()) if F else 0
