"""CVMatrix on MI355X: host-side mirror of the reference class.

Same constructor / ``fit`` / ``training_XTX`` / ``training_XTY`` / ``training_XTX_XTY`` /
``training_statistics`` surface, return structure, ``None`` pattern, shapes and
``ValueError`` messages as the reference (cvmatrix/cvmatrix.py:157-167, 207-212, 330-332,
385-387, 451-453, 519-521), with ``backend="hip"``: the fit stage and the per-fold stage
each run as one call into libcvmhip.so (include/cvmhip.h) on PyTorch-ROCm device memory.
Like the reference's ``backend="jax"`` returning ``jax.Array``, results are device arrays
(``torch.Tensor`` on the GPU); ``.cpu().numpy()`` gives the NumPy view.

New next to the reference API: the ``*_batched`` methods process many folds per launch
(the shape the reference reaches with ``jax.vmap`` in benchmarks/benchmark.py:144-152),
taking a ``Partitioner``, a list of index arrays or a prepared ``FoldBatch``.

There is no CPU path in this module: it raises if the extension or a GPU is missing.
"""

from __future__ import annotations

import contextlib
import os
import weakref

from typing import Iterable, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._request import fold_request, stat_addresses, stat_views
from ._stage import dtype_code
from .partitioner import Partitioner, partitioner_of, partitioner_pos

MSG_NEG_W = "Weights must be non-negative."
MSG_NZ_ZERO = (
    "The number of non-zero weights in the training set must be greater than zero."
)
MSG_NZ_DDOF = (
    "The number of non-zero weights in the training set must be greater than `ddof`."
)
MSG_NEITHER = "At least one of `return_XTX` and `return_XTY` must be True."
MSG_NO_Y = "Response variables `Y` are not provided."

_TORCH_DT = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32}


class _WeightsToken:
    """Identity of one validated set of weights.  A ``FoldBatch`` remembers the token its
    non-zero-weight counts were computed for; tokens are never reused, so a batch carried to
    another ``CVMatrix`` (or across a refit with other weights) is recounted."""
    __slots__ = ()


_NO_WEIGHTS = _WeightsToken()      # unweighted: the counts are the fold sizes, whoever asks


def _same_objects(a: list, b: list) -> bool:
    """Do two lists hold the very same objects, in order?  (List equality compares by identity
    first; arrays that are not identical raise on the ambiguous truth value of ``==``.)"""
    if len(a) != len(b):
        return False
    try:
        return a == b and all(x is y for x, y in zip(a[:4], b[:4]))
    except ValueError:
        return False


def _same_indices(v: np.ndarray, seg: np.ndarray) -> bool:
    """Does the caller's index array hold exactly what the private copy ``seg`` holds?  (The exact
    comparison behind every served loop: 7 us for 10 000 indices, 0.2 us for 100.)"""
    if v.size != seg.size:
        return False
    if v.dtype == seg.dtype and v.ndim == 1 and v.flags.c_contiguous:
        return v.tobytes() == seg.tobytes()
    return bool(np.array_equal(v.reshape(-1), seg))


def _resolve_backend(backend: str) -> str:
    """Counterpart of cvmatrix.py:58-96 for this package.  ``"hip"``: results stay on the device
    (torch tensors, like the reference's ``backend="jax"`` returns ``jax.Array``).  ``"numpy"``:
    the reference's NumPy contract at the seam -- ndarray in, ndarray out, the reference's
    attribute types -- so that a caller written for ``CVMatrix(backend="numpy")`` runs unchanged;
    the arithmetic is still the HIP library's (there is no CPU path in this package)."""
    if backend in ("hip", "numpy"):
        return backend
    # same form as cvmatrix.py:96 ("Invalid backend: 'x'. Must be 'numpy' or 'jax'."); the
    # reference's JAX backend lives in the reference package
    raise ValueError(f"Invalid backend: {backend!r}. Must be 'hip' or 'numpy'.")


class FoldBatch:
    """Validation indices of many folds, resident on the device in CSR form.

    idx      int64[n]     concatenated row numbers (wrapped to [0,N))
    offsets  int64[P+1]   fold f owns idx[offsets[f]:offsets[f+1]]
    Built by ``CVMatrix.prepare_folds``; reusable across ``*_batched`` calls.
    """

    def __init__(self, idx, offsets, host_offsets, nz_val, labels=None, host_idx=None, n_rows=0,
                 device=None, w_gen=None):
        self._idx, self._offsets = idx, offsets
        self.host_offsets, self._nz_val, self.labels = host_offsets, nz_val, labels
        self._nz_fn = None      # nz_val not counted yet (weights validated on the device): how to count them
        self._host_idx, self._n_rows, self._is_partition = host_idx, n_rows, None
        self._sizes = None
        self._device = device
        self._w_gen = w_gen     # CVMatrix._w_gen the non-zero counts were computed for
        self._source = None     # the Partitioner the batch was prepared from, if any

    # one fold of at most 32 rows is created without device arrays: the matrix calls hand its
    # indices to the library from the host (CVM_IDX_HOST); anything else uploads them on demand
    @property
    def inline(self) -> bool:
        return self._idx is None

    def _upload(self) -> None:
        with torch.cuda.device(self._device):
            d_all = torch.from_numpy(np.concatenate([self.host_offsets, self._host_idx])).to(self._device)
        n_off = self.host_offsets.size
        self._offsets, self._idx = d_all[:n_off], d_all[n_off:]

    @property
    def idx(self):
        if self._idx is None:
            self._upload()
        return self._idx

    @property
    def offsets(self):
        if self._offsets is None:
            self._upload()
        return self._offsets

    # every fold's number of validation rows with a non-zero weight.  With weights that were validated on the
    # device (CVMatrix(validate_weights="deferred")) they are NOT counted when the batch is made: the raises they
    # feed (cvmatrix.py:612-630, 1074-1078) are first decided on a bound that needs no per-fold count
    # (CVMatrix._validate), and counted exactly -- here, on first access -- only when that bound does not decide
    @property
    def nz_val(self):
        if self._nz_val is None and self._nz_fn is not None:
            self._nz_val = self._nz_fn(self)
        return self._nz_val

    @nz_val.setter
    def nz_val(self, v) -> None:
        self._nz_val = v

    @property
    def nz_known(self) -> bool:
        return self._nz_val is not None

    @property
    def is_partition(self) -> bool:
        """Every row of X in exactly one fold (checked once, on first use)."""
        if self._is_partition is None:
            i, n = self._host_idx, self._n_rows
            self._is_partition = bool(i is not None and n > 0 and i.size == n
                                      and (np.bincount(i, minlength=n) == 1).all())
        return self._is_partition

    @property
    def n_folds(self) -> int:
        return int(self.host_offsets.size - 1)

    @property
    def sizes(self) -> np.ndarray:
        if self._sizes is None:
            self._sizes = np.diff(self.host_offsets)
        return self._sizes


class _ReadAhead:
    """State of a read-ahead over a Partitioner's folds (CVMatrix._ra_*)."""
    __slots__ = ("p", "arrs", "n", "batch", "key", "pos", "start", "count", "chunk", "max_chunk", "xtx", "xty",
                 "stats", "req", "bad_zero", "bad_ddof", "sizes", "first", "lo", "hidx")


class CVMatrix:
    """Fast training-set ``XᵀWX`` / ``XᵀWY`` for cross-validation (Engstrøm & Jensen),
    computed on an MI355X.  Parameters as cvmatrix.py:109-155; ``dtype`` must be
    float64 or float32; ``backend`` must be ``"hip"``; ``device`` picks the GPU
    (default: the current torch device)."""

    def __init__(
        self,
        center_X: bool = True,
        center_Y: bool = True,
        scale_X: bool = True,
        scale_Y: bool = True,
        ddof: int = 1,
        dtype=np.float64,
        copy: bool = True,
        backend: str = "hip",
        device: Union[None, str, int, torch.device] = None,
        lazy_fit: Optional[bool] = None,
        output: str = "torch",
        serve_loops: Optional[bool] = None,
        reuse_outputs: bool = False,
        trust_tensor_versions: Optional[bool] = None,
        validate_weights: Optional[str] = None,
    ) -> None:
        # ``lazy_fit=None`` (default): ``fit`` may defer its arithmetic to the first use only
        # when the object owns private copies of its inputs (``copy=True``, like the reference's
        # default): nothing the caller does to its own arrays between ``fit`` and that first
        # use can then change a result.  ``copy=False`` aliases caller memory
        # (cvmatrix.py:1146-1148), so ``fit`` computes at once like cvmatrix.py:325-328.
        # CVM_LAZY_FIT=0/1 overrides the default (the test-suite runs both ways).
        if lazy_fit is None:
            env = os.environ.get("CVM_LAZY_FIT")
            lazy_fit = bool(copy) if env is None else env != "0"
        self.lazy_fit = bool(lazy_fit)
        # ``serve_loops`` (default on; CVM_SERVE_LOOPS=0/1 overrides the default): recognise the
        # reference's one-call-per-fold loop over a ``Partitioner``'s own index arrays and serve it
        # from one sweep / a read-ahead / the uploaded indices of an earlier pass.  Every such
        # short cut compares the caller's array EXACTLY with the private copy the batch was built
        # from before anything is handed out; ``serve_loops=False`` turns them all off: every call
        # then gathers from whatever the array holds and launches its own kernels, like
        # cvmatrix.py:924-941.
        if serve_loops is None:
            serve_loops = os.environ.get("CVM_SERVE_LOOPS", "1") != "0"
        self.serve_loops = bool(serve_loops)
        # ``reuse_outputs`` (default off: every call returns fresh tensors, like the reference returns fresh
        # arrays): the full-data matrices and the batched outputs / statistics of a call are written into
        # buffers the object keeps while shapes repeat, so a loop of fit + batched call allocates nothing --
        # results of an earlier call (and the XTX / XTY attributes of an earlier fit) are OVERWRITTEN by the
        # next one.  For loops that consume each step's results before the next step (a multi-GPU rank's
        # step is shorter than the allocations it would otherwise issue).
        self.reuse_outputs = bool(reuse_outputs)
        # ``trust_tensor_versions`` (default OFF; CVM_TRUST_VERSIONS=1 turns the default on): when ``fit`` is
        # handed the very device tensors of this object's previous ``fit`` and torch's version counters say
        # nothing was written to them since, skip what that fit already did -- the private copies (``copy=True``),
        # the read-back and sign check of the weights, the shape bookkeeping (a benchmark-style loop of fit +
        # batched call on resident inputs: 0.070 -> 0.040 ms of host time per step).  The version counter sees
        # every write made THROUGH torch; it does not see ``t.data`` writes, DLPack / ``__cuda_array_interface__``
        # consumers (CuPy, Numba), raw-pointer kernels or another library's in-place update.  After such a write a
        # trusting ``fit`` would return the PREVIOUS data's matrices, where the reference re-reads its inputs on
        # every ``fit`` (cvmatrix.py:207-328) -- hence off unless asked for, per object here or per call with
        # ``fit(..., assume_unchanged=True)``.
        if trust_tensor_versions is None:
            trust_tensor_versions = os.environ.get("CVM_TRUST_VERSIONS", "0") != "0"
        self.trust_tensor_versions = bool(trust_tensor_versions)
        # ``validate_weights`` -- where weights handed to ``fit`` as a DEVICE tensor are checked (weights given as
        # host arrays are always checked inside ``fit``, before they are uploaded: cvmatrix.py:1188-1189):
        #   "deferred" (default; CVM_VALIDATE_WEIGHTS overrides the default): on the device.  ``fit`` launches one
        #       small kernel that counts the negative and the non-zero weights (cvm_weights_check) and copies the two
        #       counts to pinned memory asynchronously; nothing is read back and the host does not wait.
        #       ``ValueError("Weights must be non-negative.")`` is raised by the first call that hands out a result
        #       or an attribute of that fit -- behind its launches, in front of its return -- the way the reference's
        #       JAX backend defers its data-dependent raises (cvmatrix.py:621-625, 1071-1074).  Per-fold counts of
        #       non-zero weights (the "... must be greater than zero / than `ddof`" raises) are decided on a bound
        #       that needs only the total (a fold cannot hold more non-zero weights than rows) and counted exactly
        #       only where that bound does not decide.
        #   "sync": ``fit`` reads the weights back (one blocking 8 N byte copy) and raises itself, like rounds 1-5.
        if validate_weights is None:
            validate_weights = os.environ.get("CVM_VALIDATE_WEIGHTS", "deferred")
        if validate_weights not in ("deferred", "sync"):
            raise ValueError(f"Invalid validate_weights: {validate_weights!r}. Must be 'deferred' or 'sync'.")
        self.validate_weights = validate_weights
        self._wchk = False              # a deferred weights check is pending (its counts are on their way)
        self._wchk_bufs = None          # (device int64[2], pinned int64[2], event)
        self._w_verified = False        # the current weights passed a deferred check
        self._w_bad = False             # ... or failed it: every hand-out raises until the next fit
        self._arena = {}
        self._fit_src = None
        # ``output="numpy"``: every result (matrices, statistics, the XTX/XTY/sum_* attributes)
        # is returned as a NumPy array like the reference's backend="numpy"; "torch" (default)
        # leaves results on the device, like the reference's backend="jax" returns jax.Array
        if output not in ("torch", "numpy"):
            raise ValueError(f"Invalid output: {output!r}. Must be 'torch' or 'numpy'.")
        if backend == "numpy":
            output = "numpy"
        self.output = output
        self._pending = False
        self.center_X, self.center_Y = center_X, center_Y
        self.scale_X, self.scale_Y = scale_X, scale_Y
        self.ddof = ddof
        if isinstance(dtype, torch.dtype):
            dtype = {torch.float64: np.float64, torch.float32: np.float32}.get(dtype, dtype)
        self.dtype = dtype.type if isinstance(dtype, np.dtype) else dtype
        self.copy = copy
        self.backend = _resolve_backend(backend)
        try:
            npdt = np.dtype(self.dtype)
        except TypeError as e:
            raise TypeError(f"dtype {dtype!r} is not a floating-point type") from e
        if npdt.kind != "f":
            raise TypeError(f"dtype {dtype!r} is not a floating-point type")
        # The reference's dtype surface (tests/test_cvmatrix.py:1147-1205 runs float16, float32,
        # float64 and float128).  The kernels compute in float32 or float64: float16 problems are
        # rounded to float16 like the reference rounds its inputs (cvmatrix.py:1146), computed in
        # float32 and returned as float16; wider types (np.longdouble) are computed in float64 and
        # returned as NumPy arrays of the requested type (torch has no such dtype) -- 1e-16
        # instead of 1e-19 relative, well inside the 1e-10 parity bar.
        self._res_npdt = npdt                          # what results are handed out as
        self._out_cast = None
        if npdt not in _TORCH_DT:
            if npdt.itemsize < 4:
                self._out_cast, npdt = "half", np.dtype(np.float32)
            else:
                self._out_cast, npdt = "wide", np.dtype(np.float64)
                self.output = "numpy"
        self._npdt, self._tdt = npdt, _TORCH_DT[npdt]
        self._cdt = dtype_code(self._tdt)
        self.resolution = np.finfo(self.dtype).resolution * 10  # cvmatrix.py:187
        self._device_arg = device
        self.device: Optional[torch.device] = None
        self.X = self.Y = self.weights = None
        self.N = self._Kd = self._Md = None           # device dims (columns padded to 16-byte rows)
        self._Ku = self._Mu = None                    # the caller's K, M
        self.XTX = self.XTY = None
        self._sum_w = None
        self._n_total = self._nz_total = None
        self._gstats = None
        self._globals = None
        self._w_host = None
        self._nz_mask = None
        self._stage_bufs = None
        self._ws = None
        self._nz_total_gen, self._nz_total_w = None, 0
        self._sweep = None
        self._sweep_cache = None
        self._ra = None                                 # read-ahead of a per-fold loop (_ReadAhead)
        self._pbatches = weakref.WeakKeyDictionary()   # Partitioner -> FoldBatch (uploaded indices)
        self._sweep_ws = None
        self._sweep_ids = None
        self._auto_sweep_tried = None
        self.sweep_folds = None
        self._w_checked = None
        self._w_checked_src = None
        self._w_gen = _NO_WEIGHTS  # token of the validated weights (a new object whenever they change)
        self._np_cache = {}
        self._small_ws_key = None
        self._small_ws_bytes = 0
        self._one_off = None

    # ------------------------------------------------------------------ full-data matrices
    # ``fit`` may leave them pending (``lazy_fit``): they are computed on first use -- by the
    # fit-stage kernel, or, when the first use is a batched call whose folds partition the
    # rows, as the sum of the folds' validation matrices in the same sweep that serves the
    # folds (half the arithmetic; SURVEY.md 8(f) rank 1, "behind the same API").
    def _out(self, t, key=None):
        """A result in the form ``output`` asks for: the device tensor, or its NumPy copy
        (attributes are copied once per fit: ``key``)."""
        if t is None:
            return t
        if self._out_cast == "half" and self.output != "numpy":
            return t.to(torch.float16)
        if self.output != "numpy":
            return t
        if key is None:
            return self._np_result(t)
        if key not in self._np_cache:
            self._np_cache[key] = self._np_result(t)
        return self._np_cache[key]

    def _np_result(self, t):
        a = t.cpu().numpy()
        # (the conversion has just waited for the stream: the fold stage's status word costs one more small read
        #  here -- a call whose results are poisoned raises instead of handing NaN out as numbers)
        if self.__dict__.get("_fold_status"):
            self._raise_if_poisoned()
        return a if self._out_cast is None else a.astype(self._res_npdt)

    # Results whose last dimensions are the DEVICE dims (the columns of the private device copies
    # may be padded, see ``fit``): cut back to the caller's K, M.  ``key``: an attribute (the cut
    # copy is kept per fit).  Unpadded problems pass through untouched.
    def _cut_t(self, t, kind: str):
        """The tensor cut to the caller's dims (a contiguous copy when anything is cut off)."""
        if t is None:
            return None
        K, M, Kd, Md = self._Ku, self._Mu or 0, self._Kd, self._Md or 0
        if Kd == K and Md == M:
            return t
        if kind == "XX":
            t = t[..., :K, :K]
        elif kind == "XY":
            t = t[..., :K, :M]
        elif kind == "X":
            t = t[..., :K]
        else:
            t = t[..., :M]
        return t.contiguous()

    def _cut(self, t, kind: str, key=None):
        if t is None:
            return None
        if self._Kd == self._Ku and (self._Md or 0) == (self._Mu or 0):
            return self._out(t, key)
        if key is not None:
            if ("cut", key) not in self._np_cache:
                self._np_cache[("cut", key)] = self._cut_t(t, kind)
            return self._out(self._np_cache[("cut", key)], key)
        return self._out(self._cut_t(t, kind))

    def _oXX(self, t, key=None):
        return self._cut(t, "XX", key)

    def _oXY(self, t, key=None):
        return self._cut(t, "XY", key)

    def _oX(self, t, key=None):
        return self._cut(t, "X", key)

    def _oY(self, t, key=None):
        return self._cut(t, "Y", key)

    @property
    def _conv(self):
        """The four converters in the order ``FoldRequest.pack`` takes them."""
        return self._oXX, self._oXY, self._oX, self._oY

    def _request(self, rXTX: bool, rXTY: bool):
        """What a call asks for under the object's CURRENT centre / scale flags (public attributes: looked up
        per call, never frozen)."""
        return fold_request(rXTX, rXTY, self.center_X, self.center_Y, self.scale_X, self.scale_Y)

    def _device_dims(self, K: int, M: int):
        """Columns of the device copies of X and Y: padded with zero columns to rows of whole
        16-byte pieces (float64: even K and M; float32: K a multiple of 4) when the object owns
        private copies anyway (``copy=True``) -- every shape then takes the LDS-DMA Gram kernel
        (K=511 at the C3 shape: 0.77 -> 0.51 ms per step) at the price of a cut of the results back
        to K x K.  A zero column has mean 0 and std 0 -> 1 and contributes nothing to any other
        element.  ``copy=False`` (inputs aliased) and CVM_PAD=0 keep the caller's shape (the
        general kernels)."""
        if not self.copy or os.environ.get("CVM_PAD", "1") == "0":
            return K, M
        a = 16 // np.dtype(self._npdt).itemsize
        Kd = -(-K // a) * a
        Md = M + (M & 1) if (M and a == 2) else M
        return Kd, Md

    @property
    def K(self):
        """Number of columns of X (the caller's; the device copy may be padded, see ``fit``)."""
        return self._Ku

    @property
    def M(self):
        return self._Mu

    @property
    def XTX(self):
        self._ensure_fit()
        self._resolve_weights_check()
        return self._oXX(self._G, "XTX")

    @XTX.setter
    def XTX(self, v):
        self._G = v

    @property
    def XTY(self):
        self._ensure_fit()
        self._resolve_weights_check()
        return self._oXY(self._H, "XTY")

    @XTY.setter
    def XTY(self, v):
        self._H = v

    @property
    def _gstats(self):
        self._ensure_fit()
        return self._gs

    @_gstats.setter
    def _gstats(self, v):
        self._gs = v

    def _ensure_fit(self) -> None:
        if not self.__dict__.get("_pending", False):
            return
        self._pending = False
        lib = _lib.load()
        with torch.cuda.device(self.device):
            self._launch_fit(lib)
        self._after_globals()

    def _launch_fit(self, lib) -> None:
        """The fit-stage kernel over all rows (cvm_gram_fit)."""
        M = self._Md or 0
        if self.N == 0:
            # no rows (a rank of a multi-GPU job that owns none): the matrices of nothing are
            # zeros -- no kernel, and the exchange that follows still takes place
            self._zero_globals()
            return
        neg = torch.empty(1, dtype=torch.int32, device=self.device)   # always written by fit_stats_kernel
        ws = self._workspace(lib.cvm_fit_workspace_bytes(self.N, self._Kd, M, self._cdt))
        rc = lib.cvm_gram_fit(
            self.X.data_ptr(), _lib.ptr(self.Y), _lib.ptr(self.weights), self.N, self._Kd,
            M, self._cdt, self._G.data_ptr(), _lib.ptr(self._H),
            self._gs.data_ptr(), neg.data_ptr(), ws.data_ptr(), ws.numel(),
            self._stream(),
        )
        _lib.check(rc, "cvm_gram_fit")
        self._neg = neg

    def _zero_globals(self) -> None:
        for t in ((self._globals,) if self._globals is not None else (self._G, self._H, self._gs)):
            if t is not None:
                t.zero_()
        self._neg = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _after_globals(self) -> None:
        """Hook: the full-data matrices of this process have just been launched (multi-GPU
        subclasses exchange them here)."""

    def _exchanges_globals(self) -> bool:
        """Does ``_after_globals`` change the full-data matrices (a multi-GPU exchange)?  Then the
        fold stage cannot share a call with the sweep that forms them."""
        return False

    def _sweep_worth(self, lib, batch) -> bool:
        """Do the folds of ``batch`` partition the rows, and is the one-sweep path the faster one?"""
        sizes = batch.sizes
        # worth it when the folds are large: the sweep saves one pass of the Gram kernel over all
        # rows and costs a write + read of every fold's K x (K+M) partials (about 256 rows of
        # Gram work per fold at float64); small folds have their own direct route anyway
        worth = (batch.n_folds > 0 and self.N > 0 and int(sizes.min()) > 32 and self.N >= 256 * batch.n_folds
                 and lib.cvm_sweep_workspace_bytes(batch.n_folds, int(sizes.max()), self._Kd, self._Md or 0,
                                                   self._cdt) <= (4 << 30))
        return bool(worth and batch._n_rows == self.N and batch.is_partition)

    def _lazy_sweep(self, batch) -> None:
        """First use after a lazy ``fit`` is a batched call: if its folds partition the rows,
        form the full-data matrices as the sum of the folds' validation matrices."""
        if not self.__dict__.get("_pending", False):
            return
        lib = _lib.load()
        if self._sweep_worth(lib, batch):
            self._pending = False
            with torch.cuda.device(self.device):
                neg = torch.empty(1, dtype=torch.int32, device=self.device)
                self._fit_sweep(lib, batch, neg)
            self._after_globals()
        else:
            self._ensure_fit()

    # ------------------------------------------------------------------ plumbing
    def _pick_device(self) -> torch.device:
        if not torch.cuda.is_available():
            raise RuntimeError(
                "cvmatrix_amd needs an AMD GPU visible to PyTorch-ROCm; there is no "
                "CPU fallback."
            )
        d = self._device_arg
        if d is None:
            return torch.device("cuda", torch.cuda.current_device())
        d = torch.device(d if not isinstance(d, int) else f"cuda:{d}")
        return torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())

    @staticmethod
    def _cols_of(mat) -> int:
        shp = tuple(mat.shape) if hasattr(mat, "shape") else np.asarray(mat).shape
        if len(shp) == 1:
            return 1
        if len(shp) != 2:
            raise ValueError("expected a 1-D or 2-D array")
        return int(shp[1])

    def _init_mat(self, mat, pad_cols: Optional[int] = None) -> torch.Tensor:
        """cvmatrix.py:1131-1151 on the device: cast, copy iff needed, 1-D -> (N,1).
        ``pad_cols`` > columns: the private copy gets that many columns (zeros behind the data) and
        the returned tensor is the view of its first columns (same address, row stride pad_cols)."""
        if self._out_cast == "half":                  # (the reference rounds its inputs to float16 first)
            mat = (mat.to(torch.float16) if isinstance(mat, torch.Tensor) else np.asarray(mat, dtype=np.float16))
        if isinstance(mat, torch.Tensor):
            t = mat
            fresh = False
            if t.device != self.device or t.dtype != self._tdt or not t.is_contiguous():
                t = t.to(device=self.device, dtype=self._tdt).contiguous()
                fresh = True
        else:
            h = np.ascontiguousarray(np.asarray(mat, dtype=self._npdt))
            t = torch.from_numpy(h).to(self.device)  # the upload is the private copy
            fresh = True
        if t.ndim == 1:
            t = t.reshape(-1, 1)
        if t.ndim != 2:
            raise ValueError("expected a 1-D or 2-D array")
        if pad_cols is not None and pad_cols > t.shape[1]:
            store = torch.zeros((t.shape[0], pad_cols), dtype=self._tdt, device=self.device)
            store[:, :t.shape[1]].copy_(t)
            return store[:, :t.shape[1]]
        if self.copy and not fresh:
            t = t.clone()
        return t

    def _on_device(self):
        """Context in which ``self.device`` is current (nothing to switch when it already is)."""
        if torch.cuda.current_device() == self.device.index:
            return contextlib.nullcontext()
        return torch.cuda.device(self.device)

    def _workspace(self, nbytes: int) -> torch.Tensor:
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != self.device:
            self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        return self._ws

    def _stream(self) -> int:
        """The caller's current HIP stream on this device, as the integer the C ABI takes."""
        try:
            return torch._C._cuda_getCurrentRawStream(self.device.index)
        except AttributeError:                       # (private helper of torch; fall back to the API)
            return torch.cuda.current_stream(self.device).cuda_stream

    # ------------------------------------------------------------------ fit stage
    def fit(self, X, Y=None, weights=None, folds=None, assume_unchanged: Optional[bool] = None) -> None:
        """Store ``X``, ``Y``, ``weights`` on the device and compute the full-data
        ``XᵀWX``, ``XᵀWY`` and column statistics in one pass (cvmatrix.py:207-328).  With
        ``lazy_fit`` (the default) that pass is left pending until the matrices are first needed
        (see the class properties above): a batched call over folds that partition the rows then
        produces them in the same sweep that serves the folds.

        ``folds`` (not in the reference; optional): a ``Partitioner``, a list of index arrays
        or a ``FoldBatch`` that PARTITIONS the rows.  The full-data matrices are then formed
        as the sum of the folds' validation matrices in one sweep, and a later
        ``training_*_batched`` call with the same ``FoldBatch`` (returned by
        ``prepare_folds`` / kept in ``self.sweep_folds``) only runs the correction kernels:
        half the arithmetic of ``fit`` + fold update.  Results agree to rounding.

        ``assume_unchanged`` (not in the reference; default: the object's ``trust_tensor_versions``, off): the
        caller states that device tensors which ARE the previous fit's (same objects, same torch version
        counters -- both are still checked) hold the previous fit's values, so the copies, the weight
        validation and the bookkeeping of that fit stand.  Do not state it for tensors something writes to
        behind torch's back (``.data``, DLPack, raw pointers): see ``trust_tensor_versions``.

        Raises ``ValueError("Weights must be non-negative.")`` like cvmatrix.py:1188-1189.
        """
        lib = _lib.load()
        trust = self.trust_tensor_versions if assume_unchanged is None else bool(assume_unchanged)
        self.device = self._pick_device()
        # nothing of an earlier fit may survive a fit that raises half-way
        self._sweep = None
        self._sweep_cache = None
        self._ra = None
        self._sweep_ids = None
        self._auto_sweep_tried = None
        self._pending = False
        self._np_cache = {}
        with self._on_device():
            # the same device tensors as the last fit of this object, unmodified since (object identity +
            # torch's version counter, which every in-place write through any view bumps): the device
            # copies / aliases, the validated weights and the shapes of that fit are still right
            same = trust and self._same_fit_inputs(X, Y, weights)
            if not same:
                self._fit_src = None
                Ku = self._cols_of(X)
                Mu = self._cols_of(Y) if Y is not None else None
                self._Kd, Md = self._device_dims(Ku, Mu or 0)
                self.X = self._init_mat(X, self._Kd)         # (a view of the padded copy when padded)
                self.N, self._Ku = self.X.shape
                if Y is not None:
                    self.Y = self._init_mat(Y, Md)
                    self._Mu, self._Md = self.Y.shape[1], Md
                    if self.Y.shape[0] != self.N:
                        raise ValueError("X and Y must have the same number of rows")
                else:
                    self.Y, self._Mu, self._Md = None, None, None
                self._wchk = False
                if weights is not None:
                    on_dev = isinstance(weights, torch.Tensor) and weights.device.type != "cpu"
                    if on_dev and self.validate_weights == "deferred":
                        known = trust and self._weights_known(weights)
                        self.weights = self._init_mat(weights)
                        if self.weights.shape != (self.N, 1):
                            raise ValueError("weights must have shape (N,) or (N, 1)")
                        if not known:
                            self._defer_weights_check(lib, weights)
                    else:
                        self._check_weights_host(weights, trust)
                        self.weights = self._init_mat(weights)
                        if self.weights.shape != (self.N, 1):
                            raise ValueError("weights must have shape (N,) or (N, 1)")
                else:
                    if self.weights is not None or self._w_host is not None:
                        self._w_gen = _NO_WEIGHTS
                    self.weights, self._w_host, self._w_checked, self._w_checked_src = None, None, None, None
                    self._w_verified = self._w_bad = False
                self._remember_fit_inputs(X, Y, weights)      # (what a LATER fit may be told is unchanged)
            M = self._Md or 0
            self._alloc_globals(lib.cvm_gstats_len(self._Kd, M))
            self._neg = None
            if folds is not None:
                neg = torch.empty(1, dtype=torch.int32, device=self.device)
                self._fit_sweep(lib, folds, neg)
                self._neg = neg
            elif self.lazy_fit:
                self._pending = True
            else:
                self._launch_fit(lib)
            self._publish_stats()
        if not self._pending:
            self._after_globals()

    @staticmethod
    def _tensor_key(t):
        return None if t is None else (id(t), t._version, t.data_ptr())

    def _remember_fit_inputs(self, X, Y, weights) -> None:
        """What ``fit`` was given, if all of it is device tensors (kept referenced, so that an address cannot
        be recycled by another tensor), with the version counters of that moment -- and the versions of the
        device copies this object made of them."""
        if self.serve_loops and all(t is None or (isinstance(t, torch.Tensor) and t.is_cuda) for t in (X, Y, weights)):
            self._fit_src = ((X, Y, weights), tuple(self._tensor_key(t) for t in (X, Y, weights)),
                             tuple(self._tensor_key(t) for t in (self.X, self.Y, self.weights)))
        else:
            self._fit_src = None

    def _same_fit_inputs(self, X, Y, weights) -> bool:
        src = self._fit_src
        if src is None or self.X is None:
            return False
        (x0, y0, w0), keys, own = src
        if X is not x0 or Y is not y0 or weights is not w0:
            return False
        if tuple(self._tensor_key(t) for t in (X, Y, weights)) != keys:
            return False
        # (the object's own copies may have been written through the public attributes)
        return tuple(self._tensor_key(t) for t in (self.X, self.Y, self.weights)) == own

    def _alloc_globals(self, n_gstats: int) -> None:
        """``XTX``, ``XTY`` and the float64 statistics vector as views of ONE contiguous
        buffer ``[G | H | gstats]`` (float64 problems): the multi-GPU exchange is then a single
        collective on that buffer with nothing to pack.  float32 problems keep separate
        tensors (the statistics stay float64)."""
        K, M, dev = self._Kd, self._Md or 0, self.device
        hasY = self.Y is not None
        if self.reuse_outputs:
            key = (K, M, hasY, n_gstats, self._tdt, dev)
            if self._arena.get("globals") == key:
                return                                # (the buffers of the last fit: same shapes)
            self._arena["globals"] = key
        if self._tdt == torch.float64:
            nG, nH = K * K, (K * M if hasY else 0)
            flat = torch.empty(nG + nH + n_gstats, dtype=torch.float64, device=dev)
            self._globals = flat
            self.XTX = flat[:nG].view(K, K)
            self.XTY = flat[nG:nG + nH].view(K, M) if hasY else None
            self._gstats = flat[nG + nH:]
        else:
            self._globals = None
            self.XTX = torch.empty((K, K), dtype=self._tdt, device=dev)
            self.XTY = torch.empty((K, M), dtype=self._tdt, device=dev) if hasY else None
            self._gstats = torch.empty(n_gstats, dtype=torch.float64, device=dev)

    def _fit_sweep(self, lib, folds, neg) -> None:
        """One-sweep fit: Gram kernel over all folds once, full-data matrices = their sum
        (cvm_sweep_fit); the per-fold partials stay in a dedicated workspace."""
        batch = self.prepare_folds(folds)
        if not batch.is_partition:
            raise ValueError("fit(folds=...) needs folds that contain every row exactly once")
        K, M, P = self._Kd, self._Md or 0, batch.n_folds
        want = lib.cvm_sweep_workspace_bytes(P, int(batch.sizes.max()), K, M, self._cdt)
        if (getattr(self, "_sweep_ws", None) is None or self._sweep_ws.numel() < want
                or self._sweep_ws.device != self.device):
            self._sweep_ws = torch.empty(int(want), dtype=torch.uint8, device=self.device)
        import ctypes as C

        splits = C.c_int64(0)
        rc = lib.cvm_sweep_fit(
            self.X.data_ptr(), _lib.ptr(self.Y), _lib.ptr(self.weights), batch.idx.data_ptr(),
            batch.offsets.data_ptr(), batch.host_offsets.ctypes.data, P, self.N, K, M, self._cdt,
            self._G.data_ptr(), _lib.ptr(self._H), self._gs.data_ptr(), neg.data_ptr(),
            self._sweep_ws.data_ptr(), self._sweep_ws.numel(), self._stream(), C.byref(splits),
        )
        _lib.check(rc, "cvm_sweep_fit")
        self._remember_sweep(batch, int(splits.value))

    def _remember_sweep(self, batch, token: int) -> None:
        self._sweep = (batch, token)
        self._sweep_cache = None
        self.sweep_folds = batch
        # the folds of a Partitioner can later be asked for one at a time with the very arrays it
        # holds (the reference's loop): remember them by identity; what such an array holds at the
        # time of the call is compared exactly with the batch's private copy (_sweep_fold_of)
        src = batch._source
        self._sweep_ids = None
        if (self.serve_loops and src is not None and batch._host_idx is not None
                and len(src._fold_arrays) == batch.n_folds):
            arrs = src._fold_arrays
            self._sweep_ids = ({id(a): i for i, a in enumerate(arrs)}, arrs)

    @staticmethod
    def _weights_key(w):
        if isinstance(w, torch.Tensor):
            return (w.data_ptr(), w._version, tuple(w.shape), tuple(w.stride()), w.dtype)
        return None

    def _check_weights_host(self, weights, trust: bool = False) -> None:
        """Sign check (cvmatrix.py:1188-1189) + host copy of the weights (per-fold validity
        checks), before anything is launched.  A device tensor costs one read-back; with ``trust``
        (``trust_tensor_versions`` / ``fit(assume_unchanged=True)``) the SAME tensor object, unmodified
        since the last fit by torch's version counter (the object is kept referenced, so its address
        cannot be recycled by another tensor), is not read again."""
        if isinstance(weights, torch.Tensor) and weights.device.type != "cpu":
            key = self._weights_key(weights)
            if (trust and self.serve_loops and weights is self._w_checked_src and key == self._w_checked
                    and self._w_host is not None):
                return
            h = weights.detach().reshape(-1).cpu().numpy()
            src = weights
        else:
            if isinstance(weights, torch.Tensor):
                weights = weights.detach().numpy()
            h = np.asarray(weights).reshape(-1)
            key = src = None
        if self._out_cast == "half":
            h = np.asarray(h).astype(np.float16)      # (non-zero counts are taken after the rounding, like the reference's)
        self._w_verified = self._w_bad = False
        if bool(np.any(h < 0)):
            raise ValueError(MSG_NEG_W)
        self._w_host = np.array(h, dtype=self._npdt, copy=True)
        self._w_checked, self._w_checked_src = key, src
        self._w_gen = _WeightsToken()

    # ---- weights validated on the device (validate_weights="deferred") -------------------------------------
    def _weights_known(self, weights) -> bool:
        """Is ``weights`` the very tensor -- unmodified since, by torch's version counter -- whose check (on the host,
        on the device, or still on its way) belongs to the object's current weights?"""
        return bool(self.serve_loops and weights is self._w_checked_src and self._weights_key(weights) == self._w_checked
                    and (self._w_host is not None or self._w_verified or self._wchk) and not self._w_bad)

    def _defer_weights_check(self, lib, src) -> None:
        """cvmatrix.py:1188-1189 and 1226 for device weights, without a read-back: [#(w < 0), #(w != 0)] of the
        object's own device copy (rounded like the reference rounds: _init_mat) by one small launch, copied to
        pinned memory behind it; ``_resolve_weights_check`` reads them."""
        bufs = self._wchk_bufs
        if bufs is None or bufs[0].device != self.device:
            bufs = self._wchk_bufs = (torch.empty(2, dtype=torch.int64, device=self.device),
                                      torch.empty(2, dtype=torch.int64, pin_memory=True), torch.cuda.Event())
        d, h, ev = bufs
        _lib.check(lib.cvm_weights_check(self.weights.data_ptr(), self.N, self._cdt, d.data_ptr(), self._stream()),
                   "cvm_weights_check")
        h.copy_(d, non_blocking=True)
        ev.record()
        self._wchk, self._w_verified, self._w_bad = True, False, False
        self._w_host = None
        self._w_checked, self._w_checked_src = self._weights_key(src), src
        self._w_gen = _WeightsToken()

    def _resolve_weights_check(self) -> None:
        """Await the counts of a deferred check (a wait for one small kernel that was enqueued BEFORE the Gram
        launch of its step: the device keeps working) and raise like ``fit`` would have.  A fit whose weights
        failed raises at every hand-out until the next fit."""
        if self._wchk:
            self._wchk = False
            _, h, ev = self._wchk_bufs
            ev.synchronize()
            neg, nz = int(h[0]), int(h[1])
            if neg:
                self._w_bad = True
            else:
                self._w_verified = True
                self._nz_total_w, self._nz_total_gen = nz, self._w_gen
                if self._nz_total is None:
                    self._nz_total = nz
        if self._w_bad:
            raise ValueError(MSG_NEG_W)

    def _host_weights(self) -> Optional[np.ndarray]:
        """The weights on the host (exact per-fold counts of non-zero weights need them): read back on first
        need when they were validated on the device."""
        if self._w_host is None and self.weights is not None:
            self._resolve_weights_check()
            self._w_host = np.array(self.weights.detach().reshape(-1).cpu().numpy(), dtype=self._npdt, copy=True)
        return self._w_host

    def _publish_stats(self) -> None:
        """Host-side totals used by the per-fold validity checks.  ``_n_total`` /
        ``_nz_total`` are the sample count and non-zero weight count of the WHOLE data set
        (a row-sharded multi-GPU fit overrides them with the all-reduced values)."""
        self._sum_w = None
        self._n_total = self.N
        if self.weights is None:
            self._nz_total = self.N
        elif self._wchk:
            self._nz_total = None                          # (on its way from the device: _resolve_weights_check)
        else:
            if self._nz_total_gen is not self._w_gen:      # (once per set of weights, not per fit)
                self._nz_total_w, self._nz_total_gen = int(np.count_nonzero(self._host_weights())), self._w_gen
            self._nz_total = self._nz_total_w

    def _resolve_totals(self) -> None:
        """Make ``_n_total`` / ``_nz_total`` current: the counts of a deferred weights check (multi-GPU
        subclasses then fetch the all-reduced counts)."""
        self._resolve_weights_check()

    def _totals_in_flight(self) -> bool:
        """True while those counts are still on the device (a deferred weights check; a multi-GPU exchange)."""
        return bool(self._wchk)

    def _request_totals(self) -> None:
        """Hook: start fetching those counts (asynchronously; ``_resolve_totals`` waits)."""

    def _passes_on_local_counts(self, batch, need_stats: bool, need_std: bool, only: Optional[int] = None) -> bool:
        """While the global counts are still in flight, this process's own counts (``_publish_stats``)
        are LOWER bounds of them: if even they leave every fold's training set more non-zero
        weights than ``ddof`` (and than zero), neither of the reference's raises
        (cvmatrix.py:612-630, 1074-1078) can fire whatever the other ranks hold, and the check
        needs no read-back at all."""
        if self._wchk or self._w_bad:
            return False                               # (the sign of the weights is still to be seen)
        if not need_stats:
            return True
        sel = slice(None) if only is None else slice(only, only + 1)
        if self.weights is not None:
            if self._nz_total is None:
                return False
            # (per-fold counts not taken -- weights validated on the device --: a fold holds at most as many
            #  non-zero weights as rows, still a lower bound)
            lb = self._nz_total - (batch.nz_val[sel] if batch.nz_known else batch.sizes[sel])
        else:
            lb = self._n_total - batch.sizes[sel]
        return bool(lb.size == 0 or int(lb.min()) > max(int(np.ceil(self.ddof)) if need_std else 0, 0))

    def _gslice(self, lo: int, hi: int, cond: bool):
        if not cond or self._gstats is None:
            return None
        self._resolve_weights_check()
        return self._out(self._gstats[lo:hi].to(self._tdt).reshape(1, -1), ("gstats", lo, hi))

    # The reference's global statistics attributes, present under the reference's flag
    # conditions (cvmatrix.py:1223-1243), materialised from the float64 device vector on
    # access.
    @property
    def _anyflag(self) -> bool:
        return bool(self.center_X or self.center_Y or self.scale_X or self.scale_Y)

    @property
    def sum_X(self):
        return self._gslice(0, self._Ku, self.center_X or self.center_Y or self.scale_X)

    @property
    def sum_sq_X(self):
        return self._gslice(self._Kd, self._Kd + self._Ku, self.scale_X)

    @property
    def sum_Y(self):
        M = self._Mu or 0
        return self._gslice(2 * self._Kd, 2 * self._Kd + M,
                            (self.center_X or self.center_Y or self.scale_Y)
                            and self.Y is not None)

    @property
    def sum_sq_Y(self):
        M, Md = self._Mu or 0, self._Md or 0
        return self._gslice(2 * self._Kd + Md, 2 * self._Kd + Md + M,
                            self.scale_Y and self.Y is not None)

    @property
    def num_nonzero_w(self):
        """cvmatrix.py:1226/1229; ``None`` without centre/scale flags."""
        if not self._anyflag or self.X is None:
            return None
        self._ensure_fit()
        self._resolve_totals()
        return self._nz_total

    @property
    def sum_w(self):
        """Sum of the weights (cvmatrix.py:1225/1228); ``None`` without centre/scale flags."""
        if not self._anyflag or self.X is None:
            return None
        if self.weights is None:
            self._ensure_fit()
            self._resolve_totals()
            return self._n_total
        if self._sum_w is None:
            K, M = self._Kd, self._Md or 0
            self._resolve_weights_check()
            self._sum_w = self.dtype(self._gstats[2 * K + 2 * M].item())
        return self._sum_w

    # ------------------------------------------------------------------ fold batches
    def _wrap_indices(self, v) -> np.ndarray:
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        v = np.asarray(v)
        if v.dtype == bool:
            v = np.flatnonzero(v)
        if v.size == 0:
            return np.zeros(0, dtype=np.int64)
        if v.dtype.kind not in "iu":
            raise IndexError("validation indices must be integers")
        v = v.astype(np.int64, copy=False).reshape(-1)
        if v.min() < -self.N or v.max() >= self.N:
            raise IndexError(f"validation index out of bounds for {self.N} samples")
        return np.where(v < 0, v + self.N, v) if v.min() < 0 else v

    def prepare_folds(self, folds, _trust_cached: bool = False) -> FoldBatch:
        """Upload validation indices of many folds once (CSR) and pre-compute the per-fold
        non-zero weight counts on the host.  ``folds``: a ``Partitioner``, or a sequence of
        index arrays.  (``_trust_cached``: internal -- the caller compares every fold's array
        with the batch's private copy itself before it uses that fold.)"""
        if self.X is None:
            raise RuntimeError("call fit() first")
        if isinstance(folds, FoldBatch):
            # a prepared batch is tied to the row count it was bounds-checked against (the
            # kernels do no bounds checks) and to the weights its non-zero counts came from
            if folds._n_rows != self.N:
                raise ValueError(
                    f"this FoldBatch was prepared for {folds._n_rows} samples, the fitted "
                    f"data has {self.N}: prepare the folds again after fit()")
            if folds._w_gen is not self._w_gen:
                if self.weights is not None and self._w_host is None:
                    folds.nz_val, folds._nz_fn = None, self._nz_counts      # (counted on first need: FoldBatch.nz_val)
                else:
                    folds.nz_val = self._nz_counts(folds)
                folds._w_gen = self._w_gen
            return folds
        labels = None
        source = None
        if isinstance(folds, Partitioner):
            cached = self._cached_partitioner_batch(folds, _trust_cached)
            if cached is not None:
                return self.prepare_folds(cached)      # (row count / weights checks of a FoldBatch)
            source = folds
            labels = list(folds.folds_dict)
            folds = list(folds.folds_dict.values())
            if not _same_objects(folds, source._fold_arrays):
                source = None       # folds_dict was reassigned after construction: a plain list of arrays
        if not isinstance(folds, (list, tuple)):
            folds = list(folds)
        if folds and all(type(v) is np.ndarray and v.ndim == 1 and v.dtype.kind in "iu" for v in folds):
            # integer index arrays (what a Partitioner holds): one bounds check / wrap for the
            # whole batch instead of one per fold (100 000 leave-one-out folds: 0.2 s -> ms)
            if (source is not None and source._base is not None and source._starts is None
                    and source._base.ndim == 2 and source._base.shape[0] == len(folds)
                    and source._base.flags.c_contiguous):
                # equal folds kept as the rows of one matrix (arange(N) % P, leave-one-out): that
                # matrix IS the concatenation (100 000 one-row folds: 30 ms of np.concatenate saved)
                sizes = np.full(len(folds), source._base.shape[1], dtype=np.int64)
                idx = np.array(source._base.reshape(-1), dtype=np.int64)      # (a private copy)
            else:
                sizes = np.fromiter((v.size for v in folds), dtype=np.int64, count=len(folds))
                idx = np.concatenate(folds).astype(np.int64, copy=False)
            if idx.size:
                lo, hi = int(idx.min()), int(idx.max())
                if lo < -self.N or hi >= self.N:
                    raise IndexError(f"validation index out of bounds for {self.N} samples")
                if lo < 0:
                    idx = np.where(idx < 0, idx + self.N, idx)
            parts = folds
        else:
            parts = [self._wrap_indices(v) for v in folds]
            sizes = np.array([p.size for p in parts], dtype=np.int64)
            idx = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
        host_offsets = np.zeros(len(parts) + 1, dtype=np.int64)
        np.cumsum(sizes, out=host_offsets[1:])
        lazy_nz = self.weights is not None and self._w_host is None   # (weights validated on the device)
        nz_val = None if lazy_nz else self._nz_counts_host(idx, host_offsets, sizes)
        # one host->device copy for both arrays, [offsets | idx], through a pinned staging
        # buffer and asynchronous on the stream: a pageable copy would hold the host until the
        # device has drained the stream, and the per-fold call pattern (one small copy per
        # call) would run host and device in turns instead of side by side
        n_off, n_all = host_offsets.size, host_offsets.size + idx.size
        if sizes.size and int(sizes.max()) <= 32:
            # tiny folds (leave-one-out style calls): the device work per call is shorter than
            # the host's; the plain copy costs the host less than staging does
            if len(parts) == 1:
                # the reference's call pattern, one small fold per call: no device copy at all
                fb = FoldBatch(None, None, host_offsets, nz_val, labels,
                               np.ascontiguousarray(idx, dtype=np.int64), self.N, device=self.device,
                               w_gen=self._w_gen)
                fb._nz_fn = self._nz_counts if lazy_nz else None
                return fb
            with torch.cuda.device(self.device):
                d_all = torch.from_numpy(np.concatenate([host_offsets, idx])).to(self.device)
            fb = FoldBatch(d_all[n_off:], d_all[:n_off], host_offsets, nz_val, labels, idx, self.N,
                           w_gen=self._w_gen)
            fb._nz_fn = self._nz_counts if lazy_nz else None
            return fb
        with torch.cuda.device(self.device):
            stage = self._staging(n_all)
            view = stage.numpy()
            view[:n_off] = host_offsets
            view[n_off:n_all] = idx
            d_all = torch.empty(n_all, dtype=torch.int64, device=self.device)
            d_all.copy_(stage[:n_all], non_blocking=True)
            self._stage_events[self._stage_next - 1].record()
        d_off, d_idx = d_all[:n_off], d_all[n_off:]
        fb = FoldBatch(d_idx, d_off, host_offsets, nz_val, labels, idx, self.N, w_gen=self._w_gen)
        fb._nz_fn = self._nz_counts if lazy_nz else None
        fb._source = source
        fb._device = self.device
        if self.serve_loops and source is not None and len(parts) <= 4096:
            # the same Partitioner again (a fit + per-fold loop repeated, another model on the same
            # folds): the uploaded indices are reused while its arrays still hold EXACTLY what the
            # private host copy of the batch holds (_cached_partitioner_batch)
            self._pbatches[source] = fb
        return fb

    def _cached_partitioner_batch(self, p, trust: bool = False) -> Optional[FoldBatch]:
        """The uploaded batch of an earlier ``prepare_folds(p)``, if ``p``'s arrays still hold
        what they held then -- an exact comparison with the batch's private host copy (one
        comparison of the whole index matrix for equal folds, else fold by fold).  ``trust``: the
        caller makes that comparison itself, per fold, at the time each fold is used."""
        fb = self._pbatches.get(p) if self.serve_loops else None
        if fb is None:
            return None
        arrs = p._fold_arrays
        ok = (fb._n_rows == self.N and fb._device == self.device and len(arrs) == fb.n_folds
              and fb._host_idx is not None and _same_objects(list(p.folds_dict.values()), arrs))
        if ok and not trust:
            hidx, ho = fb._host_idx, fb.host_offsets
            b = p._base
            if (b is not None and p._starts is None and b.ndim == 2 and b.shape[0] == len(arrs)
                    and b.flags.c_contiguous and b.size == hidx.size):
                ok = _same_indices(b.reshape(-1), hidx)
            else:
                ok = all(_same_indices(a, hidx[ho[i]:ho[i + 1]]) for i, a in enumerate(arrs))
        if not ok:
            del self._pbatches[p]
            return None
        return fb

    def _nz_counts_host(self, idx: np.ndarray, host_offsets: np.ndarray, sizes: np.ndarray) -> np.ndarray:
        """Non-zero weights among each fold's validation rows (exact integer counts for the
        host-side raises, cvmatrix.py:612-630, 1074-1078)."""
        if self.weights is None:
            return sizes.copy()
        wh = self._host_weights()
        if self._nz_mask is None or self._nz_mask[0] is not wh:
            self._nz_mask = (wh, (wh != 0).astype(np.int64))   # once per fit
        nzmask = self._nz_mask[1]
        if sizes.size == 1:
            return np.array([int(nzmask[idx].sum())], dtype=np.int64)
        csum = np.concatenate([[0], np.cumsum(nzmask[idx])])
        return csum[host_offsets[1:]] - csum[host_offsets[:-1]]

    def _nz_counts(self, batch: "FoldBatch") -> np.ndarray:
        """The same counts for an existing batch (after a refit with other weights)."""
        if batch._host_idx is not None:
            return self._nz_counts_host(batch._host_idx, batch.host_offsets, batch.sizes)
        if self.weights is None:
            return batch.sizes.copy()
        nzmask = (self.weights.reshape(-1) != 0).to(torch.int64)
        csum = torch.cat([torch.zeros(1, dtype=torch.int64, device=self.device),
                          torch.cumsum(nzmask[batch.idx], 0)])
        return (csum[batch.offsets[1:]] - csum[batch.offsets[:-1]]).cpu().numpy()

    def prepare_folds_from_labels(self, labels, n_labels: Optional[int] = None) -> FoldBatch:
        """Device-side ``Partitioner``: one fold label per row -- integers in ``[0, n_labels)`` (NumPy
        array or tensor), or labels of any hashable kind (strings, floats, objects: factorised on the
        host in first-seen order, one vectorised pass) -> a ``FoldBatch`` built by ``cvm_partition_labels`` without
        the host ever grouping the rows (any number of labels: up to 4096 one stable counting
        sort, more -- leave-one-out has one per row -- the same sort over 12-bit digits; labels
        that are ``arange(N) % P``, the reference benchmark's folds, or ``arange(N)`` are laid out
        by formula without a sort).  Folds are ordered by first appearance of their label, like
        the reference's ``folds_dict`` (partitioner.py:101-107); ``batch.labels`` lists the labels
        in that order."""
        if self.X is None:
            raise RuntimeError("call fit() first")
        lib = _lib.load()
        dev = self.device
        keys = None
        if not isinstance(labels, torch.Tensor):
            try:
                arr = np.asarray(labels).reshape(-1)
            except ValueError:                         # (ragged objects, e.g. tuples next to strings)
                labels = list(labels)
                arr = np.fromiter(labels, dtype=object, count=len(labels))
            if arr.dtype.kind not in "iub":
                # labels of any hashable kind (strings, floats, mixed objects: partitioner.py:101-107
                # takes them all): one vectorised host pass turns them into integer codes numbered by
                # first appearance -- the reference's dict order -- and the grouping itself runs on the
                # device like for integer labels; ``batch.labels`` lists the original labels
                if arr.dtype.kind == "O":
                    seen: dict = {}                    # (objects: the reference's own loop, partitioner.py:101-107)
                    codes = np.fromiter((seen.setdefault(v, len(seen)) for v in labels), dtype=np.int64, count=arr.size)
                    keys = list(seen)
                else:
                    # sorted unique values with the index of their first appearance, re-ranked by
                    # that index = codes in first-seen order.  equal_nan=False: every NaN is a label
                    # of its own, like in the reference's dict (nan != nan) and in Partitioner
                    uniq, first_idx, inv = np.unique(arr, return_index=True, return_inverse=True, equal_nan=False)
                    seen_order = np.argsort(first_idx, kind="stable")
                    rank = np.empty(uniq.size, dtype=np.int64)
                    rank[seen_order] = np.arange(uniq.size, dtype=np.int64)
                    codes = rank[np.asarray(inv).reshape(-1)]
                    keys = list(uniq[seen_order])
                labels, n_labels = np.asarray(codes, dtype=np.int64), len(keys)
        with torch.cuda.device(dev):
            if isinstance(labels, torch.Tensor):
                lab = labels.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
            else:
                lab = torch.from_numpy(np.ascontiguousarray(np.asarray(labels).reshape(-1),
                                                            dtype=np.int64)).to(dev)
            if lab.numel() != self.N:
                raise ValueError("one fold label per row is needed")
            # one read-back for both ends: labels outside [0, L) are refused here, before any
            # kernel sorts them (partition.hpp only flags them)
            lo_hi = torch.stack(torch.aminmax(lab)).cpu() if self.N else torch.zeros(2, dtype=torch.int64)
            lab_lo, lab_hi = int(lo_hi[0]), int(lo_hi[1])
            L = int(n_labels) if n_labels is not None else lab_hi + 1
            if lab_lo < 0 or lab_hi >= L:
                raise ValueError(f"fold labels must be integers in [0, {L})")
            if 1 <= L <= self.N:
                # the strided folds of the reference's benchmark (benchmarks/benchmark.py:232) and
                # leave-one-out: row r is the (r // L)-th row of fold r % L -- no sort needed.  One
                # launch checks the labels, lays the folds out and counts their non-zero weights
                # (cvm_partition_periodic); one read-back brings the verdict and the counts
                d_idx = torch.empty(self.N, dtype=torch.int64, device=dev)
                d_off = torch.empty(L + 1, dtype=torch.int64, device=dev)
                tail = torch.empty(L + 1, dtype=torch.int64, device=dev)      # [nz of every fold | flag]
                wt = self.weights
                rc = lib.cvm_partition_periodic(lab.data_ptr(), self.N, L, _lib.ptr(wt), self._cdt, d_idx.data_ptr(),
                                                d_off.data_ptr(), tail.data_ptr() if wt is not None else None,
                                                tail.data_ptr() + 8 * L, self._stream())
                _lib.check(rc, "cvm_partition_periodic")
                h_tail = tail.cpu().numpy()
                if int(h_tail[L:].view(np.int32)[0]) == 0:
                    sizes = (self.N - np.arange(L) + L - 1) // L
                    host_offsets = np.zeros(L + 1, dtype=np.int64)
                    np.cumsum(sizes, out=host_offsets[1:])
                    nz_val = h_tail[:L].copy() if wt is not None else sizes.astype(np.int64)
                    return FoldBatch(d_idx, d_off, host_offsets, nz_val,
                                     list(range(L)) if keys is None else [keys[i] for i in range(L)], None, self.N,
                                     w_gen=self._w_gen)
            idx = torch.empty(self.N, dtype=torch.int64, device=dev)
            offs = torch.empty(L + 1, dtype=torch.int64, device=dev)
            first = torch.empty(L, dtype=torch.int64, device=dev)
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            ws = torch.empty(int(lib.cvm_partition_workspace_bytes(self.N, L)), dtype=torch.uint8,
                             device=dev)
            rc = lib.cvm_partition_labels(lab.data_ptr(), self.N, L, idx.data_ptr(), offs.data_ptr(),
                                          first.data_ptr(), err.data_ptr(), ws.data_ptr(),
                                          ws.numel(), self._stream())
            _lib.check(rc, "cvm_partition_labels")
            h_offs, h_first = offs.cpu().numpy(), first.cpu().numpy()
            if int(err.item()) != 0:
                raise ValueError(f"fold labels must be integers in [0, {L})")
            present = np.flatnonzero(h_first < self.N)
            order = present[np.argsort(h_first[present], kind="stable")]     # first-seen order
            sizes = (h_offs[1:] - h_offs[:-1])[order]
            host_offsets = np.zeros(order.size + 1, dtype=np.int64)
            np.cumsum(sizes, out=host_offsets[1:])
            if np.array_equal(order, np.arange(L)):
                d_idx, d_off = idx, offs                    # already in fold order
            else:
                # gather the folds' segments into first-seen order on the device
                seg_start = torch.from_numpy(h_offs[:-1][order].copy()).to(dev)
                new_off = torch.from_numpy(host_offsets).to(dev)
                pos = torch.arange(self.N, dtype=torch.int64, device=dev)
                f_of = torch.searchsorted(new_off[1:], pos, right=True)
                d_idx = idx[seg_start[f_of] + (pos - new_off[f_of])]
                d_off = new_off
            if self.weights is not None:
                nzmask = (self.weights.reshape(-1) != 0).to(torch.int64)
                csum = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev),
                                  torch.cumsum(nzmask[d_idx], 0)])
                nz_val = (csum[d_off[1:]] - csum[d_off[:-1]]).cpu().numpy()
            else:
                nz_val = sizes.copy()
        return FoldBatch(d_idx, d_off, host_offsets, nz_val,
                         [int(v) for v in order] if keys is None else [keys[int(v)] for v in order], None, self.N,
                         w_gen=self._w_gen)

    def _staging(self, n: int) -> torch.Tensor:
        """Next pinned int64 staging buffer of a small ring (reused once the copy that last
        read it has completed)."""
        ring = 8
        if self._stage_bufs is None:
            self._stage_bufs, self._stage_events, self._stage_next = [None] * ring, [None] * ring, 0
        k = self._stage_next % ring
        self._stage_next = k + 1
        ev = self._stage_events[k]
        if ev is not None:
            ev.synchronize()
        buf = self._stage_bufs[k]
        if buf is None or buf.numel() < n:
            buf = torch.empty(max(n, 4096), dtype=torch.int64, pin_memory=True)
            self._stage_bufs[k] = buf
        if ev is None:
            self._stage_events[k] = torch.cuda.Event()
        return buf

    def _validate(self, batch, need_stats: bool, need_std: bool, only: Optional[int] = None) -> None:
        """The reference's data-dependent raises, in its order (zero check first, weighted
        only: cvmatrix.py:612-630; then ddof: 1074-1078), decided on exact host counts.
        ``only``: check fold ``only`` of the batch alone."""
        if not need_stats:
            self._resolve_weights_check()
            return
        if self._totals_in_flight() and self._passes_on_local_counts(batch, need_stats, need_std, only):
            return
        self._resolve_totals()
        sel = slice(None) if only is None else slice(only, only + 1)
        if self.weights is not None:
            if not batch.nz_known and self._nz_total is not None:
                # weights validated on the device, per-fold counts not taken: a fold cannot hold more non-zero
                # weights than rows -- if even that leaves every training set more than ``ddof`` (and than zero),
                # neither raise can fire and the exact counts are never needed
                sz = batch.sizes[sel]
                if sz.size == 0 or self._nz_total - int(sz.max()) > max(int(np.ceil(self.ddof)) if need_std else 0, 0):
                    return
            nz_train = self._nz_total - batch.nz_val[sel]
            if np.any(nz_train == 0):
                raise ValueError(MSG_NZ_ZERO)
        else:
            nz_train = self._n_total - batch.sizes[sel]
        if need_std and np.any(nz_train <= self.ddof):
            raise ValueError(MSG_NZ_DDOF)

    def _run(self, batch: FoldBatch, rXTX: bool, rXTY: bool, stat_flags=None,
             stats_only: bool = False, sweep_fold: Optional[int] = None, sweep_all: bool = False):
        """One cvm_fold_update call over ``batch``.  Returns raw stacked device tensors.
        ``stats_only``: keep the return flags (they select which statistics the kernel
        derives, _request.FoldRequest) but produce no matrices.  ``sweep_all``: a lazy fit is
        pending and ``batch`` partitions the rows -- the fit and the fold stage as one call
        (cvm_sweep_all)."""
        lib = _lib.load()
        if not sweep_all:
            self._ensure_fit()
        K, M, P = self._Kd, self._Md or 0, (batch.n_folds if sweep_fold is None else 1)
        flags = (self._request(rXTX, rXTY) if stat_flags is None else fold_request(rXTX, rXTY, *stat_flags)).flags
        dev, dt = self.device, self._tdt
        with self._on_device():
            mats = not stats_only
            akey = ("run", P, K, M, bool(rXTX and mats), bool(rXTY and mats), dt, dev)
            held = self._arena.get(akey) if self.reuse_outputs else None
            if held is not None:
                out_XTX, out_XTY, muX, sdX, muY, sdY, neg_held = held
            else:
                out_XTX = torch.empty((P, K, K), dtype=dt, device=dev) if (rXTX and mats) else None
                out_XTY = torch.empty((P, K, M), dtype=dt, device=dev) if (rXTY and mats) else None
                # the four statistics: one allocation [muX | sdX | muY | sdY], each block [P, 1, *]
                muX, sdX, muY, sdY = stat_views(torch.empty(P * (2 * K + 2 * M), dtype=dt, device=dev), P, K, M)
                neg_held = None
                if self.reuse_outputs:
                    neg_held = torch.empty(1, dtype=torch.int32, device=dev)
                    self._arena[akey] = (out_XTX, out_XTY, muX, sdX, muY, sdY, neg_held)
            out_fold = None       # (per-fold [sw_T, nz_T, sw_V, nz_V]: diagnostics, not requested)
            if sweep_all:
                import ctypes as C

                skey = (P, int(batch.sizes.max()), K, M, self._cdt)
                if self._arena.get("sweep_ws_key") != skey or self._sweep_ws is None or self._sweep_ws.device != dev:
                    want = lib.cvm_sweep_workspace_bytes(*skey)
                    if self._sweep_ws is None or self._sweep_ws.numel() < want or self._sweep_ws.device != dev:
                        self._sweep_ws = torch.empty(int(want), dtype=torch.uint8, device=dev)
                    self._arena["sweep_ws_key"] = skey
                neg = neg_held if neg_held is not None else torch.empty(1, dtype=torch.int32, device=dev)
                token = C.c_int64(0)
                self._pending = False
                rc = lib.cvm_sweep_all(
                    self.X.data_ptr(), _lib.ptr(self.Y), _lib.ptr(self.weights), batch.idx.data_ptr(),
                    batch.offsets.data_ptr(), batch.host_offsets.ctypes.data, P, self.N, K, M, self._cdt,
                    flags, float(self.ddof), float(self.resolution),
                    self._G.data_ptr(), _lib.ptr(self._H), self._gs.data_ptr(), neg.data_ptr(),
                    _lib.ptr(out_XTX), _lib.ptr(out_XTY), muX.data_ptr(), sdX.data_ptr(),
                    _lib.ptr(muY), _lib.ptr(sdY), _lib.ptr(out_fold),
                    self._sweep_ws.data_ptr(), self._sweep_ws.numel(), self._stream(), C.byref(token),
                )
                _lib.check(rc, "cvm_sweep_all")
                self._neg = neg
                self._remember_sweep(batch, int(token.value))
                self._after_globals()
                return out_XTX, out_XTY, (muX, sdX, muY, sdY), out_fold
            sweep = getattr(self, "_sweep", None)
            if sweep is not None and sweep[0] is batch:
                # the partials of exactly these folds are still in the sweep workspace
                rc = lib.cvm_sweep_fold_range(
                    batch.offsets.data_ptr(), batch.n_folds, 0 if sweep_fold is None else sweep_fold, P,
                    K, M, self._cdt, flags, float(self.ddof),
                    float(self.resolution), 1 if self.weights is not None else 0,
                    self._G.data_ptr(), _lib.ptr(self._H), self._gs.data_ptr(),
                    _lib.ptr(out_XTX), _lib.ptr(out_XTY), muX.data_ptr(), sdX.data_ptr(),
                    _lib.ptr(muY), _lib.ptr(sdY), _lib.ptr(out_fold),
                    self._sweep_ws.data_ptr(), self._sweep_ws.numel(), sweep[1], self._stream(),
                )
                _lib.check(rc, "cvm_sweep_fold_range")
                return out_XTX, out_XTY, (muX, sdX, muY, sdY), out_fold
            sizes = batch.sizes
            want = lib.cvm_fold_workspace_bytes(P, int(batch.host_offsets[-1]),
                                                int(sizes.max()) if P else 0, K, M,
                                                self._cdt, flags)
            ws = self._workspace(want)
            if batch.inline and mats and (rXTX or rXTY):
                flags |= _lib.IDX_HOST
                p_idx, p_off = batch._host_idx.ctypes.data, batch.host_offsets.ctypes.data
            else:
                p_idx, p_off = batch.idx.data_ptr(), batch.offsets.data_ptr()
            # (one status word per device and stream this object has launched on: words of launches in flight on
            #  other streams are never reset under them)
            words = self.__dict__.setdefault("_fold_status", {})
            skey = (dev.index, self._stream())
            status = words.get(skey)
            if status is None:
                status = words[skey] = torch.zeros(1, dtype=torch.int32, device=dev)
            rc = lib.cvm_fold_update_ex(
                self.X.data_ptr(), _lib.ptr(self.Y), _lib.ptr(self.weights),
                p_idx, p_off,
                batch.host_offsets.ctypes.data, P, self.N, K, M, self._cdt, flags,
                float(self.ddof), float(self.resolution), self._G.data_ptr(),
                _lib.ptr(self._H), self._gs.data_ptr(), _lib.ptr(out_XTX),
                _lib.ptr(out_XTY), muX.data_ptr(), sdX.data_ptr(), _lib.ptr(muY),
                _lib.ptr(sdY), _lib.ptr(out_fold), ws.data_ptr(), ws.numel(), self._stream(),
                status.data_ptr(),
            )
            _lib.check(rc, "cvm_fold_update_ex")
        return out_XTX, out_XTY, (muX, sdX, muY, sdY), out_fold

    def fold_status(self, reset: bool = True) -> int:
        """Status of the fold-stage calls made so far (``cvm_fold_update_ex``; one small device read per stream the
        object has launched on, each waits for its stream): 0 = no work item ever gave up waiting for another, 2 =
        some did and were recomputed inside their call (every result valid), 1 = results of some call hold NaN (a
        fault: the reference's contract is "raise or return correct numbers", cvmatrix.py:754-896).  ``reset``
        zeroes the words.  Results handed out as NumPy arrays (``output="numpy"``) are checked for status 1 by the
        conversion itself (it has to wait for the device anyway) and raise ``RuntimeError``; results left on the
        device are the caller's to check -- with this method -- before they are trusted: an asynchronous API cannot
        raise for a launch that has not run yet."""
        worst = 0
        for t in self.__dict__.get("_fold_status", {}).values():
            v = int(t.item())
            if reset and v:
                t.zero_()
            worst = 1 if (v == 1 or worst == 1) else max(worst, v)
        return worst

    def _raise_if_poisoned(self) -> None:
        if self.fold_status(reset=False) == 1:
            self.fold_status(reset=True)
            raise RuntimeError("cvmatrix_amd: a work item of the fold stage gave up waiting for another in both of its "
                               "launches; the affected results hold NaN (CVMatrix.fold_status() == 1)")

    def _own_results(self, xtx, xty, stats):
        """Results of ``_run`` that the object is about to KEEP (the slices a per-fold loop is served from):
        with ``reuse_outputs`` they are the arena's buffers, which the next call of the same shape -- a
        batched call the user makes between two calls of the loop -- overwrites; the kept copy must then be
        the object's own."""
        if not self.reuse_outputs:
            return xtx, xty, stats
        cl = lambda t: None if t is None else t.clone()      # noqa: E731
        return cl(xtx), cl(xty), tuple(cl(t) for t in stats)

    def _training_matrices_batched(self, rXTX: bool, rXTY: bool, folds):
        """Batched counterpart of cvmatrix.py:754-896.  Leading axis = fold."""
        if not rXTX and not rXTY:
            raise ValueError(MSG_NEITHER)
        if self.X is None:
            raise RuntimeError("call fit() first")
        if rXTY and self.Y is None:
            raise ValueError(MSG_NO_Y)
        batch = self.prepare_folds(folds)
        if (self.__dict__.get("_pending", False) and not self._exchanges_globals()
                and self._sweep_worth(_lib.load(), batch)):
            # a lazy fit is pending, the folds partition the rows and nothing is exchanged between
            # the two halves (one process): the sweep and the fold stage in one call
            return self._finish(batch, rXTX, rXTY, sweep_all=True)
        self._lazy_sweep(batch)
        return self._finish(batch, rXTX, rXTY)

    def _finish(self, batch, rXTX: bool, rXTY: bool, sweep_fold: Optional[int] = None, sweep_all: bool = False):
        """Validity checks + the fold-stage launch for ``batch`` (or for fold ``sweep_fold`` of the
        batch the sweep served)."""
        req = self._request(rXTX, rXTY)
        # the data-dependent raises come before anything is launched -- unless the counts they
        # need are still on their way from the other GPUs (multi-GPU, _totals_in_flight): then the
        # kernels are queued first (they never fault on such data) and the check, which has to
        # wait for the exchange anyway, follows; the results are only handed out after it
        need_stats, need_std = req.need_stats, req.need_std
        late = self._totals_in_flight()
        if late and self._passes_on_local_counts(batch, need_stats, need_std, only=sweep_fold):
            late = need_stats = False           # (decided on this process's own counts: nothing to wait for)
        elif late:
            self._request_totals()              # (queued behind the exchange; awaited after the launch below)
        if not late:
            self._validate(batch, need_stats, need_std, only=sweep_fold)
        xtx, xty, (muX, sdX, muY, sdY), _ = self._run(batch, rXTX, rXTY, sweep_fold=sweep_fold, sweep_all=sweep_all)
        if late:
            self._validate(batch, need_stats, need_std, only=sweep_fold)
        return req.pack(xtx, xty, muX, sdX, muY, sdY, self._conv)

    # ------------------------------------------------------------------ public API
    def training_XTX_batched(self, folds):
        """``training_XTX`` for many folds: (XTX[P,K,K], (muX[P,1,K]|None, sdX|None, None, None))."""
        return self._training_matrices_batched(True, False, folds)

    def training_XTY_batched(self, folds):
        return self._training_matrices_batched(False, True, folds)

    def training_XTX_XTY_batched(self, folds):
        """``training_XTX_XTY`` for many folds in one launch sequence:
        ((XTX[P,K,K], XTY[P,K,M]), (muX[P,1,K], sdX[P,1,K], muY[P,1,M], sdY[P,1,M]))
        with ``None`` for statistics the flags do not ask for."""
        return self._training_matrices_batched(True, True, folds)

    # ------------------------------------------------------------------ unions of folds (nested CV)
    def _training_matrices_unions(self, rXTX: bool, rXTY: bool, folds, unions):
        """The ``*_batched`` results for the complements of UNIONS of the folds: leading axis = union.  The
        matrices are formed from the partials of one sweep over ``folds`` (cvm_sweep_unions: the full-data
        matrices minus the sum of the folds' validation updates); no row of X is read again."""
        from .unions import prepare_unions

        if self._exchanges_globals():
            raise NotImplementedError("unions of folds are not available while the full-data matrices are exchanged "
                                      "between processes")
        if self.X is None:
            raise RuntimeError("call fit() first")
        if rXTY and self.Y is None:
            raise ValueError(MSG_NO_Y)
        lib = _lib.load()
        batch = self.prepare_folds(folds)
        ub = prepare_unions(unions, batch.n_folds)
        if self._sweep is None or self._sweep[0] is not batch:
            # no sweep of this very batch at hand: the one-sweep fit for these folds, as fit(folds=...) runs it
            # (it raises for folds that are not a partition, before anything of the current fit is touched)
            if not batch.is_partition:
                raise ValueError("fit(folds=...) needs folds that contain every row exactly once")
            self._sweep_cache = None
            self._ra = None
            self._np_cache = {}
            self._sum_w = None
            with self._on_device():
                neg = torch.empty(1, dtype=torch.int32, device=self.device)
                self._fit_sweep(lib, batch, neg)
                self._neg = neg
            self._pending = False
            self._after_globals()
        batch, token = self._sweep
        req = self._request(rXTX, rXTY)
        # the reference's data-dependent raises, on exact host counts, before anything is launched (_validate)
        self._resolve_totals()
        U = ub.n_unions
        if req.need_stats and U:
            per_fold = batch.nz_val if self.weights is not None else batch.sizes
            nz_val = np.add.reduceat(np.asarray(per_fold, dtype=np.int64)[ub.folds], ub.offsets[:-1])
            if self.weights is not None:
                nz_train = self._nz_total - nz_val
                if np.any(nz_train == 0):
                    raise ValueError(MSG_NZ_ZERO)
            else:
                nz_train = self._n_total - nz_val
            if req.need_std and np.any(nz_train <= self.ddof):
                raise ValueError(MSG_NZ_DDOF)
        K, M = self._Kd, self._Md or 0
        dev, dt = self.device, self._tdt
        with self._on_device():
            # fresh tensors (never the reuse_outputs arena: a nested loop keeps the pair matrices next to the folds')
            out_XTX = torch.empty((U, K, K), dtype=dt, device=dev) if rXTX else None
            out_XTY = torch.empty((U, K, M), dtype=dt, device=dev) if rXTY else None
            muX, sdX, muY, sdY = stat_views(torch.empty(U * (2 * K + 2 * M), dtype=dt, device=dev), U, K, M)
            want = int(lib.cvm_sweep_unions_workspace_bytes(U, K, M))
            ws = self.__dict__.get("_union_ws")
            if ws is None or ws.numel() < want or ws.device != dev:
                ws = self._union_ws = torch.empty(want, dtype=torch.uint8, device=dev)
            ufolds, uoffs = ub.device(dev)
            rc = _lib.CVM_OK if U == 0 else lib.cvm_sweep_unions(
                batch.offsets.data_ptr(), batch.n_folds, ufolds.data_ptr(), uoffs.data_ptr(),
                ub.offsets.ctypes.data, U, K, M, self._cdt, req.flags, float(self.ddof), float(self.resolution),
                1 if self.weights is not None else 0,
                self._G.data_ptr(), _lib.ptr(self._H), self._gs.data_ptr(),
                _lib.ptr(out_XTX), _lib.ptr(out_XTY), muX.data_ptr(), sdX.data_ptr(), _lib.ptr(muY), _lib.ptr(sdY),
                0, self._sweep_ws.data_ptr(), self._sweep_ws.numel(), token, ws.data_ptr(), ws.numel(),
                self._stream(),
            )
            _lib.check(rc, "cvm_sweep_unions")
        return req.pack(out_XTX, out_XTY, muX, sdX, muY, sdY, self._conv)

    def training_XTX_unions(self, folds, unions):
        """``training_XTX_batched`` for the complements of unions of folds (not in the reference):
        result u is ``training_XTX`` of the concatenated validation indices of the folds ``unions[u]``.

        ``folds``: a ``Partitioner``, index arrays or a ``FoldBatch`` that PARTITIONS the rows; ``unions``: a
        sequence of sequences of fold positions (in the batch's order; the order inside a union does not
        matter), an ``(n, r)`` integer array, or ``unions.prepare_unions(...)``'s result.  ``ValueError`` for an
        empty union, a repeated fold or a position out of range.  When the object's current sweep is not
        of this very batch, the one-sweep fit for these folds runs first, exactly as
        ``fit(X, Y, weights, folds=folds)`` runs it.  Results are fresh tensors."""
        return self._training_matrices_unions(True, False, folds, unions)

    def training_XTY_unions(self, folds, unions):
        return self._training_matrices_unions(False, True, folds, unions)

    def training_XTX_XTY_unions(self, folds, unions):
        """``training_XTX_XTY_batched`` for the complements of unions of folds (see ``training_XTX_unions``):
        ((XTX[U,K,K], XTY[U,K,M]), (muX[U,1,K], sdX[U,1,K], muY[U,1,M], sdY[U,1,M])) with ``None`` for
        statistics the flags do not ask for.  Nested cross-validation: ``unions.fold_pairs(P)``."""
        return self._training_matrices_unions(True, True, folds, unions)

    @staticmethod
    def _first(res):
        """Strip the fold axis of a one-fold batched result."""
        mats, stats = res
        if isinstance(mats, tuple):
            mats = tuple(m[0] for m in mats)
        else:
            mats = mats[0]
        return mats, tuple(None if s is None else s[0] for s in stats)

    def _sweep_fold_of(self, v, rXTX: bool = True, rXTY: bool = True) -> Optional[int]:
        """Is ``v`` -- handed to a one-fold call -- the very index array a ``Partitioner`` holds
        for one of the folds a sweep has served (or can serve: a lazy fit is pending and the
        Partitioner's folds partition the rows)?  Then its number in that sweep, else None.
        This is what makes the reference's loop (README.md:120-141)
        ``for fold in p.folds_dict: cvm.training_XTX_XTY(p.get_validation_indices(fold))``
        cost one pass over the data plus two small kernels per call."""
        if type(v) is not np.ndarray:
            return None
        if self.__dict__.get("_pending", False):
            p = partitioner_of(v)
            if p is not None and p is not self._auto_sweep_tried:
                self._auto_sweep_tried = p          # (one attempt per fit and Partitioner)
                # (an uploaded batch of an earlier pass is taken as it is: whatever a fold's array
                #  holds NOW is compared with the batch's private copy below, call by call; the
                #  full-data matrices are the same for any partition of the rows)
                batch = self.prepare_folds(p, _trust_cached=True)
                lib = _lib.load()
                K, M = self._Kd, self._Md or 0
                if (not self._exchanges_globals() and batch.n_folds <= 16 and self._sweep_worth(lib, batch)
                        and (rXTY is False or self.Y is not None)
                        and batch.n_folds * K * (K + M) * self.X.element_size() <= (1 << 30)):
                    # one process, few folds: the sweep and EVERY fold's matrices in one call
                    # (cvm_sweep_all); the loop's calls are then handed their fold's slices, each
                    # once (a second request for a fold recomputes it: the caller may have changed
                    # its matrices in place).  The data-dependent raises stay per call.
                    xtx, xty, st, _ = self._run(batch, rXTX, rXTY, sweep_all=True)
                    xtx, xty, st = self._own_results(xtx, xty, st)
                    c = self._cut_t                 # (padded device copies: cut once, for all folds)
                    st = (c(st[0], "X"), c(st[1], "X"), c(st[2], "Y"), c(st[3], "Y"))
                    self._sweep_cache = {"key": (rXTX, rXTY), "xtx": c(xtx, "XX"), "xty": c(xty, "XY"), "stats": st,
                                         "left": set(range(batch.n_folds))}
                else:
                    self._lazy_sweep(batch)         # sweeps if the folds partition the rows and are large
        ids = self._sweep_ids
        if ids is None or self._sweep is None:
            return None
        i = ids[0].get(id(v))
        if i is None or ids[1][i] is not v:
            return None
        batch = self._sweep[0]
        ho = batch.host_offsets
        if batch._host_idx is None or not _same_indices(v, batch._host_idx[ho[i]:ho[i + 1]]):
            return None         # the array no longer holds what the sweep gathered: the ordinary route
        return i

    def _training_matrices(self, return_XTX: bool, return_XTY: bool, val_indices):
        """cvmatrix.py:754-896 for one fold."""
        if not return_XTX and not return_XTY:
            raise ValueError(MSG_NEITHER)
        if self.X is not None and return_XTY and self.Y is None:
            raise ValueError(MSG_NO_Y)
        if self.X is not None:
            v = val_indices
            if not self.serve_loops:
                # no loop serving: the small-fold short cut (a plain launch, nothing remembered) or
                # the one-fold batched call
                if (type(v) is np.ndarray and v.ndim == 1 and 0 < v.size <= 32 and v.dtype == np.int64
                        and v.flags.c_contiguous):
                    return self._one_small_fold(v, return_XTX, return_XTY)
                return self._first(self._training_matrices_batched(return_XTX, return_XTY, [v]))
            ra = self._ra
            if ra is not None and ra.key == (return_XTX, return_XTY):
                # a per-fold loop over a Partitioner with many folds is being read ahead
                if ra.pos < ra.n and v is ra.arrs[ra.pos]:
                    res = self._ra_serve(ra, v)
                    if res is not None:
                        return res
                self._ra = ra = None
            small = (type(v) is np.ndarray and v.ndim == 1 and 0 < v.size <= 32 and v.dtype == np.int64
                     and v.flags.c_contiguous)
            if small:
                if ra is None and v.base is not None and self._ra_start(v, return_XTX, return_XTY):
                    res = self._ra_serve(self._ra, v)
                    if res is not None:
                        return res
                    self._ra = None
                return self._one_small_fold(v, return_XTX, return_XTY)
            i = self._sweep_fold_of(v, return_XTX, return_XTY)
            if i is not None:
                return self._finish_sweep_fold(i, return_XTX, return_XTY)
            if (ra is None and type(v) is np.ndarray and v.base is not None
                    and self._ra_start(v, return_XTX, return_XTY)):
                res = self._ra_serve(self._ra, v)
                if res is not None:
                    return res
                self._ra = None
        return self._first(
            self._training_matrices_batched(return_XTX, return_XTY, [val_indices]))

    # ---- read-ahead of the reference's per-fold loop over a Partitioner with MANY folds ----------
    # (leave-one-out: 100 000 calls of training_XTX_XTY with one row each, benchmarks/benchmark.py:
    #  153-158).  A call costs the host 25-80 us, the device 0.5 us: when the array handed to a call
    # is the very array a Partitioner holds for fold number pos, the folds pos .. pos + C - 1 are
    # computed by ONE batched launch sequence and the following calls -- recognised by the identity
    # of their arrays, in the Partitioner's order -- are handed their slices (each once).  The
    # data-dependent raises stay per call; an array changed in place since the chunk was computed
    # (size, ends, sum) ends the read-ahead.  Few large folds take the sweep instead (_sweep_fold_of).
    def _ra_start(self, v: np.ndarray, rXTX: bool, rXTY: bool) -> bool:
        p, pos = partitioner_pos(v)
        if p is None or len(p._fold_arrays) <= 16:
            return False
        if rXTY and self.Y is None:
            return False
        batch = self.prepare_folds(p, _trust_cached=True)   # (every fold is compared exactly when served)
        if batch._host_idx is None:
            return False
        if self._sweep_worth(_lib.load(), batch) and not self._exchanges_globals():
            return False                            # (the sweep serves this loop)
        if self._sweep is not None and self._sweep[0] is batch:
            return False
        K, M = self._Kd, self._Md or 0
        per_fold = K * ((K if rXTX else 0) + (M if rXTY else 0)) * self.X.element_size()
        ra = _ReadAhead()
        ra.p, ra.arrs, ra.n, ra.batch, ra.key = p, p._fold_arrays, len(p._fold_arrays), batch, (rXTX, rXTY)
        ra.pos = ra.start = pos
        ra.count = 0
        ra.chunk = 16
        ra.max_chunk = int(max(16, min(4096, (256 << 20) // max(per_fold, 1))))
        self._ra = ra
        return True

    def _ra_fill(self, ra: "_ReadAhead") -> None:
        """Folds ra.pos .. of the Partitioner in one batched call; per-fold witnesses and verdicts."""
        full = ra.batch
        a, b = ra.pos, min(ra.n, ra.pos + ra.chunk)
        ho = full.host_offsets
        sub = FoldBatch(full.idx, full.offsets[a:b + 1], ho[a:b + 1], full.nz_val[a:b], None, None, full._n_rows,
                        device=self.device, w_gen=full._w_gen)
        sub._sizes = full.sizes[a:b]
        rXTX, rXTY = ra.key
        xtx, xty, (muX, sdX, muY, sdY), _ = self._run(sub, rXTX, rXTY)
        xtx, xty, (muX, sdX, muY, sdY) = self._own_results(xtx, xty, (muX, sdX, muY, sdY))
        ra.req = req = self._request(rXTX, rXTY)    # (what the chunk's calls return: as asked for when it was computed)
        c = self._cut_t                             # (padded device copies: cut the chunk once)
        ra.xtx = c(xtx, "XX").unbind(0) if xtx is not None else None
        ra.xty = c(xty, "XY").unbind(0) if xty is not None else None
        ra.stats = tuple(c(t, kind).unbind(0) if w else None
                         for t, kind, w in zip((muX, sdX, muY, sdY), "XXYY", req.want))
        # the reference's raises (cvmatrix.py:612-630, 1074-1078), decided for the whole chunk
        ra.bad_zero = ra.bad_ddof = None
        self._resolve_weights_check()
        if req.need_stats:
            self._resolve_totals()
            if self.weights is not None:
                nz_train = self._nz_total - full.nz_val[a:b]
                ra.bad_zero = (nz_train == 0).tolist()
            else:
                nz_train = self._n_total - full.sizes[a:b]
            if req.need_std:
                ra.bad_ddof = (nz_train <= self.ddof).tolist()
        # what the chunk was computed from: this stretch of the batch's private copy of the indices
        # (_ra_serve compares the caller's array with its fold's piece, exactly)
        o = ho[a:b + 1]
        ra.lo = o.tolist()
        ra.sizes = np.diff(o).tolist()
        seg = full._host_idx[o[0]:o[-1]]
        ra.first = seg[(o[:-1] - o[0]).clip(max=max(seg.size - 1, 0))].tolist() if seg.size else [0] * (b - a)
        ra.hidx = full._host_idx
        ra.start, ra.count = a, b - a
        ra.chunk = min(ra.max_chunk, ra.chunk * 2)

    def _ra_serve(self, ra: "_ReadAhead", v: np.ndarray):
        j = ra.pos - ra.start
        if j >= ra.count or j < 0:
            self._ra_fill(ra)
            j = 0
        n = v.size
        if n != ra.sizes[j] or (n == 1 and int(v[0]) != ra.first[j]) or (
                n > 1 and not _same_indices(v, ra.hidx[ra.lo[j]:ra.lo[j + 1]])):
            return None                             # changed in place since the chunk was computed
        if ra.req.need_stats:
            if ra.bad_zero is not None and ra.bad_zero[j]:
                raise ValueError(MSG_NZ_ZERO)
            if ra.bad_ddof is not None and ra.bad_ddof[j]:
                raise ValueError(MSG_NZ_DDOF)
        ra.pos += 1
        return ra.req.pack(ra.xtx, ra.xty, *ra.stats, (self._out,) * 4, at=j)

    def _one_small_fold(self, v: np.ndarray, rXTX: bool, rXTY: bool):
        """One fold of at most 32 rows given as an int64 index array -- the call of the reference's
        leave-one-out loop (one ``training_XTX_XTY(validation_indices)`` per sample,
        benchmarks/benchmark.py:153-158): same checks, same library call (``cvm_fold_update`` with
        the indices inside the kernel arguments, CVM_IDX_HOST) and same results as the general route,
        without building a ``FoldBatch``, without a fold axis, with three allocations."""
        lib = _lib.load()
        self._ensure_fit()
        N, K, M = self.N, self._Kd, self._Md or 0
        n = v.size
        if n == 1:
            lo = hi = int(v[0])
        else:
            lo, hi = int(v.min()), int(v.max())
        if lo < -N or hi >= N:
            raise IndexError(f"validation index out of bounds for {N} samples")
        if lo < 0:
            v = np.where(v < 0, v + N, v)
        req = self._request(rXTX, rXTY)
        self._resolve_weights_check()
        if req.need_stats:                          # the reference's raises, in its order (_validate)
            self._resolve_totals()
            if self.weights is not None:
                wh = self._host_weights()
                nz_val = int(np.count_nonzero(wh[v])) if n > 1 else int(wh[v[0]] != 0)
                nz_train = self._nz_total - nz_val
                if nz_train == 0:
                    raise ValueError(MSG_NZ_ZERO)
            else:
                nz_train = self._n_total - n
            if req.need_std and nz_train <= self.ddof:
                raise ValueError(MSG_NZ_DDOF)
        dev, dt = self.device, self._tdt
        if torch.cuda.current_device() != dev.index:
            # (a model on another GPU than the caller's current one: the caller's device is restored)
            with torch.cuda.device(dev):
                return self._one_small_fold(v, rXTX, rXTY)
        xtx = torch.empty((K, K), dtype=dt, device=dev) if rXTX else None
        xty = torch.empty((K, M), dtype=dt, device=dev) if rXTY else None
        stat = torch.empty(2 * K + 2 * M, dtype=dt, device=dev)
        key = (K, M, self._cdt)
        if self._small_ws_key != key:
            self._small_ws_bytes = int(lib.cvm_fold_workspace_bytes(1, 32, 32, K, M, self._cdt, 0x3F))
            self._small_ws_key = key
            self._one_off = np.zeros(2, dtype=np.int64)
        ws = self._ws
        if ws is None or ws.numel() < self._small_ws_bytes or ws.device != dev:
            ws = self._workspace(self._small_ws_bytes)
        off = self._one_off
        off[1] = n
        rc = lib.cvm_fold_update(
            self.X.data_ptr(), _lib.ptr(self.Y), _lib.ptr(self.weights), v.ctypes.data, off.ctypes.data,
            off.ctypes.data, 1, N, K, M, self._cdt, req.flags | _lib.IDX_HOST, float(self.ddof), float(self.resolution),
            self._G.data_ptr(), _lib.ptr(self._H), self._gs.data_ptr(), _lib.ptr(xtx), _lib.ptr(xty),
            *stat_addresses(stat.data_ptr(), stat.element_size(), K, M),
            0, ws.data_ptr(), ws.numel(), self._stream(),
        )
        _lib.check(rc, "cvm_fold_update")
        if self.output == "numpy" or self._out_cast or K != self._Ku or M != (self._Mu or 0):
            return req.pack_one(xtx, xty, stat, K, M, self._conv)
        return req.pack_one(xtx, xty, stat, K, M)       # (device results of the caller's shape: handed out as they are)

    def _finish_sweep_fold(self, i: int, rXTX: bool, rXTY: bool):
        """One fold of the sweep, finished on its own (cvm_sweep_fold_range): the short path of
        the reference's per-fold loop -- validity verdicts cached per sweep, one allocation for
        the statistics, results without a fold axis."""
        lib = _lib.load()
        batch, token = self._sweep
        K, M = self._Kd, self._Md or 0
        req = self._request(rXTX, rXTY)
        self._validate(batch, req.need_stats, req.need_std, only=i)
        cache = self._sweep_cache
        if cache is not None and cache["key"] == (rXTX, rXTY) and i in cache["left"]:
            cache["left"].discard(i)
            if not cache["left"]:
                self._sweep_cache = None
            # (the cache holds tensors already cut to K, M)
            return req.pack(cache["xtx"], cache["xty"], *cache["stats"], (self._out,) * 4, at=i)
        dev, dt = self.device, self._tdt
        if torch.cuda.current_device() != dev.index:
            with torch.cuda.device(dev):
                return self._finish_sweep_fold(i, rXTX, rXTY)
        xtx = torch.empty((K, K), dtype=dt, device=dev) if rXTX else None
        xty = torch.empty((K, M), dtype=dt, device=dev) if rXTY else None
        stat = torch.empty(2 * K + 2 * M, dtype=dt, device=dev)
        rc = lib.cvm_sweep_fold_range(
            batch.offsets.data_ptr(), batch.n_folds, i, 1, K, M, self._cdt, req.flags, float(self.ddof),
            float(self.resolution), 1 if self.weights is not None else 0,
            self._G.data_ptr(), _lib.ptr(self._H), self._gs.data_ptr(),
            _lib.ptr(xtx), _lib.ptr(xty), *stat_addresses(stat.data_ptr(), stat.element_size(), K, M), 0,
            self._sweep_ws.data_ptr(), self._sweep_ws.numel(), token, self._stream(),
        )
        _lib.check(rc, "cvm_sweep_fold_range")
        return req.pack_one(xtx, xty, stat, K, M, self._conv)

    def training_XTX(self, validation_indices):
        """Training-set ``XᵀWX`` for every sample except ``validation_indices`` and
        (mean_X, std_X, None, None); cvmatrix.py:330-383."""
        return self._training_matrices(True, False, validation_indices)

    def training_XTY(self, validation_indices):
        """Training-set ``XᵀWY`` and the four statistics; cvmatrix.py:385-449."""
        return self._training_matrices(False, True, validation_indices)

    def training_XTX_XTY(self, validation_indices):
        """Training-set ``XᵀWX`` and ``XᵀWY`` and the four statistics; cvmatrix.py:451-517."""
        return self._training_matrices(True, True, validation_indices)

    def training_statistics_batched(self, folds):
        """Batched ``training_statistics`` (cvmatrix.py:519-574, flag map 570-573)."""
        if self.X is None:
            raise RuntimeError("call fit() first")
        batch = self.prepare_folds(folds)
        hasY = self.Y is not None
        cX, cY, sX, sY = self.center_X, self.center_Y, self.scale_X, self.scale_Y
        r_muX, r_sdX = (cX or sX), sX
        r_muY, r_sdY = ((cY or sY) and hasY), (sY and hasY)
        if not (r_muX or r_sdX or r_muY or r_sdY):
            self._resolve_weights_check()          # (nothing to compute; the reference's fit() would still have raised)
            return None, None, None, None
        self._ensure_fit()
        self._validate(batch, True, r_sdX or r_sdY)
        # the kernel derives "what to compute" from (return flags, centre/scale flags) by the rule of
        # _request.FoldRequest; pass a flag set whose derived wants cover this method's own map
        # (cvmatrix.py:570-573); surplus statistics are dropped
        _, _, (muX, sdX, muY, sdY), _ = self._run(
            batch, False, hasY, stat_flags=(r_muX, r_muY, r_sdX, r_sdY), stats_only=True)
        oX, oY = self._oX, self._oY
        return (oX(muX) if r_muX else None, oX(sdX) if r_sdX else None,
                oY(muY) if r_muY else None, oY(sdY) if r_sdY else None)

    def training_statistics(self, validation_indices):
        """(mean_X, std_X, mean_Y, std_Y) of the training set; cvmatrix.py:519-574."""
        st = self.training_statistics_batched([validation_indices])
        return tuple(None if s is None else s[0] for s in st)
