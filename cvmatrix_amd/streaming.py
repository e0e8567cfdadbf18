"""Streaming cross-validation: the folds' training matrices of data that arrives in row chunks.

``StreamingCVMatrix.partial_fit(X_chunk, Y_chunk, w_chunk, labels_chunk)`` runs the Gram kernel over the chunk
and adds every fold's raw update ``X_f' W X_f | X_f' W Y_f``, its column sums and weight totals to a float64
accumulator on the device (``cvm_stream_add``); no chunk is kept.  The ``training_*_batched`` /
``training_*_unions`` methods then return what ``CVMatrix`` returns for the folds ``labels == f`` of the
concatenated data -- centred and scaled as the flags ask, ready for ``ridge_fit_batched``, ``pls_fit_batched``,
``pcr_fit_batched``, ``enet_fit_batched`` and ``omp_fit_batched`` -- from the accumulated state alone
(``cvm_stream_close`` + the one-sweep path's finalize kernels).  Results are snapshots: more chunks may follow.

The arithmetic, the padding of the device copies and the form of the results are ``CVMatrix``'s: the class
composes one (never fitted) for its flags, dtype rule, upload and result conversion."""

from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._request import fold_request, stat_views
from ._stage import launch
from .cvmatrix import MSG_NEG_W, MSG_NEITHER, MSG_NO_Y, MSG_NZ_DDOF, MSG_NZ_ZERO, CVMatrix

__all__ = ["StreamingCVMatrix", "ChunkRules"]

_TILE, _YT = 128, 32        # csrc/geometry.hpp


def _up256(v: int) -> int:
    return -(-v // 256) * 256


def _unit_layout(K: int, M: int):
    """(bytes of one float64 unit, index of its statistics block in float64 words, Kp, Mp): make_geom(K, M, 8, 0)."""
    P = -(-K // _TILE)
    Kp = P * _TILE
    Mp = (-(-M // _YT) if M > 0 else 1) * _YT
    tiles, h, stats = _up256(P * (P + 1) // 2 * _TILE * _TILE * 8), _up256(P * _TILE * Mp * 8), _up256((2 * Kp + 2 * Mp + 4) * 8)
    return tiles + h + stats, (tiles + h) // 8, Kp, Mp


class ChunkRules:
    """What every chunk of a stream must look like, decided on the host before anything is uploaded: labels in
    ``[0, n_folds)``, one row count per chunk, and K, M, the presence of Y and of weights as the first chunk with
    rows had them (``fix``)."""

    def __init__(self, n_folds: int) -> None:
        self.n_folds = int(n_folds)
        self.K = self.M = self.has_Y = self.weighted = None

    @staticmethod
    def _shape(a):
        return tuple(a.shape) if hasattr(a, "shape") else np.asarray(a).shape

    @classmethod
    def _cols(cls, a) -> int:
        shp = cls._shape(a)
        if len(shp) not in (1, 2):
            raise ValueError("expected a 1-D or 2-D array")
        return 1 if len(shp) == 1 else int(shp[1])

    def labels(self, labels) -> np.ndarray:
        if labels is None:
            raise ValueError("labels are needed: the fold (0 .. n_folds - 1) of every row of the chunk")
        if isinstance(labels, torch.Tensor):
            labels = labels.detach().cpu().numpy()
        lab = np.asarray(labels).reshape(-1)
        if lab.size and lab.dtype.kind not in "iu":
            raise ValueError("labels must be integers")
        lab = lab.astype(np.int64, copy=False)
        if lab.size and (int(lab.min()) < 0 or int(lab.max()) >= self.n_folds):
            raise ValueError(f"label out of range for {self.n_folds} folds")
        return lab

    def check(self, X, Y, weights, labels):
        """``(labels as int64, K, M | None)`` of a chunk that may join the stream; ``ValueError`` otherwise."""
        lab = self.labels(labels)
        n = lab.size
        K = self._cols(X)
        M = self._cols(Y) if Y is not None else None
        if self._shape(X)[0] != n or (Y is not None and self._shape(Y)[0] != n):
            raise ValueError("X, Y and labels must have the same number of rows")
        if weights is not None and self._shape(weights) not in ((n,), (n, 1)):
            raise ValueError("weights must have shape (n,) or (n, 1)")
        if self.has_Y is not None:
            if K != self.K:
                raise ValueError(f"this chunk has K = {K}, the stream K = {self.K}")
            if (Y is not None) != self.has_Y:
                raise ValueError("Y must be given for every chunk of a stream, or for none")
            if Y is not None and M != self.M:
                raise ValueError(f"this chunk has M = {M}, the stream M = {self.M}")
            if (weights is not None) != self.weighted:
                raise ValueError("weights must be given for every chunk of a stream, or for none")
        return lab, K, M

    def fix(self, K: int, M, has_Y: bool, weighted: bool) -> None:
        self.K, self.M, self.has_Y, self.weighted = K, M, bool(has_Y), bool(weighted)


class _Snapshot:
    """What one ``cvm_stream_close`` left: the full-data matrices and the workspace the finalize calls read."""
    __slots__ = ("G", "H", "gs", "units_ptr", "units_bytes", "token", "offsets", "nz", "keep")


class StreamingCVMatrix:
    """Training-set ``X'WX`` / ``X'WY`` of every fold, accumulated over row chunks on an MI355X.

    ``n_folds``: labels are the fold positions ``0 .. n_folds - 1``.  The flags, ``ddof``, ``dtype`` and
    ``device`` are ``CVMatrix``'s (float16 problems are computed in float32 and returned as float16, wider types
    in float64 and returned as NumPy arrays).  ``K``, ``M``, the presence of ``Y`` and of weights are fixed by the
    first chunk with rows."""

    def __init__(self, n_folds: int, center_X: bool = False, center_Y: bool = False, scale_X: bool = False,
                 scale_Y: bool = False, ddof: int = 1, dtype=np.float64, device=None) -> None:
        if int(n_folds) != n_folds or int(n_folds) < 1:
            raise ValueError("n_folds must be a positive integer")
        self.n_folds = int(n_folds)
        self._cv = CVMatrix(center_X, center_Y, scale_X, scale_Y, ddof=ddof, dtype=dtype, copy=True, device=device)
        self._acc = None
        self.reset()

    # ------------------------------------------------------------------ the flags are CVMatrix's (public, per call)
    center_X = property(lambda s: s._cv.center_X, lambda s, v: setattr(s._cv, "center_X", v))
    center_Y = property(lambda s: s._cv.center_Y, lambda s, v: setattr(s._cv, "center_Y", v))
    scale_X = property(lambda s: s._cv.scale_X, lambda s, v: setattr(s._cv, "scale_X", v))
    scale_Y = property(lambda s: s._cv.scale_Y, lambda s, v: setattr(s._cv, "scale_Y", v))
    ddof = property(lambda s: s._cv.ddof, lambda s, v: setattr(s._cv, "ddof", v))
    dtype = property(lambda s: s._cv.dtype)
    device = property(lambda s: s._cv.device)
    K = property(lambda s: s._cv._Ku)
    M = property(lambda s: s._cv._Mu)

    def reset(self) -> None:
        """Forget every chunk (and a failed weights check); the next chunk fixes the shapes anew."""
        cv = self._cv
        cv._Ku = cv._Kd = cv._Mu = cv._Md = None
        self.N = 0
        self.n_chunks = 0
        self._sizes = np.zeros(self.n_folds, dtype=np.int64)
        self._hasY = self._weighted = None
        self._rules = ChunkRules(self.n_folds)
        self._state = np.zeros(_lib.STREAM_STATE_LEN, dtype=np.int64)
        self._acc = None
        self._wflag = None              # device int64[1]: negative weights seen in device chunks
        self._w_pending = self._w_bad = False
        self._version = 0
        self._snap: Optional[_Snapshot] = None
        self._snap_version = -1

    @property
    def fold_sizes(self) -> np.ndarray:
        """Rows accumulated per fold."""
        return self._sizes.copy()

    @property
    def accumulator_bytes(self) -> int:
        return 0 if self._acc is None else int(self._acc.numel())

    # ------------------------------------------------------------------ chunks
    def partial_fit(self, X, Y=None, weights=None, labels=None) -> None:
        """Add one chunk: ``X`` (n, K), ``Y`` (n, M) or None, ``weights`` (n,) or None, ``labels`` (n,) in
        ``[0, n_folds)`` -- host arrays or device tensors.  Every ``ValueError`` (a shape other than the first
        chunk's, Y or weights in some chunks only, a label out of range, a negative weight in a host array) is
        raised before anything is launched and leaves the accumulated state as it was.  A negative weight in a
        device tensor is found on the device and raised by the next call that hands out a result."""
        cv = self._cv
        lab, Ku, Mu = self._rules.check(X, Y, weights, labels)
        n = lab.size
        w_on_dev = isinstance(weights, torch.Tensor) and weights.device.type != "cpu"
        if weights is not None and not w_on_dev:
            h = (weights.detach().numpy() if isinstance(weights, torch.Tensor) else np.asarray(weights)).reshape(-1)
            if cv._out_cast == "half":
                h = h.astype(np.float16)
            if bool(np.any(h < 0)):
                raise ValueError(MSG_NEG_W)
        if n == 0:
            return                                       # an empty chunk: nothing to add, nothing fixed
        lib = _lib.load()
        P = self.n_folds
        first = self._hasY is None
        if first:
            cv.device = cv._pick_device()
            Kd, Md = cv._device_dims(Ku, Mu or 0)
        else:
            Kd, Md = cv._Kd, cv._Md or 0
        dev = cv.device
        with cv._on_device():
            # (the chunk is read by this call's launches alone: a device tensor that needs no cast and no padding
            #  is read in place -- later writes of the caller on the same stream are ordered behind them)
            cv.copy = False
            try:
                Xd = cv._init_mat(X, Kd)
                Yd = cv._init_mat(Y, Md) if Y is not None else None
                wd = cv._init_mat(weights) if weights is not None else None
            finally:
                cv.copy = True
            if first:
                nbytes = int(lib.cvm_stream_workspace_bytes(_lib.STREAM_ACCUMULATOR, P, 0, Kd, Md, cv._cdt))
                acc = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                _lib.check(lib.cvm_stream_reset(acc.data_ptr(), nbytes, P, Kd, Md, cv._cdt, self._state.ctypes.data,
                                                cv._stream()), "cvm_stream_reset")
                self._acc = acc
                self._wflag = torch.zeros(1, dtype=torch.int64, device=dev)
                cv._Ku, cv._Kd, cv._Mu, cv._Md = Ku, Kd, Mu, (Md if Y is not None else None)
                self._hasY, self._weighted = Y is not None, weights is not None
                self._rules.fix(Ku, Mu, self._hasY, self._weighted)
            # the chunk's rows grouped by fold (chunk-local row numbers, fold position = label, rows ascending inside
            # a fold) on the host, one upload of [idx | offsets].  (Measured against the device-side Partitioner on
            # uploaded labels, tools/bench_streaming.py: the same cost per row -- the upload -- and two launches
            # more per chunk.)  A stable sort of 16-bit keys is a radix sort.
            counts = np.bincount(lab, minlength=P).astype(np.int64)
            host_offsets = np.zeros(P + 1, dtype=np.int64)
            np.cumsum(counts, out=host_offsets[1:])
            key = lab.astype(np.uint16) if P <= 65536 else lab
            grouped = torch.from_numpy(np.concatenate([np.argsort(key, kind="stable").astype(np.int64), host_offsets])).to(dev)
            idx, offsets = grouped[:n], grouped[n:]
            if w_on_dev:
                out2 = torch.empty(2, dtype=torch.int64, device=dev)
                _lib.check(lib.cvm_weights_check(wd.data_ptr(), n, cv._cdt, out2.data_ptr(), cv._stream()),
                           "cvm_weights_check")
                self._wflag += out2[:1]
                self._w_pending = True
            want = lib.cvm_stream_workspace_bytes(_lib.STREAM_SCRATCH, P, int(counts.max()), Kd, Md, cv._cdt)
            info = np.zeros(2, dtype=np.int64)
            launch("cvm_stream_add", dev, lambda ws, nb, st: lib.cvm_stream_add(
                Xd.data_ptr(), _lib.ptr(Yd), _lib.ptr(wd), idx.data_ptr(), offsets.data_ptr(), host_offsets.ctypes.data,
                P, n, Kd, Md, cv._cdt, self._acc.data_ptr(), self._acc.numel(), self._state.ctypes.data, ws, nb, st,
                info.ctypes.data), want)
        self._last_add = (int(info[0]) & 0xfffff, (int(info[0]) >> 20) & 0xfffff, int(info[1]))   # (s_off, s_diag, bytes moved)
        self._sizes += counts
        self.N += n
        self.n_chunks += 1
        self._version += 1

    # ------------------------------------------------------------------ hand-out
    def _check_weights(self) -> None:
        if self._w_pending:
            self._w_pending = False
            if int(self._wflag.item()):
                self._w_bad = True
        if self._w_bad:
            raise ValueError(MSG_NEG_W)

    def _close(self) -> _Snapshot:
        """The accumulated state made readable (cvm_stream_close), once per set of chunks."""
        if self.N == 0:
            raise RuntimeError("no rows accumulated: call partial_fit() first")
        self._check_weights()
        if self._snap is not None and self._snap_version == self._version:
            return self._snap
        lib = _lib.load()
        cv = self._cv
        K, M, P, dev, dt = cv._Kd, cv._Md or 0, self.n_folds, cv.device, cv._tdt
        s = _Snapshot()
        with cv._on_device():
            # fresh full-data matrices per snapshot: what an earlier snapshot handed out stays as it was
            s.G = torch.empty((K, K), dtype=dt, device=dev)
            s.H = torch.empty((K, M), dtype=dt, device=dev) if self._hasY else None
            s.gs = torch.empty(int(lib.cvm_gstats_len(K, M)), dtype=torch.float64, device=dev)
            s.keep = self._acc
            ws_ptr = ws_bytes = 0
            if dt != torch.float64:
                ws_bytes = int(lib.cvm_stream_workspace_bytes(_lib.STREAM_CLOSE, P, 0, K, M, cv._cdt))
                s.keep = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
                ws_ptr = s.keep.data_ptr()
            units, nbytes, token = C.c_void_p(0), C.c_size_t(0), C.c_int64(0)
            launch("cvm_stream_close", dev, lambda _ws, _nb, st: lib.cvm_stream_close(
                self._acc.data_ptr(), self._acc.numel(), self._state.ctypes.data, P, K, M, cv._cdt, s.G.data_ptr(),
                _lib.ptr(s.H), s.gs.data_ptr(), 0, ws_ptr, ws_bytes, st, C.byref(units), C.byref(nbytes), C.byref(token)))
            s.units_ptr, s.units_bytes, s.token = int(units.value), int(nbytes.value), int(token.value)
            host_offsets = np.zeros(P + 1, dtype=np.int64)
            np.cumsum(self._sizes, out=host_offsets[1:])
            s.offsets = torch.from_numpy(host_offsets).to(dev)
            s.nz = None
        self._snap, self._snap_version = s, self._version
        return s

    def _nz_per_fold(self, s: _Snapshot) -> np.ndarray:
        """Non-zero weights accumulated per fold (unweighted: rows): one small read-back per snapshot."""
        if not self._weighted:
            return self._sizes
        if s.nz is None:
            cv = self._cv
            unit_bytes, stat0, Kp, Mp = _unit_layout(cv._Kd, cv._Md or 0)
            words = self._acc[:self.n_folds * unit_bytes].view(torch.float64).view(self.n_folds, unit_bytes // 8)
            s.nz = np.rint(words[:, stat0 + 2 * Kp + 2 * Mp + 1].cpu().numpy()).astype(np.int64)
        return s.nz

    def _validate(self, s: _Snapshot, need_stats: bool, need_std: bool, groups=None) -> None:
        """The reference's data-dependent raises (cvmatrix.py:612-630, 1074-1078) on the accumulated counts,
        decided per fold (or per union: ``groups`` = (folds, offsets) in CSR form) in order."""
        if not need_stats:
            return
        per_fold = np.asarray(self._nz_per_fold(s), dtype=np.int64)
        total = int(per_fold.sum())
        if groups is None:
            nz_val = per_fold
        else:
            nz_val = np.add.reduceat(per_fold[groups[0]], groups[1][:-1]) if len(groups[1]) > 1 else per_fold[:0]
        for v in nz_val:
            nz_train = total - int(v)
            if self._weighted and nz_train == 0:
                raise ValueError(MSG_NZ_ZERO)
            if need_std and nz_train <= self.ddof:
                raise ValueError(MSG_NZ_DDOF)

    def _outputs(self, n: int, rXTX: bool, rXTY: bool):
        cv = self._cv
        K, M, dev, dt = cv._Kd, cv._Md or 0, cv.device, cv._tdt
        xtx = torch.empty((n, K, K), dtype=dt, device=dev) if rXTX else None
        xty = torch.empty((n, K, M), dtype=dt, device=dev) if rXTY else None
        return xtx, xty, stat_views(torch.empty(n * (2 * K + 2 * M), dtype=dt, device=dev), n, K, M)

    def _fold_range(self, s: _Snapshot, flags: int, xtx, xty, stats) -> None:
        lib = _lib.load()
        cv = self._cv
        muX, sdX, muY, sdY = stats
        launch("cvm_sweep_fold_range", cv.device, lambda _ws, _nb, st: lib.cvm_sweep_fold_range(
            s.offsets.data_ptr(), self.n_folds, 0, self.n_folds, cv._Kd, cv._Md or 0, cv._cdt, flags, float(cv.ddof),
            float(cv.resolution), 1 if self._weighted else 0, s.G.data_ptr(), _lib.ptr(s.H), s.gs.data_ptr(),
            _lib.ptr(xtx), _lib.ptr(xty), muX.data_ptr(), sdX.data_ptr(), _lib.ptr(muY), _lib.ptr(sdY), 0,
            s.units_ptr, s.units_bytes, s.token, st))

    def _batched(self, rXTX: bool, rXTY: bool):
        if not rXTX and not rXTY:
            raise ValueError(MSG_NEITHER)
        s = self._close()
        if rXTY and not self._hasY:
            raise ValueError(MSG_NO_Y)
        cv = self._cv
        req = cv._request(rXTX, rXTY)
        self._validate(s, req.need_stats, req.need_std)
        with cv._on_device():
            xtx, xty, stats = self._outputs(self.n_folds, rXTX, rXTY)
            self._fold_range(s, req.flags, xtx, xty, stats)
        return req.pack(xtx, xty, *stats, cv._conv)

    def training_XTX_batched(self):
        """``CVMatrix.training_XTX_batched`` over the folds ``labels == 0 .. n_folds - 1`` of all chunks so far."""
        return self._batched(True, False)

    def training_XTY_batched(self):
        return self._batched(False, True)

    def training_XTX_XTY_batched(self):
        """((XTX[P,K,K], XTY[P,K,M]), (muX[P,1,K], sdX[P,1,K], muY[P,1,M], sdY[P,1,M])) with ``None`` for the
        statistics the flags do not ask for: a snapshot of the chunks added so far."""
        return self._batched(True, True)

    def training_statistics_batched(self):
        """``CVMatrix.training_statistics_batched`` (cvmatrix.py:519-574, flag map 570-573)."""
        s = self._close()
        cv = self._cv
        hasY = self._hasY
        cX, cY, sX, sY = cv.center_X, cv.center_Y, cv.scale_X, cv.scale_Y
        r_muX, r_sdX = (cX or sX), sX
        r_muY, r_sdY = ((cY or sY) and hasY), (sY and hasY)
        if not (r_muX or r_sdX or r_muY or r_sdY):
            return None, None, None, None
        self._validate(s, True, bool(r_sdX or r_sdY))
        # (a flag set whose derived wants cover this method's own map; surplus statistics are dropped)
        flags = fold_request(False, hasY, r_muX, r_muY, r_sdX, r_sdY).flags
        with cv._on_device():
            _, _, (muX, sdX, muY, sdY) = self._outputs(self.n_folds, False, False)
            self._fold_range(s, flags, None, None, (muX, sdX, muY, sdY))
        oX, oY = cv._oX, cv._oY
        return (oX(muX) if r_muX else None, oX(sdX) if r_sdX else None,
                oY(muY) if r_muY else None, oY(sdY) if r_sdY else None)

    # ------------------------------------------------------------------ unions of folds (nested CV, no second pass)
    def _unions(self, rXTX: bool, rXTY: bool, unions):
        from .unions import prepare_unions

        if not rXTX and not rXTY:
            raise ValueError(MSG_NEITHER)
        s = self._close()
        if rXTY and not self._hasY:
            raise ValueError(MSG_NO_Y)
        lib = _lib.load()
        cv = self._cv
        ub = prepare_unions(unions, self.n_folds)
        U = ub.n_unions
        req = cv._request(rXTX, rXTY)
        if U:
            self._validate(s, req.need_stats, req.need_std, (ub.folds, ub.offsets))
        K, M, dev = cv._Kd, cv._Md or 0, cv.device
        with cv._on_device():
            xtx, xty, (muX, sdX, muY, sdY) = self._outputs(U, rXTX, rXTY)
            if U:
                ufolds, uoffs = ub.device(dev)
                launch("cvm_sweep_unions", dev, lambda ws, nb, st: lib.cvm_sweep_unions(
                    s.offsets.data_ptr(), self.n_folds, ufolds.data_ptr(), uoffs.data_ptr(), ub.offsets.ctypes.data, U,
                    K, M, cv._cdt, req.flags, float(cv.ddof), float(cv.resolution), 1 if self._weighted else 0,
                    s.G.data_ptr(), _lib.ptr(s.H), s.gs.data_ptr(), _lib.ptr(xtx), _lib.ptr(xty), muX.data_ptr(),
                    sdX.data_ptr(), _lib.ptr(muY), _lib.ptr(sdY), 0, s.units_ptr, s.units_bytes, s.token, ws, nb, st),
                    int(lib.cvm_sweep_unions_workspace_bytes(U, K, M)))
        return req.pack(xtx, xty, muX, sdX, muY, sdY, cv._conv)

    def training_XTX_unions(self, unions):
        """``CVMatrix.training_XTX_unions`` for unions of the stream's folds (``unions.fold_pairs(n_folds)``:
        nested cross-validation), from the accumulated state: no chunk is read again."""
        return self._unions(True, False, unions)

    def training_XTY_unions(self, unions):
        return self._unions(False, True, unions)

    def training_XTX_XTY_unions(self, unions):
        return self._unions(True, True, unions)

    # ------------------------------------------------------------------ full-data attributes (CVMatrix's conditions)
    @property
    def XTX(self):
        return self._cv._oXX(self._close().G)

    @property
    def XTY(self):
        s = self._close()
        return self._cv._oXY(s.H)

    def _gslice(self, lo: int, hi: int, cond: bool):
        if not cond or self.N == 0:
            return None
        cv = self._cv
        return cv._out(self._close().gs[lo:hi].to(cv._tdt).reshape(1, -1))

    @property
    def _anyflag(self) -> bool:
        return self._cv._anyflag

    @property
    def sum_X(self):
        cv = self._cv
        return self._gslice(0, cv._Ku or 0, cv.center_X or cv.center_Y or cv.scale_X)

    @property
    def sum_sq_X(self):
        cv = self._cv
        return self._gslice(cv._Kd or 0, (cv._Kd or 0) + (cv._Ku or 0), cv.scale_X)

    @property
    def sum_Y(self):
        cv = self._cv
        M = cv._Mu or 0
        return self._gslice(2 * (cv._Kd or 0), 2 * (cv._Kd or 0) + M,
                            (cv.center_X or cv.center_Y or cv.scale_Y) and bool(self._hasY))

    @property
    def sum_sq_Y(self):
        cv = self._cv
        M, Md = cv._Mu or 0, cv._Md or 0
        return self._gslice(2 * (cv._Kd or 0) + Md, 2 * (cv._Kd or 0) + Md + M, cv.scale_Y and bool(self._hasY))

    @property
    def sum_w(self):
        """Sum of the weights of all chunks (unweighted: the row count); ``None`` without centre / scale flags."""
        if not self._anyflag or self.N == 0:
            return None
        s = self._close()
        if not self._weighted:
            return self.N
        cv = self._cv
        return cv.dtype(s.gs[2 * cv._Kd + 2 * (cv._Md or 0)].item())

    @property
    def num_nonzero_w(self):
        if not self._anyflag or self.N == 0:
            return None
        s = self._close()
        return int(self._nz_per_fold(s).sum()) if self._weighted else self.N
