"""What one fold-stage call asks for, stated once: the C ABI flag word, which of the four statistics the call
returns (the reference's rule), and the shape of the return value.  Pure host code: no torch, no library."""

from __future__ import annotations

from functools import lru_cache

from . import _lib

IDENTITY = (lambda t: t,) * 4


class FoldRequest:
    """``flags``: the ``CVM_*`` bits of (rXTX, rXTY, cX, cY, sX, sY), without ``IDX_HOST``.  ``want``: which of
    (mean of X, std of X, mean of Y, std of Y) the call returns.  ``need_stats`` / ``need_std``: any of them /
    a standard deviation (what the reference's data-dependent raises depend on)."""
    __slots__ = ("rXTX", "rXTY", "flags", "want", "need_stats", "need_std")

    def __init__(self, rXTX, rXTY, cX, cY, sX, sY):
        self.rXTX, self.rXTY = bool(rXTX), bool(rXTY)
        self.flags = ((_lib.RET_XTX if rXTX else 0) | (_lib.RET_XTY if rXTY else 0)
                      | (_lib.CENTER_X if cX else 0) | (_lib.CENTER_Y if cY else 0)
                      | (_lib.SCALE_X if sX else 0) | (_lib.SCALE_Y if sY else 0))
        r_muX = cX or (rXTY and cY)                 # cvmatrix.py:828-831
        r_muY = rXTY and (cX or cY)
        r_sdX = sX
        r_sdY = rXTY and sY
        self.want = (bool(r_muX), bool(r_sdX), bool(r_muY), bool(r_sdY))
        self.need_stats, self.need_std = any(self.want), bool(r_sdX or r_sdY)

    def pack(self, xtx, xty, muX, sdX, muY, sdY, conv=IDENTITY, at=None):
        """The return value of the call: ``((XTX, XTY) | XTX | XTY, (muX, sdX, muY, sdY))`` with ``None`` for the
        statistics that are not wanted.  Everything kept goes through ``conv = (oXX, oXY, oX, oY)``; nothing
        else is touched.  ``at``: the arguments are stacked over folds -- keep element ``at`` of each."""
        oXX, oXY, oX, oY = conv
        w0, w1, w2, w3 = self.want
        if at is not None:
            xtx, xty = xtx[at] if self.rXTX else None, xty[at] if self.rXTY else None
            muX, sdX = muX[at] if w0 else None, sdX[at] if w1 else None
            muY, sdY = muY[at] if w2 else None, sdY[at] if w3 else None
        stats = (oX(muX) if w0 else None, oX(sdX) if w1 else None,
                 oY(muY) if w2 else None, oY(sdY) if w3 else None)
        if self.rXTX and self.rXTY:
            return (oXX(xtx), oXY(xty)), stats
        return (oXX(xtx) if self.rXTX else oXY(xty)), stats

    def pack_one(self, xtx, xty, stat, K, M, conv=IDENTITY):
        """``pack`` for one fold whose statistics are the flat block ``[muX | sdX | muY | sdY]``: a (1, K) or
        (1, M) view of every wanted one, none of the others."""
        w0, w1, w2, w3 = self.want
        return self.pack(xtx, xty, stat[:K].view(1, K) if w0 else None, stat[K:2 * K].view(1, K) if w1 else None,
                         stat[2 * K:2 * K + M].view(1, M) if w2 else None,
                         stat[2 * K + M:].view(1, M) if w3 else None, conv)


_cached = lru_cache(maxsize=64)(FoldRequest)


def fold_request(rXTX, rXTY, cX, cY, sX, sY) -> FoldRequest:
    """The (shared, immutable) record of these six flags: one cached lookup per call."""
    try:
        return _cached(rXTX, rXTY, cX, cY, sX, sY)
    except TypeError:                               # (a flag that cannot be hashed: only its truth counts)
        return _cached(*(bool(f) for f in (rXTX, rXTY, cX, cY, sX, sY)))


def stat_views(stat, P: int, K: int, M: int):
    """The four ``[P, 1, *]`` blocks of one allocation ``[muX | sdX | muY | sdY]`` of ``P (2 K + 2 M)`` elements
    (``None`` for the Y side without Y)."""
    muX, sdX = stat[:P * K].view(P, 1, K), stat[P * K:2 * P * K].view(P, 1, K)
    muY = stat[2 * P * K:2 * P * K + P * M].view(P, 1, M) if M else None
    sdY = stat[2 * P * K + P * M:].view(P, 1, M) if M else None
    return muX, sdX, muY, sdY


def stat_addresses(base: int, es: int, K: int, M: int):
    """The same four blocks of ONE fold as addresses (0 for the Y side without Y): what the per-fold calls hand
    the library, so that no view exists before the launch."""
    return base, base + K * es, (base + 2 * K * es) if M else 0, (base + (2 * K + M) * es) if M else 0
