#!/usr/bin/env python
"""One fixed list of small problems through every fold-stage host entry of the library (raw C ABI: cvm_gram_fit,
cvm_fold_update_ex, cvm_sweep_fit / _folds / _fold_range / _all / _unions, cvm_stream_reset / _add / _close); one line per
output array with a digest of its bytes.  For comparing two builds of the library bit by bit:

    python tools/fold_bits.py > branch.txt;  CVM_LIB_PATH=tools/libcvmhip_parent.so python tools/fold_bits.py > parent.txt
    python tools/fold_bits.py --matrix OUTDIR [--parent LIB]    # default + CVM_FORCE_SPLITS=3,5 + every route switch,
                                                                # one child process each; with --parent: the comparison

The route switches are read once per process, hence the children."""

import argparse
import ctypes as C
import hashlib
import os
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SWITCHES = ["", "CVM_FORCE_SPLITS=3,5", "CVM_NO_FUSED=1", "CVM_FORCE_FALLBACK=1", "CVM_NO_SWEEP_MERGE=1", "CVM_NO_DIRECT=1",
            "CVM_NO_COMPACT=1", "CVM_NO_INLINE_STATS=1", "CVM_SMALL_MAXN=128", "CVM_MID_TILE=0", "CVM_MID_MINN=1",
            "CVM_MID_MAXN=1000", "CVM_FUSED_PREPASS=1", "CVM_FUSED_ORDER=1"]
RET_XTX, RET_XTY, CENTER_SCALE, IDX_HOST = 0x01, 0x02, 0x3c, 0x40


def run_cases():
    import numpy as np
    import torch

    from cvmatrix_amd import _lib

    lib = _lib.load()
    dev = torch.device("cuda")
    lines = []

    def emit(case, **arrays):
        for name, t in sorted(arrays.items()):
            if t is None:
                continue
            raw = t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes() if torch.is_tensor(t) else np.ascontiguousarray(t).tobytes()
            lines.append("%-44s %-9s %9d %s" % (case, name, len(raw), hashlib.sha256(raw).hexdigest()[:16]))

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError("%s: code %d: %s" % (what, rc, lib.cvm_last_error().decode()))

    def zeros(n, dt):
        return torch.zeros(max(int(n), 1), dtype=dt, device=dev)

    def wsbuf(nbytes):
        return torch.zeros(int(nbytes) + 256, dtype=torch.uint8, device=dev)

    class Problem:
        def __init__(self, N, K, M, dt, weighted, seed):
            g = np.random.default_rng(seed)
            npdt = np.float64 if dt is torch.float64 else np.float32
            self.N, self.K, self.M, self.dt, self.cdt = N, K, M, dt, (_lib.CVM_F64 if dt is torch.float64 else _lib.CVM_F32)
            self.X = torch.from_numpy((g.standard_normal((N, K)) + 0.5).astype(npdt)).to(dev)
            self.Y = torch.from_numpy(g.standard_normal((N, M)).astype(npdt)).to(dev) if M else None
            self.w = torch.from_numpy(g.uniform(0.5, 2.0, N).astype(npdt)).to(dev) if weighted else None
            self.G, self.H = zeros(K * K, dt), (zeros(K * M, dt) if M else None)
            self.gs, self.neg = zeros(lib.cvm_gstats_len(K, M), torch.float64), zeros(1, torch.int32)

        def outs(self, P, flags):
            K, M = self.K, self.M
            o = dict(xtx=zeros(P * K * K, self.dt) if flags & RET_XTX else None,
                     xty=zeros(P * K * M, self.dt) if flags & RET_XTY else None,
                     muX=zeros(P * K, self.dt), sdX=zeros(P * K, self.dt),
                     muY=zeros(P * M, self.dt) if M else None, sdY=zeros(P * M, self.dt) if M else None,
                     fold=zeros(P * 4, torch.float64))
            return o, [_lib.ptr(o[k]) for k in ("xtx", "xty", "muX", "sdX", "muY", "sdY", "fold")]

        def fit(self):
            ws = wsbuf(lib.cvm_fit_workspace_bytes(self.N, self.K, self.M, self.cdt))
            ok(lib.cvm_gram_fit(self.X.data_ptr(), _lib.ptr(self.Y), _lib.ptr(self.w), self.N, self.K, self.M, self.cdt,
                                self.G.data_ptr(), _lib.ptr(self.H), self.gs.data_ptr(), self.neg.data_ptr(), ws.data_ptr(),
                                ws.numel(), None), "cvm_gram_fit")
            torch.cuda.synchronize()

    def folds_of(sizes, N, seed):
        """disjoint folds of the given sizes drawn from the N rows (rows ascending inside a fold)"""
        g = np.random.default_rng(seed)
        perm = g.permutation(N)
        host = np.zeros(len(sizes) + 1, dtype=np.int64)
        np.cumsum(sizes, out=host[1:])
        idx = np.concatenate([np.sort(perm[host[i]:host[i + 1]]) for i in range(len(sizes))]).astype(np.int64)
        return idx, host

    def tag(dt, weighted, flags):
        return "%s %s %s" % ("f64" if dt is torch.float64 else "f32", "w" if weighted else "u", "cs" if flags & CENTER_SCALE else "plain")

    combos = [(dt, weighted, cs) for dt in (torch.float64, torch.float32) for weighted in (False, True) for cs in (0, CENTER_SCALE)]

    # ---- the fit; the sweep over a partition of 3 and of 5 folds: merged, in two calls, the middle fold alone; unions
    for dt, weighted, cs in combos:
        p = Problem(300, 132, 2, dt, weighted, 11)
        flags = RET_XTX | RET_XTY | cs
        t = tag(dt, weighted, flags)
        if not cs:
            p.fit()
            emit("fit N=300 K=132 M=2 " + t, G=p.G, H=p.H, gstats=p.gs, neg=p.neg)
        for P in (3, 5):
            lab = np.arange(p.N) % P
            idx_h = np.argsort(lab, kind="stable").astype(np.int64)
            host = np.zeros(P + 1, dtype=np.int64)
            np.cumsum(np.bincount(lab, minlength=P), out=host[1:])
            idx, offs = torch.from_numpy(idx_h).to(dev), torch.from_numpy(host).to(dev)
            wsn = lib.cvm_sweep_workspace_bytes(P, int(np.diff(host).max()), p.K, p.M, p.cdt)
            # cvm_sweep_all
            ws = wsbuf(wsn)
            o, optr = p.outs(P, flags)
            token = C.c_int64(0)
            ok(lib.cvm_sweep_all(p.X.data_ptr(), _lib.ptr(p.Y), _lib.ptr(p.w), idx.data_ptr(), offs.data_ptr(), host.ctypes.data,
                                 P, p.N, p.K, p.M, p.cdt, flags, 1.0, 1e-12, p.G.data_ptr(), _lib.ptr(p.H), p.gs.data_ptr(),
                                 p.neg.data_ptr(), *optr, ws.data_ptr(), wsn, None, C.byref(token)), "cvm_sweep_all")
            torch.cuda.synchronize()
            emit("sweep_all P=%d %s" % (P, t), G=p.G, H=p.H, gstats=p.gs, token=np.int64(token.value), **o)
            # cvm_sweep_fit + cvm_sweep_folds, cvm_sweep_fold_range on the middle fold, unions of 2 of the folds
            ws = wsbuf(wsn)
            token = C.c_int64(0)
            ok(lib.cvm_sweep_fit(p.X.data_ptr(), _lib.ptr(p.Y), _lib.ptr(p.w), idx.data_ptr(), offs.data_ptr(), host.ctypes.data,
                                 P, p.N, p.K, p.M, p.cdt, p.G.data_ptr(), _lib.ptr(p.H), p.gs.data_ptr(), p.neg.data_ptr(),
                                 ws.data_ptr(), wsn, None, C.byref(token)), "cvm_sweep_fit")
            torch.cuda.synchronize()
            emit("sweep_fit P=%d %s" % (P, t), G=p.G, H=p.H, gstats=p.gs, token=np.int64(token.value))
            o, optr = p.outs(P, flags)
            ok(lib.cvm_sweep_folds(offs.data_ptr(), P, p.K, p.M, p.cdt, flags, 1.0, 1e-12, int(weighted), p.G.data_ptr(),
                                   _lib.ptr(p.H), p.gs.data_ptr(), *optr, ws.data_ptr(), wsn, token.value, None), "cvm_sweep_folds")
            torch.cuda.synchronize()
            emit("sweep_folds P=%d %s" % (P, t), **o)
            for f2 in (RET_XTX | RET_XTY | cs, RET_XTY | cs, cs):
                o, optr = p.outs(1, f2)
                ok(lib.cvm_sweep_fold_range(offs.data_ptr(), P, P // 2, 1, p.K, p.M, p.cdt, f2, 1.0, 1e-12, int(weighted),
                                            p.G.data_ptr(), _lib.ptr(p.H), p.gs.data_ptr(), *optr, ws.data_ptr(), wsn,
                                            token.value, None), "cvm_sweep_fold_range")
                torch.cuda.synchronize()
                emit("sweep_fold_range P=%d mid flags=%#x %s" % (P, f2, t), **o)
            if P == 5:
                uf_h = np.array([0, 2, 1, 3, 3, 0], dtype=np.int64)       # unions of 2 of (the first) 4 folds
                uo_h = np.array([0, 2, 4, 6], dtype=np.int64)
                uf, uo = torch.from_numpy(uf_h).to(dev), torch.from_numpy(uo_h).to(dev)
                uws_n = lib.cvm_sweep_unions_workspace_bytes(3, p.K, p.M)
                uws = wsbuf(uws_n)
                o, optr = p.outs(3, flags)
                ok(lib.cvm_sweep_unions(offs.data_ptr(), P, uf.data_ptr(), uo.data_ptr(), uo_h.ctypes.data, 3, p.K, p.M, p.cdt,
                                        flags, 1.0, 1e-12, int(weighted), p.G.data_ptr(), _lib.ptr(p.H), p.gs.data_ptr(), *optr,
                                        ws.data_ptr(), wsn, token.value, uws.data_ptr(), uws_n, None), "cvm_sweep_unions")
                torch.cuda.synchronize()
                emit("sweep_unions 3 of 2 of 4 %s" % t, **o)

    # ---- cvm_fold_update_ex: ragged folds of 1 / 8 / 25 / 90 / 150 rows of N = 3000 (small, mid-tile, fused in-launch,
    # pre-pass, general route, by shape and switch), statistics only, one fold with its indices inside the call
    N = 3000
    for K, M in ((70, 0), (132, 2), (260, 34)):
        for dt, weighted, cs in combos:
            p = Problem(N, K, M, dt, weighted, 100 + K)
            p.fit()
            base = (RET_XTX | (RET_XTY if M else 0)) | cs
            t = tag(dt, weighted, base)
            for rows in (1, 8, 25, 90, 150):
                sizes = [rows, max(rows - 1, 1), rows, (rows + 1) // 2, rows, 1, rows]
                idx_h, host = folds_of(sizes, N, rows)
                P = len(sizes)
                idx, offs = torch.from_numpy(idx_h).to(dev), torch.from_numpy(host).to(dev)
                for flags in ((base, cs) if rows in (25, 150) else (base,)):          # (cs alone: statistics only)
                    wsn = lib.cvm_fold_workspace_bytes(P, len(idx_h), rows, K, M, p.cdt, flags)
                    ws = wsbuf(wsn)
                    o, optr = p.outs(P, flags)
                    status = zeros(1, torch.int32)
                    ok(lib.cvm_fold_update_ex(p.X.data_ptr(), _lib.ptr(p.Y), _lib.ptr(p.w), idx.data_ptr(), offs.data_ptr(),
                                              host.ctypes.data, P, N, K, M, p.cdt, flags, 1.0, 1e-12, p.G.data_ptr(), _lib.ptr(p.H),
                                              p.gs.data_ptr(), *optr, ws.data_ptr(), wsn, None, status.data_ptr()),
                       "cvm_fold_update_ex")
                    torch.cuda.synchronize()
                    emit("fold_update K=%d M=%d rows=%d flags=%#x %s" % (K, M, rows, flags, t), status=status, **o)
            # one fold of 8 rows, indices on the host
            idx_h, host = folds_of([8], N, 5)
            flags = base | IDX_HOST
            wsn = lib.cvm_fold_workspace_bytes(1, 8, 8, K, M, p.cdt, flags)
            ws = wsbuf(wsn)
            o, optr = p.outs(1, flags)
            ok(lib.cvm_fold_update_ex(p.X.data_ptr(), _lib.ptr(p.Y), _lib.ptr(p.w), idx_h.ctypes.data, host.ctypes.data,
                                      host.ctypes.data, 1, N, K, M, p.cdt, flags, 1.0, 1e-12, p.G.data_ptr(), _lib.ptr(p.H),
                                      p.gs.data_ptr(), *optr, ws.data_ptr(), wsn, None, None), "cvm_fold_update_ex (CVM_IDX_HOST)")
            torch.cuda.synchronize()
            emit("fold_update K=%d M=%d idx_host %s" % (K, M, t), **o)

    # ---- a stream of 3 chunks, the second empty, then close and the folds
    for dt, weighted, cs in combos:
        K, M, P = 132, 2, 4
        p = Problem(300, K, M, dt, weighted, 7)
        flags = RET_XTX | RET_XTY | cs
        t = tag(dt, weighted, flags)
        acc_n = lib.cvm_stream_workspace_bytes(_lib.STREAM_ACCUMULATOR, P, 0, K, M, p.cdt)
        acc = wsbuf(acc_n)
        state = np.zeros(_lib.STREAM_STATE_LEN, dtype=np.int64)
        ok(lib.cvm_stream_reset(acc.data_ptr(), acc_n, P, K, M, p.cdt, state.ctypes.data, None), "cvm_stream_reset")
        sizes_total = np.zeros(P, dtype=np.int64)
        for ci, (r0, r1) in enumerate(((0, 170), (170, 170), (170, 300))):
            n = r1 - r0
            lab = (np.arange(r0, r1) * 7) % P
            idx_h = np.argsort(lab, kind="stable").astype(np.int64)
            host = np.zeros(P + 1, dtype=np.int64)
            np.cumsum(np.bincount(lab, minlength=P), out=host[1:])
            sizes_total += np.diff(host)
            idx, offs = torch.from_numpy(idx_h).to(dev) if n else None, torch.from_numpy(host).to(dev)
            wsn = lib.cvm_stream_workspace_bytes(_lib.STREAM_SCRATCH, P, int(np.diff(host).max()), K, M, p.cdt)
            ws = wsbuf(wsn)
            info = np.zeros(2, dtype=np.int64)
            Xc, Yc, wc = p.X[r0:r1], p.Y[r0:r1], (p.w[r0:r1] if weighted else None)
            ok(lib.cvm_stream_add(Xc.data_ptr() if n else None, Yc.data_ptr() if n else None, _lib.ptr(wc) if n else None,
                                  _lib.ptr(idx), offs.data_ptr(), host.ctypes.data, P, n, K, M, p.cdt, acc.data_ptr(), acc_n,
                                  state.ctypes.data, ws.data_ptr(), wsn, None, info.ctypes.data), "cvm_stream_add")
            torch.cuda.synchronize()
            emit("stream_add chunk %d %s" % (ci, t), acc=acc, info=info, state=state)
        cws_n = lib.cvm_stream_workspace_bytes(_lib.STREAM_CLOSE, P, 0, K, M, p.cdt)
        cws = wsbuf(cws_n)
        units, nbytes, token = C.c_void_p(0), C.c_size_t(0), C.c_int64(0)
        ok(lib.cvm_stream_close(acc.data_ptr(), acc_n, state.ctypes.data, P, K, M, p.cdt, p.G.data_ptr(), _lib.ptr(p.H),
                                p.gs.data_ptr(), p.neg.data_ptr(), cws.data_ptr(), cws_n, None, C.byref(units), C.byref(nbytes),
                                C.byref(token)), "cvm_stream_close")
        torch.cuda.synchronize()
        emit("stream_close %s" % t, G=p.G, H=p.H, gstats=p.gs, neg=p.neg, token=np.int64(token.value), nbytes=np.int64(nbytes.value))
        host = np.zeros(P + 1, dtype=np.int64)
        np.cumsum(sizes_total, out=host[1:])
        offs = torch.from_numpy(host).to(dev)
        o, optr = p.outs(P, flags)
        ok(lib.cvm_sweep_fold_range(offs.data_ptr(), P, 0, P, K, M, p.cdt, flags, 1.0, 1e-12, int(weighted), p.G.data_ptr(),
                                    _lib.ptr(p.H), p.gs.data_ptr(), *optr, units.value, nbytes.value, token.value, None),
           "cvm_sweep_fold_range (stream)")
        torch.cuda.synchronize()
        emit("stream folds %s" % t, **o)

    print("\n".join(lines))
    print("# %d arrays, %s" % (len(lines), lib.cvm_version().decode()))


def child(switch, lib_path, out_path):
    env = dict(os.environ)
    for s in SWITCHES:
        if s:
            env.pop(s.split("=")[0], None)
    env.pop("CVM_LIB_PATH", None)
    if switch:
        k, v = switch.split("=")
        env[k] = v
    if lib_path:
        env["CVM_LIB_PATH"] = lib_path
    with open(out_path, "w") as f:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=f, stderr=subprocess.PIPE, text=True,
                           timeout=600)
    if r.returncode != 0:
        sys.exit("fold_bits child (%s, %s) failed with %d:\n%s" % (switch or "default", lib_path or "tree", r.returncode, r.stderr[-3000:]))


def matrix(outdir, parent):
    os.makedirs(outdir, exist_ok=True)
    report = ["switch: arrays compared (digests of their bytes) -> different, parent library against branch library, same inputs"]
    total = different = 0
    for sw in SWITCHES:
        name = (sw or "default").replace("=", "_").replace(",", "_")
        child(sw, None, os.path.join(outdir, "branch_%s.txt" % name))
        if not parent:
            continue
        child(sw, parent, os.path.join(outdir, "parent_%s.txt" % name))
        rows = [[l for l in open(os.path.join(outdir, "%s_%s.txt" % (who, name))).read().splitlines() if not l.startswith("#")]
                for who in ("parent", "branch")]
        diff = [b for a, b in zip(*rows) if a != b]
        if len(rows[0]) != len(rows[1]):
            diff.append("(%d lines against %d)" % (len(rows[0]), len(rows[1])))
        total += len(rows[1])
        different += len(diff)
        report.append("%-24s: %4d arrays -> %d different" % (sw or "default", len(rows[1]), len(diff)))
        report += ["    " + d for d in diff[:20]]
    if parent:
        report.append("%d arrays over %d processes per library, %d different" % (total, len(SWITCHES), different))
        text = "\n".join(report) + "\n"
        with open(os.path.join(outdir, "bits_vs_parent.txt"), "w") as f:
            f.write(text)
        print(text, end="")
        return 1 if different else 0
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", metavar="OUTDIR")
    ap.add_argument("--parent", metavar="LIB")
    a = ap.parse_args()
    if a.matrix:
        sys.exit(matrix(a.matrix, a.parent))
    run_cases()
