"""Diagnostic: per work item and compute wave cycles of ONE sweep Gram launch (build with -DCVM_STAMPS):
loop cycles per stage of the diagonal items with ti == 0 against ti > 0, and the cycles from an item's
entry to its first stage (stage 0 in LDS, both prologue barriers passed) for a workgroup's first and
later items.

    python tools/item_stamps.py tools/libcvmhip_stamps.so [C3|C2|C4|C5]
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cvmatrix_amd._lib as L  # noqa: E402

L.LIB_PATH = sys.argv[1]
from cvmatrix_amd import CVMatrix, Partitioner  # noqa: E402

SHAPES = {"C3": (100000, 512, 16, 10, torch.float64, True), "C4": (1000000, 1024, 32, 64, torch.float64, True),
          "C5": (200000, 4096, 1, 20, torch.float32, True), "C2": (100000, 512, 16, 10, torch.float64, False)}
name = sys.argv[2] if len(sys.argv) > 2 else "C3"
N, K, M, P, tdt, weighted = SHAPES[name]
dev = torch.device("cuda:0")
g = torch.Generator(device=dev)
g.manual_seed(0)
X = torch.rand((N, K), dtype=tdt, device=dev, generator=g)
Y = torch.rand((N, M), dtype=tdt, device=dev, generator=g)
w = torch.rand((N,), dtype=tdt, device=dev, generator=g) if weighted else None
fl = (True,) * 4 if weighted else (False,) * 4
m = CVMatrix(*fl, lazy_fit=True, dtype=np.float64 if tdt == torch.float64 else np.float32, copy=False, device=dev,
             reuse_outputs=True, trust_tensor_versions=True)
m.fit(X, Y, w)
b = m.prepare_folds(Partitioner(np.arange(N) % P))
lib = L.load()
print(lib.cvm_version().decode(), name)
NI, NW, NFIELD = 8 * 128, 4, 8
buf = (C.c_ulonglong * (NI * NW * NFIELD))()
for _ in range(200):       # the chip at its steady clock
    m.fit(X, Y, w)
    m.training_XTX_XTY_batched(b)
torch.cuda.synchronize()
lib.cvm_debug_stamps5(buf, 1)
m.fit(X, Y, w)
m.training_XTX_XTY_batched(b)
torch.cuda.synchronize()
lib.cvm_debug_stamps5(buf, 0)
a = np.frombuffer(buf, dtype=np.uint64).reshape(NI, NW, NFIELD).astype(np.int64)
a = a[a[:, 0, 5] > 0]
meta = a[:, 0, 6]
ti, tj, wg = meta & 255, (meta >> 8) & 255, meta >> 32
st = a[:, :, 5].astype(np.float64)
print("items", len(a), "workgroups", len(np.unique(wg)), "stages per item: diagonal", np.unique(a[ti == tj, 0, 5]),
      "off-diagonal", np.unique(a[ti != tj, 0, 5]))
# the ordinal of an item inside its workgroup, by entry time
order = np.zeros(len(a), dtype=int)
for b_ in np.unique(wg):
    ix = np.where(wg == b_)[0]
    order[ix[np.argsort(a[ix, 0, 0])]] = np.arange(len(ix))


def row(label, sel):
    if not sel.any():
        return
    loop, comp, wait = a[sel, :, 2] / st[sel], a[sel, :, 3] / st[sel], a[sel, :, 4] / st[sel]
    print(f"{label:28s} n={sel.sum():4d}  loop/stage by wave {np.round(loop.mean(0), 1)}  computing {np.round(comp.mean(0), 1)}"
          f"  at the barrier {np.round(wait.mean(0), 1)}  item loop cycles mean {a[sel, 0, 2].mean():.0f} max {a[sel, 0, 2].max()}")


print("-- loop cycles per 16-row stage, per compute wave")
diag = ti == tj
row("diagonal ti == 0", diag & (ti == 0))
for t in sorted(set(ti[diag]) - {0}):
    row(f"diagonal ti == {t}", diag & (ti == t))
row("diagonal ti > 0", diag & (ti > 0))
row("off-diagonal", ~diag)
for o in range(order.max() + 1):
    row(f"diagonal ti == 0, item #{o} of its workgroup", diag & (ti == 0) & (order == o))
    row(f"diagonal ti > 0, item #{o}", diag & (ti > 0) & (order == o))
print("-- whole item (entry -> exit, stores acknowledged), cycles, wave 0")
for lab, sel in (("diagonal ti == 0", diag & (ti == 0)), ("diagonal ti > 0", diag & (ti > 0)), ("off-diagonal", ~diag)):
    if sel.any():
        d = a[sel, 0, 7] - a[sel, 0, 0]
        print(f"{lab:28s} mean {d.mean():.0f}  min {d.min()}  max {d.max()}")
print("-- cycles from an item's entry to its first stage (wave 0 .. 3)")
for o in range(order.max() + 1):
    for lab, sel in (("diagonal", diag), ("off-diagonal", ~diag)):
        s_ = sel & (order == o)
        if s_.any():
            print(f"item #{o} of its workgroup, {lab:13s} n={s_.sum():4d}  {np.round(a[s_, :, 1].mean(0))}  max {a[s_, :, 1].max()}")
print("-- gap between a workgroup's items (exit of one -> entry of the next), wave 0")
gaps = []
for b_ in np.unique(wg):
    ix = np.where(wg == b_)[0]
    ix = ix[np.argsort(a[ix, 0, 0])]
    gaps += [a[ix[k + 1], 0, 0] - a[ix[k], 0, 7] for k in range(len(ix) - 1)]
if gaps:
    print("mean %.0f  max %d  n=%d" % (np.mean(gaps), np.max(gaps), len(gaps)))
