"""Streaming cross-validation (StreamingCVMatrix: cvm_stream_add per chunk, cvm_stream_close + the finalize kernels
at hand-out) against the one-shot sweep over the same rows, fit(folds=p) + training_XTX_XTY_batched(p), in one
process on one device, alternating step by step; medians after a warm-up.

    python tools/bench_streaming.py         # prints; kept in profiles/streaming/bench_streaming.txt

Shape: the C3 workload (BASELINE.json: N = 100 000, K = 512, M = 16, 10 folds, weighted, all four flags,
float64), X, Y and the weights resident on the device (neither side copies them: copy=False / chunks read in
place), fed in 1, 4 and 16 chunks of consecutive rows; the labels are host arrays, as a reader of files has them.
A step is timed on the host clock around a device synchronisation (the chunks' grouping by fold is host work and
belongs to the price of a chunk).  A second pass records every chunk's Gram launch and accumulate kernel with the
library's own event pairs (cvm_timing_enable / cvm_timing_read_stream); the bytes the accumulate kernel moves are
the library's count (every partial of the folds present read once, their accumulator units read and written
once), held against cvm_fill_probe on the accumulator in the same run."""
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cvmatrix_amd import CVMatrix, Partitioner, StreamingCVMatrix, _lib  # noqa: E402


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main(N=100000, K=512, M=16, P=10, dtype=np.float64, reps=15, warm=3, chunkings=(1, 4, 16)):
    lib = _lib.load()
    rng = np.random.default_rng(42)
    dev = torch.device("cuda:0")
    X = torch.from_numpy(rng.random((N, K)).astype(dtype)).to(dev)
    Y = torch.from_numpy(rng.random((N, M)).astype(dtype)).to(dev)
    w = torch.from_numpy((rng.random(N) + 0.1).astype(dtype)).to(dev)
    labels = np.arange(N) % P
    flags = (True,) * 4
    cvm = CVMatrix(*flags, dtype=dtype, copy=False)
    batch = Partitioner(labels)                            # (fold position = label: the labels appear in order)

    def one_shot():
        cvm.fit(X, Y, w, folds=batch)
        return cvm.training_XTX_XTY_batched(batch)

    scv = StreamingCVMatrix(P, *flags, dtype=dtype)
    steps = {}
    for C in chunkings:
        bounds = np.linspace(0, N, C + 1).astype(int)
        parts = [(X[a:b], Y[a:b], w[a:b], labels[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]

        def step(parts=parts):
            scv.reset()
            for p in parts:
                scv.partial_fit(*p)
            return scv.training_XTX_XTY_batched()
        steps[C] = (step, parts)
    for _ in range(warm):
        for fn in [one_shot] + [s for s, _ in steps.values()]:
            res = fn()
            del res
    (ax, _), _ = one_shot()
    (bx, _), _ = steps[max(chunkings)][0]()
    diff = float((ax - bx).abs().max() / ax.abs().max())
    del ax, bx
    t_one, t_str = [], {C: [] for C in chunkings}
    for _ in range(reps):                                  # alternating: the clock and the neighbours are shared
        t_one.append(wall_ms(one_shot))
        for C in chunkings:
            t_str[C].append(wall_ms(steps[C][0]))
    one = float(np.median(t_one))
    spread = (float(np.min(t_one)), float(np.max(t_one)))
    print(f"C3 shape N={N} K={K} M={M} folds={P} weighted {np.dtype(dtype).name}, flags 1111; max diff of the streamed "
          f"XTX ({max(chunkings)} chunks) against the one-shot {diff:.1e}")
    print(f"one-shot fit(folds=p) + training_XTX_XTY_batched(p): {one:8.3f} ms per step (min {spread[0]:.3f}, max {spread[1]:.3f}; host clock)")
    # the device's write ceiling, same run: on the accumulator itself (a few MB: it lives in the caches) and on a
    # buffer of the bytes one accumulate launch moves at the single-chunk plan
    acc = scv._acc
    nbytes = acc.numel() // 16 * 16
    fill = float(np.median([event_ms(lambda: lib.cvm_fill_probe(acc.data_ptr(), nbytes, 0)) for _ in range(reps + warm)][warm:]))
    big = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    fill_big = float(np.median([event_ms(lambda: lib.cvm_fill_probe(big.data_ptr(), big.numel(), 0)) for _ in range(reps + warm)][warm:]))
    fill_rate = big.numel() / fill_big / 1e9
    del big
    gram_row_ms = None
    rows = []
    for C in chunkings:
        step, parts = steps[C]
        # the chunks' own launches, by the library's event pairs
        lib.cvm_timing_enable(1)
        gram, accm, moved = [], [], []
        for _ in range(reps):
            scv.reset()
            for p in parts:
                scv.partial_fit(*p)
                moved.append(scv._last_add[2])
            torch.cuda.synchronize()
            g, a = ctypes.c_double(0), ctypes.c_double(0)
            ng, na = ctypes.c_int64(0), ctypes.c_int64(0)
            lib.cvm_timing_read_stream(ctypes.byref(g), ctypes.byref(ng), ctypes.byref(a), ctypes.byref(na))
            assert ng.value == na.value == C
            gram.append(g.value / C)
            accm.append(a.value / C)
        lib.cvm_timing_enable(0)
        close = float(np.median([event_ms(lambda: (setattr(scv, "_snap_version", -1), scv.training_XTX_XTY_batched()))
                                 for _ in range(reps)]))
        s = float(np.median(t_str[C]))
        g_ms, a_ms, b = float(np.median(gram)), float(np.median(accm)), float(np.median(moved))
        if C == 1:
            gram_row_ms = g_ms / N
        rows.append((C, N // C, s, g_ms, a_ms, b, close))
        print(f"{C:3d} chunks of {N // C:6d} rows: {s:8.3f} ms per step = {s / one:5.2f} x one-shot, "
              f"{(s - one) / C:7.3f} ms over the one-shot per chunk | per chunk: Gram launch {g_ms:7.3f} ms, accumulate kernel "
              f"{a_ms:7.4f} ms moving {b / 1e6:7.2f} MB = {b / a_ms / 1e9:5.2f} TB/s = {b / a_ms / 1e9 / fill_rate:4.2f} of the fill "
              f"probe | close + finalize at hand-out {close:6.3f} ms")
    print(f"cvm_fill_probe: on the accumulator ({nbytes / 1e6:.1f} MB, cache-resident) {fill:7.4f} ms = {nbytes / fill / 1e9:5.2f} TB/s; "
          f"on 1 GiB {fill_big:7.4f} ms = {fill_rate:5.2f} TB/s (the rate the fractions above are taken of)")
    # the price of a chunk over the one-shot step, as a line  a + b n  through the measured chunk sizes (host clock),
    # against the chunk's own Gram work (time per row of the single chunk's launch)
    ns = np.array([r[1] for r in rows], dtype=float)
    over = np.array([(r[2] - one) / r[0] for r in rows])
    b_, a_ = np.polyfit(ns, over, 1) if len(rows) > 1 else (0.0, over[0])
    print(f"overhead per chunk on the host clock ~ {a_:.3f} ms + {b_ * 1e6:.2f} ns per row (fit through {len(rows)} chunk sizes); "
          f"a chunk's Gram work costs {gram_row_ms * 1e6:.2f} ns per row")
    if 0.02 * gram_row_ms > b_:
        print(f"  -> below 2 % of the chunk's Gram time from {int(np.ceil(a_ / (0.02 * gram_row_ms - b_))):,d} rows per chunk")
    else:
        print("  -> the row-proportional part alone (labels uploaded and grouped per chunk, the weights check) is above 2 % "
              "of the Gram work per row: the host-clock overhead does not fall below 2 % at any chunk size")
    for C, n, s_, g_ms, a_ms, b, close in rows:
        print(f"  device side alone at {n} rows per chunk: accumulate kernel {a_ms:.4f} ms = {100 * a_ms / g_ms:.1f} % of the chunk's "
              f"Gram launch; below 2 % of a Gram launch from {int(np.ceil(a_ms / (0.02 * gram_row_ms))):,d} rows per chunk at this plan")


if __name__ == "__main__":
    print(torch.cuda.get_device_name(0), "|", _lib.load().cvm_version().decode(), flush=True)
    main()
