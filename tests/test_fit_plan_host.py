"""CPU: the plans the fit-stage solvers share (cvmatrix_amd/csrc/fit_plan.hpp) -- the slot-to-problem map, the slot
plan, the chunk plan and the dtype dispatch in a host-only C++ program (tests/fit_plan_check.cpp); the workspace
sizes of the seven solvers as closed forms of those plans; and CVM_EWORKSPACE, decided from the arguments alone,
for the entries whose own host tests do not ask for it."""

import ctypes
import os
import shutil
import subprocess

import pytest

from cvmatrix_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_fit_plan_in_a_host_program(tmp_path):
    """fit_plan.hpp under a host compiler, with the undefined-behaviour and address sanitizers where the compiler
    has their runtimes: slot_first is a permutation of 0 .. G-1 that keeps the blocks of one residue b & 7 on
    consecutive problems, for every G in 1 .. 600; slot_count, slot_workspace_bytes and folds_per_chunk against
    their closed forms / a linear scan."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "fit_plan_check")
    cmd = [gxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "fit_plan_check.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=undefined,address", "-fno-sanitize-recover=all"], capture_output=True,
                         text=True, timeout=300)
    if san.returncode != 0:                       # (no sanitizer runtime here: the plain program)
        plain = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert plain.returncode == 0, plain.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("fit plan ok"), out.stdout + out.stderr


SHAPES = [(0, 33, 3, 5), (1, 1, 1, 1),(3, 33, 3, 5), (9, 512, 64, 64), (100, 70, 2, 5), (600, 513, 17, 33), (2000, 4096, 64, 64)]


@pytest.mark.parametrize("F,K,M,L", SHAPES)
def test_slot_solvers_workspace_is_the_slot_plan(lib, F, K, M, L):
    """min(max(P, 1), cap) slots of one problem's bytes: ridge P = F L, enet and omp P = F M, pcr and pcr_blocked
    P = F (pcr: K <= 512; omp, pcr: A <= K)."""
    A = min(L, K)
    assert lib.cvm_ridge_workspace_bytes(F, K, M, L) == min(max(F * L, 1), 512) * lib.cvm_ridge_workspace_bytes(1, K, M, 1)
    assert lib.cvm_enet_workspace_bytes(F, K, M, L) == min(max(F * M, 1), 1024) * lib.cvm_enet_workspace_bytes(1, K, 1, L)
    assert lib.cvm_omp_workspace_bytes(F, K, M, A) == min(max(F * M, 1), 1024) * lib.cvm_omp_workspace_bytes(1, K, 1, A)
    assert lib.cvm_pcr_blocked_workspace_bytes(F, K, M, A) == min(max(F, 1), 512) * lib.cvm_pcr_blocked_workspace_bytes(1, K, M, A)
    if K <= 512:
        assert lib.cvm_pcr_workspace_bytes(F, K, M, A) == min(max(F, 1), 512) * lib.cvm_pcr_workspace_bytes(1, K, M, A)


def lda_layout_bytes(F, K, C, L):
    """The records of F folds in cvm_lda_fit's workspace (csrc/lda.hpp), each region rounded up to 256 bytes."""
    up = lambda n: (n + 255) // 256 * 256
    return (up(F * K * K * 8) + up(F * K * C * 8) + up(F * L * K * C * 8) + up(F * 4 * 8) + up(F * 4) + up(F * L * 4))


@pytest.mark.parametrize("K,C,L", [(1, 2, 1), (33, 3, 8), (512, 64, 64), (4096, 7, 256)])
def test_chunk_solvers_workspace_grows_with_the_folds(lib, K, C, L):
    """lda: the fold records in front of the ridge slots.  lda and pcalda: never decreasing in F, which is what the
    search for the folds per chunk rests on, and strictly increasing wherever one fold's share of a region is at
    least the 256 bytes the regions are rounded to (K K 8 for lda, A A 8 for pcalda: all shapes here but the
    first, whose records of two folds fit the rounding of one)."""
    A = min(L, K, 64)
    last_lda = last_pcl = 0
    for F in (1, 2, 3, 7, 100, 600):
        lda = lib.cvm_lda_workspace_bytes(F, K, C, L)
        assert lda - lib.cvm_ridge_workspace_bytes(F, K, C, L) == lda_layout_bytes(F, K, C, L), F
        pcl = lib.cvm_pcalda_workspace_bytes(F, K, C, A)
        assert lda >= last_lda and pcl >= last_pcl and lda > 0 and pcl > 0, F
        if K * K * 8 >= 256:
            assert lda > last_lda, F
        if A * A * 8 >= 256:
            assert pcl > last_pcl, F
        last_lda, last_pcl = lda, pcl
    assert lib.cvm_lda_workspace_bytes(0, K, C, L) == lib.cvm_lda_workspace_bytes(1, K, C, L)
    assert lib.cvm_pcalda_workspace_bytes(0, K, C, A) == lib.cvm_pcalda_workspace_bytes(1, K, C, A)


def test_less_than_one_slot_is_refused_before_the_device(lib):
    """cvm_ridge_fit, cvm_enet_fit, cvm_pcr_fit and cvm_pcr_blocked_fit with one byte less than one slot:
    CVM_EWORKSPACE from the arguments alone, with folds and without (the data pointers are never followed; the
    penalties are read, so they are real); one slot and no fold launches nothing."""
    buf = (ctypes.c_double * 64)(*([1.0] * 64))
    p = ctypes.addressof(buf)
    K, M, L, A, f64 = 33, 3, 5, 5, _lib.CVM_F64
    entries = {
        "ridge": (lib.cvm_ridge_workspace_bytes(1, K, M, 1),
                  lambda F, n: lib.cvm_ridge_fit(p, p, F, K, M, p, L, f64, p, p, p, n, None)),
        "enet": (lib.cvm_enet_workspace_bytes(1, K, 1, L),
                 lambda F, n: lib.cvm_enet_fit(p, p, F, K, M, p, L, 0.5, 1e-8, 100, f64, p, p, p, p, n, None)),
        "pcr": (lib.cvm_pcr_workspace_bytes(1, K, M, A),
                lambda F, n: lib.cvm_pcr_fit(p, p, F, K, M, A, f64, 0.0, p, p, p, p, p, p, n, None)),
        "pcr_blocked": (lib.cvm_pcr_blocked_workspace_bytes(1, K, M, A),
                        lambda F, n: lib.cvm_pcr_blocked_fit(p, p, F, K, M, A, f64, 0.0, 60, p, p, p, p, p, p, n, None)),
    }
    for name, (one, call) in entries.items():
        assert one > 0, name
        for F in (3, 0):
            assert call(F, one - 1) == _lib.CVM_EWORKSPACE, (name, F)
            err = lib.cvm_last_error()
            assert b"workspace too small" in err and f"cvm_{name}_fit".encode() in err, (name, err)
        assert call(0, one) == _lib.CVM_OK, name
