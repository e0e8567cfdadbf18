"""CPU: what the fold-stage entries share on the host before any launch (cvmatrix_amd/csrc/fold_plan.hpp) -- the plan
token, the scan of the folds' offsets, the parser of the route switches -- in a host-only C++ program
(tests/fold_plan_check.cpp)."""

import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_fold_plan_in_a_host_program(tmp_path):
    """fold_plan.hpp under a host compiler, with the undefined-behaviour and address sanitizers where the compiler
    has their runtimes.  Token: round trip over s_off, s_diag in {1, 2, 7, 2^20 - 1} x compacted, refusal of 0,
    negatives, a bit above 40, s_off = 0, s_diag = 0.  fold_rows / folds_cover: empty folds, one fold, a decreasing
    pair (code and message), max_rows and present against a plain loop, a cover one row short or long.  The switch
    record from a table of strings: defaults, the CVM_SMALL_MAXN clamps, set-means-on for the four CVM_NO_* ones."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "fold_plan_check")
    cmd = [gxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "fold_plan_check.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=undefined,address", "-fno-sanitize-recover=all"], capture_output=True,
                         text=True, timeout=300)
    if san.returncode != 0:                       # (no sanitizer runtime here: the plain program)
        plain = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert plain.returncode == 0, plain.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("fold plan ok"), out.stdout + out.stderr
