"""The even static K split's index arithmetic (cuda-qr_amd/csrc/qr_tn_even.h) on the CPU: tests/c/tn_even_check.c, built with the host
compiler, sweeps (tiles, k-tiles, workgroups) and asserts coverage, tile-local segments, slot order and the reduce's inverse map."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_even_split_index_arithmetic(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no host C compiler")
    exe = str(tmp_path / "tn_even_check")
    out = subprocess.run([cc, "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "c", "tn_even_check.c"), "-o", exe],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    assert run.stdout.startswith("tn_even_check ok ")
    assert int(run.stdout.split()[2]) == 40 * 40 * 96 + 199 * 1024 * 2
