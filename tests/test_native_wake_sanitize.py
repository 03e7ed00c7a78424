"""TSan and ASan/UBSan lane for the admission batcher's lock-free futex
waiters (csrc/wake_tree.h): csrc/wake_tree_test.cpp is a stand-alone binary built
twice and run by scripts/sanitize_wake.sh; nothing is loaded into Python."""

import shutil
import subprocess

import pytest


@pytest.mark.timeout(240)
def test_wake_tree_under_sanitizers():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    proc = subprocess.run(
        ["bash", "scripts/sanitize_wake.sh"],
        capture_output=True,
        timeout=220,
        cwd=__file__.rsplit("/tests/", 1)[0],
    )
    out = (proc.stdout + proc.stderr).decode()
    assert proc.returncode == 0, out[-3000:]
    assert out.count("wake tree tests passed") == 2, out[-3000:]
