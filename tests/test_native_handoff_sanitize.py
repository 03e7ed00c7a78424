"""ASan/UBSan lane for the admission handoff: the SSE2-vs-scalar scan
differential (csrc/native_scan_diff_test.cpp) and the content-checked
text handoff through the native server and its batcher
(csrc/fastpath_handoff_test.cpp). Both are stand-alone binaries built and
run by scripts/sanitize_handoff.sh; nothing is loaded into Python."""

import shutil
import subprocess

import pytest


@pytest.mark.timeout(240)
def test_handoff_under_sanitizers():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    proc = subprocess.run(
        ["bash", "scripts/sanitize_handoff.sh"],
        capture_output=True,
        timeout=220,
        cwd=__file__.rsplit("/tests/", 1)[0],
    )
    out = (proc.stdout + proc.stderr).decode()
    assert proc.returncode == 0, out[-3000:]
    assert "native scan diff passed" in out
    assert "fastpath handoff tests passed" in out
