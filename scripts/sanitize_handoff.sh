#!/usr/bin/env bash
# ASan/UBSan build + run of the two stand-alone handoff programs:
#  - csrc/native_scan_diff_test.cpp: SSE2 vs scalar string search in
#    aigw_core::Scan, on exact-size heap buffers;
#  - csrc/fastpath_handoff_test.cpp: request text through the native
#    server and DirectGpuBatcher with a content-checking fake admission.
# CPU-only, baseline x86-64 flags; runs in seconds. Invoked by
# tests/test_native_handoff_sanitize.py.
set -euo pipefail
cd "$(dirname "$0")/.."
tmp="$(mktemp -d)"
trap 'rm -rf "$tmp"' EXIT
flags=(-std=c++17 -O1 -g -fno-omit-frame-pointer
       -fsanitize=address,undefined -fno-sanitize-recover=all
       -D_GLIBCXX_ASSERTIONS)

g++ "${flags[@]}" csrc/native_scan_diff_test.cpp -o "$tmp/scan_diff"
"$tmp/scan_diff" tests/golden/bench_chat_body.json

g++ "${flags[@]}" csrc/fastpath_handoff_test.cpp csrc/fastpath.cpp \
    -o "$tmp/handoff" -lpthread
"$tmp/handoff"
