#!/usr/bin/env bash
# TSan and ASan/UBSan builds + runs of csrc/wake_tree_test.cpp, the
# stand-alone test of the admission batcher's lock-free futex waiters
# (csrc/wake_tree.h). CPU-only; nothing is loaded into Python and nothing
# is preloaded. Invoked by tests/test_native_wake_sanitize.py.
set -euo pipefail
cd "$(dirname "$0")/.."
tmp="$(mktemp -d)"
trap 'rm -rf "$tmp"' EXIT
flags=(-std=c++17 -O1 -g -fno-omit-frame-pointer -D_GLIBCXX_ASSERTIONS
       -Icsrc)

g++ "${flags[@]}" -fsanitize=thread csrc/wake_tree_test.cpp \
    -o "$tmp/wake_tsan" -lpthread
TSAN_OPTIONS=halt_on_error=1 "$tmp/wake_tsan"

g++ "${flags[@]}" -fsanitize=address,undefined -fno-sanitize-recover=all \
    csrc/wake_tree_test.cpp -o "$tmp/wake_asan" -lpthread
"$tmp/wake_asan"
