// One-shot waiters without a mutex or condition variable. Header-only,
// C++17, Linux futex; no HIP, so a stand-alone program can test it
// (csrc/wake_tree_test.cpp).
//
// A waiter type T derives from wake_tree::Node. One thread (the publisher)
// completes a batch of waiters with publish(); each waiter's owner thread
// calls await() on its own waiter, before, during or after that.
//
// The name is historical: the first version had woken owners wake two more
// waiters each (a binary relay tree), so that the publisher made one futex
// call per batch. It was correct and took the publisher's share from
// ~100 us to 7 us per batch, and the benchmark ran 14 % slower for it
// (profiles/admission_fulfil.md), so the publisher wakes every sleeper
// itself.
//
// state is DONE | SLEEPING.
//   publisher: plain stores of the waiter's results, then state |= DONE
//              with release; FUTEX_WAKE if the previous state had SLEEPING.
//   owner:     sees DONE (acquire) -> may read the results; otherwise CAS
//              0 -> SLEEPING and FUTEX_WAIT while the word is SLEEPING.
//
// Why no wake-up is lost:
//  - SLEEPING is only ever set by the CAS from 0, so it cannot become set
//    after DONE: an owner that arrives after DONE never sleeps, and the
//    publisher's fetch_or sees SLEEPING whenever the owner committed to
//    sleeping first.
//  - FUTEX_WAIT compares the word with SLEEPING inside the kernel: if DONE
//    is already there it returns at once; if DONE comes later, the
//    publisher has seen SLEEPING and sends the wake. A wake that finds
//    nobody asleep (the owner was between CAS and wait, woke by itself, or
//    is leaving on its deadline) does nothing.
//  - A deadline leaves with CAS SLEEPING -> 0. If that fails, DONE arrived
//    and the waiter proceeds as done; if it succeeds the owner has seen no
//    DONE and must not read the results. A later publish finds no SLEEPING
//    and makes no call.
#pragma once

#include <linux/futex.h>
#include <sys/syscall.h>
#include <time.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <memory>

// Test hook: a test defines it before including this header to stretch
// publish() so that owners arrive in the middle of it.
#ifndef WAKE_TREE_HOOK
#define WAKE_TREE_HOOK(index) ((void)0)
#endif

namespace wake_tree {

constexpr uint32_t DONE = 1u;
constexpr uint32_t SLEEPING = 2u;

struct Node {
  std::atomic<uint32_t> state{0};
};

inline long futex(std::atomic<uint32_t>* word, int op, uint32_t val,
                  const struct timespec* timeout) {
  static_assert(sizeof(std::atomic<uint32_t>) == sizeof(uint32_t),
                "futex word must be a plain 32-bit integer");
  return syscall(SYS_futex, reinterpret_cast<uint32_t*>(word), op, val,
                 timeout, nullptr, 0);
}

// Publisher: complete ws[0..n). fill(i, T&) writes position i's results
// with plain stores. None of the waiters may have been published before;
// the caller's references keep them alive across the wake.
template <class T, class Fill>
void publish(const std::shared_ptr<T>* ws, size_t n, Fill&& fill) {
  for (size_t i = 0; i < n; ++i) {
    T& w = *ws[i];
    fill(i, w);
    if (w.state.fetch_or(DONE, std::memory_order_release) & SLEEPING)
      futex(&w.state, FUTEX_WAKE_PRIVATE, 1, nullptr);
    WAKE_TREE_HOOK(i);
  }
}

// Owner: wait until w is published or `timeout` has passed. True means
// DONE was observed and the results may be read. False means the deadline
// fired: the results must not be read.
template <class T>
bool await(T* w, std::chrono::nanoseconds timeout) {
  uint32_t s = w->state.load(std::memory_order_acquire);
  if (s & DONE) return true;
  s = 0;
  if (!w->state.compare_exchange_strong(s, SLEEPING,
                                        std::memory_order_acq_rel,
                                        std::memory_order_acquire))
    return true;  // with one owner per waiter only DONE makes the CAS fail
  auto deadline = std::chrono::steady_clock::now() + timeout;
  for (;;) {
    auto left = std::chrono::duration_cast<std::chrono::nanoseconds>(
                    deadline - std::chrono::steady_clock::now())
                    .count();
    if (left <= 0) {
      s = SLEEPING;
      // failure means DONE arrived first
      return !w->state.compare_exchange_strong(s, 0,
                                               std::memory_order_acq_rel,
                                               std::memory_order_acquire);
    }
    struct timespec ts;
    ts.tv_sec = (time_t)(left / 1000000000);
    ts.tv_nsec = (long)(left % 1000000000);
    futex(&w->state, FUTEX_WAIT_PRIVATE, SLEEPING, &ts);
    if (w->state.load(std::memory_order_acquire) & DONE) return true;
  }
}

}  // namespace wake_tree
