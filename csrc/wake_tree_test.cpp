// Stand-alone test of csrc/wake_tree.h (built with -fsanitize=thread and
// with -fsanitize=address,undefined by scripts/sanitize_wake.sh). Seeded
// batches of waiters are published while their owner threads collect
// before, during and after publish(). A lost wake-up shows as a fired 2 s
// deadline, not as a hang.
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <vector>

static void test_hook(size_t index);
#define WAKE_TREE_HOOK(index) test_hook(index)
#include "wake_tree.h"

namespace {

struct W : wake_tree::Node {
  int64_t value = 0;  // plain, like the batcher's result fields
};

std::atomic<int> g_stretch_us{0};  // sleep inside publish(), see test_hook

}  // namespace

// after the first two waiters and after every 64th, so that owners arrive
// while a batch is half published
static void test_hook(size_t index) {
  if (index > 1 && index % 64 != 0) return;
  int us = g_stretch_us.load(std::memory_order_relaxed);
  if (us > 0) std::this_thread::sleep_for(std::chrono::microseconds(us));
}

namespace {

// Futex barrier: with a mutex and condition variable, 1025 threads queue
// for the mutex at every release and the test takes minutes.
class Barrier {
 public:
  explicit Barrier(size_t n) : n_(n) {}
  void wait() {
    uint32_t g = gen_.load(std::memory_order_acquire);
    if (count_.fetch_add(1, std::memory_order_acq_rel) + 1 == n_) {
      count_.store(0, std::memory_order_relaxed);
      gen_.store(g + 1, std::memory_order_release);
      wake_tree::futex(&gen_, FUTEX_WAKE_PRIVATE, INT32_MAX, nullptr);
    } else {
      while (gen_.load(std::memory_order_acquire) == g)
        wake_tree::futex(&gen_, FUTEX_WAIT_PRIVATE, g, nullptr);
    }
  }

 private:
  std::atomic<uint32_t> gen_{0};
  std::atomic<size_t> count_{0};
  size_t n_;
};

enum Case {
  kAllAsleep,      // every owner is in FUTEX_WAIT (or past its CAS) first
  kNoneAsleep,     // every owner collects after publish() has returned
  kMix,            // owners arrive before, during and after publish()
  kShortDeadline,  // some owners leave on a 2 ms deadline before publish
  kTwoPublishers,  // results and a fail_all-style publish, disjoint waiters
  kNumCases
};
const char* kCaseName[] = {"all-asleep", "none-asleep", "mix",
                           "short-deadline", "two-publishers"};

enum When : uint8_t { kEarly, kJitter, kAfterPublish };

struct Plan {
  When when = kEarly;
  uint32_t delay_us = 0;
  bool short_deadline = false;
};

struct Round {
  std::vector<std::shared_ptr<W>> ws;
  std::vector<Plan> plan;
  std::vector<int64_t> got;
  std::vector<char> fired;
  std::atomic<uint32_t> published{0};  // owners that collect late sleep on it
  std::atomic<size_t> short_left{0};
};

constexpr auto kLong = std::chrono::seconds(2);
constexpr auto kShort = std::chrono::milliseconds(2);

int64_t expected_value(int c, size_t n, int b, size_t i) {
  return ((int64_t)c << 40) + ((int64_t)n << 24) + (int64_t)b * 4096 +
         (int64_t)i + 1;
}

long g_failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      if (++g_failures <= 20) {          \
        std::fprintf(stderr, "FAIL: ");  \
        std::fprintf(stderr, __VA_ARGS__); \
        std::fprintf(stderr, "\n");      \
      }                                  \
    }                                    \
  } while (0)

void run_case(int c, size_t n, int batches) {
  Round R;
  R.ws.resize(n);
  R.plan.resize(n);
  R.got.resize(n);
  R.fired.resize(n);
  Barrier bar(n + 1);
  std::vector<std::thread> owners;
  owners.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    owners.emplace_back([&, i] {
      for (int b = 0; b < batches; ++b) {
        bar.wait();  // the main thread has prepared batch b
        std::shared_ptr<W> w = R.ws[i];
        Plan p = R.plan[i];
        if (p.when == kAfterPublish) {
          while (R.published.load(std::memory_order_acquire) == 0)
            wake_tree::futex(&R.published, FUTEX_WAIT_PRIVATE, 0, nullptr);
        } else if (p.when == kJitter) {
          if (p.delay_us == 0)
            std::this_thread::yield();
          else
            std::this_thread::sleep_for(
                std::chrono::microseconds(p.delay_us));
        }
        bool ok = p.short_deadline ? wake_tree::await(w.get(), kShort)
                                   : wake_tree::await(w.get(), kLong);
        R.fired[i] = !ok;
        R.got[i] = ok ? w->value : 0;  // no DONE seen: hands off the results
        if (p.short_deadline)
          R.short_left.fetch_add(1, std::memory_order_release);
        bar.wait();  // batch b is over
      }
    });
  }

  std::mt19937 rng(1234567u + (unsigned)c * 7919u + (unsigned)n);
  for (int b = 0; b < batches; ++b) {
    size_t n_short = 0;
    for (size_t i = 0; i < n; ++i) {
      R.ws[i] = std::make_shared<W>();
      Plan p;
      switch (c) {
        case kAllAsleep:
          p.when = kEarly;
          break;
        case kNoneAsleep:
          p.when = kAfterPublish;
          break;
        case kShortDeadline:
          // the root in every third batch, one waiter in four elsewhere
          if ((i == 0 && b % 3 == 0) || rng() % 4 == 0) {
            p.short_deadline = true;
            ++n_short;
            break;
          }
          [[fallthrough]];
        default: {
          unsigned r = rng() % 4;
          p.when = r == 0 ? kEarly : r == 3 ? kAfterPublish : kJitter;
          p.delay_us = r == 1 ? 0 : rng() % 300;
        }
      }
      R.plan[i] = p;
    }
    R.published.store(0, std::memory_order_relaxed);
    R.short_left.store(0, std::memory_order_relaxed);
    g_stretch_us.store(c == kAllAsleep || c == kNoneAsleep ? 0 : 60,
                       std::memory_order_relaxed);
    bar.wait();  // owners start

    if (c == kAllAsleep) {
      for (size_t i = 0; i < n; ++i)
        while (!(R.ws[i]->state.load(std::memory_order_acquire) &
                 wake_tree::SLEEPING))
          std::this_thread::yield();
    } else if (c == kShortDeadline) {
      while (R.short_left.load(std::memory_order_acquire) < n_short)
        std::this_thread::yield();
    } else if (c != kNoneAsleep) {
      std::this_thread::sleep_for(std::chrono::microseconds(rng() % 200));
    }

    auto fill = [&](size_t base) {
      return [&, base](size_t i, W& w) {
        w.value = expected_value(c, n, b, base + i);
      };
    };
    if (c == kTwoPublishers) {
      // the batcher publishes the front half while a fail_all-style
      // publish of defaults runs over the back half
      size_t split = (n + 1) / 2;
      std::thread failer([&] {
        wake_tree::publish(R.ws.data() + split, n - split,
                           [](size_t, W& w) { w.value = -1; });
      });
      wake_tree::publish(R.ws.data(), split, fill(0));
      failer.join();
    } else {
      wake_tree::publish(R.ws.data(), n, fill(0));
    }
    R.published.store(1, std::memory_order_release);
    wake_tree::futex(&R.published, FUTEX_WAKE_PRIVATE, INT32_MAX, nullptr);
    bar.wait();  // owners are back

    size_t fired = 0;
    for (size_t i = 0; i < n; ++i) {
      const Plan& p = R.plan[i];
      fired += R.fired[i] ? 1 : 0;
      CHECK((bool)R.fired[i] == p.short_deadline,
            "%s n=%zu batch %d pos %zu: deadline fired=%d, short=%d",
            kCaseName[c], n, b, i, (int)R.fired[i], (int)p.short_deadline);
      int64_t want =
          p.short_deadline ? 0
          : (c == kTwoPublishers && i >= (n + 1) / 2)
              ? -1
              : expected_value(c, n, b, i);
      CHECK(R.got[i] == want, "%s n=%zu batch %d pos %zu: got %lld want %lld",
            kCaseName[c], n, b, i, (long long)R.got[i], (long long)want);
    }
    CHECK(fired == n_short, "%s n=%zu batch %d: %zu deadlines fired, %zu short",
          kCaseName[c], n, b, fired, n_short);
  }
  for (auto& t : owners) t.join();
}

}  // namespace

int main(int argc, char** argv) {
  int batches = argc > 1 ? std::atoi(argv[1]) : 200;
  const size_t sizes[] = {1, 2, 3, 4, 7, 44, 1024};
  for (int c = 0; c < kNumCases; ++c)
    for (size_t n : sizes) run_case(c, n, batches);
  if (g_failures != 0) {
    std::fprintf(stderr, "wake tree tests FAILED (%ld checks)\n", g_failures);
    return 1;
  }
  std::printf("wake tree tests passed\n");
  return 0;
}
