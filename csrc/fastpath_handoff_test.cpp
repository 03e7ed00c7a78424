// Content check of the request-text handoff through the native server
// (csrc/fastpath.cpp): ConnHandler body read -> Scan -> Waiter2-owned
// text -> DirectGpuBatcher take/pack -> staging. Built stand-alone by
// scripts/sanitize_handoff.sh with -fsanitize=address,undefined.
//
// Unlike the fake in fastpath_sanitize_test.cpp this fake admission
// looks at the bytes: admission_submit sets each request's count to a
// 31-bit FNV-1a of that request's bytes in admission_staging(set). The
// test computes the same hash over the text it expects the server to have
// extracted and requires stats().gpu_tokens to equal the sum. The sum is
// order-independent, and a torn, stale, truncated or misplaced text
// changes it.

#include <arpa/inet.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <sys/socket.h>
#include <sys/time.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "fastpath.h"

static uint32_t fnv31(const char* p, size_t n) {
  uint32_t h = 2166136261u;
  for (size_t i = 0; i < n; ++i) {
    h ^= (unsigned char)p[i];
    h *= 16777619u;
  }
  return h & 0x7fffffffu;
}

namespace aigw_fast {
class GpuAdmissionDirect {
 public:
  struct FakeSet {
    std::vector<int32_t> counts;
    std::vector<char> staging;
    int n_req = 0;
  };
  FakeSet sets[2];
};
GpuAdmissionDirect* admission_create(const long long*, const int32_t*, int,
                                     size_t max_bytes, int, int) {
  auto* a = new GpuAdmissionDirect();
  a->sets[0].staging.resize(max_bytes);
  a->sets[1].staging.resize(max_bytes);
  return a;
}
char* admission_staging(GpuAdmissionDirect* a, int set) {
  return a->sets[set].staging.data();
}
bool admission_submit(GpuAdmissionDirect* a, int set, const char*, size_t n,
                      const int64_t* offsets, int n_req, const int32_t*) {
  auto& s = a->sets[set];
  if (n > s.staging.size()) return false;
  s.counts.assign((size_t)n_req, 0);
  s.n_req = n_req;
  for (int i = 0; i < n_req; ++i) {
    long long b = offsets[i];
    long long e = (i + 1 < n_req) ? offsets[i + 1] : (long long)n;
    if (b < 0 || e < b || (size_t)e > n) return false;
    s.counts[(size_t)i] =
        (int32_t)fnv31(s.staging.data() + b, (size_t)(e - b));
  }
  return true;
}
bool admission_wait(GpuAdmissionDirect* a, int set, int n_req,
                    int32_t* counts_out, int32_t* rows_out,
                    float* scores_out) {
  std::this_thread::sleep_for(std::chrono::microseconds(100));
  auto& s = a->sets[set];
  if (s.n_req != n_req) return false;
  for (int i = 0; i < n_req; ++i) {
    counts_out[i] = s.counts[(size_t)i];
    if (rows_out != nullptr) rows_out[i] = -1;
    if (scores_out != nullptr) scores_out[i] = 0.f;
  }
  // scribble over the consumed staging so a later batch that failed to
  // pack a text cannot pass by finding the old bytes still there
  std::memset(s.staging.data(), 0xEE, s.staging.size());
  return true;
}
bool admission_count(GpuAdmissionDirect* a, const char* bytes, size_t n,
                     const int64_t* offsets, int n_req, int32_t* counts_out) {
  return admission_submit(a, 0, bytes, n, offsets, n_req, nullptr) &&
         admission_wait(a, 0, n_req, counts_out, nullptr, nullptr);
}
bool admission_init_cache(GpuAdmissionDirect*, const uint16_t*, int,
                          const uint16_t*, int, long long, float, int, bool) {
  return false;
}
bool admission_count_lookup(GpuAdmissionDirect* a, const char* bytes, size_t n,
                            const int64_t* offsets, int n_req,
                            int32_t* counts_out, const int32_t*,
                            int32_t* rows_out, float* scores_out) {
  return admission_submit(a, 0, bytes, n, offsets, n_req, nullptr) &&
         admission_wait(a, 0, n_req, counts_out, rows_out, scores_out);
}
long long admission_cache_insert(GpuAdmissionDirect*, int) { return -1; }
void admission_destroy(GpuAdmissionDirect* a) { delete a; }
}  // namespace aigw_fast

using namespace aigw_fast;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

static const size_t kLens[] = {1, 15, 16, 17, 4096, 30000};

// the text the server must extract for (conn, seq): `len` bytes, the last
// one the '\n' the scanner appends after a message's content
static std::string expected_text(int conn, int seq, size_t len, bool esc) {
  std::string t;
  char tag[48];
  int tn = std::snprintf(tag, sizeof(tag), "c%d-s%d:", conn, seq);
  for (size_t i = 0; i + 1 < len; ++i) {
    if (i < (size_t)tn && len > (size_t)tn + 1)
      t.push_back(tag[i]);
    else
      t.push_back((char)('a' + (i * 7 + (size_t)conn * 3 + (size_t)seq) % 26));
  }
  if (esc && t.size() >= 12) {
    // characters the body has to escape; placed around a 16-byte step
    size_t m = t.size() >= 40 ? 14 : t.size() - 6;
    t[m] = '"';
    t[m + 1] = '\\';
    t[m + 2] = '\n';
    t[m + 3] = '\xC3';  // U+00E9, sent as é
    t[m + 4] = '\xA9';
    t[t.size() - 1] = '\t';
  }
  t.push_back('\n');
  return t;
}

static std::string request_for(const std::string& text, bool stream) {
  std::string content;
  for (size_t i = 0; i + 1 < text.size(); ++i) {
    unsigned char c = (unsigned char)text[i];
    if (c == '"') content += "\\\"";
    else if (c == '\\') content += "\\\\";
    else if (c == '\n') content += "\\n";
    else if (c == '\t') content += "\\t";
    else if (c == 0xC3 && (unsigned char)text[i + 1] == 0xA9) {
      content += "\\u00e9";
      ++i;
    } else content.push_back((char)c);
  }
  std::string body = std::string("{\"model\":\"model-a\",") +
                     (stream ? "\"stream\":true," : "") +
                     "\"messages\":[{\"role\":\"user\",\"content\":\"" +
                     content + "\"}]}";
  return "POST /v1/chat/completions HTTP/1.1\r\nhost: t\r\n"
         "content-type: application/json\r\ncontent-length: " +
         std::to_string(body.size()) + "\r\n\r\n" + body;
}

static int connect_to(int port) {
  int fd = ::socket(AF_INET, SOCK_STREAM, 0);
  if (fd < 0) return -1;
  struct sockaddr_in a;
  std::memset(&a, 0, sizeof(a));
  a.sin_family = AF_INET;
  a.sin_port = htons((uint16_t)port);
  inet_pton(AF_INET, "127.0.0.1", &a.sin_addr);
  if (::connect(fd, (struct sockaddr*)&a, sizeof(a)) != 0) {
    ::close(fd);
    return -1;
  }
  int one = 1;
  setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));
  struct timeval tv = {10, 0};  // a lost reply fails the test, never hangs it
  setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof(tv));
  setsockopt(fd, SOL_SOCKET, SO_SNDTIMEO, &tv, sizeof(tv));
  return fd;
}

static bool send_all(int fd, const std::string& s) {
  size_t off = 0;
  while (off < s.size()) {
    ssize_t w = ::send(fd, s.data() + off, s.size() - off, MSG_NOSIGNAL);
    if (w <= 0) return false;
    off += (size_t)w;
  }
  return true;
}

// reads one response off `fd` (left-over bytes stay in *buf); returns the
// status code, or -1 on a broken connection
static int read_response(int fd, std::string* buf) {
  char tmp[8192];
  size_t he;
  while ((he = buf->find("\r\n\r\n")) == std::string::npos) {
    ssize_t r = ::recv(fd, tmp, sizeof(tmp), 0);
    if (r <= 0) return -1;
    buf->append(tmp, (size_t)r);
  }
  std::string head = buf->substr(0, he + 4);
  for (auto& c : head) c = (char)std::tolower((unsigned char)c);
  int status = std::atoi(head.c_str() + 9);
  size_t total;
  if (head.find("transfer-encoding: chunked") != std::string::npos) {
    size_t end;
    while ((end = buf->find("\r\n0\r\n\r\n", he + 2)) == std::string::npos) {
      ssize_t r = ::recv(fd, tmp, sizeof(tmp), 0);
      if (r <= 0) return -1;
      buf->append(tmp, (size_t)r);
    }
    total = end + 7;
  } else {
    size_t cl = head.find("content-length:");
    size_t n = cl == std::string::npos
                   ? 0
                   : (size_t)std::atoll(head.c_str() + cl + 15);
    total = he + 4 + n;
    while (buf->size() < total) {
      ssize_t r = ::recv(fd, tmp, sizeof(tmp), 0);
      if (r <= 0) return -1;
      buf->append(tmp, (size_t)r);
    }
  }
  buf->erase(0, total);
  return status;
}

static FastRoute make_route(int port) {
  FastRoute r;
  r.name = "r";
  r.model_match = "model-a";
  r.retries = 0;
  r.has_costs = true;
  FastBackend be;
  be.name = "live";
  be.host = "127.0.0.1";
  be.port = (uint16_t)port;
  be.bearer = "sk-test";
  r.backends.push_back(be);
  return r;
}

struct Drive {
  std::atomic<uint64_t> expect{0};
  std::atomic<uint64_t> ok{0};
  std::atomic<uint64_t> bad{0};
};

// `conns` connections x `per_conn` requests of distinct texts; every
// eighth text has escapes; lengths cycle through `n_lens` of kLens
static void drive(int port, int conns, int per_conn, size_t n_lens,
                  bool stream, Drive* d, bool tolerate_errors = false) {
  std::vector<std::thread> th;
  for (int c = 0; c < conns; ++c)
    th.emplace_back([=] {
      int fd = connect_to(port);
      if (fd < 0) {
        d->bad++;
        return;
      }
      std::string rbuf;
      for (int s = 0; s < per_conn; ++s) {
        size_t len = kLens[(size_t)(s + c) % n_lens];
        std::string text = expected_text(c, s, len, (s + c) % 8 == 0);
        if (!send_all(fd, request_for(text, stream)) ||
            read_response(fd, &rbuf) != 200) {
          d->bad++;
          if (tolerate_errors) break;
          continue;
        }
        d->expect += fnv31(text.data(), text.size());
        d->ok++;
      }
      ::close(fd);
    });
  for (auto& t : th) t.join();
}

static void start_gpu(FastServer& srv, int max_batch, size_t max_bytes) {
  std::vector<long long> hk(16, -1);
  std::vector<int32_t> hr(16, -1);
  srv.enable_gpu_direct(hk.data(), hr.data(), 16, max_batch, max_bytes, 512, 0);
}

int main() {
  std::string body =
      "{\"id\":\"x\",\"object\":\"chat.completion\",\"choices\":[],"
      "\"usage\":{\"prompt_tokens\":5,\"completion_tokens\":2,"
      "\"total_tokens\":7}}";
  std::string canned = "HTTP/1.1 200 OK\r\ncontent-type: application/json\r\n"
                       "content-length: " +
                       std::to_string(body.size()) + "\r\n\r\n" + body;
  FastMock mock;
  int up_port = mock.start("127.0.0.1", canned);

  std::string ev =
      "data: {\"id\":\"x\",\"object\":\"chat.completion.chunk\",\"choices\":"
      "[{\"index\":0,\"delta\":{\"content\":\"hi\"}}]}\n\n"
      "data: {\"id\":\"x\",\"object\":\"chat.completion.chunk\",\"choices\":[],"
      "\"usage\":{\"prompt_tokens\":5,\"completion_tokens\":2,"
      "\"total_tokens\":7}}\n\ndata: [DONE]\n\n";
  char hex[16];
  std::snprintf(hex, sizeof(hex), "%zx", ev.size());
  std::string canned_sse =
      "HTTP/1.1 200 OK\r\ncontent-type: text/event-stream\r\n"
      "transfer-encoding: chunked\r\n\r\n" +
      std::string(hex) + "\r\n" + ev + "\r\n0\r\n\r\n";
  FastMock sse_mock;
  int sse_port = sse_mock.start("127.0.0.1", canned_sse);

  // 1. whole-queue swap branch: 8 connections never exceed the limits
  {
    FastServer srv;
    srv.add_route(make_route(up_port));
    start_gpu(srv, 256, 1 << 20);
    int port = srv.start("127.0.0.1", 0);
    Drive d;
    drive(port, 8, 200, 6, false, &d);
    CHECK(d.bad.load() == 0 && d.ok.load() == 1600);
    CHECK(srv.stats().gpu_tokens.load() == d.expect.load());
    CHECK(srv.gpu_direct_stats()[1] == 1600);  // texts
    CHECK(srv.gpu_direct_stats()[4] == 0);     // errors
    CHECK(srv.drain(2.0) == 0);
    srv.stop();
  }

  // 2. partial-take branch: max_batch 4 under 8 connections, and a byte
  // limit that two 30 000-byte texts fit but three do not
  {
    FastServer srv;
    srv.add_route(make_route(up_port));
    start_gpu(srv, 4, 70000);
    int port = srv.start("127.0.0.1", 0);
    Drive d;
    drive(port, 8, 200, 6, false, &d);
    CHECK(d.bad.load() == 0 && d.ok.load() == 1600);
    CHECK(srv.stats().gpu_tokens.load() == d.expect.load());
    std::vector<uint64_t> gs = srv.gpu_direct_stats();
    CHECK(gs.size() == 9 && gs[1] == 1600 && gs[4] == 0);
    CHECK(gs[0] >= 400);  // at most 4 texts per batch

    // two pipelined requests in one write on a fresh connection
    uint64_t before = srv.stats().gpu_tokens.load();
    std::string t1 = expected_text(90, 1, 4096, true);
    std::string t2 = expected_text(90, 2, 17, false);
    int fd = connect_to(port);
    CHECK(fd >= 0);
    std::string rbuf;
    CHECK(send_all(fd, request_for(t1, false) + request_for(t2, false)));
    CHECK(read_response(fd, &rbuf) == 200);
    CHECK(read_response(fd, &rbuf) == 200);
    ::close(fd);
    CHECK(srv.stats().gpu_tokens.load() - before ==
          (uint64_t)fnv31(t1.data(), t1.size()) + fnv31(t2.data(), t2.size()));
    CHECK(srv.drain(2.0) == 0);
    srv.stop();
  }

  // 3. streamed requests through a chunked mock: enqueue before the
  // upstream dispatch, collect at stream end
  {
    FastServer srv;
    srv.add_route(make_route(sse_port));
    start_gpu(srv, 256, 1 << 20);
    int port = srv.start("127.0.0.1", 0);
    Drive d;
    drive(port, 8, 48, 6, true, &d);
    CHECK(d.bad.load() == 0 && d.ok.load() == 8 * 48);
    // the count is collected after the last chunk went out, so a
    // connection's final request is only accounted once it has drained
    CHECK(srv.drain(2.0) == 0);
    CHECK(srv.stats().gpu_tokens.load() == d.expect.load());
    srv.stop();
  }

  // 4. stop() with batches in flight: clients see broken connections,
  // every waiter is fulfilled exactly once, nothing hangs or leaks
  {
    FastServer srv;
    srv.add_route(make_route(up_port));
    start_gpu(srv, 4, 1 << 20);
    int port = srv.start("127.0.0.1", 0);
    Drive d;
    std::thread load(
        [&] { drive(port, 8, 100000, 6, false, &d, true); });
    while (d.ok.load() < 200)
      std::this_thread::sleep_for(std::chrono::milliseconds(1));
    srv.stop();
    load.join();
    CHECK(d.ok.load() >= 200);
  }

  sse_mock.stop();
  mock.stop();
  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("fastpath handoff tests passed\n");
  return 0;
}
