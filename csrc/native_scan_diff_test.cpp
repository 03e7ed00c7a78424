// Differential test of the two string searches in aigw_core::Scan
// (csrc/native_core.h): every input is scanned once with simd=true and
// once with simd=false, and ok, model, stream, text, the four spans and
// the consumed length must be equal. Built stand-alone with
// -fsanitize=address,undefined by scripts/sanitize_handoff.sh.
//
// Inputs live in exact-size heap allocations (new char[n]) so ASan sees a
// load of even one byte at or past `end`; std::string is not used for
// them because short strings sit inside the object.
//
// usage: native_scan_diff_test [path to the benchmark body fixture]

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "native_core.h"

using aigw_core::Scan;

static int failures = 0;
static long cases = 0;
static long simd_ok = 0;

struct Out {
  bool ok;
  std::string model, text;
  int stream;
  size_t model_vs, model_ve, msgs_vs, msgs_ve, consumed;
  bool operator==(const Out& o) const {
    return ok == o.ok && model == o.model && text == o.text &&
           stream == o.stream && model_vs == o.model_vs &&
           model_ve == o.model_ve && msgs_vs == o.msgs_vs &&
           msgs_ve == o.msgs_ve && consumed == o.consumed;
  }
};

static Out run(const char* p, size_t n, bool simd) {
  Scan sc{p, p + n};
  sc.base = p;
  sc.simd = simd;
  bool ok = sc.parse_value(0, "", true) && sc.ok;
  if (ok) {
    sc.ws();
    ok = sc.p == sc.end;
  }
  return {ok, sc.model, sc.text, sc.stream, sc.model_vs, sc.model_ve,
          sc.msgs_vs, sc.msgs_ve, (size_t)(sc.p - p)};
}

// returns the SIMD result so callers can also pin expected values
static Out diff(const std::string& body) {
  size_t n = body.size();
  char* heap = new char[n];  // exact size: no slack after the last byte
  std::memcpy(heap, body.data(), n);
  Out a = run(heap, n, true);
  Out b = run(heap, n, false);
  delete[] heap;
  ++cases;
  if (a.ok) ++simd_ok;
  if (!(a == b)) {
    ++failures;
    if (failures <= 10)
      std::fprintf(stderr,
                   "MISMATCH n=%zu ok %d/%d consumed %zu/%zu text %zu/%zu: "
                   "%.120s\n",
                   n, a.ok, b.ok, a.consumed, b.consumed, a.text.size(),
                   b.text.size(), body.c_str());
  }
  return a;
}

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

static const char kHead[] = "{\"model\":\"m\",\"messages\":[{\"content\":\"";

// body whose text string holds `inner` (raw JSON string contents) and is
// followed by `tail` bytes up to the buffer end; tail >= 3 closes the JSON
// ("}]}" then spaces), shorter tails leave the body malformed
static std::string wrap(const std::string& inner, size_t tail) {
  std::string s = kHead + inner + "\"";
  static const char close[] = "}]}";
  for (size_t i = 0; i < tail; ++i) s.push_back(i < 3 ? close[i] : ' ');
  return s;
}

static std::string letters(size_t n, size_t seed = 0) {
  std::string s;
  for (size_t i = 0; i < n; ++i) s.push_back((char)('a' + (i + seed) % 26));
  return s;
}

static void test_lengths_and_tails() {
  // string of every length 0..48 ending 0..17 bytes before the buffer end
  // (the closing quote is the byte `tail` positions before the end)
  for (size_t len = 0; len <= 48; ++len)
    for (size_t tail = 0; tail <= 17; ++tail) {
      Out r = diff(wrap(letters(len, tail), tail));
      if (tail >= 3) {
        CHECK(r.ok);
        CHECK(r.text == letters(len, tail) + "\n");
      } else {
        CHECK(!r.ok);
      }
    }
}

static void test_specials_at_every_offset() {
  for (size_t off = 0; off <= 33; ++off)
    for (size_t after = 0; after <= 17; after += (after < 2 ? 1 : 5)) {
      // an escaped quote and an escaped backslash at `off`
      Out r = diff(wrap(letters(off) + "\\\"" + letters(after), 3));
      CHECK(r.ok && r.text == letters(off) + "\"" + letters(after) + "\n");
      r = diff(wrap(letters(off) + "\\\\" + letters(after), 3));
      CHECK(r.ok && r.text == letters(off) + "\\" + letters(after) + "\n");
      // a bare quote at `off` ends the string there: what follows makes
      // the body malformed unless nothing follows
      r = diff(wrap(letters(off) + "\"" + letters(after), 3));
      CHECK(!r.ok);
      // a bare backslash before a letter is an invalid escape
      r = diff(wrap(letters(off) + "\\" + "q" + letters(after), 3));
      CHECK(!r.ok);
    }
}

static void test_escapes_straddling_steps() {
  struct Esc {
    const char* json;
    const char* utf8;
  };
  const Esc kinds[] = {
      {"\\\"", "\""},   {"\\\\", "\\"},  {"\\/", "/"},
      {"\\b", "\b"},    {"\\f", "\f"},   {"\\n", "\n"},
      {"\\r", "\r"},    {"\\t", "\t"},   {"\\u0041", "A"},
      {"\\u00e9", "\xC3\xA9"},           {"\\u20AC", "\xE2\x82\xAC"},
      {"\\uD834\\uDD1E", "\xF0\x9D\x84\x9E"},  // surrogate pair
      {"\\uD834x", "\xED\xA0\xB4x"},           // lone high surrogate
  };
  // pad so the escape starts at every position across two 16-byte steps,
  // measured from the string start and (via the fixed head) the buffer
  for (const Esc& e : kinds)
    for (size_t pad = 0; pad <= 33; ++pad) {
      Out r = diff(wrap(letters(pad) + e.json + letters(20), 3));
      CHECK(r.ok);
      CHECK(r.text == letters(pad) + e.utf8 + letters(20) + "\n");
      // and with no collection (a key outside the messages tree)
      std::string body = "{\"k\":\"" + letters(pad) + e.json + letters(20) +
                         "\",\"model\":\"m\"}";
      r = diff(body);
      CHECK(r.ok && r.text.empty());
    }
}

static void test_unterminated() {
  // the string never closes; 0..17 bytes remain after the last full step
  for (size_t len = 0; len <= 48; ++len) {
    Out r = diff(kHead + letters(len));
    CHECK(!r.ok);
  }
  for (size_t tail = 0; tail <= 17; ++tail) {
    Out r = diff(kHead + letters(32) + "\\n" + letters(tail));
    CHECK(!r.ok);
    r = diff(kHead + letters(16 + tail) + "\\");  // backslash is the last byte
    CHECK(!r.ok);
    r = diff(kHead + letters(16 + tail) + "\\u00");  // cut-off \u
    CHECK(!r.ok);
  }
}

static void test_invalid_escape_positions() {
  // in the 16-byte region (plenty of bytes follow) and in the scalar tail
  CHECK(!diff(wrap(letters(5) + "\\q" + letters(40), 3)).ok);
  CHECK(!diff(wrap(letters(40) + "\\q" + letters(2), 3)).ok);
  CHECK(!diff(wrap(letters(5) + "\\u12G4" + letters(40), 3)).ok);
  CHECK(!diff(wrap(letters(40) + "\\u12G4", 3)).ok);
  CHECK(!diff("{\"k\":\"" + letters(5) + "\\q" + letters(40) + "\"}").ok);
  CHECK(!diff("{\"k\":\"" + letters(40) + "\\q\"}").ok);
}

static void test_high_bytes() {
  // bytes >= 0x80 must compare unequal to '"' and '\\' as signed or
  // unsigned lanes; 0xA2 and 0xDC share low bits with them
  std::string hi;
  for (int c = 0x80; c <= 0xFF; ++c) hi.push_back((char)c);
  Out r = diff(wrap(hi, 3));
  CHECK(r.ok && r.text == hi + "\n");
  for (size_t pad = 0; pad <= 17; ++pad) {
    std::string in = letters(pad) + "\xA2\xDC\xFF\x80" + letters(pad);
    r = diff(wrap(in, 3));
    CHECK(r.ok && r.text == in + "\n");
  }
  // control bytes and NUL pass through the search the same way
  std::string ctl("a\0b\x01\x1f", 5);
  r = diff(wrap(ctl + letters(30), 3));
  CHECK(r.ok && r.text == ctl + letters(30) + "\n");
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint32_t next_rand() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 32);
}

static void fuzz() {
  const char alphabet[] = "{}[]\",:\\utrue falsn0123456789.eE-+\x01\xff\x80 ";
  for (int iter = 0; iter < 20000; ++iter) {
    size_t len = next_rand() % 64;
    std::string body;
    for (size_t i = 0; i < len; ++i)
      body.push_back(alphabet[next_rand() % (sizeof(alphabet) - 1)]);
    diff(body);
  }
  // single-byte mutations of a valid body long enough for several steps
  const std::string valid =
      "{\"model\":\"gpt-4o\",\"stream\":true,\"messages\":[{\"content\":"
      "\"hello \xC3\xA9 the quick brown fox \\n jumps \\u00e9 over\"},"
      "{\"content\":[{\"type\":\"text\",\"text\":\"and a second part\"}]}]}";
  CHECK(diff(valid).ok);
  for (int iter = 0; iter < 20000; ++iter) {
    std::string body = valid;
    size_t pos = next_rand() % body.size();
    body[pos] = (char)(next_rand() % 256);
    diff(body);
  }
}

static void test_benchmark_body(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (f == nullptr) {
    std::fprintf(stderr, "FAIL cannot open %s\n", path);
    ++failures;
    return;
  }
  std::string body;
  char tmp[4096];
  size_t r;
  while ((r = std::fread(tmp, 1, sizeof(tmp), f)) > 0) body.append(tmp, r);
  std::fclose(f);
  Out o = diff(body);
  CHECK(o.ok && o.model == "bench-llm" && o.stream == 0);
  CHECK(o.text.size() > 20000);
  CHECK(o.msgs_ve > o.msgs_vs && o.msgs_ve <= body.size());
  CHECK(o.consumed == body.size());
  // every truncation point near the end and a sample across the body
  for (size_t cut = 1; cut <= 40 && cut < body.size(); ++cut)
    CHECK(!diff(body.substr(0, body.size() - cut)).ok);
  for (size_t cut = 0; cut < body.size(); cut += 997)
    diff(body.substr(0, cut));
}

int main(int argc, char** argv) {
  if (argc > 1) test_benchmark_body(argv[1]);
  test_lengths_and_tails();
  test_specials_at_every_offset();
  test_escapes_straddling_steps();
  test_unterminated();
  test_invalid_escape_positions();
  test_high_bytes();
  fuzz();
  if (failures) {
    std::fprintf(stderr, "%d failure(s) in %ld cases\n", failures, cases);
    return 1;
  }
#if defined(__SSE2__)
  const char* mode = "sse2";
#else
  const char* mode = "scalar only";
#endif
  std::printf("native scan diff passed: %ld cases (%ld accepted), %s\n", cases,
              simd_ok, mode);
  return 0;
}
