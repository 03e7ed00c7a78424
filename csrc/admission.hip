// Torch-free GPU admission path for the native fast front.
//
// The round-1 serving design shipped every chat text to a Python GPU
// service over UDS (msgpack) for BPE token counting; measured on
// hardware, one host process decodes ~900 MB/s and sharding hosts
// thrashes GPU contexts (4 processes: 36k -> 10k req/s). This module
// removes the whole detour: the C++ gateway owns ONE HIP stream and
// launches the same gfx950 BPE kernels (csrc/bpe_kernels.cuh) directly —
// pack texts into a pinned staging buffer, one H2D copy, the sync-free
// segmentation/scan/merge pipeline (device-resident totals, every kernel
// self-bounds), one D2H of per-request counts, one event wait. Zero
// Python, zero IPC, zero extra GPU contexts.
//
// The merge table is supplied by the caller (aigw.ops.tokenizer
// make_merges) so counts stay bit-identical to the Python/CPU oracle.
//
// Reference parity anchor: the reference does NOT tokenize locally —
// token accounting comes from provider usage JSON
// (translator/openai_openai.go:185-223) and /tokenize passes through to
// the backend (translator/tokenize.go:24-81). This module is the
// MI355X-native replacement BASELINE.json demands: gateway-side GPU
// token accounting feeding the same llm_*_token cost metadata.

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "bpe_kernels.cuh"
#include "cache_kernels.cuh"

namespace aigw_fast {

namespace {

// Exclusive block-scan over int32 counts with the total appended:
// single-block Hillis-Steele over 256-element chunks with a running
// carry. The input is per-256-byte-block flag counts (<= ~256k entries
// for a 64 MiB batch) — microseconds of work on one CU, and keeping it
// on-device is what keeps the pipeline free of host syncs.
__global__ void excl_scan_kernel(const int32_t* __restrict__ in, int n,
                                 int32_t* __restrict__ excl,
                                 int32_t* __restrict__ total) {
  // wave-level scan: 6 shfl_up rounds per 64-wide wave (no syncs),
  // wave totals staged through LDS, TWO barriers per 256-element chunk.
  // The previous LDS Hillis-Steele spent 16 barriers per chunk and
  // measured ~12 us per 4k-element call (3 calls per admission batch).
  __shared__ int32_t wave_sum[4];
  __shared__ int32_t carry_s;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  int lane = (int)threadIdx.x & 63;
  int wave = (int)threadIdx.x >> 6;
  for (int base = 0; base < n; base += 256) {
    int i = base + (int)threadIdx.x;
    int32_t orig = (i < n) ? in[i] : 0;
    int32_t v = orig;
    for (int off = 1; off < 64; off <<= 1) {
      int32_t t = __shfl_up(v, off);
      if (lane >= off) v += t;
    }
    if (lane == 63) wave_sum[wave] = v;
    __syncthreads();
    int32_t wave_off = 0;
    for (int w = 0; w < wave; ++w) wave_off += wave_sum[w];
    if (i < n) excl[i] = carry_s + wave_off + v - orig;  // exclusive
    int32_t chunk_total =
        wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
    __syncthreads();  // wave_sum reused next chunk; carry_s update below
    if (threadIdx.x == 0) carry_s += chunk_total;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry_s;
}

__global__ void f32_to_bf16_kernel(const float* __restrict__ in,
                                   bf16* __restrict__ out, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (bf16)in[i];
}

// Token-position flags for the compaction that feeds the token-dense
// meanpool: out_ids is pre-filled with -1 on the cache path, so byte
// position i carries a token iff out_ids[i] >= 0.
__global__ void tok_flags_kernel(const int32_t* __restrict__ out_ids, int n,
                                 uint8_t* __restrict__ flags) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flags[i] = out_ids[i] >= 0;
}

// Token-dense meanpool: iterate the COMPACTED token list (ghead[j] =
// byte position of token j, request r owns [req_excl[r],
// req_excl[r]+counts[r])) instead of scanning every byte for -1 holes.
// submit_cache() builds that list (it reuses the group-head buffer once
// the BPE kernel has consumed the group heads).
// The byte-indexed version (cache_kernels.cuh meanpool_accum_kernel,
// still used by the torch-tensor path) walked ~25k bytes per request to
// touch ~4k tokens and measured 808 us/batch = 63% of cache-mode GPU
// time; this walks the 4k tokens directly.
__global__ void meanpool_tokens_kernel(
    const int32_t* __restrict__ ids, const int32_t* __restrict__ ghead,
    const int32_t* __restrict__ req_excl, const int32_t* __restrict__ counts,
    int n_req, const bf16* __restrict__ emb, int dim, int P,
    float* __restrict__ out, int32_t* __restrict__ cnt) {
  // Block (r, p) owns a CONTIGUOUS chunk of request r's tokens. The
  // chunk's (ghead -> ids) indirections are staged through LDS by 64
  // threads in parallel, so the embedding-row gathers in the inner loop
  // have no dependent-load chain and the compiler can keep many in
  // flight — the strided two-chain version measured 549 us/batch
  // (344 GB/s, 4% of HBM peak) with this kernel as 54% of cache-mode
  // GPU time.
  // Launched with dim/2 threads: each thread owns a PAIR of columns
  // loaded as one 4-byte bfloat16x2 (the scalar version was VALU-bound
  // per the PMC counters — the embedding table is L2-resident — so
  // halving the instruction stream is the lever, not bandwidth).
  constexpr int STAGE = 128;
  __shared__ int32_t tok_ids[STAGE];
  int r = blockIdx.x;
  int p = blockIdx.y;
  if (r >= n_req) return;
  int dim2 = dim >> 1;
  int col2 = threadIdx.x;
  int s = req_excl[r], c = counts[r];
  int chunk = (c + P - 1) / P;
  int j0 = p * chunk;
  int j1 = j0 + chunk;
  if (j1 > c) j1 = c;
  const uint32_t* emb2 = reinterpret_cast<const uint32_t*>(emb);
  float acc_lo = 0.f, acc_hi = 0.f;
  int n = 0;
  for (int base = j0; base < j1; base += STAGE) {
    if (threadIdx.x < STAGE && base + (int)threadIdx.x < j1)
      tok_ids[threadIdx.x] = ids[ghead[s + base + threadIdx.x]];
    __syncthreads();
    int here = j1 - base < STAGE ? j1 - base : STAGE;
    if (col2 < dim2) {
      for (int q = 0; q < here; ++q) {
        int tok = tok_ids[q];
        if (tok < 0) continue;
        uint32_t v = emb2[(long long)tok * dim2 + col2];
        bf16 lo, hi;
        uint16_t vlo = (uint16_t)(v & 0xffffu), vhi = (uint16_t)(v >> 16);
        memcpy(&lo, &vlo, 2);
        memcpy(&hi, &vhi, 2);
        acc_lo += __bfloat162float(lo);
        acc_hi += __bfloat162float(hi);
        ++n;
      }
    }
    __syncthreads();
  }
  if (col2 < dim2 && n) {
    atomicAdd(&out[(long long)r * dim + 2 * col2], acc_lo);
    atomicAdd(&out[(long long)r * dim + 2 * col2 + 1], acc_hi);
    if (col2 == 0) atomicAdd(&cnt[r], n);
  }
}

// bf16 -> OCP e4m3 via the gfx950 packed-convert instruction (the same
// format torch.float8_e4m3fn uses on this architecture, so the fp8
// index is interchangeable with the Python cache's)
// scatter the batch's query vectors into their pending-pool slots in
// ONE launch (a per-request hipMemcpyAsync costs ~10 us of enqueue CPU
// each; at 100 misses/batch that dominated the whole cache batch)
__global__ void park_pending_kernel(const bf16* __restrict__ q,
                                    const int32_t* __restrict__ slots,
                                    int n_req, int dim,
                                    bf16* __restrict__ pending) {
  int r = blockIdx.x;
  int col = threadIdx.x;
  if (r >= n_req || col >= dim) return;
  int slot = slots[r];
  if (slot < 0) return;
  pending[(size_t)slot * dim + col] = q[(size_t)r * dim + col];
}

__global__ void bf16_to_fp8_kernel(const bf16* __restrict__ in,
                                   uint8_t* __restrict__ out, int n) {
  int i = (blockIdx.x * blockDim.x + threadIdx.x) * 2;
  if (i >= n) return;
  float a = (float)in[i];
  float b = (i + 1 < n) ? (float)in[i + 1] : 0.f;
  int packed = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  out[i] = (uint8_t)(packed & 0xff);
  if (i + 1 < n) out[i + 1] = (uint8_t)((packed >> 8) & 0xff);
}

#define HIP_OK(expr)                                                   \
  do {                                                                 \
    hipError_t _e = (expr);                                            \
    if (_e != hipSuccess) {                                            \
      fprintf(stderr, "aigw admission: %s failed: %s\n", #expr,        \
              hipGetErrorString(_e));                                  \
      return false;                                                    \
    }                                                                  \
  } while (0)

}  // namespace

// One instance per fast server; init once. TWO batch sets on TWO
// streams let the batcher keep one batch on the GPU while it packs,
// fulfills, and submits the next (classic copy/compute overlap — the
// per-batch pipeline is launch-bound, so overlapping whole batches
// nearly doubles admission throughput).
class GpuAdmissionDirect {
 public:
  static constexpr int kSets = 2;

  struct BatchSet {
    hipStream_t stream{};
    hipEvent_t event{};
    char* h_bytes = nullptr;
    int64_t* h_off = nullptr;
    int32_t* h_counts = nullptr;
    unsigned long long* h_best = nullptr;
    int32_t* h_slots = nullptr;
    uint8_t* d_bytes = nullptr;
    int64_t* d_off = nullptr;
    uint8_t* d_flags = nullptr;
    uint8_t* d_gflags = nullptr;
    int32_t* d_blk = nullptr;
    int32_t* d_excl = nullptr;
    int32_t* d_totals = nullptr;
    int32_t* d_seg_start = nullptr;
    int32_t* d_seg_req = nullptr;
    int32_t* d_ghead = nullptr;
    int32_t* d_out_ids = nullptr;
    int32_t* d_counts = nullptr;
    int32_t* d_req_excl = nullptr;
    // cache-pipeline intermediates (allocated by init_cache)
    float* d_pool = nullptr;
    int32_t* d_poolcnt = nullptr;
    bf16* d_poolbf = nullptr;
    float* d_gout = nullptr;
    bf16* d_q = nullptr;
    uint8_t* d_q8 = nullptr;
    unsigned long long* d_best = nullptr;
    int32_t* d_slots = nullptr;
    long long rows_in_flight = 0;  // index rows visible to this batch
  };

  bool init(const long long* htab_keys, const int32_t* htab_rank, int htab_n,
            size_t max_bytes, int max_req, int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return false;
    device_ = device >= 0 && device < count ? device : 0;
    HIP_OK(hipSetDevice(device_));
    max_bytes_ = max_bytes;
    max_req_ = max_req;
    htab_mask_ = htab_n - 1;
    HIP_OK(hipMalloc(&d_htab_keys_, sizeof(long long) * htab_n));
    HIP_OK(hipMalloc(&d_htab_rank_, sizeof(int32_t) * htab_n));
    HIP_OK(hipMemcpy(d_htab_keys_, htab_keys, sizeof(long long) * htab_n,
                     hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_htab_rank_, htab_rank, sizeof(int32_t) * htab_n,
                     hipMemcpyHostToDevice));
    int max_blocks = (int)((max_bytes + 255) / 256);
    for (int s = 0; s < kSets; ++s) {
      BatchSet& b = sets_[s];
      HIP_OK(hipStreamCreateWithFlags(&b.stream, hipStreamNonBlocking));
      // hipEventBlockingSync: the batcher thread YIELDS while the batch
      // runs instead of busy-spinning — the serving container is
      // CPU-quota bound, so a spinning core is ~6% of the budget
      HIP_OK(hipEventCreateWithFlags(
          &b.event, hipEventDisableTiming | hipEventBlockingSync));
      HIP_OK(hipHostMalloc(&b.h_bytes, max_bytes, hipHostMallocDefault));
      HIP_OK(hipHostMalloc(&b.h_off, sizeof(int64_t) * (max_req + 1),
                           hipHostMallocDefault));
      HIP_OK(hipHostMalloc(&b.h_counts, sizeof(int32_t) * max_req,
                           hipHostMallocDefault));
      HIP_OK(hipMalloc(&b.d_bytes, max_bytes));
      HIP_OK(hipMalloc(&b.d_off, sizeof(int64_t) * (max_req + 1)));
      HIP_OK(hipMalloc(&b.d_flags, max_bytes));
      HIP_OK(hipMalloc(&b.d_gflags, max_bytes));
      HIP_OK(hipMalloc(&b.d_blk, sizeof(int32_t) * max_blocks));
      HIP_OK(hipMalloc(&b.d_excl, sizeof(int32_t) * max_blocks));
      HIP_OK(hipMalloc(&b.d_totals, sizeof(int32_t) * 2));
      HIP_OK(hipMalloc(&b.d_seg_start, sizeof(int32_t) * max_bytes));
      HIP_OK(hipMalloc(&b.d_seg_req, sizeof(int32_t) * max_bytes));
      HIP_OK(hipMalloc(&b.d_ghead, sizeof(int32_t) * max_bytes));
      HIP_OK(hipMalloc(&b.d_out_ids, sizeof(int32_t) * max_bytes));
      HIP_OK(hipMalloc(&b.d_counts, sizeof(int32_t) * max_req));
      // +1: the excl-scan total lands at d_req_excl[max_req]
      HIP_OK(hipMalloc(&b.d_req_excl, sizeof(int32_t) * (max_req + 1)));
    }
    ready_ = true;
    return true;
  }

  // texts: concatenated; offsets[i] is text i's start (n_req entries,
  // matching the kernel contract in aigw/ops/tokenizer.py pack()).
  // Synchronous single-set wrapper (kept for the GPU-off fallbacks and
  // simple callers); the pipelined batcher uses submit()/wait_set().
  bool count(const char* bytes, size_t n, const int64_t* offsets, int n_req,
             int32_t* counts_out) {
    if (!submit(0, bytes, n, offsets, n_req, nullptr)) return false;
    return wait_set(0, n_req, counts_out, nullptr, nullptr);
  }

  // Launch one batch on set `s` (H2D + BPE + optional cache pipeline when
  // pending_slots != nullptr and the cache is on), then record its event.
  // The caller owns set rotation: a set must be wait_set()ed before reuse.
  bool submit(int s, const char* bytes, size_t n, const int64_t* offsets,
              int n_req, const int32_t* pending_slots) {
    if (!ready_ || n == 0 || n_req == 0 || n > max_bytes_ || n_req > max_req_)
      return false;
    BatchSet& b = sets_[s];
    // launches follow the CALLER thread's current device; the batcher
    // thread differs from the init thread, so pin it here (no-op when
    // already current) — rank N of an 8-GPU node must stay on device N
    HIP_OK(hipSetDevice(device_));
    // bytes == nullptr: the caller packed straight into staging(s)
    // (skips a ~125 us memcpy of a 2.5 MB batch — most of the submit
    // phase by stats_submit_us)
    if (bytes != nullptr) memcpy(b.h_bytes, bytes, n);
    memcpy(b.h_off, offsets, sizeof(int64_t) * (size_t)n_req);
    hipStream_t st = b.stream;
    HIP_OK(hipMemcpyAsync(b.d_bytes, b.h_bytes, n, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(b.d_off, b.h_off, sizeof(int64_t) * (size_t)n_req,
                          hipMemcpyHostToDevice, st));
    int blocks = (int)((n + 255) / 256);
    // fused front end: class-rule flags + forced request starts + block
    // counts in one pass; it also zeroes d_counts for the BPE kernel
    hipLaunchKernelGGL(seg_flags_count_kernel, dim3(blocks), dim3(256), 0, st,
                       b.d_bytes, (int)n, b.d_off, n_req, b.d_flags, b.d_blk,
                       b.d_counts);
    hipLaunchKernelGGL(excl_scan_kernel, dim3(1), dim3(256), 0, st,
                       b.d_blk, blocks, b.d_excl, b.d_totals);
    hipLaunchKernelGGL(seg_write_kernel, dim3(blocks), dim3(256), 0, st,
                       b.d_flags, (int)n, b.d_excl, b.d_off, n_req,
                       b.d_seg_start, b.d_seg_req);
    // groups (device-bounded; every gflags[i < n] is written, 0 beyond
    // n_segs, so the buffer needs no clearing)
    hipLaunchKernelGGL(group_flags_count_kernel, dim3(blocks), dim3(256), 0,
                       st, b.d_seg_start, b.d_seg_req, b.d_totals, b.d_off,
                       (int)n, b.d_gflags, b.d_blk);
    hipLaunchKernelGGL(excl_scan_kernel, dim3(1), dim3(256), 0, st,
                       b.d_blk, blocks, b.d_excl, b.d_totals + 1);
    hipLaunchKernelGGL(flag_compact_write_kernel, dim3(blocks), dim3(256), 0,
                       st, b.d_gflags, (int)n, b.d_excl, b.d_ghead);
    bool want_cache = pending_slots != nullptr && cache_on_;
    // the cache pipeline finds tokens by out_ids >= 0: merged-away byte
    // positions must read -1, not whatever the previous batch left there
    if (want_cache)
      HIP_OK(hipMemsetAsync(b.d_out_ids, 0xFF, sizeof(int32_t) * n, st));
    long long group_bound = (long long)n / 32 + n_req + 1;
    // 8 groups per block: the kernel sums a block's token counts per
    // request before its atomicAdd, and the atomics on the few d_counts
    // words, not the merge loop, were what set its duration at one per
    // wave (profiles/admission_cycle.md: 256/512/1024 threads measured)
    constexpr int kBpeBlock = 512;
    constexpr int kGroupsPerBlock = kBpeBlock / 64;
    int blocks2 = (int)((group_bound + kGroupsPerBlock - 1) / kGroupsPerBlock);
    hipLaunchKernelGGL(bpe_encode_grouped_dev_kernel, dim3(blocks2),
                       dim3(kBpeBlock), 0, st, b.d_bytes, b.d_seg_start, b.d_seg_req,
                       b.d_totals, (int)n, b.d_ghead, b.d_totals + 1,
                       d_htab_keys_, d_htab_rank_, htab_mask_, b.d_out_ids,
                       b.d_counts);
    if (want_cache) {
      if (!submit_cache(b, n, n_req, pending_slots)) return false;
    }
    HIP_OK(hipMemcpyAsync(b.h_counts, b.d_counts, sizeof(int32_t) * n_req,
                          hipMemcpyDeviceToHost, st));
    HIP_OK(hipEventRecord(b.event, st));
    return true;
  }

  // Block until set `s` finishes; copy out counts (and lookup results
  // when the batch ran the cache pipeline and rows/scores != nullptr).
  bool wait_set(int s, int n_req, int32_t* counts_out, int32_t* rows_out,
                float* scores_out) {
    BatchSet& b = sets_[s];
    HIP_OK(hipEventSynchronize(b.event));
    memcpy(counts_out, b.h_counts, sizeof(int32_t) * (size_t)n_req);
    if (rows_out != nullptr && scores_out != nullptr) {
      long long rows_now = b.rows_in_flight;
      for (int i = 0; i < n_req; ++i) {
        rows_out[i] = -1;
        scores_out[i] = 0.f;
        if (rows_now > 0) {
          unsigned long long u = b.h_best[i];
          unsigned hi = (unsigned)(u >> 32);
          unsigned bits = (hi >= 0x80000000u) ? (hi ^ 0x80000000u) : ~hi;
          float score;
          memcpy(&score, &bits, 4);
          if (score >= threshold_) {
            rows_out[i] = (int32_t)(u & 0xFFFFFFFFu);
            scores_out[i] = score;
          }
        }
      }
    }
    return true;
  }

  // ---- semantic cache (native path) ---------------------------------------
  //
  // Same pipeline as aigw/ops/semcache.py embed/lookup, launched on the
  // admission stream right after the BPE batch: meanpool(out_ids) ->
  // bf16 cast -> MFMA projection GEMM -> l2norm -> fused cosine/argmax
  // over the HBM-resident index. Query vectors are parked in a pending
  // pool so a later insert (after the upstream 200) can append them to
  // the index without keeping the batch buffers alive.

  // pinned staging buffer of set s: the batcher may pack request text
  // straight into it once the set is idle (wait_set returned)
  char* staging(int s) { return sets_[s].h_bytes; }

  bool init_cache(const uint16_t* emb, int vocab, const uint16_t* proj,
                  int dim, long long capacity, float threshold,
                  int pending_cap, bool fp8) {
    if (!ready_ || dim != 384) return false;  // one tuned topk instantiation
    HIP_OK(hipSetDevice(device_));
    dim_ = dim;
    cap_ = capacity;
    threshold_ = threshold;
    vocab_ = vocab;
    pending_cap_ = pending_cap;
    fp8_ = fp8;
    HIP_OK(hipMalloc(&d_emb_, sizeof(bf16) * (size_t)vocab * dim));
    HIP_OK(hipMemcpy(d_emb_, emb, sizeof(bf16) * (size_t)vocab * dim,
                     hipMemcpyHostToDevice));
    HIP_OK(hipMalloc(&d_proj_, sizeof(bf16) * (size_t)dim * dim));
    HIP_OK(hipMemcpy(d_proj_, proj, sizeof(bf16) * (size_t)dim * dim,
                     hipMemcpyHostToDevice));
    size_t elt = fp8 ? 1 : sizeof(bf16);
    HIP_OK(hipMalloc(&d_index_, elt * (size_t)capacity * dim));
    HIP_OK(hipMemset(d_index_, 0, elt * (size_t)capacity * dim));
    HIP_OK(hipMalloc(&d_pending_, sizeof(bf16) * (size_t)pending_cap * dim));
    HIP_OK(hipStreamCreateWithFlags(&insert_stream_, hipStreamNonBlocking));
    for (int s = 0; s < kSets; ++s) {
      BatchSet& b = sets_[s];
      HIP_OK(hipMalloc(&b.d_pool, sizeof(float) * (size_t)max_req_ * dim));
      HIP_OK(hipMalloc(&b.d_poolcnt, sizeof(int32_t) * max_req_));
      HIP_OK(hipMalloc(&b.d_poolbf, sizeof(bf16) * (size_t)max_req_ * dim));
      HIP_OK(hipMalloc(&b.d_gout, sizeof(float) * (size_t)max_req_ * dim));
      HIP_OK(hipMalloc(&b.d_q, sizeof(bf16) * (size_t)max_req_ * dim));
      if (fp8) HIP_OK(hipMalloc(&b.d_q8, (size_t)max_req_ * dim));
      HIP_OK(hipMalloc(&b.d_best, sizeof(unsigned long long) * max_req_));
      HIP_OK(hipHostMalloc(&b.h_best, sizeof(unsigned long long) * max_req_,
                           hipHostMallocDefault));
      HIP_OK(hipMalloc(&b.d_slots, sizeof(int32_t) * max_req_));
      HIP_OK(hipHostMalloc(&b.h_slots, sizeof(int32_t) * max_req_,
                           hipHostMallocDefault));
    }
    cache_on_ = true;
    return true;
  }

  bool cache_on() const { return cache_on_; }

  // The embed/lookup tail of one batch, launched on the set's stream
  // right after the BPE pipeline (same pipeline as
  // aigw/ops/semcache.py embed/lookup).
  bool submit_cache(BatchSet& b, size_t n, int n_req,
                    const int32_t* pending_slots) {
    int dim = dim_;
    hipStream_t st = b.stream;
    HIP_OK(hipMemsetAsync(b.d_pool, 0, sizeof(float) * (size_t)n_req * dim, st));
    HIP_OK(hipMemsetAsync(b.d_poolcnt, 0, sizeof(int32_t) * n_req, st));
    constexpr int P = 32;
    // compact the token byte positions into d_ghead (ordered, so request
    // r's tokens are the d_counts[r] entries from d_req_excl[r]); the
    // group heads it held were last read by the BPE kernel above
    int tblocks = (int)((n + 255) / 256);
    hipLaunchKernelGGL(tok_flags_kernel, dim3(tblocks), dim3(256), 0, st,
                       b.d_out_ids, (int)n, b.d_gflags);
    hipLaunchKernelGGL(seg_block_count_kernel, dim3(tblocks), dim3(256), 0, st,
                       b.d_gflags, (int)n, b.d_blk);
    hipLaunchKernelGGL(excl_scan_kernel, dim3(1), dim3(256), 0, st,
                       b.d_blk, tblocks, b.d_excl, b.d_req_excl + max_req_);
    hipLaunchKernelGGL(flag_compact_write_kernel, dim3(tblocks), dim3(256), 0,
                       st, b.d_gflags, (int)n, b.d_excl, b.d_ghead);
    hipLaunchKernelGGL(excl_scan_kernel, dim3(1), dim3(256), 0, st,
                       b.d_counts, n_req, b.d_req_excl,
                       b.d_req_excl + max_req_);
    hipLaunchKernelGGL(meanpool_tokens_kernel, dim3(n_req, P),
                       dim3(dim / 2), 0,
                       st, b.d_out_ids, b.d_ghead, b.d_req_excl, b.d_counts,
                       n_req, d_emb_, dim, P, b.d_pool, b.d_poolcnt);
    hipLaunchKernelGGL(meanpool_div_kernel, dim3(n_req), dim3(dim), 0, st,
                       b.d_pool, b.d_poolcnt, n_req, dim);
    int total = n_req * dim;
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((total + 255) / 256), dim3(256),
                       0, st, b.d_pool, b.d_poolbf, total);
    dim3 ggrid((n_req + 15) / 16, (dim + 63) / 64);
    hipLaunchKernelGGL(gemm_bf16_nt_kernel, ggrid, dim3(256), 0, st,
                       b.d_poolbf, d_proj_, b.d_gout, n_req, dim, dim,
                       nullptr, 0);
    hipLaunchKernelGGL(l2norm_rows_kernel, dim3(n_req), dim3(dim), 0, st,
                       b.d_gout, b.d_q, n_req, dim);
    // park query vectors for possible insert: one gather launch
    memcpy(b.h_slots, pending_slots, sizeof(int32_t) * (size_t)n_req);
    HIP_OK(hipMemcpyAsync(b.d_slots, b.h_slots, sizeof(int32_t) * n_req,
                          hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(park_pending_kernel, dim3(n_req), dim3(dim), 0, st,
                       b.d_q, b.d_slots, n_req, dim, d_pending_);
    long long rows_now = rows_visible_.load(std::memory_order_acquire);
    b.rows_in_flight = rows_now;
    if (rows_now > 0) {
      HIP_OK(hipMemsetAsync(b.d_best, 0, sizeof(unsigned long long) * n_req, st));
      constexpr int ROWTILES = 16;
      long long blocks = (rows_now + 64 * ROWTILES - 1) / (64 * ROWTILES);
      if (fp8_) {
        // fp8 index streams HBM at half the bytes per row (2x rows in
        // the 288 GB budget)
        hipLaunchKernelGGL(bf16_to_fp8_kernel,
                           dim3((n_req * dim / 2 + 255) / 256), dim3(256), 0,
                           st, b.d_q, b.d_q8, n_req * dim);
        constexpr size_t L8 = 128 * (12 * 32 + 16) + 128 * 8;
        (void)hipFuncSetAttribute(
            reinterpret_cast<const void*>(
                &cache_topk_fp8_lds_kernel_t<12, ROWTILES>),
            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        for (int q0 = 0; q0 < n_req; q0 += 128) {
          int kq = (n_req - q0) < 128 ? (n_req - q0) : 128;
          hipLaunchKernelGGL((cache_topk_fp8_lds_kernel_t<12, ROWTILES>),
                             dim3((unsigned)blocks), dim3(256), L8, st,
                             (const uint8_t*)d_index_, rows_now,
                             b.d_q8 + (size_t)q0 * dim, kq, dim, b.d_best + q0);
        }
      } else {
        constexpr size_t L = 128 * (12 * 32 + 8) * sizeof(bf16) + 128 * 8;
        (void)hipFuncSetAttribute(
            reinterpret_cast<const void*>(&cache_topk_lds_kernel_t<12, ROWTILES>),
            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        for (int q0 = 0; q0 < n_req; q0 += 128) {
          int kq = (n_req - q0) < 128 ? (n_req - q0) : 128;
          hipLaunchKernelGGL((cache_topk_lds_kernel_t<12, ROWTILES>),
                             dim3((unsigned)blocks), dim3(256), L, st,
                             (const bf16*)d_index_, rows_now,
                             b.d_q + (size_t)q0 * dim, kq, dim, b.d_best + q0);
        }
      }
      HIP_OK(hipMemcpyAsync(b.h_best, b.d_best,
                            sizeof(unsigned long long) * n_req,
                            hipMemcpyDeviceToHost, st));
    }
    return true;
  }

  // Synchronous single-set wrapper (simple callers / tests).
  bool count_lookup(const char* bytes, size_t n, const int64_t* offsets,
                    int n_req, int32_t* counts_out,
                    const int32_t* pending_slots, int32_t* rows_out,
                    float* scores_out) {
    if (!cache_on_) return false;
    if (!submit(0, bytes, n, offsets, n_req, pending_slots)) return false;
    return wait_set(0, n_req, counts_out, rows_out, scores_out);
  }

  // Append a parked query vector to the index ring; returns the row.
  // Called from connection threads (post-response) on a dedicated stream;
  // host-side ring state is guarded by the caller's mutex. A topk racing
  // a half-written row can at worst misscore THAT row; the row→value
  // mapping stays correct because the value is stored first.
  long long cache_insert(int pending_slot) {
    if (!cache_on_ || pending_slot < 0 || pending_slot >= pending_cap_)
      return -1;
    long long row = head_;
    head_ = (head_ + 1) % cap_;
    if (fp8_) {
      hipLaunchKernelGGL(bf16_to_fp8_kernel, dim3((dim_ / 2 + 255) / 256),
                         dim3(256), 0, insert_stream_,
                         d_pending_ + (size_t)pending_slot * dim_,
                         (uint8_t*)d_index_ + (size_t)row * dim_, dim_);
      if (hipGetLastError() != hipSuccess) return -1;
    } else {
      hipError_t e = hipMemcpyAsync(
          (bf16*)d_index_ + (size_t)row * dim_,
          d_pending_ + (size_t)pending_slot * dim_, sizeof(bf16) * dim_,
          hipMemcpyDeviceToDevice, insert_stream_);
      if (e != hipSuccess) return -1;
    }
    long long vis = rows_visible_.load(std::memory_order_relaxed);
    long long want = row + 1 > vis ? row + 1 : vis;
    if (want > cap_) want = cap_;
    rows_visible_.store(want, std::memory_order_release);
    return row;
  }

  ~GpuAdmissionDirect() {
    if (!ready_) return;
    for (int s = 0; s < kSets; ++s) {
      BatchSet& b = sets_[s];
      (void)hipStreamDestroy(b.stream);
      (void)hipEventDestroy(b.event);
      (void)hipHostFree(b.h_bytes);
      (void)hipHostFree(b.h_off);
      (void)hipHostFree(b.h_counts);
      (void)hipHostFree(b.h_best);
      (void)hipHostFree(b.h_slots);
      for (void* p : {(void*)b.d_bytes, (void*)b.d_off, (void*)b.d_flags,
                      (void*)b.d_gflags, (void*)b.d_blk, (void*)b.d_excl,
                      (void*)b.d_totals, (void*)b.d_seg_start,
                      (void*)b.d_seg_req, (void*)b.d_ghead,
                      (void*)b.d_out_ids, (void*)b.d_counts, (void*)b.d_pool,
                      (void*)b.d_poolcnt, (void*)b.d_poolbf, (void*)b.d_gout,
                      (void*)b.d_q, (void*)b.d_q8, (void*)b.d_best,
                      (void*)b.d_slots})
        (void)hipFree(p);
    }
    if (cache_on_) {
      (void)hipStreamDestroy(insert_stream_);
      for (void* p : {(void*)d_emb_, (void*)d_proj_, (void*)d_index_,
                      (void*)d_pending_})
        (void)hipFree(p);
    }
    for (void* p : {(void*)d_htab_keys_, (void*)d_htab_rank_})
      (void)hipFree(p);
  }

  bool ready() const { return ready_; }

 private:
  bool ready_ = false;
  bool cache_on_ = false;
  int device_ = 0;
  int dim_ = 0;
  int vocab_ = 0;
  int pending_cap_ = 0;
  long long cap_ = 0;
  long long head_ = 0;  // writers hold the caller's insert mutex
  std::atomic<long long> rows_visible_{0};  // read lock-free by the batcher
  float threshold_ = 0.f;
  bool fp8_ = false;
  bf16* d_emb_ = nullptr;
  bf16* d_proj_ = nullptr;
  void* d_index_ = nullptr;
  bf16* d_pending_ = nullptr;
  hipStream_t insert_stream_{};
  size_t max_bytes_ = 0;
  int max_req_ = 0;
  int htab_mask_ = 0;
  long long* d_htab_keys_ = nullptr;
  int32_t* d_htab_rank_ = nullptr;
  BatchSet sets_[kSets];
};

// C-style entry points used by fastpath.cpp (keeps fastpath free of HIP
// headers; admission.hip is the only HIP translation unit in aigw_fast).
GpuAdmissionDirect* admission_create(const long long* htab_keys,
                                     const int32_t* htab_rank, int htab_n,
                                     size_t max_bytes, int max_req, int device) {
  auto* a = new GpuAdmissionDirect();
  if (!a->init(htab_keys, htab_rank, htab_n, max_bytes, max_req, device)) {
    delete a;
    return nullptr;
  }
  return a;
}

bool admission_count(GpuAdmissionDirect* a, const char* bytes, size_t n,
                     const int64_t* offsets, int n_req, int32_t* counts_out) {
  return a->count(bytes, n, offsets, n_req, counts_out);
}

void admission_destroy(GpuAdmissionDirect* a) { delete a; }

bool admission_init_cache(GpuAdmissionDirect* a, const uint16_t* emb, int vocab,
                          const uint16_t* proj, int dim, long long capacity,
                          float threshold, int pending_cap, bool fp8) {
  return a->init_cache(emb, vocab, proj, dim, capacity, threshold, pending_cap,
                       fp8);
}

bool admission_count_lookup(GpuAdmissionDirect* a, const char* bytes, size_t n,
                            const int64_t* offsets, int n_req,
                            int32_t* counts_out, const int32_t* pending_slots,
                            int32_t* rows_out, float* scores_out) {
  return a->count_lookup(bytes, n, offsets, n_req, counts_out, pending_slots,
                         rows_out, scores_out);
}

long long admission_cache_insert(GpuAdmissionDirect* a, int pending_slot) {
  return a->cache_insert(pending_slot);
}

bool admission_submit(GpuAdmissionDirect* a, int set, const char* bytes,
                      size_t n, const int64_t* offsets, int n_req,
                      const int32_t* pending_slots) {
  return a->submit(set, bytes, n, offsets, n_req, pending_slots);
}

bool admission_wait(GpuAdmissionDirect* a, int set, int n_req,
                    int32_t* counts_out, int32_t* rows_out,
                    float* scores_out) {
  return a->wait_set(set, n_req, counts_out, rows_out, scores_out);
}

char* admission_staging(GpuAdmissionDirect* a, int set) {
  return a->staging(set);
}

}  // namespace aigw_fast
