// Front end of the native admission batch (csrc/admission.hip): three
// kernels between the upload and the BPE kernel, where the kernels of
// bpe_kernels.cuh need six.
//
//   1. front_flags_kernel   derives BOTH flag sets (segment start, group
//                           head) and both per-block counts in one pass
//                           over the bytes.
//   2. dual_excl_scan_kernel scans the two block-count arrays in one launch.
//   3. front_write_kernel   one ordered compaction for both: seg_start,
//                           seg_req and ghead.
//
// The text is uploaded by the copy engine: front_flags_kernel reading it
// from pinned host memory itself was measured at 305 us per batch against
// 12 us from device memory (profiles/admission_submit.md).
//
// Group heads in byte space. bpe_kernels.cuh defines a group head over the
// SEGMENT array: segment j heads a group when j == 0, when it belongs to
// another request than segment j-1, or when its start lies in another
// 32-byte cell (relative to the request start) than the start of segment
// j-1. A request's first byte is always a segment start, so the segment
// before a start at byte i of request r is the nearest start below i, and
// it lies in the same cell of the same request exactly when it lies in
// [off[r] + 32*((i - off[r]) >> 5), i). Hence: a segment start at byte i
// is a group head iff no other segment start lies in that byte range. The
// range is at most 31 bytes long, so a block needs the 31 bytes before its
// own 256 (plus one more as the class-rule predecessor of the first of
// them); their segment flags are recomputed from the bytes and the
// offsets, never read from what a neighbouring block writes.
// tests/test_group_heads_bytespace_cpu.py pins the equivalence.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "bpe_kernels.cuh"

namespace aigw_front {

constexpr int kTile = 256;      // bytes (and threads) per block
constexpr int kLookBack = 32;   // 31 bytes of cell look-back + 1 predecessor
constexpr uint8_t kSegFlag = 1;   // front flag byte, bit 0: segment start
constexpr uint8_t kHeadFlag = 2;  // bit 1: group head

// class rule of seg_flags_kernel (b = byte, p = its predecessor)
__device__ __forceinline__ bool class_start(uint8_t b, uint8_t p) {
  return (b == ' ') || (byte_class(b) != byte_class(p) && p != ' ');
}

// 16 bytes -> LDS. `wide` says that src + idx is 16-byte aligned; a tail
// shorter than 16 bytes, or an unaligned buffer, goes byte by byte.
__device__ __forceinline__ void load16(const uint8_t* __restrict__ src, int idx,
                                       int n, bool wide, uint8_t* lds) {
  if (wide && idx + 16 <= n) {
    *reinterpret_cast<uint4*>(lds) = *reinterpret_cast<const uint4*>(src + idx);
  } else {
    for (int k = 0; k < 16 && idx + k < n; ++k) lds[k] = src[idx + k];
  }
}

// One 256-thread block per 256 bytes. The block's bytes and the 32 before
// them go to LDS with 16-byte loads by 18 of the threads; every later
// access is to LDS.
//
// Forced request starts, as in seg_flags_count_kernel: a lower-bound
// search of the (non-decreasing) offsets, then a strided walk over the
// offsets that fall inside the window. The walk starts one entry early
// and so also finds the largest offset below `base`: the start of the
// request that owns the block's first byte. Several empty requests may
// share one offset; an offset at or past n belongs to an empty trailing
// request and forces nothing.
//
// The grid also zeroes req_counts[0..n_req) for the BPE kernel.
__global__ void __launch_bounds__(kTile)
front_flags_kernel(const uint8_t* __restrict__ src, int n,
                   const int64_t* __restrict__ src_off, int n_req,
                   uint8_t* __restrict__ flags,
                   int32_t* __restrict__ seg_blk,
                   int32_t* __restrict__ grp_blk,
                   int32_t* __restrict__ req_counts) {
  __shared__ __attribute__((aligned(16))) uint8_t sb[kLookBack + kTile];
  __shared__ uint8_t forced[kLookBack + kTile];
  __shared__ int prev_start;      // largest request offset below base
  __shared__ int wave_start[4];   // per wave: nearest request start at or below
  __shared__ uint32_t bm[10];     // segment-start bitmap, see below
  __shared__ int seg_cnt[4], grp_cnt[4];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int base = blockIdx.x * kTile;
  const int i = base + tid;
  const int end = min(base + kTile, n);
  const int lo_byte = max(base - kLookBack, 0);
  // position p of the 288-byte window is byte base - 32 + p
  forced[tid] = 0;
  if (tid < kLookBack) forced[kTile + tid] = 0;
  if (tid == 0) prev_start = -1;
  for (int r = i; r < n_req; r += gridDim.x * kTile) req_counts[r] = 0;

  const bool wide = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
  if (tid < 16)
    load16(src, base + 16 * tid, n, wide, sb + kLookBack + 16 * tid);
  else if (tid < 18 && base > 0)
    load16(src, base - kLookBack + 16 * (tid - 16), n, wide,
           sb + 16 * (tid - 16));

  // lower_bound(src_off, lo_byte): first request starting in the window
  int lo = 0, hi = n_req;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (src_off[mid] < lo_byte) lo = mid + 1; else hi = mid;
  }
  __syncthreads();  // forced[] and prev_start are initialised
  for (int r = max(lo - 1, 0) + tid; r < n_req; r += kTile) {
    long long off = src_off[r];
    if (off >= end) break;
    if (off < 0) continue;
    if (off < base) atomicMax(&prev_start, (int)off);
    if (off >= lo_byte) forced[(int)off - (base - kLookBack)] = 1;
  }
  __syncthreads();  // text, forced starts and prev_start are in LDS

  // segment flags: mine, and for the first 32 threads a look-back byte
  // (position 0 is only a predecessor: no cell reaches back 32 bytes)
  bool f = false;
  if (i < n)
    f = i == 0 || forced[kLookBack + tid] ||
        class_start(sb[kLookBack + tid], sb[kLookBack + tid - 1]);
  bool fb = false;
  if (base > 0 && tid >= 1 && tid < kLookBack)
    fb = forced[tid] || class_start(sb[tid], sb[tid - 1]);
  uint64_t tile_ballot = __ballot(f);
  uint64_t back_ballot = __ballot(fb);  // wave 0 holds the 32 look-back bits
  // bm[1 + (p >> 5)] bit (p & 31) = segment start at window position p;
  // bm[0] is a zero pad so that a two-word read below position 32 is valid
  if (lane == 0) {
    if (wave == 0) {
      bm[0] = 0;
      bm[1] = (uint32_t)back_ballot;
    }
    bm[2 + 2 * wave] = (uint32_t)tile_ballot;
    bm[3 + 2 * wave] = (uint32_t)(tile_ballot >> 32);
  }
  // start of the request that owns byte i: inclusive max-scan of the
  // forced starts of the tile, seeded with prev_start
  int rs = (i < n && forced[kLookBack + tid]) ? i : -1;
  for (int d = 1; d < 64; d <<= 1) {
    int t = __shfl_up(rs, d);
    if (lane >= d) rs = max(rs, t);
  }
  if (lane == 63) wave_start[wave] = rs;
  __syncthreads();
  int carry = prev_start;
  for (int w = 0; w < wave; ++w) carry = max(carry, wave_start[w]);
  rs = max(max(rs, carry), 0);  // no request at or below i: one starts at 0

  // group head: no other segment start among the k bytes of my 32-byte
  // cell below me. They are window positions [q - k, q), q = 32 + tid,
  // all inside the two bitmap words that end with the word of q - 1.
  bool g = false;
  if (f) {
    int k = (i - rs) & 31;
    int q = kLookBack + tid;
    int a = 1 + ((q - 1) >> 5);
    uint64_t two = ((uint64_t)bm[a] << 32) | bm[a - 1];
    g = true;
    if (k > 0) {  // then the shift is at most 63
      uint64_t mask = ((1ull << k) - 1ull) << (((q - 1) & 31) + 33 - k);
      g = (two & mask) == 0;
    }
  }
  if (i < n) flags[i] = (f ? kSegFlag : 0) | (g ? kHeadFlag : 0);
  uint64_t head_ballot = __ballot(g);
  if (lane == 0) {
    seg_cnt[wave] = __popcll(tile_ballot);
    grp_cnt[wave] = __popcll(head_ballot);
  }
  __syncthreads();
  if (tid == 0) {
    seg_blk[blockIdx.x] = seg_cnt[0] + seg_cnt[1] + seg_cnt[2] + seg_cnt[3];
    grp_blk[blockIdx.x] = grp_cnt[0] + grp_cnt[1] + grp_cnt[2] + grp_cnt[3];
  }
}

// Exclusive scans of the two block-count arrays in one launch of two
// blocks: block 0 scans in0 -> ex0, block 1 scans in1 -> ex1, and
// totals[blockIdx.x] receives the sum. Each thread owns one contiguous run
// of ceil(n / 256) counts: sum the run, one block scan of the 256 sums
// (two barriers in all, against three per 256 counts in a chunked scan),
// then write the run's prefixes.
__global__ void __launch_bounds__(256)
dual_excl_scan_kernel(const int32_t* __restrict__ in0,
                      const int32_t* __restrict__ in1, int n,
                      int32_t* __restrict__ ex0, int32_t* __restrict__ ex1,
                      int32_t* __restrict__ totals) {
  __shared__ int32_t wave_sum[4];
  const int32_t* __restrict__ in = blockIdx.x ? in1 : in0;
  int32_t* __restrict__ ex = blockIdx.x ? ex1 : ex0;
  int tid = threadIdx.x;
  int lane = tid & 63;
  int wave = tid >> 6;
  int run = (n + 255) / 256;
  long long b64 = (long long)tid * run;
  int b = b64 < n ? (int)b64 : n;
  int e = min(b + run, n);
  int32_t own = 0;
  for (int j = b; j < e; ++j) own += in[j];
  int32_t v = own;
  for (int d = 1; d < 64; d <<= 1) {
    int32_t t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  if (lane == 63) wave_sum[wave] = v;
  __syncthreads();
  int32_t wave_off = 0;
  for (int w = 0; w < wave; ++w) wave_off += wave_sum[w];
  int32_t acc = wave_off + v - own;
  for (int j = b; j < e; ++j) {
    int32_t c = in[j];
    ex[j] = acc;
    acc += c;
  }
  if (tid == 255) totals[blockIdx.x] = wave_off + v;
}

// One ordered compaction pass for both flag sets: segment position ->
// seg_start / seg_req (owning request: upper_bound(req_off, i) - 1, as in
// seg_write_kernel), group position -> ghead = the head's segment position.
__global__ void __launch_bounds__(kTile)
front_write_kernel(const uint8_t* __restrict__ flags, int n,
                   const int32_t* __restrict__ seg_excl,
                   const int32_t* __restrict__ grp_excl,
                   const int64_t* __restrict__ req_off, int n_req,
                   int32_t* __restrict__ seg_start,
                   int32_t* __restrict__ seg_req,
                   int32_t* __restrict__ ghead) {
  __shared__ int seg_base[4], grp_base[4];
  int i = blockIdx.x * kTile + threadIdx.x;
  int lane = threadIdx.x & 63;
  int wave = threadIdx.x >> 6;
  uint8_t fl = (i < n) ? flags[i] : 0;
  bool f = fl & kSegFlag;
  bool g = fl & kHeadFlag;
  uint64_t seg_ballot = __ballot(f);
  uint64_t grp_ballot = __ballot(g);
  if (lane == 0) {
    seg_base[wave] = __popcll(seg_ballot);
    grp_base[wave] = __popcll(grp_ballot);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int sacc = 0, gacc = 0;
    for (int w = 0; w < 4; ++w) {
      int sc = seg_base[w], gc = grp_base[w];
      seg_base[w] = sacc;
      grp_base[w] = gacc;
      sacc += sc;
      gacc += gc;
    }
  }
  __syncthreads();
  if (!f) return;
  uint64_t below = (1ull << lane) - 1ull;
  int pos = seg_excl[blockIdx.x] + seg_base[wave] + __popcll(seg_ballot & below);
  seg_start[pos] = i;
  int lo = 0, hi = n_req;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (req_off[mid] <= i) lo = mid + 1; else hi = mid;
  }
  seg_req[pos] = lo - 1;
  if (g)
    ghead[grp_excl[blockIdx.x] + grp_base[wave] + __popcll(grp_ballot & below)] =
        pos;
}

}  // namespace aigw_front
