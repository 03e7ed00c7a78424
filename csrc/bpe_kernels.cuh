// Byte-level BPE tokenizer kernels (gfx950 / CDNA4), shared between the
// torch extension (csrc/aigw_kernels.hip, Python data plane) and the
// torch-free native admission path (csrc/admission.hip, C++ fast front).
// Definitions live in this header because the two users are separate
// shared objects; each translation unit that includes it gets its own
// copy (no cross-.so linking).
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

// Byte classes for the segmentation rule (must match aigw/ops/bpe_ref.py):
// segment starts at i iff i==0, byte==' ', or class(b[i])!=class(b[i-1]) and
// b[i-1]!=' '.
__device__ __forceinline__ int byte_class(uint8_t b) {
  if (b == ' ') return 0;
  if (b == '\t' || b == '\n' || b == '\r' || b == 0x0b || b == 0x0c) return 1;
  if (b >= '0' && b <= '9') return 2;
  if ((b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z') || b >= 0x80) return 3;
  return 4;  // punctuation / other
}

__global__ void seg_flags_kernel(const uint8_t* __restrict__ bytes, int n,
                                 uint8_t* __restrict__ flags) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint8_t f;
  if (i == 0) {
    f = 1;
  } else {
    uint8_t b = bytes[i], p = bytes[i - 1];
    f = (b == ' ') || (byte_class(b) != byte_class(p) && p != ' ');
  }
  flags[i] = f;
}

// A request that starts at or past byte n is empty (a trailing empty text
// has req_off == n) and forces no start: same `off < n` guard as
// bpe_ref.segment_starts, and flags[] holds only n bytes.
__global__ void seg_force_starts_kernel(const int64_t* __restrict__ req_off,
                                        int n_req, int n,
                                        uint8_t* __restrict__ flags) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_req) return;
  long long off = req_off[i];
  if (off >= 0 && off < n) flags[off] = 1;
}

// per-256-byte-block flag counts (for the ordered compaction scan)
__global__ void seg_block_count_kernel(const uint8_t* __restrict__ flags, int n,
                                       int32_t* __restrict__ blk_counts) {
  __shared__ int cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t ballot = __ballot(i < n && flags[i]);
  if ((threadIdx.x & 63) == 0) atomicAdd(&cnt, __popcll(ballot));
  __syncthreads();
  if (threadIdx.x == 0) blk_counts[blockIdx.x] = cnt;
}

// block-wide count of a per-thread flag for a 256-thread block (wave
// ballots staged through LDS); the result is valid in every thread
__device__ __forceinline__ int block256_flag_count(bool f) {
  __shared__ int wave_cnt[4];
  uint64_t ballot = __ballot(f);
  if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = __popcll(ballot);
  __syncthreads();
  return wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// Fused front end of the native admission pipeline: seg_flags_kernel +
// seg_force_starts_kernel + seg_block_count_kernel in one pass, while the
// flag is still in a register. One 256-thread block per 256 bytes. Forced
// request starts are applied per block: a lower-bound search of the
// (non-decreasing) req_off for the block's first byte, then a strided
// walk over the offsets that fall inside the block into an LDS byte mask
// (several empty requests may share one offset; an offset at or past n
// belongs to an empty trailing request and forces nothing, as in
// seg_force_starts_kernel). The kernel also zeroes req_counts[0..n_req)
// for the BPE kernel's atomicAdd — n > 0 guarantees at least one block.
__global__ void __launch_bounds__(256)
seg_flags_count_kernel(const uint8_t* __restrict__ bytes, int n,
                       const int64_t* __restrict__ req_off, int n_req,
                       uint8_t* __restrict__ flags,
                       int32_t* __restrict__ blk_counts,
                       int32_t* __restrict__ req_counts) {
  __shared__ uint8_t forced[256];
  int tid = threadIdx.x;
  int base = blockIdx.x * 256;
  int i = base + tid;
  forced[tid] = 0;
  for (int r = i; r < n_req; r += gridDim.x * 256) req_counts[r] = 0;
  __syncthreads();
  // lower_bound(req_off, base): first request starting at or after base
  int lo = 0, hi = n_req;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (req_off[mid] < base) lo = mid + 1; else hi = mid;
  }
  int end = min(base + 256, n);
  for (int r = lo + tid; r < n_req; r += 256) {
    long long off = req_off[r];
    if (off >= end) break;
    if (off >= base) forced[off - base] = 1;
  }
  __syncthreads();
  bool f = false;
  if (i < n) {
    if (i == 0) {
      f = true;
    } else {
      uint8_t b = bytes[i], p = bytes[i - 1];
      f = (b == ' ') || (byte_class(b) != byte_class(p) && p != ' ') ||
          forced[tid];
    }
    flags[i] = f;
  }
  int cnt = block256_flag_count(f);
  if (tid == 0) blk_counts[blockIdx.x] = cnt;
}

// write segment start offsets + owning request id (ordered compaction)
__global__ void seg_write_kernel(const uint8_t* __restrict__ flags, int n,
                                 const int32_t* __restrict__ blk_excl,  // exclusive scan
                                 const int64_t* __restrict__ req_off, int n_req,
                                 int32_t* __restrict__ seg_start,
                                 int32_t* __restrict__ seg_req) {
  __shared__ int wave_base[4];
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int lane = threadIdx.x & 63;
  int wave = threadIdx.x >> 6;
  bool f = (i < n) && flags[i];
  uint64_t ballot = __ballot(f);
  // block-local exclusive offsets: wave sums staged through LDS
  if (lane == 0) wave_base[wave] = __popcll(ballot);
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int w = 0; w < 4; ++w) {
      int c = wave_base[w];
      wave_base[w] = acc;
      acc += c;
    }
  }
  __syncthreads();
  if (!f) return;
  int pos_in_wave = __popcll(ballot & ((1ull << lane) - 1ull));
  int pos = blk_excl[blockIdx.x] + wave_base[wave] + pos_in_wave;
  seg_start[pos] = i;
  // owning request: upper_bound(req_off, i) - 1
  int lo = 0, hi = n_req;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (req_off[mid] <= i) lo = mid + 1; else hi = mid;
  }
  seg_req[pos] = lo - 1;
}

// The BPE merge loop, shared by both scheduling paths. Tokens live in lane
// registers; the merge-pair table is an open-addressing hash in HBM (hot
// entries L2-resident). Occurrence selection and merging operate on
// wave-uniform 64-bit masks.
// `myseg` confines merges to a segment: a pair is valid only when both
// lanes carry the same segment id (constant 0 for the single-segment
// path), so packing several small segments into one wave changes nothing
// semantically.
// SEGMENTED=false (one segment in the wave): the lowest pair rank is a
// wave min-reduce with __shfl_xor.
// SEGMENTED=true (packed group): segments are independent, so every
// segment merges ITS OWN lowest-rank pair each round instead of waiting
// for the round in which that rank is also the wave-wide minimum. Inside
// a segment the sequence of merges is unchanged (the rounds it used to
// sit out simply disappear), so the output is bit-identical; the bench
// payload drops from ~12.5 to ~4.6 rounds per wave. The per-segment
// minimum is a segmented inclusive prefix-min (six __shfl_up steps gated
// by loop-invariant "lane - 2^k is in my segment" bits) read back from
// the segment's last lane. Lanes never move and myseg never changes, so
// both the bits and the last-lane index are computed once. Inactive tail
// lanes past the window share the last segment's id; their rank is
// always INT_MAX, which leaves that segment's minimum untouched.
template <bool SEGMENTED>
__device__ __forceinline__ uint64_t bpe_merge_lanes(
    int& tok, int myseg, uint64_t active, int lane,
    const long long* __restrict__ htab_keys, const int32_t* __restrict__ htab_rank,
    int htab_mask) {
  int inseg = 0;      // bit k: lane - 2^k carries my segment id
  int seg_last = 63;  // last lane carrying my segment id
  if (SEGMENTED) {
    #pragma unroll
    for (int k = 0; k < 6; ++k) {
      int s = __shfl_up(myseg, 1 << k);
      if (lane >= (1 << k) && s == myseg) inseg |= 1 << k;
    }
    int upseg = __shfl_down(myseg, 1);
    uint64_t ends = __ballot(lane == 63 || upseg != myseg);
    seg_last = __ffsll((long long)(ends & (~0ull << lane))) - 1;
  }
  // pair-rank memo: a merge round only changes the pairs adjacent to a
  // merge site, so most lanes can reuse last round's hash-probe result
  // (the probe's L2 loads dominate the VALU-bound loop otherwise)
  long long cached_key = -1;
  int cached_rank = INT_MAX;
  for (;;) {
    // next active lane above mine
    uint64_t above = (lane < 63) ? (active & (~0ull << (lane + 1))) : 0ull;
    int nxt = above ? (__ffsll((long long)above) - 1) : -1;
    int nxttok = __shfl(tok, nxt < 0 ? 0 : nxt);
    int nxtseg = __shfl(myseg, nxt < 0 ? 0 : nxt);
    int rank = INT_MAX;
    if (tok >= 0 && nxt >= 0 && nxtseg == myseg) {
      long long key = ((long long)tok << 32) | (unsigned)nxttok;
      if (key == cached_key) {
        rank = cached_rank;
      } else {
        uint64_t h = (uint64_t)key * 0x9E3779B97F4A7C15ull;
        int idx = (int)(h >> 40) & htab_mask;
        for (;;) {
          long long k = htab_keys[idx];
          if (k == key) { rank = htab_rank[idx]; break; }
          if (k == -1) break;
          idx = (idx + 1) & htab_mask;
        }
        cached_key = key;
        cached_rank = rank;
      }
    }
    int minrank = rank;
    uint64_t occ;
    if (SEGMENTED) {
      // segmented inclusive prefix-min, then my segment's last lane
      // holds the segment minimum
      #pragma unroll
      for (int k = 0; k < 6; ++k) {
        int t = __shfl_up(minrank, 1 << k);
        if ((inseg >> k) & 1) minrank = min(minrank, t);
      }
      minrank = __shfl(minrank, seg_last);
      if (__ballot(minrank != INT_MAX) == 0) return active;
      occ = __ballot(rank == minrank && rank != INT_MAX);
    } else {
      // wave min-reduce of rank
      #pragma unroll
      for (int off = 32; off > 0; off >>= 1)
        minrank = min(minrank, __shfl_xor(minrank, off));
      if (minrank == INT_MAX) return active;
      occ = __ballot(rank == minrank);
    }
    // greedy leftmost non-overlapping selection (wave-uniform scalar
    // loop); overlap only arises inside a segment, and a segment's last
    // lane never holds a valid pair
    uint64_t m = occ, sel = 0;
    while (m) {
      int i = __ffsll((long long)m) - 1;
      sel |= 1ull << i;
      int ni = __shfl(nxt, i);
      m &= ~(1ull << i);
      if (ni >= 0) m &= ~(1ull << ni);
    }
    int newid = 256 + minrank;  // per lane in the segmented mode
    // previous active lane (my potential merge head)
    uint64_t below = active & ((lane ? (1ull << lane) : 1ull) - 1ull);
    int prev = below ? (63 - __clzll((long long)below)) : -1;
    bool merged_into_prev = (prev >= 0) && ((sel >> prev) & 1);
    if ((sel >> lane) & 1) tok = newid;
    if (merged_into_prev) tok = -1;
    active = __ballot(tok >= 0);
  }
}

// Single-segment path: 64-byte chunks of one segment per wave (also used
// for group tail segments that do not fit the packed window). Returns the
// number of tokens written.
__device__ __forceinline__ int bpe_encode_one_segment(
    const uint8_t* __restrict__ bytes, int s, int e, int lane,
    const long long* __restrict__ htab_keys, const int32_t* __restrict__ htab_rank,
    int htab_mask, int32_t* __restrict__ out_ids) {
  int written = 0;
  for (int chunk = s; chunk < e; chunk += 64) {
    int len = min(e - chunk, 64);
    int tok = (lane < len) ? (int)bytes[chunk + lane] : -1;
    uint64_t active = __ballot(tok >= 0);
    active = bpe_merge_lanes<false>(tok, 0, active, lane, htab_keys, htab_rank,
                                    htab_mask);
    int cnt = __popcll(active);
    if (tok >= 0) {
      int pos = __popcll(active & ((lane ? (1ull << lane) : 1ull) - 1ull));
      out_ids[s + written + pos] = tok;
    }
    written += cnt;
  }
  return written;
}

// Grouped scheduling: one wave per GROUP of consecutive segments (group =
// segments of one request whose starts share a 32-byte cell relative to
// the request start, computed by group_head_flags_kernel). Grouping is
// scheduling-only — token output is bit-identical to segment-per-wave.
// Typical English text has ~5-byte segments, so segment-per-wave leaves
// ~58/64 lanes idle; packing a whole group into the lanes recovers wave
// occupancy. The 32-byte cell rule bounds the packed window: all group
// segments start within one 32-byte cell, so the span up to the last
// segment's start is < 32 bytes, and the whole group is packed whenever
// it ends within 64 bytes of the group start (long tails fall back to the
// chunked path).
__device__ __forceinline__ void bpe_encode_grouped_body(
    const uint8_t* __restrict__ bytes, const int32_t* __restrict__ seg_start,
    const int32_t* __restrict__ seg_req, int n_segs, int n_bytes,
    const int32_t* __restrict__ ghead, int n_groups,
    const long long* __restrict__ htab_keys,
    const int32_t* __restrict__ htab_rank, int htab_mask,
    int32_t* __restrict__ out_ids, int32_t* __restrict__ req_counts) {
  // per-wave (request, tokens written), summed per request within the
  // block before touching req_counts (see the end of this function)
  __shared__ int32_t wave_req[16];
  __shared__ int32_t wave_cnt[16];
  int g = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  int lane = threadIdx.x & 63;
  int wave = threadIdx.x >> 6;
  int req = -1;
  int written = 0;
  if (g < n_groups) {  // wave-uniform; idle waves still reach the barrier
    int first = ghead[g];
    int next_first = (g + 1 < n_groups) ? ghead[g + 1] : n_segs;
    int lastseg = next_first - 1;
    int s0 = seg_start[first];
    int sE = (next_first < n_segs) ? seg_start[next_first] : n_bytes;

    if (lastseg == first) {
      written = bpe_encode_one_segment(bytes, s0, sE, lane, htab_keys, htab_rank,
                                       htab_mask, out_ids);
    } else {
      int sL = seg_start[lastseg];
      bool include_last = (sE - s0) <= 64;
      int win_end = include_last ? sE : sL;
      int pos = s0 + lane;
      int tok = (pos < win_end) ? (int)bytes[pos] : -1;
      // reconstruct per-lane segment-start flags (same rule as
      // seg_flags_kernel; no request boundary can occur inside a group)
      bool f = false;
      if (pos < win_end) {
        if (pos == s0) {
          f = true;
        } else {
          uint8_t b = bytes[pos], pb = bytes[pos - 1];
          f = (b == ' ') || (byte_class(b) != byte_class(pb) && pb != ' ');
        }
      }
      uint64_t startmask = __ballot(f);
      int myseg = __popcll(startmask & ((lane ? (1ull << lane) : 1ull) - 1ull)) + (f ? 1 : 0);
      uint64_t active = __ballot(tok >= 0);
      active = bpe_merge_lanes<true>(tok, myseg, active, lane, htab_keys, htab_rank,
                                     htab_mask);
      written = __popcll(active);
      if (tok >= 0) {
        // my segment's first lane = highest start flag at or below me; its
        // lane offset equals the segment's byte offset within the window
        uint64_t at_or_below =
            startmask & ((lane < 63 ? (1ull << (lane + 1)) : 0ull) - 1ull);
        int start_lane = 63 - __clzll((long long)at_or_below);
        int pos_in_seg =
            __popcll(active & ((lane ? (1ull << lane) : 1ull) - 1ull) &
                     ~((start_lane ? (1ull << start_lane) : 1ull) - 1ull));
        out_ids[s0 + start_lane + pos_in_seg] = tok;
      }
      if (!include_last)
        written += bpe_encode_one_segment(bytes, sL, sE, lane, htab_keys, htab_rank,
                                          htab_mask, out_ids);
    }
    if (written > 0) req = seg_req[first];
  }
  // One atomicAdd per (block, request) instead of one per wave. Every
  // group of a request adds to the same counter and a batch's counters
  // share a cache line or two, so per-wave atomics (~800 per 25 kB
  // request, ~27k per serving batch) queue behind one another and set
  // the kernel's duration whatever the merge loop costs: measured
  // 237 us -> 75 us per batch from this change alone at 4 waves per
  // block, 52 us at 8 (profiles/admission_cycle.md). A block's groups
  // are consecutive, so each request is one contiguous run of waves: the
  // first wave of a run adds the run's total. Integer sums: the counts
  // are the same in any order. Up to 16 waves per block.
  if (lane == 0) {
    wave_req[wave] = req;
    wave_cnt[wave] = written;
  }
  __syncthreads();
  if (lane == 0 && req >= 0 && (wave == 0 || wave_req[wave - 1] != req)) {
    int nwaves = blockDim.x >> 6;
    int sum = written;
    for (int w = wave + 1; w < nwaves && wave_req[w] == req; ++w)
      sum += wave_cnt[w];
    atomicAdd(&req_counts[req], sum);
  }
}

__global__ void __launch_bounds__(256)
bpe_encode_grouped_kernel(const uint8_t* __restrict__ bytes,
                          const int32_t* __restrict__ seg_start,
                          const int32_t* __restrict__ seg_req, int n_segs,
                          int n_bytes,
                          const int32_t* __restrict__ ghead, int n_groups,
                          const long long* __restrict__ htab_keys,
                          const int32_t* __restrict__ htab_rank, int htab_mask,
                          int32_t* __restrict__ out_ids,
                          int32_t* __restrict__ req_counts) {
  bpe_encode_grouped_body(bytes, seg_start, seg_req, n_segs, n_bytes, ghead,
                          n_groups, htab_keys, htab_rank, htab_mask, out_ids,
                          req_counts);
}

// Sync-free variant: segment/group totals live in DEVICE scalars (the scan
// tails), so the host never calls .item() — the whole pipeline is launched
// blind with upper-bound grids and each kernel self-bounds. This is what
// lets the serving path await a hipEvent cooperatively instead of
// busy-polling a host sync (ROCm host syncs spin a core).
__global__ void __launch_bounds__(1024)
bpe_encode_grouped_dev_kernel(const uint8_t* __restrict__ bytes,
                              const int32_t* __restrict__ seg_start,
                              const int32_t* __restrict__ seg_req,
                              const int32_t* __restrict__ n_segs_dev,
                              int n_bytes,
                              const int32_t* __restrict__ ghead,
                              const int32_t* __restrict__ n_groups_dev,
                              const long long* __restrict__ htab_keys,
                              const int32_t* __restrict__ htab_rank, int htab_mask,
                              int32_t* __restrict__ out_ids,
                              int32_t* __restrict__ req_counts) {
  bpe_encode_grouped_body(bytes, seg_start, seg_req, *n_segs_dev, n_bytes, ghead,
                          *n_groups_dev, htab_keys, htab_rank, htab_mask, out_ids,
                          req_counts);
}

// group-head flags over the segment array: a group breaks on request
// change or a new 32-byte cell (relative to the request start)
__global__ void group_head_flags_kernel(const int32_t* __restrict__ seg_start,
                                        const int32_t* __restrict__ seg_req,
                                        int n_segs,
                                        const int64_t* __restrict__ req_off,
                                        uint8_t* __restrict__ flags) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_segs) return;
  uint8_t f;
  if (i == 0 || seg_req[i] != seg_req[i - 1]) {
    f = 1;
  } else {
    long long off = req_off[seg_req[i]];
    f = ((seg_start[i] - off) >> 5) != ((seg_start[i - 1] - off) >> 5);
  }
  flags[i] = f;
}

__global__ void group_head_flags_dev_kernel(const int32_t* __restrict__ seg_start,
                                            const int32_t* __restrict__ seg_req,
                                            const int32_t* __restrict__ n_segs_dev,
                                            const int64_t* __restrict__ req_off,
                                            uint8_t* __restrict__ flags) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= *n_segs_dev) return;
  uint8_t f;
  if (i == 0 || seg_req[i] != seg_req[i - 1]) {
    f = 1;
  } else {
    long long off = req_off[seg_req[i]];
    f = ((seg_start[i] - off) >> 5) != ((seg_start[i - 1] - off) >> 5);
  }
  flags[i] = f;
}

// Fused group front end of the native admission pipeline:
// group_head_flags_dev_kernel + seg_block_count_kernel over a grid that
// covers all n byte positions. Positions at or past *n_segs_dev get flag
// 0 and every position below n is written, so the flag buffer needs no
// clearing and stale contents from an earlier batch cannot leak in.
__global__ void __launch_bounds__(256)
group_flags_count_kernel(const int32_t* __restrict__ seg_start,
                         const int32_t* __restrict__ seg_req,
                         const int32_t* __restrict__ n_segs_dev,
                         const int64_t* __restrict__ req_off, int n,
                         uint8_t* __restrict__ flags,
                         int32_t* __restrict__ blk_counts) {
  int i = blockIdx.x * 256 + threadIdx.x;
  bool f = false;
  if (i < n) {
    if (i < *n_segs_dev) {
      if (i == 0 || seg_req[i] != seg_req[i - 1]) {
        f = true;
      } else {
        long long off = req_off[seg_req[i]];
        f = ((seg_start[i] - off) >> 5) != ((seg_start[i - 1] - off) >> 5);
      }
    }
    flags[i] = f;
  }
  int cnt = block256_flag_count(f);
  if (threadIdx.x == 0) blk_counts[blockIdx.x] = cnt;
}

// generic ordered index-compaction write (flag positions -> indices)
__global__ void flag_compact_write_kernel(const uint8_t* __restrict__ flags, int n,
                                          const int32_t* __restrict__ blk_excl,
                                          int32_t* __restrict__ out_idx) {
  __shared__ int wave_base[4];
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int lane = threadIdx.x & 63;
  int wave = threadIdx.x >> 6;
  bool f = (i < n) && flags[i];
  uint64_t ballot = __ballot(f);
  if (lane == 0) wave_base[wave] = __popcll(ballot);
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int w = 0; w < 4; ++w) {
      int c = wave_base[w];
      wave_base[w] = acc;
      acc += c;
    }
  }
  __syncthreads();
  if (!f) return;
  int pos_in_wave = __popcll(ballot & ((1ull << lane) - 1ull));
  out_idx[blk_excl[blockIdx.x] + wave_base[wave] + pos_in_wave] = i;
}

