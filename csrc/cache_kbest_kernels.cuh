// k-best cache lookup (k <= 8) fused into the MFMA index scan (gfx950).
//
// The arg-max kernels of cache_kernels.cuh fold a tile into one packed
// 64-bit atomicMax per query, which cannot be stretched past k = 1. These
// kernels keep the k best eligible rows per query instead, on the same
// packed keys: pack_score(score, row) is unique per row and orders by score
// first and by the higher row among equal scores, so the k-best set and its
// order do not depend on the order in which tiles, waves or blocks finish.
//
// Front half: cache_topk_scoped_kernel_t's (query block staged in LDS with
// the same bank padding, A-tile ping-pong, ks-outer MFMAs with one
// accumulator per query tile, load_row_tags and the same eligibility rule
// applied per element before anything is reduced). Sibling, not a flag, so
// the arg-max kernels' code does not move.
//
// Selection:
//  - Every wave owns a private k-entry list per query in LDS, so no list is
//    ever written by two waves and no atomics are needed. A list is
//    unsorted with one invariant: slot 0 holds its minimum. Lists start as
//    all 0 (0 = no row; pack_score of a real score is never 0), so a list
//    that is not full yet has minimum 0 and takes any key. The slot-0
//    invariant replaces a separate minimum array and a fill count.
//  - List stride is (k | 1) keys: an odd number of 8-byte slots, so the 16
//    queries of a query tile read their slot 0 from 16 distinct bank pairs.
//    LDS for the lists is sized by the call's k, not by KMAX, so small k
//    keeps the fp8 kernel's occupancy.
//  - Fast path, per result tile and query tile: a lane packs its four
//    eligible elements, takes their maximum and compares it with the list
//    minimum; one wave ballot says whether any lane has something to insert.
//  - Slow path: walk r (4) x kgrp (4) in a fixed order. Within one step the
//    16 active lanes hold 16 different queries, so at most one lane writes a
//    given list at any moment. All four of a lane's elements are walked, not
//    only its maximum: two of a lane's rows may both belong in the list. The
//    minimum read on the fast path only filters (a list minimum never
//    decreases, so a key at or below a stale minimum is still rejected);
//    the insert itself re-reads slot 0. An insert overwrites the minimum
//    and restores the invariant with one scan of the other k - 1 slots.
//    List accesses are volatile: lanes of one wave hand a list to each
//    other between steps, which the compiler must not cache across.
//  - Block end: after __syncthreads(), one thread per query merges the four
//    wave lists by k rounds of "largest key below the previous one" and
//    writes the block's sorted k-best, padded with 0, to part[blocks][n_q][k].
//  - cache_topk_k_merge_kernel, a second launch on the stream (no "last
//    block" fence, no spin): one wave per query, a sorted KMAX-entry list
//    per lane in registers, then k rounds of wave-wide max extraction.
//
// A block scans 64 * ROWTILES rows, as the arg-max kernels' blocks do; a
// wave's list therefore restarts every 16 * ROWTILES rows and the first
// tiles of every block take the slow path.
//
// k = 1 returns the key cache_topk_scoped returns. The unscoped cache_topk
// kernels break an exact score tie between two of one lane's four rows
// towards the lower row (strict > in their 4-way max), against the packed
// key's order everywhere else; this kernel follows the key order throughout,
// so it differs from them in that one case only.
#pragma once

#include <hip/hip_runtime.h>

#include "cache_kernels.cuh"

constexpr int kKbestMax = 8;
constexpr int kKbestLdsLimit = 160 * 1024;

__host__ __device__ constexpr int kbest_list_stride(int k) { return k | 1; }

// Query tiles (of 16 queries) per pass: 8, as in the arg-max kernels, unless
// the query block plus KMAX-sized lists would not fit the LDS (bf16 at dim
// 512); then 4, and the host runs passes of 64 queries.
template <class E, int KSTEPS>
constexpr int kbest_qtiles() {
  constexpr int per_query = (KSTEPS * 32 + E::kPad) * (int)sizeof(typename E::elem) +
                            4 * kbest_list_stride(kKbestMax) * 8 + 8;
  return 128 * per_query <= kKbestLdsLimit ? 8 : 4;
}

// Put x into the list at L if it beats the list's minimum (slot 0).
__device__ __forceinline__ void kbest_insert(volatile unsigned long long* L, int k,
                                             unsigned long long x) {
  if (x <= L[0]) return;
  // minimum of {x} and the k - 1 entries that stay
  unsigned long long mn = x;
  int pos = 0;
  for (int j = 1; j < k; ++j) {
    unsigned long long v = L[j];
    if (v < mn) { mn = v; pos = j; }
  }
  if (pos) L[pos] = x;
  L[0] = mn;
}

// Dynamic LDS: QB * (KSTEPS*32 + kPad) * sizeof(elem) query block, then
// 4 * QB * (k|1) * 8 wave lists, then (SCOPED) QB * 8 q_scope; QB = QT * 16.
// part points at this pass's first query; part_stride = n_q of the call * k.
template <class E, int KSTEPS, int ROWTILES, bool SCOPED>
__global__ void __launch_bounds__(256)
cache_topk_k_kernel_t(const typename E::elem* __restrict__ index, long long n_rows,
                      const typename E::elem* __restrict__ q, int n_q /* <= QB */,
                      int dim, int k, unsigned long long* __restrict__ part,
                      long long part_stride,
                      const long long* __restrict__ row_scope,
                      const int* __restrict__ row_expiry,
                      const long long* __restrict__ q_scope, int now) {
  using elem = typename E::elem;
  using frag_t = typename E::frag;
  constexpr int QT = kbest_qtiles<E, KSTEPS>();
  constexpr int QB = QT * 16;
  constexpr int DIMP = KSTEPS * 32 + E::kPad;
  constexpr int QS_BYTES = QB * DIMP * (int)sizeof(elem);
  const int ls = kbest_list_stride(k);
  extern __shared__ unsigned char smem[];
  elem* qs = reinterpret_cast<elem*>(smem);
  unsigned long long* lists = reinterpret_cast<unsigned long long*>(smem + QS_BYTES);
  long long* qsc_s = reinterpret_cast<long long*>(lists + 4 * QB * ls);
  for (int i = threadIdx.x; i < 4 * QB * ls; i += 256) lists[i] = 0;
  if constexpr (SCOPED) {
    if (threadIdx.x < QB)
      qsc_s[threadIdx.x] = threadIdx.x < (unsigned)n_q ? q_scope[threadIdx.x] : 0;
  }
  int chunks_per_row = dim / 8;
  for (int idx = threadIdx.x; idx < n_q * chunks_per_row; idx += 256) {
    int r = idx / chunks_per_row, c = (idx - r * chunks_per_row) * 8;
    *reinterpret_cast<frag_t*>(&qs[r * DIMP + c]) =
        *reinterpret_cast<const frag_t*>(&q[(long long)r * dim + c]);
  }
  __syncthreads();
  int wave = threadIdx.x >> 6;
  int lane = threadIdx.x & 63;
  int row = lane & 15;
  int kgrp = lane >> 4;
  volatile unsigned long long* wave_lists = lists + wave * QB * ls;
  auto load_tile = [&](frag_t (&frag)[KSTEPS], RowTags& tg, int t) {
    long long i0 = ((long long)blockIdx.x * 4 * ROWTILES + wave * ROWTILES + t) * 16;
    bool i_ok = i0 < n_rows && (i0 + row) < n_rows;
    #pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      int kk = ks * 32 + kgrp * 8;
      if (i_ok)
        frag[ks] = *reinterpret_cast<const frag_t*>(&index[(i0 + row) * dim + kk]);
      else
        frag[ks] = E::zero();
    }
    if constexpr (SCOPED) {
      // compute_tile skips a tile with i0 >= n_rows, so its tags stay unread
      if (i0 < n_rows) load_row_tags(tg, row_scope, row_expiry, i0 + kgrp * 4, n_rows);
    }
  };
  auto compute_tile = [&](frag_t (&frag)[KSTEPS], const RowTags& tg, int t) {
    long long i0 = ((long long)blockIdx.x * 4 * ROWTILES + wave * ROWTILES + t) * 16;
    if (i0 >= n_rows) return;
    floatx4 acc[QT];
    #pragma unroll
    for (int qt = 0; qt < QT; ++qt) acc[qt] = floatx4{0.f, 0.f, 0.f, 0.f};
    int qrow = min(row, n_q - 1);  // LDS reads always in-bounds
    #pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      int kk = ks * 32 + kgrp * 8;
      #pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        frag_t b = *reinterpret_cast<const frag_t*>(&qs[(qt * 16 + qrow) * DIMP + kk]);
        acc[qt] = E::mfma(frag[ks], b, acc[qt]);
      }
    }
    int lim = (int)min((long long)16, n_rows - i0);
    bool live[4];  // in range and not expired: the query-independent half
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      live[r] = kgrp * 4 + r < lim;
      if constexpr (SCOPED) live[r] = live[r] && tg.expiry[r] > now;
    }
    unsigned row0 = (unsigned)((i0 + kgrp * 4) & 0xFFFFFFFF);
    #pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      int ql = qt * 16 + row;
      bool q_in = ql < n_q;
      long long qsc = 0;
      if constexpr (SCOPED) qsc = qsc_s[ql];
      // Mask per element, before anything is reduced: 0 = not eligible
      unsigned long long key[4], p = 0;
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        bool ok = q_in && live[r];
        if constexpr (SCOPED) ok = ok && (qsc == 0 || tg.scope[r] == qsc);
        key[r] = ok ? pack_score(acc[qt][r], row0 + r) : 0ull;
        if (key[r] > p) p = key[r];
      }
      volatile unsigned long long* L = wave_lists + ql * ls;
      unsigned long long m = L[0];
      if (!__any(p > m)) continue;  // fast path: nothing in this tile beats a list
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        bool cand = key[r] > m;
        if (!__any(cand)) continue;
        #pragma unroll
        for (int kg = 0; kg < 4; ++kg) {
          if (cand && kgrp == kg) kbest_insert(L, k, key[r]);
          __builtin_amdgcn_wave_barrier();
        }
      }
    }
  };
  frag_t frag_a[KSTEPS], frag_b[KSTEPS];
  RowTags tag_a, tag_b;
  load_tile(frag_a, tag_a, 0);
  static_assert(ROWTILES % 2 == 0, "pipeline assumes even ROWTILES");
  for (int t = 0; t < ROWTILES; t += 2) {
    load_tile(frag_b, tag_b, t + 1);
    compute_tile(frag_a, tag_a, t);
    if (t + 2 < ROWTILES) load_tile(frag_a, tag_a, t + 2);
    compute_tile(frag_b, tag_b, t + 1);
  }
  __syncthreads();
  // merge the four wave lists: round j takes the largest key below round
  // j - 1's (keys are unique; once a round finds nothing the rest are 0)
  if (threadIdx.x < (unsigned)n_q) {
    unsigned long long* out = part + blockIdx.x * part_stride + (long long)threadIdx.x * k;
    unsigned long long prev = ~0ull;
    for (int j = 0; j < k; ++j) {
      unsigned long long best = 0;
      for (int w = 0; w < 4; ++w) {
        const unsigned long long* Lw = lists + (w * QB + threadIdx.x) * ls;
        for (int e = 0; e < k; ++e) {
          unsigned long long v = Lw[e];
          if (v < prev && v > best) best = v;
        }
      }
      out[j] = best;
      prev = best;
    }
  }
}

// One wave per query: every lane folds its share of the query's blocks * k
// partial keys into a sorted (descending) KMAX-entry register list, then k
// rounds take the wave-wide maximum of the list heads; the lane that held
// it shifts its list down. out[q][0..k) descending, 0 = no row.
template <int KMAX>
__global__ void __launch_bounds__(256)
cache_topk_k_merge_kernel(const unsigned long long* __restrict__ part, long long blocks,
                          int n_q, int k, unsigned long long* __restrict__ out) {
  int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (qi >= n_q) return;  // wave-uniform
  int lane = threadIdx.x & 63;
  unsigned long long l[KMAX];
  #pragma unroll
  for (int j = 0; j < KMAX; ++j) l[j] = 0;
  long long total = blocks * k;
  for (long long i = lane; i < total; i += 64) {
    long long b = i / k;
    int j = (int)(i - b * k);
    unsigned long long x = part[(b * n_q + qi) * k + j];
    if (x > l[KMAX - 1]) {
      l[KMAX - 1] = x;
      #pragma unroll
      for (int s = KMAX - 1; s > 0; --s) {
        if (l[s] > l[s - 1]) {
          unsigned long long tmp = l[s];
          l[s] = l[s - 1];
          l[s - 1] = tmp;
        }
      }
    }
  }
  for (int j = 0; j < k; ++j) {
    unsigned long long mx = l[0];
    #pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      unsigned long long o = shfl_xor_u64(mx, off);
      if (o > mx) mx = o;
    }
    if (mx != 0 && l[0] == mx) {  // keys are unique: exactly one lane
      #pragma unroll
      for (int s = 0; s + 1 < KMAX; ++s) l[s] = l[s + 1];
      l[KMAX - 1] = 0;
    }
    if (lane == 0) out[(long long)qi * k + j] = mx;
  }
}
