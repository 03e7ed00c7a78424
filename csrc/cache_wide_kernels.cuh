// Wide-row cache lookup: 512 < dim <= 2048, a runtime multiple of 128, bf16
// and fp8 rows (gfx950).
//
// The arg-max kernels of cache_kernels.cuh keep a whole 16-row tile in
// registers, twice for their ping-pong, and stage 128 full-width queries in
// LDS; past dim 512 neither fits (a bf16 tile at dim 1024 is 2 x 128 VGPRs,
// 128 queries are 264 KB). This kernel returns the same packed key as
// cache_topk_scoped, best[q] = max over eligible rows of pack_score(score,
// row) with 0 = no row may answer, from a pipeline whose register state does
// not depend on dim. Sibling, not a flag: the narrow kernels do not move.
//
// Work split: the narrow kernels' grid. A block is 4 waves over
// 64 * kWideRowTiles rows, a wave owns kWideRowTiles consecutive 16-row
// tiles and walks them kWideTiles at a time (a "group": 32 consecutive rows).
//
// K-chunked register pipeline: a group is consumed in chunks of 128
// elements, 4 MFMA k-steps of 16x16x32. One flat sequence of chunks runs
// over the wave's groups, (group 0, chunk 0..n-1), (group 1, chunk 0..), and
// two register buffers alternate along it: while the MFMAs of one chunk
// issue, the loads of the next one in the sequence are in flight, which at a
// group's last chunk is chunk 0 of the next group. The loop body is two steps
// with the buffers swapped, so both are indexed at compile time, and an odd
// chunk count only shifts which buffer a group starts in; the loop tests for
// the end between the two steps as well. A buffer is 16 VGPRs per tile in
// bf16 and 8 in fp8; the accumulators (8 query tiles x 4 per row tile) live
// across a group's chunks; the epilogue (mask, pack, fold, LDS atomicMax)
// runs once per group after its last chunk.
//
// A lane's share of a chunk is one 16-byte vector per 64 bytes of the row's
// chunk, at byte kgrp * 16 of each. In bf16 that is the MFMA's own operand
// (8 elements of one k-step). In fp8 a vector holds two operands, so the
// two MFMAs fed by it see k-step elements in the order (kgrp*16 + j) and
// (kgrp*16 + 8 + j): a permutation of the 64 elements both steps cover,
// applied to row and query alike, which a dot product does not notice. It
// halves the global loads and the ds_reads per MFMA against 8-byte operands.
//
// Two row tiles per group share every query fragment read from LDS: one
// ds_read_b128 feeds two MFMAs in bf16 and four in fp8. With one tile per
// read, 4 waves x 1 KB per 16x16x32 bf16 MFMA is the LDS's whole bandwidth.
//
// Query block in LDS, sized by width: full-width queries are staged once per
// block with the narrow kernels' bank padding (row stride dim + 8 elements in
// bf16, dim + 16 bytes in fp8: 4 or 36 mod 64 dwords, so the 16 rows of a
// query tile start 4 banks apart). As many 16-query tiles as fit 160 KB next
// to blk_best and the q_scope stage, at most 8: wide_queries_per_pass, used
// by the launch and the LDS size alike; the host loops passes of that many
// queries, each of which streams the index again. Only the ceil(n_q / 16)
// tiles a pass fills are staged (tail rows zeroed) and computed: the bound on
// the unrolled q-tile loops is wave-uniform, as in cache_topk_mxfp4_kernel_t.
//
// Row tags are loaded with a group's chunk 0 into an incoming set and moved
// to the current set when that chunk is computed (its data has arrived by
// then, so the move waits for nothing new); they are compared only in the
// epilogue. Every element is packed before anything is reduced, so the key
// order holds everywhere: an exact tie goes to the higher row, also between
// two of one lane's rows.
#pragma once

#include <hip/hip_runtime.h>

#include "cache_kernels.cuh"

typedef __attribute__((ext_vector_type(4))) int wide_vec;  // 16 bytes of a row
typedef __attribute__((ext_vector_type(2))) long wide_long2;

constexpr int kWideLdsLimit = 160 * 1024;
constexpr int kWideChunk = 128;    // elements per K chunk
constexpr int kWideRowTiles = 16;  // 16-row tiles per wave
constexpr int kWideTiles = 2;      // row tiles per group
constexpr int kWideMaxDim = 2048;

// acc += rows(a) x queries(b) over the elements of one 16-byte vector
template <class E>
struct WideMfma;

template <>
struct WideMfma<CacheElemBf16> {
  static __device__ __forceinline__ floatx4 run(wide_vec a, wide_vec b, floatx4 c) {
    return CacheElemBf16::mfma(__builtin_bit_cast(short8, a), __builtin_bit_cast(short8, b),
                               c);
  }
};

template <>
struct WideMfma<CacheElemFp8> {
  static __device__ __forceinline__ floatx4 run(wide_vec a, wide_vec b, floatx4 c) {
    wide_long2 a2 = __builtin_bit_cast(wide_long2, a);
    wide_long2 b2 = __builtin_bit_cast(wide_long2, b);
    c = CacheElemFp8::mfma(a2[0], b2[0], c);
    return CacheElemFp8::mfma(a2[1], b2[1], c);
  }
};

// Bytes between two staged query rows.
template <class E>
__host__ __device__ constexpr int wide_row_stride(int dim) {
  return (dim + E::kPad) * (int)sizeof(typename E::elem);
}

// blk_best, and the q_scope stage when SCOPED, ahead of the query block
template <bool SCOPED>
__host__ __device__ constexpr int wide_aux_bytes() {
  return (SCOPED ? 2 : 1) * 128 * 8;
}

// Queries per pass: the 16-query tiles that fit the LDS, at most 8.
template <class E, bool SCOPED>
__host__ __device__ constexpr int wide_queries_per_pass(int dim) {
  int tiles = (kWideLdsLimit - wide_aux_bytes<SCOPED>()) / (16 * wide_row_stride<E>(dim));
  return 16 * (tiles < 8 ? tiles : 8);
}

// Dynamic LDS of a pass of n_q queries.
template <class E, bool SCOPED>
__host__ __device__ constexpr int wide_lds_bytes(int dim, int n_q) {
  return wide_aux_bytes<SCOPED>() + (n_q + 15) / 16 * 16 * wide_row_stride<E>(dim);
}

template <int VECS>
struct WideChunkBuf {
  wide_vec a[kWideTiles][VECS];
};

// n_q in 1..wide_queries_per_pass(dim); dim a multiple of 128 in 640..2048.
// row_scope, row_expiry and q_scope are read only when SCOPED.
template <class E, bool SCOPED>
__global__ void __launch_bounds__(256)
cache_topk_wide_kernel_t(const typename E::elem* __restrict__ index, long long n_rows,
                         const typename E::elem* __restrict__ q, int n_q, int dim,
                         unsigned long long* __restrict__ best,
                         const long long* __restrict__ row_scope,
                         const int* __restrict__ row_expiry,
                         const long long* __restrict__ q_scope, int now) {
  constexpr int ES = (int)sizeof(typename E::elem);
  constexpr int VECS = kWideChunk * ES / 64;  // a lane's 16-byte vectors per chunk
  constexpr int QT = 8;
  constexpr int TI = kWideTiles;
  constexpr int GROUPS = kWideRowTiles / TI;
  static_assert(kWideRowTiles % TI == 0, "a wave's tiles split into whole groups");
  using Buf = WideChunkBuf<VECS>;

  extern __shared__ unsigned char smem[];
  unsigned long long* blk_best = reinterpret_cast<unsigned long long*>(smem);
  long long* qsc_s = reinterpret_cast<long long*>(smem + 128 * 8);
  unsigned char* qs = smem + wide_aux_bytes<SCOPED>();
  const int stride = wide_row_stride<E>(dim);
  const int n_qt = (n_q + 15) >> 4;
  const int n_chunks = dim / kWideChunk;
  if (threadIdx.x < 128) {
    blk_best[threadIdx.x] = 0;
    if (SCOPED) qsc_s[threadIdx.x] = threadIdx.x < (unsigned)n_q ? q_scope[threadIdx.x] : 0;
  }
  const unsigned char* q_bytes = reinterpret_cast<const unsigned char*>(q);
  const int vpr = dim * ES / 16;  // 16-byte vectors per query row
  for (int idx = threadIdx.x; idx < n_qt * 16 * vpr; idx += 256) {
    int r = idx / vpr, c = (idx - r * vpr) * 16;
    wide_vec v = {0, 0, 0, 0};
    if (r < n_q) v = *reinterpret_cast<const wide_vec*>(&q_bytes[(long long)r * dim * ES + c]);
    *reinterpret_cast<wide_vec*>(&qs[r * stride + c]) = v;
  }
  __syncthreads();

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int row = lane & 15;
  const int kgrp = lane >> 4;
  const long long tile0 = ((long long)blockIdx.x * 4 + wave) * kWideRowTiles;
  const unsigned char* i_bytes = reinterpret_cast<const unsigned char*>(index);
  const unsigned char* q_lane = qs + row * stride + kgrp * 16;

  // first row of group g; a group at or past n_rows is neither loaded nor
  // computed, and neither is any group after it
  auto group_row0 = [&](int g) { return (tile0 + (long long)g * TI) * 16; };

  auto load_chunk = [&](Buf& buf, int g, int c) __attribute__((always_inline)) {
    long long i0 = group_row0(g);
    #pragma unroll
    for (int ti = 0; ti < TI; ++ti) {
      long long ir = i0 + ti * 16 + row;
      const unsigned char* rp =
          i_bytes + (ir * dim + (long long)c * kWideChunk) * ES + kgrp * 16;
      #pragma unroll
      for (int v = 0; v < VECS; ++v) {
        buf.a[ti][v] = wide_vec{0, 0, 0, 0};
        if (ir < n_rows) buf.a[ti][v] = *reinterpret_cast<const wide_vec*>(rp + v * 64);
      }
    }
  };

  // chunk 0 of group g and the group's row tags
  auto load_first = [&](Buf& buf, RowTags (&tg)[TI], int g) __attribute__((always_inline)) {
    if (g >= GROUPS || group_row0(g) >= n_rows) return;
    load_chunk(buf, g, 0);
    if (SCOPED) {
      #pragma unroll
      for (int ti = 0; ti < TI; ++ti)  // reads no row at or past n_rows
        load_row_tags(tg[ti], row_scope, row_expiry, group_row0(g) + ti * 16 + kgrp * 4,
                      n_rows);
    }
  };

  auto mfma_chunk = [&](const Buf& buf, floatx4 (&acc)[TI][QT], int c)
                        __attribute__((always_inline)) {
    const unsigned char* bp = q_lane + c * (kWideChunk * ES);
    #pragma unroll
    for (int v = 0; v < VECS; ++v) {
      #pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        if (qt < n_qt) {
          wide_vec b = *reinterpret_cast<const wide_vec*>(bp + qt * 16 * stride + v * 64);
          #pragma unroll
          for (int ti = 0; ti < TI; ++ti)
            acc[ti][qt] = WideMfma<E>::run(buf.a[ti][v], b, acc[ti][qt]);
        }
      }
    }
  };

  auto epilogue = [&](const floatx4 (&acc)[TI][QT], const RowTags (&tg)[TI], int g)
                      __attribute__((always_inline)) {
    long long i0 = group_row0(g);
    bool live[TI][4];  // in range (and not expired): the query-independent half
    #pragma unroll
    for (int ti = 0; ti < TI; ++ti) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        live[ti][r] = i0 + ti * 16 + kgrp * 4 + r < n_rows;
        if (SCOPED) live[ti][r] = live[ti][r] && tg[ti].expiry[r] > now;
      }
    }
    #pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      if (qt < n_qt) {
        int q0 = qt * 16;
        long long qsc = SCOPED ? qsc_s[q0 + row] : 0;
        // the lane's best key over its 4 rows of every tile of the group;
        // 0 = nothing eligible (pack_score of a real score is never 0)
        unsigned long long p = 0;
        if (q0 + row < n_q) {
          #pragma unroll
          for (int ti = 0; ti < TI; ++ti) {
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
              bool ok = live[ti][r] && (!SCOPED || qsc == 0 || tg[ti].scope[r] == qsc);
              long long irow = i0 + ti * 16 + kgrp * 4 + r;
              unsigned long long key = pack_score(acc[ti][qt][r], (unsigned)(irow & 0xFFFFFFFF));
              if (ok && key > p) p = key;
            }
          }
        }
        #pragma unroll
        for (int off = 16; off < 64; off <<= 1) {
          unsigned long long o = shfl_xor_u64(p, off);
          if (o > p) p = o;
        }
        // no eligible row in the group for this query: no atomic, and a
        // query nothing may answer keeps the best == 0 sentinel
        if (kgrp == 0 && p) atomicMax(&blk_best[q0 + row], p);
      }
    }
  };

  Buf buf_a, buf_b;
  RowTags tag_in[TI], tag_cur[TI];  // read only when SCOPED
  floatx4 acc[TI][QT];
  auto clear_acc = [&]() __attribute__((always_inline)) {
    #pragma unroll
    for (int ti = 0; ti < TI; ++ti)
      #pragma unroll
      for (int qt = 0; qt < QT; ++qt) acc[ti][qt] = floatx4{0.f, 0.f, 0.f, 0.f};
  };
  int g = 0, c = 0;  // the group and chunk whose MFMAs issue next
  auto done = [&]() { return g >= GROUPS || group_row0(g) >= n_rows; };
  // cur holds chunk (g, c), loaded or in flight; nxt takes the chunk after it
  auto step = [&](const Buf& cur, Buf& nxt) __attribute__((always_inline)) {
    if (c == 0 && SCOPED) {
      #pragma unroll
      for (int ti = 0; ti < TI; ++ti) tag_cur[ti] = tag_in[ti];
    }
    if (c + 1 < n_chunks)
      load_chunk(nxt, g, c + 1);
    else
      load_first(nxt, tag_in, g + 1);
    mfma_chunk(cur, acc, c);
    if (++c == n_chunks) {
      epilogue(acc, tag_cur, g);
      clear_acc();
      c = 0;
      ++g;
    }
  };
  clear_acc();
  load_first(buf_a, tag_in, 0);
  for (;;) {
    if (done()) break;
    step(buf_a, buf_b);
    if (done()) break;
    step(buf_b, buf_a);
  }
  __syncthreads();
  if (threadIdx.x < (unsigned)n_q && blk_best[threadIdx.x])
    atomicMax(&best[threadIdx.x], blk_best[threadIdx.x]);
}
