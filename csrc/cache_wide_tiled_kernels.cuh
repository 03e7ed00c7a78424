// Wide-row cache lookup, K-chunked on both operands: up to 256 queries in one
// pass over the index at any width (512 < dim <= 2048, a runtime multiple of
// 128, bf16 and fp8 rows; gfx950).
//
// cache_topk_wide (cache_wide_kernels.cuh) stages full-width queries in LDS,
// so a pass holds 32 bf16 queries at dim 2048 and every further pass streams
// the index again. This kernel returns the same packed key, best[q] = max
// over eligible rows of pack_score(score, row) with 0 = no row may answer,
// from a GEMM tiling whose LDS footprint does not depend on dim. Sibling, not
// a flag: the wide kernel does not move, its helpers are reused.
//
// Queries: a [16 * ceil(n_q / 16) queries x 256 bytes] tile per K step (128
// bf16 or 256 fp8 elements), staged by the whole block from global memory
// (the query matrix is at most 1 MB and stays in L2) into one of two LDS
// buffers while the MFMAs of the previous chunk read the other; one block
// barrier per chunk. A thread's share of a stage goes through registers in two
// halves of 8 query tiles, each held over half a chunk's MFMAs, so its L2
// latency is covered, and is written to LDS behind them. Rows keep the wide kernel's bank padding
// (stride 256 + 16 bytes = 68 dwords, 4 mod 64) and the tail rows of a
// partial query tile are zero. 256 queries: 2 x 69.6 KB, plus 2 KB of
// blk_best and 2 KB of q_scope when scoped.
//
// Index rows go global -> registers as in the wide kernel (every row is
// consumed by exactly one wave): a lane's share of a chunk is one 16-byte
// vector per 64 bytes at byte kgrp * 16, which in fp8 holds two MFMA operands
// and so permutes the 64 elements two k-steps cover, for row and query alike.
// An fp8 row of an odd multiple of 128 elements ends in half a chunk: the
// vectors past the row's end are neither loaded nor multiplied.
//
// Work split: a block is 4 waves over 64 * kWideTiledTiles consecutive rows,
// a wave owns kWideTiledTiles 16-row tiles. Accumulators cover every query
// tile of the call, 16 x kWideTiledTiles x 4 per lane, across the K loop;
// every query fragment read from LDS feeds kWideTiledTiles MFMAs (twice that
// in fp8). The register ping-pong of the row chunks and the LDS double
// buffer alternate along the chunks; the loop body is two steps with the
// buffers swapped, so both are indexed at compile time. Every bound that
// reaches a barrier is block-uniform; a wave whose rows lie past n_rows
// stages queries and loads, multiplies and reduces nothing. A block that
// walked two or four such row groups along one flat chunk sequence measured
// 1% to 5% slower than this and is gone (profiles/cache_topk_wide_tiled.md).
//
// Epilogue: the wide kernel's, once per block. Row tags are loaded under the
// last chunk's MFMAs, into the registers the row prefetch no longer needs, and
// read only there. Every element is
// packed before anything is reduced, so an exact tie goes to the higher row
// everywhere, also between two of one lane's rows.
#pragma once

#include <hip/hip_runtime.h>

#include "cache_wide_kernels.cuh"

// Block-tile variants, for the measurement in profiles/cache_topk_wide_tiled.md.
// Four row tiles per wave (256 accumulator registers) do not fit next to the
// two row buffers and the query stage: the compiler spills to scratch, which
// the project does not ship, so 2 it is.
#ifndef AIGW_WIDE_TILED_TI
#define AIGW_WIDE_TILED_TI 2
#endif
constexpr int kWideTiledTiles = AIGW_WIDE_TILED_TI;  // row tiles per wave
constexpr int kWideTiledBlockRows = 64 * kWideTiledTiles;
constexpr int kWideTiledChunkBytes = 256;
constexpr int kWideTiledStride = kWideTiledChunkBytes + 16;  // bytes between staged rows
constexpr int kWideTiledMaxQueries = 256;

// blk_best, and the q_scope stage when SCOPED, ahead of the two query buffers
template <bool SCOPED>
__host__ __device__ constexpr int wide_tiled_aux_bytes() {
  return (SCOPED ? 2 : 1) * kWideTiledMaxQueries * 8;
}

__host__ __device__ constexpr int wide_tiled_buf_bytes(int n_q) {
  return (n_q + 15) / 16 * 16 * kWideTiledStride;
}

// Dynamic LDS of a call of n_q queries.
template <bool SCOPED>
__host__ __device__ constexpr int wide_tiled_lds_bytes(int n_q) {
  return wide_tiled_aux_bytes<SCOPED>() + 2 * wide_tiled_buf_bytes(n_q);
}
static_assert(wide_tiled_lds_bytes<true>(kWideTiledMaxQueries) <= kWideLdsLimit,
              "a full batch fits the LDS");

struct WideTiledBuf {
  wide_vec a[kWideTiledTiles][kWideTiledChunkBytes / 64];
};

// n_q in 1..256; dim a multiple of 128 in 640..2048. row_scope, row_expiry
// and q_scope are read only when SCOPED.
template <class E, bool SCOPED>
__global__ void __launch_bounds__(256)
cache_topk_wide_tiled_kernel_t(const typename E::elem* __restrict__ index, long long n_rows,
                               const typename E::elem* __restrict__ q, int n_q, int dim,
                               unsigned long long* __restrict__ best,
                               const long long* __restrict__ row_scope,
                               const int* __restrict__ row_expiry,
                               const long long* __restrict__ q_scope, int now) {
  constexpr int ES = (int)sizeof(typename E::elem);
  constexpr int CB = kWideTiledChunkBytes;
  constexpr int VECS = CB / 64;  // a lane's 16-byte vectors per chunk and row
  constexpr int QT = kWideTiledMaxQueries / 16;
  constexpr int TI = kWideTiledTiles;
  constexpr int STRIDE = kWideTiledStride;
  using Buf = WideTiledBuf;

  extern __shared__ unsigned char smem[];
  unsigned long long* blk_best = reinterpret_cast<unsigned long long*>(smem);
  // the q_scope stage exists only when SCOPED
  long long* qsc_s =
      SCOPED ? reinterpret_cast<long long*>(smem + kWideTiledMaxQueries * 8) : nullptr;
  const int n_qt = (n_q + 15) >> 4;
  const int row_bytes = dim * ES;
  const int n_chunks = (row_bytes + CB - 1) / CB;
  unsigned char* qs0 = smem + wide_tiled_aux_bytes<SCOPED>();
  unsigned char* qs1 = qs0 + n_qt * 16 * STRIDE;
  blk_best[threadIdx.x] = 0;
  if (SCOPED) qsc_s[threadIdx.x] = threadIdx.x < (unsigned)n_q ? q_scope[threadIdx.x] : 0;

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int row = lane & 15;
  const int kgrp = lane >> 4;
  const unsigned char* i_bytes = reinterpret_cast<const unsigned char*>(index);
  const unsigned char* q_bytes = reinterpret_cast<const unsigned char*>(q);
  // the thread's share of a query stage: one 16-byte vector of row srow of
  // every query tile
  const int srow = threadIdx.x >> 4;
  const int scol = (threadIdx.x & 15) * 16;
  const int q_lane = row * STRIDE + kgrp * 16;

  // first row of this wave's tiles; a wave past n_rows loads and computes
  // nothing (wave-uniform, and no barrier depends on it)
  const long long i0 = ((long long)blockIdx.x * 4 + wave) * (TI * 16);
  const bool mine = i0 < n_rows;

  // a stage goes through registers in two halves of 8 query tiles
  constexpr int QH = QT / 2;
  wide_vec qreg[QH];
  auto load_q = [&](int c, int half) __attribute__((always_inline)) {
    #pragma unroll
    for (int i = 0; i < QH; ++i) {
      int qt = half * QH + i;
      if (qt < n_qt) {
        int r = qt * 16 + srow, kb = c * CB + scol;
        qreg[i] = wide_vec{0, 0, 0, 0};
        if (r < n_q && kb < row_bytes)
          qreg[i] =
              *reinterpret_cast<const wide_vec*>(&q_bytes[(long long)r * row_bytes + kb]);
      }
    }
  };
  auto store_q = [&](unsigned char* qs, int half) __attribute__((always_inline)) {
    #pragma unroll
    for (int i = 0; i < QH; ++i) {
      int qt = half * QH + i;
      if (qt < n_qt)
        *reinterpret_cast<wide_vec*>(&qs[(qt * 16 + srow) * STRIDE + scol]) = qreg[i];
    }
  };

  auto load_rows = [&](Buf& buf, int c) __attribute__((always_inline)) {
    #pragma unroll
    for (int ti = 0; ti < TI; ++ti) {
      long long ir = i0 + ti * 16 + row;
      const unsigned char* rp = i_bytes + ir * row_bytes + c * CB + kgrp * 16;
      #pragma unroll
      for (int v = 0; v < VECS; ++v) {
        buf.a[ti][v] = wide_vec{0, 0, 0, 0};
        if (ir < n_rows && (ES == 2 || c * CB + v * 64 < row_bytes))
          buf.a[ti][v] = *reinterpret_cast<const wide_vec*>(rp + v * 64);
      }
    }
  };

  // vectors v0..v1-1 of chunk c against the staged query chunk
  auto mfma_chunk = [&](const Buf& buf, floatx4 (&acc)[TI][QT], const unsigned char* qs,
                        int c, int v0, int v1) __attribute__((always_inline)) {
    const unsigned char* bp = qs + q_lane;
    #pragma unroll
    for (int v = v0; v < v1; ++v) {
      if (ES == 2 || c * CB + v * 64 < row_bytes) {
        #pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
          if (qt < n_qt) {
            wide_vec b = *reinterpret_cast<const wide_vec*>(bp + qt * 16 * STRIDE + v * 64);
            #pragma unroll
            for (int ti = 0; ti < TI; ++ti)
              acc[ti][qt] = WideMfma<E>::run(buf.a[ti][v], b, acc[ti][qt]);
          }
        }
      }
    }
  };

  auto epilogue = [&](const floatx4 (&acc)[TI][QT], const RowTags (&tg)[TI])
                      __attribute__((always_inline)) {
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
        // the lane's best key over its 4 rows of every tile of the wave;
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
        // no eligible row in the wave's tiles for this query: no atomic, and a
        // query nothing may answer keeps the best == 0 sentinel
        if (kgrp == 0 && p) atomicMax(&blk_best[q0 + row], p);
      }
    }
  };

  Buf buf_a, buf_b;
  RowTags tags[TI];  // read only when SCOPED
  floatx4 acc[TI][QT];
  #pragma unroll
  for (int ti = 0; ti < TI; ++ti)
    #pragma unroll
    for (int qt = 0; qt < QT; ++qt) acc[ti][qt] = floatx4{0.f, 0.f, 0.f, 0.f};
  int c = 0;  // the chunk whose MFMAs issue next
  // cur and q_cur hold chunk c; nxt and q_nxt take the chunk after it
  auto step = [&](const Buf& cur, Buf& nxt, const unsigned char* q_cur, unsigned char* q_nxt)
                  __attribute__((always_inline)) {
    const bool more = c + 1 < n_chunks;  // block-uniform
    if (more) {
      // the first half ahead of the row loads, so that storing it waits for
      // L2 only, not for the rows
      load_q(c + 1, 0);
      load_rows(nxt, c + 1);
    } else if (SCOPED && mine) {
      // the last chunk has no successor: its registers take the row tags
      #pragma unroll
      for (int ti = 0; ti < TI; ++ti)  // reads no row at or past n_rows
        load_row_tags(tags[ti], row_scope, row_expiry, i0 + ti * 16 + kgrp * 4, n_rows);
    }
    if (mine) mfma_chunk(cur, acc, q_cur, c, 0, VECS / 2);
    // q_nxt was last read before the barrier that ended the previous step
    if (more) {
      store_q(q_nxt, 0);
      load_q(c + 1, 1);
    }
    if (mine) mfma_chunk(cur, acc, q_cur, c, VECS / 2, VECS);
    if (more) {
      store_q(q_nxt, 1);  // behind the row loads, which the next step needs anyway
      __syncthreads();
    }
    ++c;
  };
  load_q(0, 0);
  store_q(qs0, 0);
  load_q(0, 1);
  load_rows(buf_a, 0);
  store_q(qs0, 1);
  __syncthreads();
  for (;;) {
    step(buf_a, buf_b, qs0, qs1);
    if (c == n_chunks) break;
    step(buf_b, buf_a, qs1, qs0);
    if (c == n_chunks) break;
  }
  if (mine) epilogue(acc, tags);
  __syncthreads();
  if (threadIdx.x < (unsigned)n_q && blk_best[threadIdx.x])
    atomicMax(&best[threadIdx.x], blk_best[threadIdx.x]);
}
