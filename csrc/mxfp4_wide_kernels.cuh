// MXFP4 cache lookup for wide rows: dim a runtime multiple of 128 in
// 640..2048, fp4 index rows against fp8 queries on the block-scaled MFMA
// (gfx950).
//
// cache_topk_mxfp4_kernel_t keeps a whole 16-row tile in registers twice and
// stages 128 full-width queries; cache_topk_wide_kernel_t is built on the
// 16x16x32 MFMAs, whose operands share one element order and take no scale.
// This kernel has the contract of the first, best[q] = max over eligible rows
// of pack_score((fp4 row . fp8 query) * inv_norm[row], row) with 0 = no row
// may answer and ties to the higher row, on the pipeline of the second:
// register state that does not depend on dim. A sibling of both, not a flag.
//
// Operands of v_mfma_scale_f32_16x16x128_f8f6f4 (the layouts probed for
// cache_topk_mxfp4_kernel_t, see its comment): per k-step of 128 elements a
// lane holds, for row l&15, the 16 bytes of nibbles at row byte
// ks * 64 + kgrp * 16 (kgrp = l>>4; 32 elements = one MX block) and the
// row's dword of four scale bytes of the k-step, byte kgrp of which is
// shifted into byte 0 when the MFMA issues (a shift at load time would wait
// for the load). The fp8 B operand is 8 VGPRs from two ds_read_b128 64 B
// apart: elements kgrp*16..+15 and 64 + kgrp*16..+15 of the k-step.
//
// Work split: the siblings' grid, 4 waves per block and kMxWideRowTiles
// 16-row tiles per wave, walked kMxWideTiles = 2 tiles (a "group": 32
// consecutive rows) at a time. The two tiles of a group share every query
// fragment, so the two ds_read_b128 of a B operand feed two MFMAs.
//
// K-chunked register pipeline: a group is consumed in chunks of
// kMxWideKsteps k-steps; the last chunk of a row holds what is left
// (dim 640: 4 + 1), a wave-uniform bound on the unrolled k-step loops.
// One flat sequence of chunks runs over the wave's groups and two register
// buffers alternate along it: while one chunk's MFMAs issue, the loads of the
// next chunk in the sequence are in flight, which at a group's last chunk is
// chunk 0 of the next group. Accumulators (8 query tiles x 4 per row tile)
// live across a group's chunks. inv_norm and the row tags are loaded with a
// group's chunk 0 into an incoming set, moved to the current set when that
// chunk is computed, and read only by the epilogue, which runs once per
// group: times inv_norm, mask, pack every element, fold, LDS atomicMax.
//
// Queries in LDS: the fp8 layout of cache_topk_wide_kernel_t (row stride
// dim + 16 bytes, only the ceil(n_q / 16) tiles of a pass staged, tail rows
// zeroed) and its sizing functions: wide_queries_per_pass<CacheElemFp8> is 8
// tiles up to dim 1152, 7 at 1280, 4 at 2048. The host loops passes.
//
// Rows at or past n_rows are never loaded (nibbles, scales, inv_norm, tags);
// a group at or past n_rows ends the wave's work.
#pragma once

#include <hip/hip_runtime.h>

#include "cache_wide_kernels.cuh"
#include "mxfp4_kernels.cuh"

constexpr int kMxWideRowTiles = 16;  // 16-row tiles per wave
constexpr int kMxWideTiles = 2;      // row tiles per group
// k-steps per chunk. One k-step is 20 B per lane per tile (16 B of nibbles,
// a scale dword), so a buffer of KS k-steps keeps KS * 2.5 KB per wave in
// flight. A full pass of 8 query tiles at dim 1024 takes 133 KB of LDS, one
// block per CU and so one wave per SIMD whatever the registers allow: there
// the bytes in flight come from the chunk alone. Measured at 2, 4 and 8
// (profiles/cache_topk_mxfp4_wide.md; 1M rows, 128 queries): 0.351 / 0.348 /
// 0.379 ms at dim 1024 and 0.818 / 0.721 / 0.705 ms at dim 2048. 4 is kept:
// level with 2 at dim 1024, 12% ahead at 2048 and ahead of it in every
// scoped call, and within 4% of 8 where 8 wins; 8 costs 255 VGPRs and loses
// 9% at dim 1024. What 4 gives up: 2 fits two waves per SIMD unscoped (182
// against 223 VGPRs) and is 8% / 22% faster at dim 1024 with 1 / 37 queries.
// The macro is there for that measurement.
#ifndef AIGW_MXWIDE_KSTEPS
#define AIGW_MXWIDE_KSTEPS 4
#endif
constexpr int kMxWideKsteps = AIGW_MXWIDE_KSTEPS;

// a * b as one v_mul_f32. Written as plain products, the epilogue's four
// independent score * inv_norm per accumulator compile to v_pk_mul_f32,
// which this project keeps out of its kernels (mxfp4_kernels.cuh); a
// per-kernel target attribute instead would stop the helpers from inlining.
__device__ __forceinline__ float mx_wide_mul(float a, float b) {
  float r;
  asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

struct MxWideChunkBuf {
  mx_int4 a[kMxWideTiles][kMxWideKsteps];    // 32 nibbles per k-step
  unsigned sc[kMxWideTiles][kMxWideKsteps];  // the row's 4 scale bytes of the k-step
};

// inv_norm and tags of the lane's 4 result rows of each tile of a group
struct MxWideRowMeta {
  floatx4 inv[kMxWideTiles];
  RowTags tg[kMxWideTiles];  // read only when SCOPED
};

// n_q in 1..wide_queries_per_pass<CacheElemFp8, SCOPED>(dim); dynamic LDS
// wide_lds_bytes<CacheElemFp8, SCOPED>(dim, n_q): blk_best, the q_scope stage
// when SCOPED, the query block. row_scope, row_expiry and q_scope are read
// only when SCOPED.
template <bool SCOPED>
__global__ void __launch_bounds__(256)
cache_topk_mxfp4_wide_kernel_t(const uint8_t* __restrict__ packed,
                               const uint8_t* __restrict__ scale,
                               const float* __restrict__ inv_norm, long long n_rows,
                               const uint8_t* __restrict__ q, int n_q, int dim,
                               unsigned long long* __restrict__ best,
                               const long long* __restrict__ row_scope,
                               const int* __restrict__ row_expiry,
                               const long long* __restrict__ q_scope, int now) {
  constexpr int QT = 8;
  constexpr int TI = kMxWideTiles;
  constexpr int KS = kMxWideKsteps;
  constexpr int GROUPS = kMxWideRowTiles / TI;
  static_assert(kMxWideRowTiles % TI == 0, "a wave's tiles split into whole groups");
  using Buf = MxWideChunkBuf;
  using Meta = MxWideRowMeta;

  extern __shared__ unsigned char smem[];
  unsigned long long* blk_best = reinterpret_cast<unsigned long long*>(smem);
  long long* qsc_s = reinterpret_cast<long long*>(smem + 128 * 8);
  unsigned char* qs = smem + wide_aux_bytes<SCOPED>();
  const int stride = wide_row_stride<CacheElemFp8>(dim);
  const int n_qt = (n_q + 15) >> 4;
  const int n_ks = dim >> 7;                     // k-steps per row
  const int n_chunks = (n_ks + KS - 1) / KS;
  if (threadIdx.x < 128) {
    blk_best[threadIdx.x] = 0;
    if (SCOPED) qsc_s[threadIdx.x] = threadIdx.x < (unsigned)n_q ? q_scope[threadIdx.x] : 0;
  }
  const int vpr = dim >> 4;  // 16-byte vectors per query row
  for (int idx = threadIdx.x; idx < n_qt * 16 * vpr; idx += 256) {
    int r = idx / vpr, c = (idx - r * vpr) * 16;
    mx_int4 v = {0, 0, 0, 0};
    if (r < n_q) v = *reinterpret_cast<const mx_int4*>(&q[(long long)r * dim + c]);
    *reinterpret_cast<mx_int4*>(&qs[r * stride + c]) = v;
  }
  __syncthreads();

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int row = lane & 15;
  const int kgrp = lane >> 4;
  const long long tile0 = ((long long)blockIdx.x * 4 + wave) * kMxWideRowTiles;
  const int row_bytes = dim >> 1, row_scales = dim >> 5;
  const unsigned char* q_lane = qs + row * stride + kgrp * 16;

  // first row of group g; a group at or past n_rows is neither loaded nor
  // computed, and neither is any group after it
  auto group_row0 = [&](int g) { return (tile0 + (long long)g * TI) * 16; };

  // chunk c of group g: k-steps c * KS .. of both tiles, those the row has
  auto load_chunk = [&](Buf& buf, int g, int c) __attribute__((always_inline)) {
    long long i0 = group_row0(g);
    #pragma unroll
    for (int ti = 0; ti < TI; ++ti) {
      long long ir = i0 + ti * 16 + row;
      const uint8_t* ap = packed + ir * row_bytes + c * (KS * 64) + kgrp * 16;
      const uint8_t* sp = scale + ir * row_scales + c * (KS * 4);
      #pragma unroll
      for (int k = 0; k < KS; ++k) {
        buf.a[ti][k] = mx_int4{0, 0, 0, 0};
        buf.sc[ti][k] = 0;
        if (c * KS + k < n_ks && ir < n_rows) {
          buf.a[ti][k] = *reinterpret_cast<const mx_int4*>(ap + k * 64);
          buf.sc[ti][k] = *reinterpret_cast<const unsigned*>(sp + k * 4);
        }
      }
    }
  };

  // chunk 0 of group g, and the group's inv_norm and row tags
  auto load_first = [&](Buf& buf, Meta& m, int g) __attribute__((always_inline)) {
    if (g >= GROUPS || group_row0(g) >= n_rows) return;
    load_chunk(buf, g, 0);
    #pragma unroll
    for (int ti = 0; ti < TI; ++ti) {
      // one 16-byte load per full group of 4 result rows; the one that
      // straddles n_rows is read row by row and never past the end
      long long g0 = group_row0(g) + ti * 16 + kgrp * 4;
      if (g0 + 4 <= n_rows) {
        m.inv[ti] = *reinterpret_cast<const floatx4*>(&inv_norm[g0]);
      } else {
        #pragma unroll
        for (int r = 0; r < 4; ++r) m.inv[ti][r] = g0 + r < n_rows ? inv_norm[g0 + r] : 0.f;
      }
      if (SCOPED) load_row_tags(m.tg[ti], row_scope, row_expiry, g0, n_rows);
    }
  };

  auto mfma_chunk = [&](const Buf& buf, floatx4 (&acc)[TI][QT], int c)
                        __attribute__((always_inline)) {
    const unsigned char* bp = q_lane + c * (KS * 128);
    #pragma unroll
    for (int k = 0; k < KS; ++k) {
      if (c * KS + k < n_ks) {
        mx_int8 a[TI];
        int sa[TI];
        #pragma unroll
        for (int ti = 0; ti < TI; ++ti) {
          a[ti] = mx_int8{buf.a[ti][k][0], buf.a[ti][k][1], buf.a[ti][k][2], buf.a[ti][k][3],
                          0, 0, 0, 0};
          sa[ti] = (int)((buf.sc[ti][k] >> (kgrp * 8)) & 0xFFu);
        }
        #pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
          if (qt < n_qt) {
            const unsigned char* p = bp + qt * 16 * stride + k * 128;
            mx_int4 b0 = *reinterpret_cast<const mx_int4*>(p);
            mx_int4 b1 = *reinterpret_cast<const mx_int4*>(p + 64);
            mx_int8 b = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
            #pragma unroll
            for (int ti = 0; ti < TI; ++ti)
              acc[ti][qt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                  a[ti], b, acc[ti][qt], 4 /* A: fp4 e2m1 */, 0 /* B: fp8 e4m3 */, 0, sa[ti],
                  0, 127 /* B scale 2^0 */);
          }
        }
      }
    }
  };

  auto epilogue = [&](const floatx4 (&acc)[TI][QT], const Meta& m, int g)
                      __attribute__((always_inline)) {
    long long i0 = group_row0(g);
    bool live[TI][4];  // in range (and not expired): the query-independent half
    #pragma unroll
    for (int ti = 0; ti < TI; ++ti) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        live[ti][r] = i0 + ti * 16 + kgrp * 4 + r < n_rows;
        if (SCOPED) live[ti][r] = live[ti][r] && m.tg[ti].expiry[r] > now;
      }
    }
    #pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      if (qt < n_qt) {
        int q0 = qt * 16;
        long long qsc = SCOPED ? qsc_s[q0 + row] : 0;
        // the lane's best key over its 4 rows of every tile of the group:
        // every element is packed before anything is reduced, so an exact
        // tie goes to the higher row between two of one lane's rows too;
        // 0 = nothing eligible (pack_score of a real score is never 0)
        unsigned long long p = 0;
        if (q0 + row < n_q) {
          #pragma unroll
          for (int ti = 0; ti < TI; ++ti) {
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
              bool ok = live[ti][r] && (!SCOPED || qsc == 0 || m.tg[ti].scope[r] == qsc);
              long long irow = i0 + ti * 16 + kgrp * 4 + r;
              unsigned long long key = pack_score(mx_wide_mul(acc[ti][qt][r], m.inv[ti][r]),
                                                  (unsigned)(irow & 0xFFFFFFFF));
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
  Meta meta_in, meta_cur;
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
    if (c == 0) {
      #pragma unroll
      for (int ti = 0; ti < TI; ++ti) {
        meta_cur.inv[ti] = meta_in.inv[ti];
        if (SCOPED) meta_cur.tg[ti] = meta_in.tg[ti];
      }
    }
    if (c + 1 < n_chunks)
      load_chunk(nxt, g, c + 1);
    else
      load_first(nxt, meta_in, g + 1);
    mfma_chunk(cur, acc, c);
    if (++c == n_chunks) {
      epilogue(acc, meta_cur, g);
      clear_acc();
      c = 0;
      ++g;
    }
  };
  clear_acc();
  load_first(buf_a, meta_in, 0);
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
