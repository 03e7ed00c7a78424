// MXFP4 semantic-cache index (gfx950): the row quantiser and the fused
// similarity + argmax lookup on the block-scaled MFMA. The format is
// specified by aigw/ops/mxfp4_ref.py: 32-element blocks, one E8M0 scale
// byte per block (smallest power of two that does not clip), e2m1 nibbles
// with element 2i in the low nibble of byte i, one fp32 inv_norm per row.
// Included after cache_kernels.cuh, whose pack_score, shfl_xor_u64, RowTags
// and load_row_tags it reuses.
#pragma once

#include <hip/hip_runtime.h>

#include "cache_kernels.cuh"

typedef __attribute__((ext_vector_type(4))) int mx_int4;
typedef __attribute__((ext_vector_type(8))) int mx_int8;

// ---------------------------------------------------------------------------
// Quantiser: bf16 [n, dim] -> packed nibbles, scale bytes, inv_norm.
// One wave per row, lane l owns elements 8l..8l+7 (dim <= 512), so the
// four lanes 4b..4b+3 hold MX block b and its amax is two xor-shuffles.
// Finite inputs only. Every scaling by a power of two is an ldexpf (exact,
// one v_ldexp_f32 each) and the only other fp32 arithmetic is the serial
// fma chain of the norm, so the compiler has no independent fp32 multiplies
// or adds to pair into packed ops (v_pk_mul_f32 and kin), which this
// kernel's bit-exact outputs must not depend on.
// ---------------------------------------------------------------------------

// The wave's work on one row, given the row's own pointers; shared with the
// native cache's ring insert (admission_mxfp4_kernels.cuh). PUBLISH orders
// the row's stores for a concurrent lookup: nibbles and scales, a device-wide
// fence, inv_norm last.
template <bool PUBLISH>
__device__ __forceinline__ void mxfp4_quantize_row(
    const bf16* __restrict__ x, int dim, uint8_t* __restrict__ packed,
    uint8_t* __restrict__ scale, float* __restrict__ inv_norm) {
  int lane = threadIdx.x & 63;
  bool on = lane * 8 < dim;
  short8 raw = {0, 0, 0, 0, 0, 0, 0, 0};
  if (on) raw = *reinterpret_cast<const short8*>(&x[lane * 8]);
  // |bf16| bit patterns order like the magnitudes they encode
  int am = 0;
  #pragma unroll
  for (int j = 0; j < 8; ++j) am = max(am, (int)raw[j] & 0x7FFF);
  am = max(am, __shfl_xor(am, 1));
  am = max(am, __shfl_xor(am, 2));
  // Smallest e with 6 * 2^e >= amax, from the exponent and mantissa fields
  // (no log2f: amax == 6 * 2^k must give k and the next bf16 k + 1).
  // amax = (1 + mant/128) * 2^(E-127) and 6 * 2^e = 1.5 * 2^(e+2), so
  // e = E - 127 - 2 when mant/128 <= 0.5 and one more otherwise. A bf16
  // subnormal amax lands below -127 and clamps with the small normals.
  int e = (am >> 7) - 127 - ((am & 0x7F) <= 0x40 ? 2 : 1);
  e = max(e, -127);
  if (am == 0) e = 0;  // all-zero block: scale byte 127
  // Row-wide exponent for the norm: squares of 2^100 or 2^-120 values do
  // not fit fp32, so the sum runs over values scaled by 2^-emax.
  int emax = (on && am) ? e : -1000;
  #pragma unroll
  for (int off = 1; off < 64; off <<= 1) emax = max(emax, __shfl_xor(emax, off));
  // below 2^-60 of the largest block a term is far under the sum's ulp
  bool counts = emax > -1000 && e - emax >= -60;
  unsigned word = 0;
  float ss = 0.f;
  #pragma unroll
  for (int j = 0; j < 8; ++j) {
    unsigned bits = (unsigned short)raw[j];
    float a = ldexpf(__uint_as_float((bits & 0x7FFFu) << 16), -e);  // |x| / 2^e, exact
    // Round to nearest e2m1 {0 .5 1 1.5 2 3 4 6}: one compare per midpoint,
    // inclusive where the code above has the even mantissa bit (ties to
    // even). a <= 6 by the choice of e; the clamp is the last code.
    bool c1 = a > 0.25f, c2 = a >= 0.75f, c3 = a > 1.25f, c4 = a >= 1.75f;
    bool c5 = a > 2.5f, c6 = a >= 3.5f, c7 = a > 5.f;
    unsigned code = c1 + c2 + c3 + c4 + c5 + c6 + c7;
    int twice = c1 + c2 + c3 + c4 + 2 * (c5 + c6) + 4 * c7;  // 2 * |e2m1 value|
    word |= (code | ((bits >> 15) << 3)) << (4 * j);  // sign kept, -0 too
    float d = counts ? ldexpf((float)twice, e - emax - 1) : 0.f;
    ss = fmaf(d, d, ss);
  }
  if (on) {
    *reinterpret_cast<unsigned*>(&packed[lane * 4]) = word;
    if ((lane & 3) == 0) scale[lane >> 2] = (uint8_t)(e + 127);
  }
  #pragma unroll
  for (int off = 1; off < 64; off <<= 1) ss += __shfl_xor(ss, off);
  if (PUBLISH) __threadfence();
  if (lane == 0) *inv_norm = ss > 0.f ? ldexpf(rsqrtf(ss), -emax) : 0.f;
}

__global__ void __launch_bounds__(256)
mxfp4_quantize_rows_kernel(const bf16* __restrict__ x, long long n, int dim,
                           uint8_t* __restrict__ packed, uint8_t* __restrict__ scale,
                           float* __restrict__ inv_norm) {
  long long r = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (r >= n) return;  // wave-uniform
  mxfp4_quantize_row<false>(x + r * dim, dim, packed + r * (dim / 2),
                            scale + r * (dim / 32), inv_norm + r);
}

// Wide rows: dim a multiple of 128 in 640..2048. Still one wave per row; the
// row is cut into slabs of 512 elements and lane l owns elements 8l..8l+7 of
// every slab, so a row is at most 4 short8 per lane and MX block b of a slab
// is lanes 4b..4b+3 as above. The last slab may be partial (640 = 512 + 128):
// a lane with s * 512 + 8l >= dim is off for that slab. The row-wide emax is
// reduced over every slab before any square is summed, and the squares of all
// slabs run down one fma chain per lane, so the arithmetic discipline of the
// kernel above holds here too. A sibling: the kernel above does not move.
constexpr int kMxQuantSlab = 512;
constexpr int kMxQuantMaxSlabs = 4;

__global__ void __launch_bounds__(256)
mxfp4_quantize_rows_wide_kernel(const bf16* __restrict__ x, long long n, int dim,
                                uint8_t* __restrict__ packed, uint8_t* __restrict__ scale,
                                float* __restrict__ inv_norm) {
  long long r = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (r >= n) return;  // wave-uniform
  int lane = threadIdx.x & 63;
  short8 raw[kMxQuantMaxSlabs];
  int e[kMxQuantMaxSlabs];
  int emax = -1000;
  #pragma unroll
  for (int s = 0; s < kMxQuantMaxSlabs; ++s) {
    raw[s] = short8{0, 0, 0, 0, 0, 0, 0, 0};
    e[s] = 0;
    if (s * kMxQuantSlab >= dim) continue;  // wave-uniform: the row has no such slab
    bool on = s * kMxQuantSlab + lane * 8 < dim;
    if (on)
      raw[s] = *reinterpret_cast<const short8*>(&x[r * dim + s * kMxQuantSlab + lane * 8]);
    int am = 0;
    #pragma unroll
    for (int j = 0; j < 8; ++j) am = max(am, (int)raw[s][j] & 0x7FFF);
    am = max(am, __shfl_xor(am, 1));
    am = max(am, __shfl_xor(am, 2));
    // the scale rule of mxfp4_quantize_rows_kernel
    int es = (am >> 7) - 127 - ((am & 0x7F) <= 0x40 ? 2 : 1);
    es = max(es, -127);
    if (am == 0) es = 0;
    e[s] = es;
    if (on && am) emax = max(emax, es);
  }
  #pragma unroll
  for (int off = 1; off < 64; off <<= 1) emax = max(emax, __shfl_xor(emax, off));
  float ss = 0.f;
  #pragma unroll
  for (int s = 0; s < kMxQuantMaxSlabs; ++s) {
    if (s * kMxQuantSlab >= dim) continue;
    bool on = s * kMxQuantSlab + lane * 8 < dim;
    bool counts = emax > -1000 && e[s] - emax >= -60;
    unsigned word = 0;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      unsigned bits = (unsigned short)raw[s][j];
      float a = ldexpf(__uint_as_float((bits & 0x7FFFu) << 16), -e[s]);  // exact
      bool c1 = a > 0.25f, c2 = a >= 0.75f, c3 = a > 1.25f, c4 = a >= 1.75f;
      bool c5 = a > 2.5f, c6 = a >= 3.5f, c7 = a > 5.f;
      unsigned code = c1 + c2 + c3 + c4 + c5 + c6 + c7;
      int twice = c1 + c2 + c3 + c4 + 2 * (c5 + c6) + 4 * c7;  // 2 * |e2m1 value|
      word |= (code | ((bits >> 15) << 3)) << (4 * j);
      float d = counts ? ldexpf((float)twice, e[s] - emax - 1) : 0.f;
      ss = fmaf(d, d, ss);
    }
    if (on) {
      long long el = s * kMxQuantSlab + lane * 8;  // the lane's first element
      *reinterpret_cast<unsigned*>(&packed[r * (dim / 2) + el / 2]) = word;
      if ((lane & 3) == 0) scale[r * (dim / 32) + el / 32] = (uint8_t)(e[s] + 127);
    }
  }
  #pragma unroll
  for (int off = 1; off < 64; off <<= 1) ss += __shfl_xor(ss, off);
  if (lane == 0) inv_norm[r] = ss > 0.f ? ldexpf(rsqrtf(ss), -emax) : 0.f;
}

// ---------------------------------------------------------------------------
// Lookup: best[q] = max over rows of pack_score(score, row),
//   score = (fp4 row . fp8 query) * inv_norm[row],
// same contract as cache_topk / cache_topk_scoped (ties to the higher row;
// SCOPED masks per element before any reduction and leaves best == 0 for a
// query no row may answer).
//
// One v_mfma_scale_f32_16x16x128_f8f6f4 per (16 rows x 16 queries x 128 k):
//   A (fp4 index, cbsz 4): lane l holds row l&15, elements (l>>4)*32..+31 of
//     the k-step = 16 B = one dwordx4 load in the low 4 VGPRs of the
//     operand. Those 32 elements are one MX block, so the lane's scale is
//     byte (l>>4) of the row's 4 scale bytes of the k-step: one dword load,
//     shifted into byte 0 (opsel is per instruction, not per lane).
//   B (fp8 e4m3 queries, blgp 0): lane l holds query l&15 in 8 VGPRs, and
//     an 8-bit operand is laid out as two 64-element halves: bytes 0..15
//     are elements (l>>4)*16..+15 of the k-step, bytes 16..31 elements
//     64 + (l>>4)*16..+15. Two ds_read_b128, 64 B apart, from the staged
//     block; scale 127.
//   C: lane l, reg r -> row (l>>4)*4 + r, query l&15, as the 16x16x32 MFMAs.
// Found by a one-hot probe of the instruction on an MI355X (the 4-bit and
// 8-bit operands do not share an element order) and held by
// tests/test_gpu_cache_mxfp4.py: asymmetric inputs, per-block scale spread.
//
// Only n_qt = ceil(n_q/16) query tiles are staged and computed: the bound
// on the unrolled q-tile loops is wave-uniform, so accumulators stay in
// registers and a skipped tile costs one scalar branch. LDS holds
// n_qt*16 query rows (tail rows zeroed), so small batches also fit more
// CTAs per CU. Query row stride dim+16 B: dim/4 is 32 or 0 mod 64 dwords,
// +4 makes the stride 4*odd mod 64, so the 16 rows a 16-lane group reads
// with one ds_read_b128 start 4 banks apart and tile all 64 banks.
//
// A 16-row tile is ~3 KB at dim 384 (20 B per lane per k-step). Two tiles
// in flight per wave (the siblings' register ping-pong) measured within 2%
// of four and ahead of eight: profiles/cache_topk_mxfp4.md.
// ---------------------------------------------------------------------------

template <int KSTEPS>
struct Mxfp4Tile {
  mx_int4 a[KSTEPS];    // 32 nibbles per k-step
  unsigned sc[KSTEPS];  // the row's 4 scale bytes of the k-step
  floatx4 inv;          // inv_norm of the lane's 4 result rows
};

// Dynamic LDS: blk_best 128*8, q_scope 128*8 when SCOPED, then the query
// block of n_qt*16 rows of dim+16 bytes.
template <int KSTEPS, int ROWTILES, bool SCOPED>
__global__ void __launch_bounds__(256)
cache_topk_mxfp4_kernel_t(const uint8_t* __restrict__ packed,
                          const uint8_t* __restrict__ scale,
                          const float* __restrict__ inv_norm, long long n_rows,
                          const uint8_t* __restrict__ q, int n_q /* 1..128 */,
                          unsigned long long* __restrict__ best,
                          const long long* __restrict__ row_scope,
                          const int* __restrict__ row_expiry,
                          const long long* __restrict__ q_scope, int now) {
  constexpr int DIM = KSTEPS * 128;
  constexpr int DIMP = DIM + 16;
  constexpr int QT = 8;  // 128 queries / 16
  static_assert(ROWTILES % 2 == 0, "pipeline assumes even ROWTILES");
  extern __shared__ unsigned char smem[];
  unsigned long long* blk_best = reinterpret_cast<unsigned long long*>(smem);
  long long* qsc_s = reinterpret_cast<long long*>(smem + 128 * 8);
  uint8_t* qs = smem + (SCOPED ? 2 : 1) * 128 * 8;
  const int n_qt = (n_q + 15) >> 4;
  if (threadIdx.x < 128) {
    blk_best[threadIdx.x] = 0;
    if (SCOPED) qsc_s[threadIdx.x] = threadIdx.x < (unsigned)n_q ? q_scope[threadIdx.x] : 0;
  }
  constexpr int CPR = DIM / 16;  // 16-byte chunks per query row
  for (int idx = threadIdx.x; idx < n_qt * 16 * CPR; idx += 256) {
    int r = idx / CPR, c = (idx - r * CPR) * 16;
    mx_int4 v = {0, 0, 0, 0};
    if (r < n_q) v = *reinterpret_cast<const mx_int4*>(&q[(long long)r * DIM + c]);
    *reinterpret_cast<mx_int4*>(&qs[r * DIMP + c]) = v;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int row = lane & 15;
  const int kgrp = lane >> 4;
  const long long tile0 = ((long long)blockIdx.x * 4 + wave) * ROWTILES;

  auto load_tile = [&](Mxfp4Tile<KSTEPS>& tl, RowTags& tg, int t) {
    long long i0 = (tile0 + t) * 16;
    if (i0 >= n_rows) return;  // compute_tile skips it too
    long long ir = i0 + row;
    #pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      tl.a[ks] = mx_int4{0, 0, 0, 0};
      tl.sc[ks] = 0;
      if (ir < n_rows) {
        tl.a[ks] = *reinterpret_cast<const mx_int4*>(
            &packed[ir * (DIM / 2) + ks * 64 + kgrp * 16]);
        tl.sc[ks] = *reinterpret_cast<const unsigned*>(&scale[ir * (DIM / 32) + ks * 4]);
      }
    }
    // one 16-byte load per full group of 4 result rows; the group that
    // straddles n_rows is read row by row and never past the end
    long long g0 = i0 + kgrp * 4;
    if (g0 + 4 <= n_rows) {
      tl.inv = *reinterpret_cast<const floatx4*>(&inv_norm[g0]);
    } else {
      #pragma unroll
      for (int r = 0; r < 4; ++r) tl.inv[r] = g0 + r < n_rows ? inv_norm[g0 + r] : 0.f;
    }
    if (SCOPED) load_row_tags(tg, row_scope, row_expiry, g0, n_rows);
  };

  auto compute_tile = [&](const Mxfp4Tile<KSTEPS>& tl, const RowTags& tg,
                          int t) {
    long long i0 = (tile0 + t) * 16;
    if (i0 >= n_rows) return;
    floatx4 acc[QT];
    #pragma unroll
    for (int qt = 0; qt < QT; ++qt) acc[qt] = floatx4{0.f, 0.f, 0.f, 0.f};
    #pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      mx_int8 a = {tl.a[ks][0], tl.a[ks][1], tl.a[ks][2], tl.a[ks][3], 0, 0, 0, 0};
      int sa = (int)((tl.sc[ks] >> (kgrp * 8)) & 0xFFu);
      #pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        if (qt < n_qt) {
          const uint8_t* bp = &qs[(qt * 16 + row) * DIMP + ks * 128 + kgrp * 16];
          mx_int4 b0 = *reinterpret_cast<const mx_int4*>(bp);
          mx_int4 b1 = *reinterpret_cast<const mx_int4*>(bp + 64);
          mx_int8 b = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
          acc[qt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              a, b, acc[qt], 4 /* A: fp4 e2m1 */, 0 /* B: fp8 e4m3 */, 0, sa, 0,
              127 /* B scale 2^0 */);
        }
      }
    }
    int lim = (int)min((long long)16, n_rows - i0);
    bool live[4];  // in range (and not expired): the query-independent half
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      live[r] = kgrp * 4 + r < lim;
      if (SCOPED) live[r] = live[r] && tg.expiry[r] > now;
    }
    #pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      if (qt < n_qt) {
        int q0 = qt * 16;
        long long qsc = SCOPED ? qsc_s[q0 + row] : 0;
        // mask per element, before the lane's 4-way max; ties go to the
        // higher row, as pack_score's do across lanes
        float best_s = 0.f;
        int best_r = -1;
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          float s = acc[qt][r] * tl.inv[r];
          bool ok = live[r] && (!SCOPED || qsc == 0 || tg.scope[r] == qsc);
          if (ok && (best_r < 0 || s >= best_s)) {
            best_s = s;
            best_r = r;
          }
        }
        // 0 = nothing eligible (pack_score of a real score is never 0)
        unsigned long long p = 0;
        if (best_r >= 0 && (q0 + row) < n_q) {
          long long irow = i0 + kgrp * 4 + best_r;
          p = pack_score(best_s, (unsigned)(irow & 0xFFFFFFFF));
        }
        #pragma unroll
        for (int off = 16; off < 64; off <<= 1) {
          unsigned long long o = shfl_xor_u64(p, off);
          if (o > p) p = o;
        }
        if (kgrp == 0 && p) atomicMax(&blk_best[q0 + row], p);
      }
    }
  };

  Mxfp4Tile<KSTEPS> tile_a, tile_b;
  RowTags tag_a, tag_b;  // read only when SCOPED
  load_tile(tile_a, tag_a, 0);
  for (int t = 0; t < ROWTILES; t += 2) {
    load_tile(tile_b, tag_b, t + 1);
    compute_tile(tile_a, tag_a, t);
    if (t + 2 < ROWTILES) load_tile(tile_a, tag_a, t + 2);
    compute_tile(tile_b, tag_b, t + 1);
  }
  __syncthreads();
  if (threadIdx.x < (unsigned)n_q && blk_best[threadIdx.x])
    atomicMax(&best[threadIdx.x], blk_best[threadIdx.x]);
}
