// Native cache, MXFP4 index (gfx950): the two kernels csrc/admission.hip adds
// around cache_topk_mxfp4_kernel_t when the in-process index stores MXFP4 rows
// (dim 384: 192 B of nibbles, 12 scale bytes and one fp32 inv_norm per row).
//
//   mxfp4_query_tail_kernel  the batch's query tail in one launch: l2norm of
//                            the fp32 GEMM rows -> bf16 query, its parked copy
//                            for a later insert, and the e4m3 query the lookup
//                            reads. On the other formats these are three
//                            launches (l2norm_rows_kernel, bf16_to_fp8_kernel,
//                            park_pending_kernel); the cache batch is bound by
//                            submit cost, not by GPU time.
//   mxfp4_ring_insert_kernel one wave quantises a parked vector straight into
//                            its ring row, published in the order a racing
//                            lookup needs.
#pragma once

#include <hip/hip_runtime.h>

#include "cache_kernels.cuh"
#include "mxfp4_kernels.cuh"

constexpr int kAdmMxDim = 384;               // the native cache's one row width
constexpr int kAdmMxPerLane = kAdmMxDim / 64;  // 6 elements per lane

// 12 bytes at a 4-byte-aligned address (6 bf16 of lane l start at byte 12 l)
struct alignas(4) AdmMxBf16x6 {
  unsigned w[3];
};

// One wave per request, four requests per block. Lane l owns elements
// 6l..6l+5 of its row: three 8-byte loads, one 12-byte bf16 store per
// destination and three 2-byte e4m3 stores, all contiguous across the wave.
//
// The bf16 row must be bit-identical to l2norm_rows_kernel's, whose lane l
// sums elements l, l+64, .., l+320 in that order before the xor-shuffles run
// from 32 down to 1. fp32 addition does not reassociate, so the sum of
// squares is taken in exactly that order: the row goes through LDS once
// (1536 B per wave, written 8 bytes per lane, read back at stride 64, both
// free of bank conflicts) and the strided lanes run the same fma chain and
// the same shuffle order. The scaled values come from the lane's own
// registers.
__global__ void __launch_bounds__(256)
mxfp4_query_tail_kernel(const float* __restrict__ gout,
                        const int32_t* __restrict__ slots, int n_req,
                        bf16* __restrict__ q, uint8_t* __restrict__ q8,
                        bf16* __restrict__ pending) {
  __shared__ float rows_s[4][kAdmMxDim];
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + wave;
  const bool live = r < n_req;  // wave-uniform; no return before the barrier
  float x[kAdmMxPerLane] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (live) {
    const float2* src = reinterpret_cast<const float2*>(
        &gout[(long long)r * kAdmMxDim + lane * kAdmMxPerLane]);
    #pragma unroll
    for (int j = 0; j < 3; ++j) {
      float2 v = src[j];
      x[2 * j] = v.x;
      x[2 * j + 1] = v.y;
      *reinterpret_cast<float2*>(&rows_s[wave][lane * kAdmMxPerLane + 2 * j]) = v;
    }
  }
  __syncthreads();
  if (!live) return;
  float ss = 0.f;
  for (int c = lane; c < kAdmMxDim; c += 64) {
    float v = rows_s[wave][c];
    ss += v * v;  // the expression of l2norm_rows_kernel, contracted alike
  }
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
  float inv = rsqrtf(ss + 1e-12f);

  AdmMxBf16x6 row;
  unsigned short e4m3[3];
  #pragma unroll
  for (int j = 0; j < 3; ++j) {
    bf16 lo = __float2bfloat16(x[2 * j] * inv);
    bf16 hi = __float2bfloat16(x[2 * j + 1] * inv);
    unsigned short ulo, uhi;
    memcpy(&ulo, &lo, 2);
    memcpy(&uhi, &hi, 2);
    row.w[j] = (unsigned)ulo | ((unsigned)uhi << 16);
    // e4m3 from the bf16-rounded values, as bf16_to_fp8_kernel converts them
    int pk = __builtin_amdgcn_cvt_pk_fp8_f32((float)lo, (float)hi, 0, false);
    e4m3[j] = (unsigned short)(pk & 0xffff);
  }
  const long long at = (long long)r * kAdmMxDim + lane * kAdmMxPerLane;
  *reinterpret_cast<AdmMxBf16x6*>(&q[at]) = row;
  int slot = slots[r];
  if (slot >= 0)
    *reinterpret_cast<AdmMxBf16x6*>(
        &pending[(long long)slot * kAdmMxDim + lane * kAdmMxPerLane]) = row;
  unsigned short* q8_at = reinterpret_cast<unsigned short*>(&q8[at]);
  #pragma unroll
  for (int j = 0; j < 3; ++j) q8_at[j] = e4m3[j];
}

// Ring insert: the quantiser's wave (mxfp4_quantize_row, bit-identical to
// aigw/ops/mxfp4_ref.py) on one parked bf16 vector, written straight into
// ring row `row`: no temporaries, no copies. The row's nibbles and scale
// bytes are stored first, then a device-wide fence, then inv_norm: a lookup
// that races the write may mis-score this one row and no other.
__global__ void __launch_bounds__(64)
mxfp4_ring_insert_kernel(const bf16* __restrict__ vec, long long row,
                         uint8_t* __restrict__ packed, uint8_t* __restrict__ scale,
                         float* __restrict__ inv_norm) {
  mxfp4_quantize_row<true>(vec, kAdmMxDim, packed + row * (kAdmMxDim / 2),
                           scale + row * (kAdmMxDim / 32), inv_norm + row);
}
