// aigw MI355X (gfx950 / CDNA4) kernels.
//
// GPU tier of the gateway (BASELINE.json north star; no counterpart code in
// the reference, which does this work CPU-side or not at all —
// SURVEY.md §2.4):
//
//   1. Byte-level BPE tokenizer (segmenter + wave-per-segment merge loop)
//      — replaces the reference's provider-usage-JSON token accounting
//      (translator/openai_openai.go:185-223) and /tokenize passthrough
//      (translator/tokenize.go:24-81) with gateway-local counting.
//   2. Mean-pool embedding + MFMA bf16 projection GEMM — semantic response
//      cache (the reference's cache is provider-side passthrough).
//   3. Fused MFMA similarity + argmax over the HBM-resident cache index.
//   4. KV-occupancy endpoint scorer — replaces the external EPP service
//      (extensionserver/inferencepool.go:39-54).
//   5. Prefix-cache-aware picking: chained token-block hashes and an
//      HBM-resident block -> replica-mask index feeding the scorer (the
//      EPP's prefix-cache-scorer, on real token blocks).
//
// CDNA4 specifics used (per the MI355X HIP guide): 64-wide wavefronts
// (64-bit ballot masks), __builtin_amdgcn_mfma_f32_16x16x32_bf16 with the
// C/D mapping col=lane&15 / row=(lane>>4)*4+reg, LDS staging, short8
// vectorized bf16 loads, grid-stride loops sized for 256 CUs.

#include <hip/hip_runtime.h>
#include <algorithm>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdint>

#define AIGW_CHECK(cond, msg) TORCH_CHECK(cond, msg)

using bf16 = __hip_bfloat16;
typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) float floatx4;
typedef __attribute__((ext_vector_type(4))) short short4v;

static inline hipStream_t current_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

// ---------------------------------------------------------------------------
// 1. BPE tokenizer
// ---------------------------------------------------------------------------

#include "bpe_kernels.cuh"

// ---------------------------------------------------------------------------
// 2. Embedding: mean-pool token embeddings per request (memory-bound)
// ---------------------------------------------------------------------------

#include "cache_kernels.cuh"

// ---------------------------------------------------------------------------
// 5. Prefix-cache-aware endpoint picking (block hashes, HBM block index)
// ---------------------------------------------------------------------------

#include "prefix_kernels.cuh"

// ---------------------------------------------------------------------------
// Host wrappers
// ---------------------------------------------------------------------------

static void check_cuda(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// Returns (seg_start, seg_req, n_segs is seg_start.numel())

std::vector<at::Tensor> bpe_segment(at::Tensor bytes, at::Tensor req_off) {
  check_cuda(bytes, "bytes");
  check_cuda(req_off, "req_off");
  int n = (int)bytes.numel();
  TORCH_CHECK(n > 0, "empty batch");
  auto stream = current_stream();
  auto u8 = at::TensorOptions().dtype(at::kByte).device(bytes.device());
  auto i32 = at::TensorOptions().dtype(at::kInt).device(bytes.device());
  at::Tensor flags = at::empty({n}, u8);
  int blocks = (n + 255) / 256;
  hipLaunchKernelGGL(seg_flags_kernel, dim3(blocks), dim3(256), 0, stream,
                     bytes.data_ptr<uint8_t>(), n, flags.data_ptr<uint8_t>());
  int n_req = (int)req_off.numel();
  hipLaunchKernelGGL(seg_force_starts_kernel, dim3((n_req + 255) / 256), dim3(256), 0,
                     stream, req_off.data_ptr<int64_t>(), n_req, n,
                     flags.data_ptr<uint8_t>());
  at::Tensor blk_counts = at::empty({blocks}, i32);
  hipLaunchKernelGGL(seg_block_count_kernel, dim3(blocks), dim3(256), 0, stream,
                     flags.data_ptr<uint8_t>(), n, blk_counts.data_ptr<int32_t>());
  at::Tensor scan = blk_counts.cumsum(0, at::kInt);
  at::Tensor blk_excl = at::zeros({blocks}, i32);
  if (blocks > 1)
    blk_excl.narrow(0, 1, blocks - 1).copy_(scan.narrow(0, 0, blocks - 1));
  int n_segs = scan[blocks - 1].item<int>();  // one D2H sync per batch
  at::Tensor seg_start = at::empty({n_segs}, i32);
  at::Tensor seg_req = at::empty({n_segs}, i32);
  hipLaunchKernelGGL(seg_write_kernel, dim3(blocks), dim3(256), 0, stream,
                     flags.data_ptr<uint8_t>(), n, blk_excl.data_ptr<int32_t>(),
                     req_off.data_ptr<int64_t>(), n_req,
                     seg_start.data_ptr<int32_t>(), seg_req.data_ptr<int32_t>());
  return {seg_start, seg_req};
}

std::vector<at::Tensor> bpe_encode(at::Tensor bytes, at::Tensor req_off,
                                   at::Tensor htab_keys, at::Tensor htab_rank) {
  check_cuda(bytes, "bytes");
  check_cuda(req_off, "req_off");
  check_cuda(htab_keys, "htab_keys");
  check_cuda(htab_rank, "htab_rank");
  auto segs = bpe_segment(bytes, req_off);
  at::Tensor seg_start = segs[0], seg_req = segs[1];
  int n_segs = (int)seg_start.numel();
  int n = (int)bytes.numel();
  int n_req = (int)req_off.numel();
  auto i32 = at::TensorOptions().dtype(at::kInt).device(bytes.device());
  at::Tensor out_ids = at::full({n}, -1, i32);
  at::Tensor req_counts = at::zeros({n_req}, i32);
  int htab_mask = (int)htab_keys.numel() - 1;
  TORCH_CHECK((htab_keys.numel() & htab_mask) == 0, "htab size must be power of 2");
  auto stream = current_stream();

  // group segments (scheduling-only wave packing; see
  // bpe_encode_grouped_kernel)
  auto u8 = at::TensorOptions().dtype(at::kByte).device(bytes.device());
  at::Tensor gflags = at::empty({n_segs}, i32.dtype(at::kByte));
  int seg_blocks = (n_segs + 255) / 256;
  hipLaunchKernelGGL(group_head_flags_kernel, dim3(seg_blocks), dim3(256), 0, stream,
                     seg_start.data_ptr<int32_t>(), seg_req.data_ptr<int32_t>(),
                     n_segs, req_off.data_ptr<int64_t>(), gflags.data_ptr<uint8_t>());
  at::Tensor gblk = at::empty({seg_blocks}, i32);
  hipLaunchKernelGGL(seg_block_count_kernel, dim3(seg_blocks), dim3(256), 0, stream,
                     gflags.data_ptr<uint8_t>(), n_segs, gblk.data_ptr<int32_t>());
  at::Tensor gscan = gblk.cumsum(0, at::kInt);
  at::Tensor gexcl = at::zeros({seg_blocks}, i32);
  if (seg_blocks > 1)
    gexcl.narrow(0, 1, seg_blocks - 1).copy_(gscan.narrow(0, 0, seg_blocks - 1));
  int n_groups = gscan[seg_blocks - 1].item<int>();
  at::Tensor ghead = at::empty({n_groups}, i32);
  hipLaunchKernelGGL(flag_compact_write_kernel, dim3(seg_blocks), dim3(256), 0, stream,
                     gflags.data_ptr<uint8_t>(), n_segs, gexcl.data_ptr<int32_t>(),
                     ghead.data_ptr<int32_t>());
  (void)u8;

  int blocks = (n_groups + 3) / 4;  // 4 waves per 256-thread block
  hipLaunchKernelGGL(bpe_encode_grouped_kernel, dim3(blocks), dim3(256), 0, stream,
                     bytes.data_ptr<uint8_t>(), seg_start.data_ptr<int32_t>(),
                     seg_req.data_ptr<int32_t>(), n_segs, n,
                     ghead.data_ptr<int32_t>(), n_groups,
                     reinterpret_cast<long long*>(htab_keys.data_ptr<int64_t>()),
                     htab_rank.data_ptr<int32_t>(), htab_mask,
                     out_ids.data_ptr<int32_t>(), req_counts.data_ptr<int32_t>());
  return {out_ids, req_counts, seg_start, seg_req};
}

// Fully async tokenize: ZERO host syncs. Segment/group totals stay in
// device scalars (scan tails) and every kernel self-bounds; intermediate
// arrays use upper bounds (#segments <= n bytes; #groups <= n/32 + n_req).
// The caller awaits a hipEvent instead of a blocking sync — on ROCm a
// blocking host sync busy-spins a core, which was measured to halve the
// serving throughput with 12 gateway workers per GPU (profiles/r01).
std::vector<at::Tensor> bpe_count_async(at::Tensor bytes, at::Tensor req_off,
                                        at::Tensor htab_keys, at::Tensor htab_rank) {
  check_cuda(bytes, "bytes");
  check_cuda(req_off, "req_off");
  int n = (int)bytes.numel();
  int n_req = (int)req_off.numel();
  TORCH_CHECK(n > 0, "empty batch");
  int htab_mask = (int)htab_keys.numel() - 1;
  auto stream = current_stream();
  auto u8 = at::TensorOptions().dtype(at::kByte).device(bytes.device());
  auto i32 = at::TensorOptions().dtype(at::kInt).device(bytes.device());
  int blocks = (n + 255) / 256;

  at::Tensor flags = at::empty({n}, u8);
  hipLaunchKernelGGL(seg_flags_kernel, dim3(blocks), dim3(256), 0, stream,
                     bytes.data_ptr<uint8_t>(), n, flags.data_ptr<uint8_t>());
  hipLaunchKernelGGL(seg_force_starts_kernel, dim3((n_req + 255) / 256), dim3(256), 0,
                     stream, req_off.data_ptr<int64_t>(), n_req, n,
                     flags.data_ptr<uint8_t>());
  at::Tensor blk_counts = at::empty({blocks}, i32);
  hipLaunchKernelGGL(seg_block_count_kernel, dim3(blocks), dim3(256), 0, stream,
                     flags.data_ptr<uint8_t>(), n, blk_counts.data_ptr<int32_t>());
  at::Tensor scan = blk_counts.cumsum(0, at::kInt);
  at::Tensor blk_excl = at::zeros({blocks}, i32);
  if (blocks > 1)
    blk_excl.narrow(0, 1, blocks - 1).copy_(scan.narrow(0, 0, blocks - 1));
  const int32_t* n_segs_dev = scan.data_ptr<int32_t>() + (blocks - 1);

  at::Tensor seg_start = at::empty({n}, i32);
  at::Tensor seg_req = at::empty({n}, i32);
  hipLaunchKernelGGL(seg_write_kernel, dim3(blocks), dim3(256), 0, stream,
                     flags.data_ptr<uint8_t>(), n, blk_excl.data_ptr<int32_t>(),
                     req_off.data_ptr<int64_t>(), n_req,
                     seg_start.data_ptr<int32_t>(), seg_req.data_ptr<int32_t>());

  at::Tensor gflags = at::zeros({n}, u8);  // beyond n_segs stays 0
  hipLaunchKernelGGL(group_head_flags_dev_kernel, dim3(blocks), dim3(256), 0, stream,
                     seg_start.data_ptr<int32_t>(), seg_req.data_ptr<int32_t>(),
                     n_segs_dev, req_off.data_ptr<int64_t>(),
                     gflags.data_ptr<uint8_t>());
  at::Tensor gblk = at::empty({blocks}, i32);
  hipLaunchKernelGGL(seg_block_count_kernel, dim3(blocks), dim3(256), 0, stream,
                     gflags.data_ptr<uint8_t>(), n, gblk.data_ptr<int32_t>());
  at::Tensor gscan = gblk.cumsum(0, at::kInt);
  at::Tensor gexcl = at::zeros({blocks}, i32);
  if (blocks > 1)
    gexcl.narrow(0, 1, blocks - 1).copy_(gscan.narrow(0, 0, blocks - 1));
  const int32_t* n_groups_dev = gscan.data_ptr<int32_t>() + (blocks - 1);
  at::Tensor ghead = at::empty({n}, i32);
  hipLaunchKernelGGL(flag_compact_write_kernel, dim3(blocks), dim3(256), 0, stream,
                     gflags.data_ptr<uint8_t>(), n, gexcl.data_ptr<int32_t>(),
                     ghead.data_ptr<int32_t>());

  at::Tensor out_ids = at::full({n}, -1, i32);
  at::Tensor req_counts = at::zeros({n_req}, i32);
  long long group_bound = (long long)n / 32 + n_req + 1;
  int blocks2 = (int)((group_bound + 3) / 4);
  hipLaunchKernelGGL(bpe_encode_grouped_dev_kernel, dim3(blocks2), dim3(256), 0,
                     stream, bytes.data_ptr<uint8_t>(), seg_start.data_ptr<int32_t>(),
                     seg_req.data_ptr<int32_t>(), n_segs_dev, n,
                     ghead.data_ptr<int32_t>(), n_groups_dev,
                     reinterpret_cast<long long*>(htab_keys.data_ptr<int64_t>()),
                     htab_rank.data_ptr<int32_t>(), htab_mask,
                     out_ids.data_ptr<int32_t>(), req_counts.data_ptr<int32_t>());
  return {out_ids, req_counts};
}

at::Tensor meanpool(at::Tensor ids, at::Tensor req_off, at::Tensor emb) {
  check_cuda(ids, "ids");
  check_cuda(req_off, "req_off");
  check_cuda(emb, "emb");
  TORCH_CHECK(emb.scalar_type() == at::kBFloat16, "emb must be bf16");
  int n_req = (int)req_off.numel();
  int dim = (int)emb.size(1);
  TORCH_CHECK(dim <= 1024, "dim too large for one block");
  auto out = at::zeros({n_req, dim},
                       at::TensorOptions().dtype(at::kFloat).device(ids.device()));
  auto cnt = at::zeros({n_req},
                       at::TensorOptions().dtype(at::kInt).device(ids.device()));
  constexpr int P = 8;
  hipLaunchKernelGGL(meanpool_accum_kernel, dim3(n_req, P), dim3(dim), 0,
                     current_stream(), ids.data_ptr<int32_t>(),
                     req_off.data_ptr<int64_t>(), n_req, (int)ids.numel(),
                     reinterpret_cast<bf16*>(emb.data_ptr<at::BFloat16>()), dim, P,
                     out.data_ptr<float>(), cnt.data_ptr<int32_t>());
  hipLaunchKernelGGL(meanpool_div_kernel, dim3(n_req), dim3(dim), 0, current_stream(),
                     out.data_ptr<float>(), cnt.data_ptr<int32_t>(), n_req, dim);
  return out;
}

at::Tensor gemm_bf16_nt(at::Tensor a, at::Tensor bt, c10::optional<at::Tensor> bias,
                        bool relu) {
  check_cuda(a, "a");
  check_cuda(bt, "bt");
  TORCH_CHECK(a.scalar_type() == at::kBFloat16 && bt.scalar_type() == at::kBFloat16,
              "bf16 required");
  int M = (int)a.size(0), K = (int)a.size(1), N = (int)bt.size(0);
  TORCH_CHECK(bt.size(1) == K, "K mismatch");
  TORCH_CHECK(K % 8 == 0, "K must be a multiple of 8");
  auto c = at::empty({M, N}, at::TensorOptions().dtype(at::kFloat).device(a.device()));
  const float* bias_ptr = nullptr;
  if (bias.has_value()) {
    check_cuda(*bias, "bias");
    bias_ptr = bias->data_ptr<float>();
  }
  if (M % 128 == 0 && N % 128 == 0 && K % 32 == 0) {
    dim3 grid(N / 128, M / 128);
    hipLaunchKernelGGL(gemm_bf16_nt_tiled_kernel, grid, dim3(256), 0,
                       current_stream(),
                       reinterpret_cast<bf16*>(a.data_ptr<at::BFloat16>()),
                       reinterpret_cast<bf16*>(bt.data_ptr<at::BFloat16>()),
                       c.data_ptr<float>(), M, N, K, bias_ptr, relu ? 1 : 0);
    return c;
  }
  dim3 grid((M + 15) / 16, (N + 63) / 64);
  hipLaunchKernelGGL(gemm_bf16_nt_kernel, grid, dim3(256), 0, current_stream(),
                     reinterpret_cast<bf16*>(a.data_ptr<at::BFloat16>()),
                     reinterpret_cast<bf16*>(bt.data_ptr<at::BFloat16>()),
                     c.data_ptr<float>(), M, N, K, bias_ptr, relu ? 1 : 0);
  return c;
}

at::Tensor l2norm_rows(at::Tensor x) {
  check_cuda(x, "x");
  TORCH_CHECK(x.scalar_type() == at::kFloat, "fp32 required");
  int rows = (int)x.size(0), dim = (int)x.size(1);
  auto out = at::empty({rows, dim},
                       at::TensorOptions().dtype(at::kBFloat16).device(x.device()));
  int blocks = (rows + 3) / 4;
  hipLaunchKernelGGL(l2norm_rows_kernel, dim3(blocks), dim3(256), 0, current_stream(),
                     x.data_ptr<float>(),
                     reinterpret_cast<bf16*>(out.data_ptr<at::BFloat16>()), rows, dim);
  return out;
}

std::vector<at::Tensor> cache_topk(at::Tensor index, at::Tensor q) {
  check_cuda(index, "index");
  check_cuda(q, "q");
  bool fp8 = index.scalar_type() == at::kFloat8_e4m3fn;
  TORCH_CHECK(index.scalar_type() == q.scalar_type(), "index/q dtype mismatch");
  TORCH_CHECK(fp8 || index.scalar_type() == at::kBFloat16,
              "bf16 or float8_e4m3fn required");
  long long n_rows = index.size(0);
  int n_q = (int)q.size(0), dim = (int)q.size(1);
  TORCH_CHECK(index.size(1) == dim, "dim mismatch");
  TORCH_CHECK(dim % 32 == 0 && dim <= 512, "dim must be a multiple of 32, <= 512");
  auto best = at::zeros({n_q}, at::TensorOptions()
                                   .dtype(at::kLong)
                                   .device(q.device()));
  TORCH_CHECK(n_q <= 256, "cache_topk: at most 256 queries per call");
  constexpr int ROWTILES = 16;
  long long blocks = (n_rows + 64 * ROWTILES - 1) / (64 * ROWTILES);
  auto* best_p = reinterpret_cast<unsigned long long*>(best.data_ptr<int64_t>());
  if (fp8) {
    auto* ip = reinterpret_cast<const uint8_t*>(index.data_ptr());
    auto* q_base = reinterpret_cast<const uint8_t*>(q.data_ptr());
    auto launch_fp8 = [&](auto kernel, int kq, const uint8_t* qp,
                          unsigned long long* bp, size_t lds_bytes) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024);
      hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), lds_bytes,
                         current_stream(), ip, n_rows, qp, kq, dim, bp);
    };
    for (int q0 = 0; q0 < n_q; q0 += 128) {
      int kq = std::min(128, n_q - q0);
      const uint8_t* qp = q_base + (long long)q0 * dim;
      unsigned long long* bp = best_p + q0;
      switch (dim >> 5) {
        case 12: {
          constexpr size_t L = 128 * (12 * 32 + 16) + 128 * 8;
          launch_fp8(&cache_topk_fp8_lds_kernel_t<12, ROWTILES>, kq, qp, bp, L);
          break;
        }
        case 8: {
          constexpr size_t L = 128 * (8 * 32 + 16) + 128 * 8;
          launch_fp8(&cache_topk_fp8_lds_kernel_t<8, ROWTILES>, kq, qp, bp, L);
          break;
        }
        case 16: {
          constexpr size_t L = 128 * (16 * 32 + 16) + 128 * 8;
          launch_fp8(&cache_topk_fp8_lds_kernel_t<16, ROWTILES>, kq, qp, bp, L);
          break;
        }
        case 4: {
          constexpr size_t L = 128 * (4 * 32 + 16) + 128 * 8;
          launch_fp8(&cache_topk_fp8_lds_kernel_t<4, ROWTILES>, kq, qp, bp, L);
          break;
        }
        default:
          TORCH_CHECK(false, "cache_topk fp8: unsupported dim ", dim);
      }
    }
    auto hi = best.bitwise_right_shift(32).to(at::kLong);
    auto idx = best.bitwise_and(0xFFFFFFFFLL).to(at::kInt);
    return {hi, idx};
  }
  auto* index_p = reinterpret_cast<bf16*>(index.data_ptr<at::BFloat16>());
  auto* q_p = reinterpret_cast<bf16*>(q.data_ptr<at::BFloat16>());
  // bf16 path: LDS-staged kernel, <=128 queries per pass (the query block
  // lives in LDS; see cache_topk_lds_kernel_t). The index streams once
  // per pass — two passes for 256 queries still beat the register-tile
  // kernel's latency stalls by a wide margin.
  auto launch_lds = [&](auto kernel, int kq, const bf16* qp, unsigned long long* bp,
                        size_t lds_bytes) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), lds_bytes,
                       current_stream(), index_p, n_rows, qp, kq, dim, bp);
  };
  for (int q0 = 0; q0 < n_q; q0 += 128) {
    int kq = std::min(128, n_q - q0);
    const bf16* qp = q_p + (long long)q0 * dim;
    unsigned long long* bp = best_p + q0;
    switch (dim >> 5) {
      case 12: {  // dim = 384 (bge-small) — the hot path
        constexpr size_t L = 128 * (12 * 32 + 8) * sizeof(bf16) + 128 * 8;
        launch_lds(&cache_topk_lds_kernel_t<12, ROWTILES>, kq, qp, bp, L);
        break;
      }
      case 8: {  // dim = 256
        constexpr size_t L = 128 * (8 * 32 + 8) * sizeof(bf16) + 128 * 8;
        launch_lds(&cache_topk_lds_kernel_t<8, ROWTILES>, kq, qp, bp, L);
        break;
      }
      case 16: {  // dim = 512
        constexpr size_t L = 128 * (16 * 32 + 8) * sizeof(bf16) + 128 * 8;
        launch_lds(&cache_topk_lds_kernel_t<16, ROWTILES>, kq, qp, bp, L);
        break;
      }
      case 4: {  // dim = 128
        constexpr size_t L = 128 * (4 * 32 + 8) * sizeof(bf16) + 128 * 8;
        launch_lds(&cache_topk_lds_kernel_t<4, ROWTILES>, kq, qp, bp, L);
        break;
      }
      default:
        TORCH_CHECK(false, "cache_topk: unsupported dim ", dim,
                    " (supported: 128/256/384/512)");
    }
  }
  // unpack: score = orderable^-1(hi32), idx = lo32
  auto hi = best.bitwise_right_shift(32).to(at::kLong);
  auto idx = best.bitwise_and(0xFFFFFFFFLL).to(at::kInt);
  return {hi, idx};
}

// cache_topk with the per-row (scope, expiry) filter of
// cache_topk_scoped_kernel_t: a query sees row r only if
// row_expiry[r] > now and (q_scope == 0 or row_scope[r] == q_scope).
// idx is -1 and hi is 0 for a query that no row may answer.
template <class E>
static void launch_cache_topk_scoped(const at::Tensor& index, const at::Tensor& q,
                                     const at::Tensor& row_scope,
                                     const at::Tensor& row_expiry,
                                     const at::Tensor& q_scope, int now,
                                     at::Tensor& best) {
  using elem = typename E::elem;
  constexpr int ROWTILES = 16;
  long long n_rows = index.size(0);
  int n_q = (int)q.size(0), dim = (int)q.size(1);
  long long blocks = (n_rows + 64 * ROWTILES - 1) / (64 * ROWTILES);
  auto* ip = reinterpret_cast<const elem*>(index.data_ptr());
  auto* q_base = reinterpret_cast<const elem*>(q.data_ptr());
  auto* best_p = reinterpret_cast<unsigned long long*>(best.data_ptr<int64_t>());
  auto* rs = reinterpret_cast<const long long*>(row_scope.data_ptr<int64_t>());
  auto* re = row_expiry.data_ptr<int32_t>();
  auto* qsc = reinterpret_cast<const long long*>(q_scope.data_ptr<int64_t>());
  // query block + blk_best + q_scope stage
  size_t lds_bytes = 128 * (size_t)(dim + E::kPad) * sizeof(elem) + 128 * 8 + 128 * 8;
  auto launch = [&](auto kernel, int q0) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), lds_bytes,
                       current_stream(), ip, n_rows, q_base + (long long)q0 * dim,
                       std::min(128, n_q - q0), dim, best_p + q0, rs, re, qsc + q0, now);
  };
  for (int q0 = 0; q0 < n_q; q0 += 128) {
    switch (dim >> 5) {
      case 12: launch(&cache_topk_scoped_kernel_t<E, 12, ROWTILES>, q0); break;
      case 8: launch(&cache_topk_scoped_kernel_t<E, 8, ROWTILES>, q0); break;
      case 16: launch(&cache_topk_scoped_kernel_t<E, 16, ROWTILES>, q0); break;
      case 4: launch(&cache_topk_scoped_kernel_t<E, 4, ROWTILES>, q0); break;
      default:
        TORCH_CHECK(false, "cache_topk_scoped: unsupported dim ", dim,
                    " (supported: 128/256/384/512)");
    }
  }
}

std::vector<at::Tensor> cache_topk_scoped(at::Tensor index, at::Tensor q,
                                          at::Tensor row_scope, at::Tensor row_expiry,
                                          at::Tensor q_scope, int64_t now) {
  check_cuda(index, "index");
  check_cuda(q, "q");
  check_cuda(row_scope, "row_scope");
  check_cuda(row_expiry, "row_expiry");
  check_cuda(q_scope, "q_scope");
  bool fp8 = index.scalar_type() == at::kFloat8_e4m3fn;
  TORCH_CHECK(index.scalar_type() == q.scalar_type(), "index/q dtype mismatch");
  TORCH_CHECK(fp8 || index.scalar_type() == at::kBFloat16,
              "bf16 or float8_e4m3fn required");
  TORCH_CHECK(index.dim() == 2 && q.dim() == 2, "index and q must be 2-D");
  long long n_rows = index.size(0);
  int n_q = (int)q.size(0), dim = (int)q.size(1);
  TORCH_CHECK(index.size(1) == dim, "dim mismatch");
  TORCH_CHECK(dim % 32 == 0 && dim <= 512, "dim must be a multiple of 32, <= 512");
  TORCH_CHECK(n_q <= 256, "cache_topk_scoped: at most 256 queries per call");
  TORCH_CHECK(row_scope.scalar_type() == at::kLong && row_scope.dim() == 1 &&
                  row_scope.size(0) == n_rows,
              "row_scope must be int64[n_rows]");
  TORCH_CHECK(row_expiry.scalar_type() == at::kInt && row_expiry.dim() == 1 &&
                  row_expiry.size(0) == n_rows,
              "row_expiry must be int32[n_rows]");
  TORCH_CHECK(q_scope.scalar_type() == at::kLong && q_scope.dim() == 1 &&
                  q_scope.size(0) == n_q,
              "q_scope must be int64[n_q]");
  TORCH_CHECK(row_scope.device() == index.device() &&
                  row_expiry.device() == index.device() &&
                  q_scope.device() == index.device() && q.device() == index.device(),
              "cache_topk_scoped: all tensors must be on one device");
  // the kernel reads a lane's 4 row tags as 16-byte vectors
  TORCH_CHECK(reinterpret_cast<uintptr_t>(row_scope.data_ptr()) % 32 == 0 &&
                  reinterpret_cast<uintptr_t>(row_expiry.data_ptr()) % 16 == 0,
              "row_scope/row_expiry must start 32/16-byte aligned (row 4k of the "
              "allocation)");
  TORCH_CHECK(now >= INT32_MIN && now <= INT32_MAX, "now must fit int32");
  auto best = at::zeros({n_q}, at::TensorOptions().dtype(at::kLong).device(q.device()));
  if (n_q == 0 || n_rows == 0)
    return {best, at::full({n_q}, -1, best.options().dtype(at::kInt))};
  if (fp8)
    launch_cache_topk_scoped<CacheElemFp8>(index, q, row_scope, row_expiry, q_scope,
                                           (int)now, best);
  else
    launch_cache_topk_scoped<CacheElemBf16>(index, q, row_scope, row_expiry, q_scope,
                                            (int)now, best);
  auto hi = best.bitwise_right_shift(32).to(at::kLong);
  auto idx = at::where(best == 0, -1, best.bitwise_and(0xFFFFFFFFLL)).to(at::kInt);
  return {hi, idx};
}

at::Tensor kv_score_assign(at::Tensor stats, at::Tensor pred_tokens, double w_kv,
                           double w_q, double w_a) {
  check_cuda(stats, "stats");
  check_cuda(pred_tokens, "pred_tokens");
  int n_rep = (int)stats.size(0);
  TORCH_CHECK(n_rep <= 64, "at most 64 replicas");
  int n_req = (int)pred_tokens.numel();
  auto assign = at::empty({n_req},
                          at::TensorOptions().dtype(at::kInt).device(stats.device()));
  hipLaunchKernelGGL(kv_scorer_kernel, dim3(1), dim3(64), 0, current_stream(),
                     stats.data_ptr<float>(), n_rep, pred_tokens.data_ptr<float>(),
                     n_req, (float)w_kv, (float)w_q, (float)w_a,
                     assign.data_ptr<int32_t>());
  return assign;
}

// ---- prefix index ----------------------------------------------------------

#define PREFIX_INSERT_WAVES 512

static void check_prefix_table(const at::Tensor& keys, const at::Tensor& masks,
                               const at::Tensor& stamps, const char* who) {
  check_cuda(keys, "keys");
  check_cuda(masks, "masks");
  check_cuda(stamps, "stamps");
  TORCH_CHECK(keys.scalar_type() == at::kLong && keys.dim() == 1, who,
              ": keys must be int64[n_buckets*16]");
  TORCH_CHECK(masks.scalar_type() == at::kLong && masks.dim() == 1 &&
                  masks.size(0) == keys.size(0),
              who, ": masks must be int64[n_buckets*16]");
  TORCH_CHECK(stamps.scalar_type() == at::kInt && stamps.dim() == 1 &&
                  stamps.size(0) == keys.size(0),
              who, ": stamps must be int32[n_buckets*16]");
  long long n_slots = keys.size(0);
  long long n_buckets = n_slots / PREFIX_SLOTS;
  TORCH_CHECK(n_slots % PREFIX_SLOTS == 0 && n_buckets >= 1 &&
                  (n_buckets & (n_buckets - 1)) == 0 && n_buckets <= (1LL << 27),
              who, ": n_buckets must be a power of two, at most 2^27");
  TORCH_CHECK(masks.device() == keys.device() && stamps.device() == keys.device(), who,
              ": all tensors must be on one device");
}

static void check_prefix_hashes(const at::Tensor& hashes, const at::Tensor& n_blocks,
                                const at::Tensor& table, const char* who) {
  check_cuda(hashes, "hashes");
  check_cuda(n_blocks, "n_blocks");
  TORCH_CHECK(hashes.scalar_type() == at::kLong && hashes.dim() == 2, who,
              ": hashes must be int64[n_req, max_blocks]");
  TORCH_CHECK(hashes.size(1) >= 1 && hashes.size(1) <= PREFIX_MAX_BLOCKS, who,
              ": max_blocks must be in [1, 256]");
  TORCH_CHECK(n_blocks.scalar_type() == at::kInt && n_blocks.dim() == 1 &&
                  n_blocks.size(0) == hashes.size(0),
              who, ": n_blocks must be int32[n_req]");
  TORCH_CHECK(hashes.size(0) <= (1 << 20), who, ": at most 2^20 requests per call");
  TORCH_CHECK(hashes.device() == table.device() && n_blocks.device() == table.device(),
              who, ": all tensors must be on one device");
}

std::vector<at::Tensor> prefix_block_hashes(at::Tensor out_ids, at::Tensor req_off,
                                            int64_t n_bytes, int64_t block_tokens,
                                            int64_t max_blocks, int64_t salt) {
  check_cuda(out_ids, "out_ids");
  check_cuda(req_off, "req_off");
  TORCH_CHECK(out_ids.scalar_type() == at::kInt && out_ids.dim() == 1,
              "prefix_block_hashes: out_ids must be int32[n_bytes]");
  TORCH_CHECK(req_off.scalar_type() == at::kLong && req_off.dim() == 1,
              "prefix_block_hashes: req_off must be int64[n_req]");
  TORCH_CHECK(out_ids.device() == req_off.device(),
              "prefix_block_hashes: all tensors must be on one device");
  TORCH_CHECK(n_bytes >= 0 && n_bytes <= out_ids.numel(),
              "prefix_block_hashes: n_bytes must be in [0, out_ids.numel()]");
  TORCH_CHECK(block_tokens == 8 || block_tokens == 16 || block_tokens == 32 ||
                  block_tokens == 64,
              "prefix_block_hashes: block_tokens must be 8, 16, 32 or 64");
  TORCH_CHECK(max_blocks >= 1 && max_blocks <= PREFIX_MAX_BLOCKS,
              "prefix_block_hashes: max_blocks must be in [1, 256]");
  long long n_req = req_off.numel();
  TORCH_CHECK(n_req <= (1 << 20), "prefix_block_hashes: at most 2^20 requests per call");
  auto hashes = at::empty({n_req, max_blocks},
                          at::TensorOptions().dtype(at::kLong).device(out_ids.device()));
  auto n_blocks = at::empty({n_req},
                            at::TensorOptions().dtype(at::kInt).device(out_ids.device()));
  if (n_req == 0) return {hashes, n_blocks};
  hipLaunchKernelGGL(prefix_block_hash_kernel, dim3((unsigned)n_req), dim3(256), 0,
                     current_stream(), out_ids.data_ptr<int32_t>(),
                     req_off.data_ptr<int64_t>(), (int)n_req, (long long)n_bytes,
                     (int)block_tokens, (int)max_blocks, (pfx_u64)salt,
                     hashes.data_ptr<int64_t>(), n_blocks.data_ptr<int32_t>());
  return {hashes, n_blocks};
}

at::Tensor prefix_match(at::Tensor keys, at::Tensor masks, at::Tensor stamps,
                        at::Tensor hashes, at::Tensor n_blocks, int64_t live_mask,
                        int64_t now, int64_t ttl) {
  check_prefix_table(keys, masks, stamps, "prefix_match");
  check_prefix_hashes(hashes, n_blocks, keys, "prefix_match");
  TORCH_CHECK(now >= 0 && now <= INT32_MAX && ttl >= 0 && ttl <= INT32_MAX,
              "prefix_match: now and ttl must fit a non-negative int32");
  long long n_req = hashes.size(0);
  auto matched = at::empty({n_req, 64},
                           at::TensorOptions().dtype(at::kInt).device(keys.device()));
  if (n_req == 0) return matched;
  unsigned bucket_mask = (unsigned)(keys.size(0) / PREFIX_SLOTS - 1);
  hipLaunchKernelGGL(prefix_match_kernel, dim3((unsigned)((n_req + 3) / 4)), dim3(256), 0,
                     current_stream(), keys.data_ptr<int64_t>(), masks.data_ptr<int64_t>(),
                     stamps.data_ptr<int32_t>(), bucket_mask, hashes.data_ptr<int64_t>(),
                     n_blocks.data_ptr<int32_t>(), (int)n_req, (int)hashes.size(1),
                     (pfx_u64)live_mask, (int)now, (int)ttl, matched.data_ptr<int32_t>());
  return matched;
}

void prefix_insert(at::Tensor keys, at::Tensor masks, at::Tensor stamps,
                   at::Tensor counters, at::Tensor hashes, at::Tensor n_blocks,
                   at::Tensor assign, at::Tensor bit_of, int64_t now, int64_t ttl,
                   int64_t waves) {
  check_prefix_table(keys, masks, stamps, "prefix_insert");
  check_prefix_hashes(hashes, n_blocks, keys, "prefix_insert");
  check_cuda(counters, "counters");
  check_cuda(assign, "assign");
  check_cuda(bit_of, "bit_of");
  TORCH_CHECK(counters.scalar_type() == at::kInt && counters.dim() == 1 &&
                  counters.size(0) == 4,
              "prefix_insert: counters must be int32[4]");
  TORCH_CHECK(assign.scalar_type() == at::kInt && assign.dim() == 1 &&
                  assign.size(0) == hashes.size(0),
              "prefix_insert: assign must be int32[n_req]");
  TORCH_CHECK(bit_of.scalar_type() == at::kLong && bit_of.dim() == 1,
              "prefix_insert: bit_of must be int64[n_rep]");
  TORCH_CHECK(bit_of.size(0) <= 64, "prefix_insert: at most 64 replicas");
  TORCH_CHECK(counters.device() == keys.device() && assign.device() == keys.device() &&
                  bit_of.device() == keys.device(),
              "prefix_insert: all tensors must be on one device");
  TORCH_CHECK(now >= 0 && now <= INT32_MAX && ttl >= 0 && ttl <= INT32_MAX,
              "prefix_insert: now and ttl must fit a non-negative int32");
  long long n_req = hashes.size(0);
  if (n_req == 0 || bit_of.size(0) == 0) return;
  long long n_buckets = keys.size(0) / PREFIX_SLOTS;
  // W = 4 * grid waves share the buckets (bucket % W). The table state does
  // not depend on W; the default is from profiles/prefix_picker.md.
  TORCH_CHECK(waves >= 0 && waves <= 4096, "prefix_insert: waves must be in [0, 4096]");
  if (waves == 0) waves = PREFIX_INSERT_WAVES;
  unsigned grid = (unsigned)((std::min<long long>(n_buckets, waves) + 3) / 4);
  hipLaunchKernelGGL(prefix_insert_kernel, dim3(grid), dim3(256), 0, current_stream(),
                     keys.data_ptr<int64_t>(), masks.data_ptr<int64_t>(),
                     stamps.data_ptr<int32_t>(), (unsigned)(n_buckets - 1),
                     counters.data_ptr<int32_t>(), hashes.data_ptr<int64_t>(),
                     n_blocks.data_ptr<int32_t>(), assign.data_ptr<int32_t>(),
                     bit_of.data_ptr<int64_t>(), (int)bit_of.size(0), (int)n_req,
                     (int)hashes.size(1), (int)now, (int)ttl);
}

#define PREFIX_EXPORT_MAX_GROUPS 1024

static void check_repl_counters(const at::Tensor& repl_counters, const at::Tensor& table,
                                const char* who) {
  check_cuda(repl_counters, "repl_counters");
  TORCH_CHECK(repl_counters.scalar_type() == at::kInt && repl_counters.dim() == 1 &&
                  repl_counters.size(0) == 4,
              who, ": repl_counters must be int32[4]");
  TORCH_CHECK(repl_counters.device() == table.device(), who,
              ": all tensors must be on one device");
}

void prefix_export(at::Tensor keys, at::Tensor masks, at::Tensor stamps, at::Tensor hashes,
                   at::Tensor n_blocks, at::Tensor assign, at::Tensor bit_of,
                   at::Tensor key_of, at::Tensor log, at::Tensor log_n,
                   at::Tensor repl_counters, int64_t now, int64_t ttl, int64_t refresh) {
  check_prefix_table(keys, masks, stamps, "prefix_export");
  check_prefix_hashes(hashes, n_blocks, keys, "prefix_export");
  check_cuda(assign, "assign");
  check_cuda(bit_of, "bit_of");
  check_cuda(key_of, "key_of");
  check_cuda(log, "log");
  check_cuda(log_n, "log_n");
  check_repl_counters(repl_counters, keys, "prefix_export");
  TORCH_CHECK(assign.scalar_type() == at::kInt && assign.dim() == 1 &&
                  assign.size(0) == hashes.size(0),
              "prefix_export: assign must be int32[n_req]");
  TORCH_CHECK(bit_of.scalar_type() == at::kLong && bit_of.dim() == 1,
              "prefix_export: bit_of must be int64[n_rep]");
  TORCH_CHECK(bit_of.size(0) <= 64, "prefix_export: at most 64 replicas");
  TORCH_CHECK(key_of.scalar_type() == at::kLong && key_of.dim() == 1 &&
                  key_of.size(0) == bit_of.size(0),
              "prefix_export: key_of must be int64[n_rep]");
  TORCH_CHECK(log.scalar_type() == at::kLong && log.dim() == 2 && log.size(1) == 2 &&
                  log.size(0) <= INT32_MAX,
              "prefix_export: log must be int64[cap, 2]");
  TORCH_CHECK(log_n.scalar_type() == at::kInt && log_n.dim() == 1 && log_n.size(0) == 1,
              "prefix_export: log_n must be int32[1]");
  TORCH_CHECK(assign.device() == keys.device() && bit_of.device() == keys.device() &&
                  key_of.device() == keys.device() && log.device() == keys.device() &&
                  log_n.device() == keys.device(),
              "prefix_export: all tensors must be on one device");
  TORCH_CHECK(now >= 0 && now <= INT32_MAX && ttl >= 0 && ttl <= INT32_MAX &&
                  refresh >= 0 && refresh <= INT32_MAX,
              "prefix_export: now, ttl and refresh must fit a non-negative int32");
  long long n_req = hashes.size(0);
  if (n_req == 0 || bit_of.size(0) == 0) return;
  // scratch from the caching allocator (no sync, no kernel), as the outputs
  // of prefix_match and prefix_block_hashes are
  auto flag_words = at::empty({n_req, PREFIX_MAX_BLOCKS / 64},
                              at::TensorOptions().dtype(at::kLong).device(keys.device()));
  auto counts = at::empty({n_req + 1},
                          at::TensorOptions().dtype(at::kInt).device(keys.device()));
  unsigned bucket_mask = (unsigned)(keys.size(0) / PREFIX_SLOTS - 1);
  hipLaunchKernelGGL(prefix_export_flag_kernel, dim3((unsigned)((n_req + 3) / 4)), dim3(256),
                     0, current_stream(), keys.data_ptr<int64_t>(),
                     masks.data_ptr<int64_t>(), stamps.data_ptr<int32_t>(), bucket_mask,
                     hashes.data_ptr<int64_t>(), n_blocks.data_ptr<int32_t>(),
                     assign.data_ptr<int32_t>(), bit_of.data_ptr<int64_t>(),
                     (int)bit_of.size(0), (int)n_req, (int)hashes.size(1), (int)now, (int)ttl,
                     (int)refresh, log_n.data_ptr<int32_t>(),
                     reinterpret_cast<pfx_u64*>(flag_words.data_ptr<int64_t>()),
                     counts.data_ptr<int32_t>());
  // a workgroup writes 4 requests at a time; past 4 * 1024 workgroups' worth
  // each takes more groups, so the bases cost at most 1024 passes over counts
  long long groups = (n_req + 3) / 4;
  long long per = 4 * ((groups + PREFIX_EXPORT_MAX_GROUPS - 1) / PREFIX_EXPORT_MAX_GROUPS);
  unsigned grid = (unsigned)((n_req + per - 1) / per);
  hipLaunchKernelGGL(prefix_export_write_kernel, dim3(grid), dim3(256), 0, current_stream(),
                     hashes.data_ptr<int64_t>(), assign.data_ptr<int32_t>(),
                     key_of.data_ptr<int64_t>(), (int)n_req, (int)hashes.size(1), (int)per,
                     reinterpret_cast<const pfx_u64*>(flag_words.data_ptr<int64_t>()),
                     counts.data_ptr<int32_t>(), log.data_ptr<int64_t>(),
                     (long long)log.size(0), log_n.data_ptr<int32_t>(),
                     repl_counters.data_ptr<int32_t>());
}

void prefix_apply_remote(at::Tensor keys, at::Tensor masks, at::Tensor stamps,
                         at::Tensor counters, at::Tensor rec, int64_t n_rec,
                         at::Tensor member_keys, at::Tensor member_bits,
                         at::Tensor repl_counters, int64_t now, int64_t ttl, int64_t waves) {
  check_prefix_table(keys, masks, stamps, "prefix_apply_remote");
  check_cuda(counters, "counters");
  check_cuda(rec, "rec");
  check_cuda(member_keys, "member_keys");
  check_cuda(member_bits, "member_bits");
  check_repl_counters(repl_counters, keys, "prefix_apply_remote");
  TORCH_CHECK(counters.scalar_type() == at::kInt && counters.dim() == 1 &&
                  counters.size(0) == 4,
              "prefix_apply_remote: counters must be int32[4]");
  TORCH_CHECK(rec.scalar_type() == at::kLong && rec.dim() == 2 && rec.size(1) == 2,
              "prefix_apply_remote: rec must be int64[n, 2]");
  TORCH_CHECK(n_rec >= 0 && n_rec <= rec.size(0),
              "prefix_apply_remote: n_rec must be in [0, rec.size(0)]");
  TORCH_CHECK(member_keys.scalar_type() == at::kLong && member_keys.dim() == 1,
              "prefix_apply_remote: member_keys must be int64[n_rep]");
  TORCH_CHECK(member_keys.size(0) <= 64, "prefix_apply_remote: at most 64 replicas");
  TORCH_CHECK(member_bits.scalar_type() == at::kLong && member_bits.dim() == 1 &&
                  member_bits.size(0) == member_keys.size(0),
              "prefix_apply_remote: member_bits must be int64[n_rep]");
  TORCH_CHECK(counters.device() == keys.device() && rec.device() == keys.device() &&
                  member_keys.device() == keys.device() &&
                  member_bits.device() == keys.device(),
              "prefix_apply_remote: all tensors must be on one device");
  TORCH_CHECK(now >= 0 && now <= INT32_MAX && ttl >= 0 && ttl <= INT32_MAX,
              "prefix_apply_remote: now and ttl must fit a non-negative int32");
  TORCH_CHECK(waves >= 0 && waves <= 4096, "prefix_apply_remote: waves must be in [0, 4096]");
  if (n_rec == 0) return;
  long long n_buckets = keys.size(0) / PREFIX_SLOTS;
  if (waves == 0) waves = PREFIX_INSERT_WAVES;  // as prefix_insert: never changes the result
  unsigned grid = (unsigned)((std::min<long long>(n_buckets, waves) + 3) / 4);
  hipLaunchKernelGGL(prefix_apply_remote_kernel, dim3(grid), dim3(256), 0, current_stream(),
                     keys.data_ptr<int64_t>(), masks.data_ptr<int64_t>(),
                     stamps.data_ptr<int32_t>(), (unsigned)(n_buckets - 1),
                     counters.data_ptr<int32_t>(), rec.data_ptr<int64_t>(),
                     (long long)n_rec, member_keys.data_ptr<int64_t>(),
                     member_bits.data_ptr<int64_t>(), (int)member_keys.size(0),
                     repl_counters.data_ptr<int32_t>(), (int)now, (int)ttl);
}

void prefix_clear_bits(at::Tensor masks, int64_t mask) {
  check_cuda(masks, "masks");
  TORCH_CHECK(masks.scalar_type() == at::kLong && masks.dim() == 1,
              "prefix_clear_bits: masks must be int64[n_buckets*16]");
  long long n = masks.numel();
  if (n == 0 || mask == 0) return;
  unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(prefix_clear_bits_kernel, dim3(grid), dim3(256), 0, current_stream(),
                     masks.data_ptr<int64_t>(), n, (long long)~mask);
}

at::Tensor kv_score_assign_prefix(at::Tensor stats, at::Tensor pred_tokens,
                                  at::Tensor matched, int64_t block_tokens, double w_kv,
                                  double w_q, double w_a, double w_p) {
  check_cuda(stats, "stats");
  check_cuda(pred_tokens, "pred_tokens");
  check_cuda(matched, "matched");
  TORCH_CHECK(stats.scalar_type() == at::kFloat && stats.dim() == 2 && stats.size(1) == 4,
              "kv_score_assign_prefix: stats must be float32[n_rep, 4]");
  TORCH_CHECK(pred_tokens.scalar_type() == at::kFloat && pred_tokens.dim() == 1,
              "kv_score_assign_prefix: pred_tokens must be float32[n_req]");
  int n_rep = (int)stats.size(0);
  TORCH_CHECK(n_rep <= 64, "at most 64 replicas");
  long long n_req = pred_tokens.numel();
  TORCH_CHECK(matched.scalar_type() == at::kInt && matched.dim() == 2 &&
                  matched.size(0) == n_req && matched.size(1) >= n_rep,
              "kv_score_assign_prefix: matched must be int32[n_req, >= n_rep]");
  TORCH_CHECK(block_tokens == 8 || block_tokens == 16 || block_tokens == 32 ||
                  block_tokens == 64,
              "kv_score_assign_prefix: block_tokens must be 8, 16, 32 or 64");
  TORCH_CHECK(pred_tokens.device() == stats.device() && matched.device() == stats.device(),
              "kv_score_assign_prefix: all tensors must be on one device");
  auto assign = at::empty({n_req},
                          at::TensorOptions().dtype(at::kInt).device(stats.device()));
  if (n_req == 0) return assign;
  hipLaunchKernelGGL(kv_scorer_prefix_kernel, dim3(1), dim3(64), 0, current_stream(),
                     stats.data_ptr<float>(), n_rep, pred_tokens.data_ptr<float>(),
                     (int)n_req, matched.data_ptr<int32_t>(), (int)matched.size(1),
                     (int)block_tokens, (float)w_kv, (float)w_q, (float)w_a, (float)w_p,
                     assign.data_ptr<int32_t>());
  return assign;
}

// MFMA layout probe: C = A(16x32) @ B(32x16) as one intrinsic call; used by
// the HW test to verify the documented fragment layouts against torch.
__global__ void mfma_probe_kernel(const bf16* __restrict__ A, const bf16* __restrict__ Bt,
                                  float* __restrict__ C) {
  int lane = threadIdx.x & 63;
  short8 a = *reinterpret_cast<const short8*>(&A[(lane & 15) * 32 + (lane >> 4) * 8]);
  short8 b = *reinterpret_cast<const short8*>(&Bt[(lane & 15) * 32 + (lane >> 4) * 8]);
  floatx4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
  #pragma unroll
  for (int r = 0; r < 4; ++r) C[((lane >> 4) * 4 + r) * 16 + (lane & 15)] = acc[r];
}

at::Tensor mfma_probe(at::Tensor a, at::Tensor bt) {
  check_cuda(a, "a");
  check_cuda(bt, "bt");
  auto c = at::empty({16, 16}, at::TensorOptions().dtype(at::kFloat).device(a.device()));
  hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, current_stream(),
                     reinterpret_cast<bf16*>(a.data_ptr<at::BFloat16>()),
                     reinterpret_cast<bf16*>(bt.data_ptr<at::BFloat16>()),
                     c.data_ptr<float>());
  return c;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("bpe_segment", &bpe_segment, "segment bytes (GPU)");
  m.def("bpe_encode", &bpe_encode, "BPE encode a packed byte batch (GPU)");
  m.def("bpe_count_async", &bpe_count_async,
        "sync-free BPE encode: returns (out_ids, req_counts) without host syncs");
  m.def("meanpool", &meanpool, "mean-pool token embeddings per request");
  m.def("gemm_bf16_nt", &gemm_bf16_nt, "C = A @ Bt^T (MFMA bf16)",
        py::arg("a"), py::arg("bt"), py::arg("bias") = py::none(),
        py::arg("relu") = false);
  m.def("l2norm_rows", &l2norm_rows, "row-wise L2 normalize fp32->bf16");
  m.def("cache_topk", &cache_topk, "fused cosine-sim argmax over cache index");
  m.def("cache_topk_scoped", &cache_topk_scoped,
        "cache_topk over the rows a query may see: row r answers query j iff "
        "row_expiry[r] > now and (q_scope[j] == 0 or row_scope[r] == q_scope[j]). "
        "Returns (hi, idx); idx -1 / hi 0 where no row is eligible. Unlike "
        "cache_topk, row_scope must start 32-byte and row_expiry 16-byte "
        "aligned (the kernel reads 4 row tags as 16-byte vectors): pass "
        "tensors sliced from row 4k of their allocation, not e.g. row_scope[1:].");
  m.def("kv_score_assign", &kv_score_assign, "greedy KV-occupancy assignment");
  m.def("prefix_block_hashes", &prefix_block_hashes,
        "chained token-block hashes per request: (hashes int64[n_req, max_blocks], "
        "n_blocks int32[n_req]); semantics in aigw/ops/prefix_ref.py");
  m.def("prefix_match", &prefix_match,
        "per request and replica bit, the leading run of blocks the index holds "
        "for that bit: int32[n_req, 64]");
  m.def("prefix_insert", &prefix_insert,
        "apply (hash, replica bit) entries to the index in list order per bucket; "
        "waves (0 = default) sets how many waves share the buckets and never "
        "changes the result",
        py::arg("keys"), py::arg("masks"), py::arg("stamps"), py::arg("counters"),
        py::arg("hashes"), py::arg("n_blocks"), py::arg("assign"), py::arg("bit_of"),
        py::arg("now"), py::arg("ttl"), py::arg("waves") = 0);
  m.def("prefix_export", &prefix_export,
        "append the entries of one batch's insert list that other shards need to hear "
        "of, as (hash, member key) rows in list order, to log[log_n...]; run before "
        "prefix_insert of the same batch. repl_counters: exported, dropped, applied, "
        "skipped. No host sync.",
        py::arg("keys"), py::arg("masks"), py::arg("stamps"), py::arg("hashes"),
        py::arg("n_blocks"), py::arg("assign"), py::arg("bit_of"), py::arg("key_of"),
        py::arg("log"), py::arg("log_n"), py::arg("repl_counters"), py::arg("now"),
        py::arg("ttl"), py::arg("refresh"));
  m.def("prefix_apply_remote", &prefix_apply_remote,
        "apply (hash, member key) records of another shard in list order per bucket; "
        "the replica bit is looked up among member_keys; waves as in prefix_insert",
        py::arg("keys"), py::arg("masks"), py::arg("stamps"), py::arg("counters"),
        py::arg("rec"), py::arg("n_rec"), py::arg("member_keys"), py::arg("member_bits"),
        py::arg("repl_counters"), py::arg("now"), py::arg("ttl"), py::arg("waves") = 0);
  m.def("prefix_clear_bits", &prefix_clear_bits, "masks &= ~mask over the whole table");
  m.def("kv_score_assign_prefix", &kv_score_assign_prefix,
        "greedy KV-occupancy assignment with a prefix-hit term");
  m.def("mfma_probe", &mfma_probe, "16x16x32 bf16 MFMA layout probe");
}
