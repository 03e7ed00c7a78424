// ---------------------------------------------------------------------------
// 5. Prefix-cache-aware endpoint picking: chained token-block hashes, an
//    HBM-resident "which replica has seen this block" index, and the greedy
//    scorer with a prefix-hit term. Semantics are normative in
//    aigw/ops/prefix_ref.py; everything up to the final score is integer
//    arithmetic mod 2^64 and must match it bit for bit.
//
//    Table: n_buckets (power of two) buckets of 16 slots; keys/masks are
//    int64, stamps int32 (whole seconds of the index's clock). One bucket's
//    keys are one 128-byte line. Key 0 is an empty slot; a slot is live iff
//    key != 0 and now - stamp < ttl.
// ---------------------------------------------------------------------------
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#define PREFIX_SLOTS 16
#define PREFIX_MAX_BLOCKS 256
#define PREFIX_MUL 0x9E3779B97F4A7C15ULL

typedef unsigned long long pfx_u64;

__device__ __forceinline__ pfx_u64 prefix_mix(pfx_u64 z) {
  // splitmix64 finaliser
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ULL;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBULL;
  z ^= z >> 31;
  return z;
}

__device__ __forceinline__ bool prefix_live(long long key, int stamp, int now, int ttl) {
  return key != 0 && (long long)now - (long long)stamp < (long long)ttl;
}

// One 256-thread workgroup per request. The request's byte range is walked
// in 256-position chunks; each token (out_ids >= 0) gets its rank by
// ballot/popcount inside the wave plus a 4-wave LDS combine on top of a
// running count, and adds (id+1) * MUL^(rank%B + 1) into c[rank / B] with a
// 64-bit LDS atomic. Integer adds commute, so the sums do not depend on
// which lane arrives first. Thread 0 then runs the (at most 256-step) chain
// h_k = mix(h_{k-1} + c_k).
__global__ __launch_bounds__(256) void prefix_block_hash_kernel(
    const int32_t* __restrict__ out_ids, const int64_t* __restrict__ req_off, int n_req,
    long long n_bytes, int block_tokens, int max_blocks, pfx_u64 salt,
    int64_t* __restrict__ hashes,  // n_req x max_blocks
    int32_t* __restrict__ n_blocks) {
  __shared__ pfx_u64 c[PREFIX_MAX_BLOCKS];
  __shared__ pfx_u64 pw[64];
  __shared__ int wcnt[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = blockIdx.x;
  long long hi = (r + 1 < n_req) ? (long long)req_off[r + 1] : n_bytes;
  if (hi > n_bytes) hi = n_bytes;
  long long lo = (long long)req_off[r];
  if (lo < 0) lo = 0;
  c[tid] = 0;
  if (tid < 64) {
    pfx_u64 p = PREFIX_MUL;
    for (int j = 0; j < tid; ++j) p *= PREFIX_MUL;
    pw[tid] = p;  // MUL^(tid+1)
  }
  __syncthreads();
  const int shift = 31 - __clz(block_tokens);  // block_tokens is 8/16/32/64
  const int cap = max_blocks << shift;
  int running = 0;  // tokens ranked so far; identical in every thread
  int parity = 0;   // wcnt is double-buffered: one barrier per chunk
  // four chunks' loads are issued together (a chunk is one dependent
  // global-load latency otherwise); they are then ranked one by one
  for (long long base = lo; base < hi && running < cap; base += 4 * 256) {
    int ids[4];
    #pragma unroll
    for (int u = 0; u < 4; ++u) {
      long long pos = base + u * 256 + tid;
      ids[u] = pos < hi ? out_ids[pos] : -1;
    }
    #pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (base + u * 256 >= hi || running >= cap) break;  // uniform
      int id = ids[u];
      bool valid = id >= 0;
      pfx_u64 b = __ballot(valid);
      int wave_rank = __popcll(b & ((1ULL << lane) - 1ULL));
      if (lane == 0) wcnt[parity][wave] = __popcll(b);
      __syncthreads();
      int before = 0, total = 0;
      #pragma unroll
      for (int w = 0; w < 4; ++w) {
        int n = wcnt[parity][w];
        if (w < wave) before += n;
        total += n;
      }
      int rank = running + before + wave_rank;
      if (valid && rank < cap)
        atomicAdd(&c[rank >> shift],
                  (pfx_u64)(unsigned)(id + 1) * pw[rank & (block_tokens - 1)]);
      running += total;
      parity ^= 1;  // the next chunk's counts go to the other buffer
    }
  }
  __syncthreads();  // every block sum is complete before the chain
  int nb = running >> shift;  // only full blocks count
  if (nb > max_blocks) nb = max_blocks;
  int64_t* out = hashes + (long long)r * max_blocks;
  if (tid == 0) {
    n_blocks[r] = nb;
    pfx_u64 h = salt;
    for (int k = 0; k < nb; ++k) {
      h = prefix_mix(h + c[k]);
      if (h == 0) h = 1;  // key 0 is the empty slot
      out[k] = (int64_t)h;
    }
  }
  for (int k = nb + tid; k < max_blocks; k += 256) out[k] = 0;
}

// One wave per request (4 per workgroup). Lanes stride over the request's
// blocks: each reads one bucket and stages mask_k (the OR of the live slots
// holding h_k, under live_mask) in LDS. Then lane = replica bit walks the
// running AND m_k and counts its leading run; the walk ends as soon as no
// replica is left in the run.
__global__ __launch_bounds__(256) void prefix_match_kernel(
    const int64_t* __restrict__ keys, const int64_t* __restrict__ masks,
    const int32_t* __restrict__ stamps, unsigned bucket_mask,
    const int64_t* __restrict__ hashes, const int32_t* __restrict__ n_blocks, int n_req,
    int max_blocks, pfx_u64 live_mask, int now, int ttl,
    int32_t* __restrict__ matched) {  // n_req x 64
  __shared__ pfx_u64 mk[4][PREFIX_MAX_BLOCKS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + wave;
  int nb = 0;
  if (r < n_req) {
    nb = n_blocks[r];
    if (nb > max_blocks) nb = max_blocks;
    if (nb > PREFIX_MAX_BLOCKS) nb = PREFIX_MAX_BLOCKS;
  }
  for (int k = lane; k < nb; k += 64) {
    long long h = hashes[(long long)r * max_blocks + k];
    long long slot0 = (long long)((unsigned)(pfx_u64)h & bucket_mask) * PREFIX_SLOTS;
    pfx_u64 m = 0;
    #pragma unroll
    for (int s = 0; s < PREFIX_SLOTS; ++s) {
      long long key = keys[slot0 + s];
      if (key == h && prefix_live(key, stamps[slot0 + s], now, ttl))
        m |= (pfx_u64)masks[slot0 + s];
    }
    mk[wave][k] = m & live_mask;
  }
  __syncthreads();
  if (r >= n_req) return;
  pfx_u64 acc = ~0ULL;
  int run = 0;
  for (int k = 0; k < nb; ++k) {  // acc is wave-uniform (broadcast LDS read)
    acc &= mk[wave][k];
    if (acc == 0) break;
    run += (int)((acc >> lane) & 1ULL);
  }
  matched[(long long)r * 64 + lane] = run;
}

// Slot events of one wave (wave-uniform); counters[0..3] of the table.
struct PrefixSlotEvents {
  int c_new, c_refresh, c_reuse, c_evict;
};

// One (hash, replica bit) entry applied to its bucket by the whole wave;
// he/be/now/ttl are wave-uniform. Lanes 0..15 each own one slot of the
// bucket: the owning lane is the only thread that reads or writes that
// slot, so a wave that applies its entries one after another needs no
// other ordering. Shared by prefix_insert_kernel and
// prefix_apply_remote_kernel.
__device__ __forceinline__ void prefix_bucket_update(
    int64_t* __restrict__ keys, int64_t* __restrict__ masks, int32_t* __restrict__ stamps,
    unsigned bucket_mask, long long he, long long be, int lane, int now, int ttl,
    PrefixSlotEvents& ev) {
  const bool slot_lane = lane < PREFIX_SLOTS;
  long long slot = (long long)((unsigned)(pfx_u64)he & bucket_mask) * PREFIX_SLOTS + lane;
  long long key = 0, mask = 0;
  int stamp = 0;
  if (slot_lane) {  // one round of loads per entry
    key = keys[slot];
    stamp = stamps[slot];
    mask = masks[slot];
  }
  bool live = prefix_live(key, stamp, now, ttl);
  pfx_u64 hit = __ballot(slot_lane && key == he);
  if (hit) {
    int s = __ffsll((long long)hit) - 1;
    bool was_live = (__ballot(live) >> s) & 1ULL;
    if (lane == s) {
      masks[slot] = was_live ? (mask | be) : be;
      stamps[slot] = now;
    }
    ev.c_refresh += 1;
    ev.c_reuse += was_live ? 0 : 1;
    return;
  }
  pfx_u64 empty = __ballot(slot_lane && key == 0);
  pfx_u64 expired = __ballot(slot_lane && key != 0 && !live);
  int v;
  if (empty) {
    v = __ffsll((long long)empty) - 1;
  } else if (expired) {
    v = __ffsll((long long)expired) - 1;
    ev.c_reuse += 1;
  } else {
    // oldest stamp, lowest slot on ties: min of (stamp, slot) packed
    pfx_u64 p = slot_lane ? (((pfx_u64)(unsigned)stamp << 4) | (pfx_u64)lane) : ~0ULL;
    #pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
      pfx_u64 o = __shfl_xor(p, off);
      if (o < p) p = o;
    }
    v = (int)(__shfl(p, 0) & 15ULL);
    ev.c_evict += 1;
  }
  if (lane == v) {
    keys[slot] = he;
    masks[slot] = be;
    stamps[slot] = now;
  }
  ev.c_new += 1;
}

__device__ __forceinline__ void prefix_add_slot_events(int32_t* __restrict__ counters,
                                                       const PrefixSlotEvents& ev, int lane) {
  if (lane == 0) {
    if (ev.c_new) atomicAdd(&counters[0], ev.c_new);
    if (ev.c_refresh) atomicAdd(&counters[1], ev.c_refresh);
    if (ev.c_reuse) atomicAdd(&counters[2], ev.c_reuse);
    if (ev.c_evict) atomicAdd(&counters[3], ev.c_evict);
  }
}

// Deterministic, wait-free insert. Wave w of W owns the buckets with
// bucket % W == w. Every wave scans the whole (request-major, block-minor)
// entry grid 64 entries at a time, ballots the entries whose bucket it
// owns, and applies them one by one in list order. Lanes 0..15 each own one
// slot of the bucket being updated: the owning lane is the only thread that
// ever reads or writes that slot, in this launch, so its own program order
// is all the ordering the table needs. No wave ever waits on another.
//
// counters: [0] new keys written, [1] existing keys refreshed, [2] expired
// slots reused (by their own key or as a victim), [3] live slots evicted.
__global__ __launch_bounds__(256) void prefix_insert_kernel(
    int64_t* __restrict__ keys, int64_t* __restrict__ masks, int32_t* __restrict__ stamps,
    unsigned bucket_mask, int32_t* __restrict__ counters,
    const int64_t* __restrict__ hashes, const int32_t* __restrict__ n_blocks,
    const int32_t* __restrict__ assign, const int64_t* __restrict__ bit_of, int n_rep,
    int n_req, int max_blocks, int now, int ttl) {
  const int lane = threadIdx.x & 63;
  const unsigned W = gridDim.x * 4;
  const unsigned w = blockIdx.x * 4 + (threadIdx.x >> 6);
  const long long n_ent = (long long)n_req * max_blocks;
  PrefixSlotEvents ev = {0, 0, 0, 0};
  // four 64-entry groups are loaded together (the loads of one group are
  // two dependent global-load latencies otherwise), then applied in order
  for (long long e0 = 0; e0 < n_ent; e0 += 4 * 64) {
    long long hs[4], bits[4];
    bool mines[4];
    #pragma unroll
    for (int u = 0; u < 4; ++u) {
      long long e = e0 + u * 64 + lane;
      hs[u] = 0;
      bits[u] = 0;
      mines[u] = false;
      if (e < n_ent) {
        int r = (int)(e / max_blocks), k = (int)(e - (long long)r * max_blocks);
        int a = assign[r];
        if (k < n_blocks[r] && a >= 0 && a < n_rep) {
          hs[u] = hashes[e];
          bits[u] = bit_of[a];
          mines[u] = hs[u] != 0 && ((unsigned)(pfx_u64)hs[u] & bucket_mask) % W == w;
        }
      }
    }
    #pragma unroll
    for (int u = 0; u < 4; ++u) {
      long long h = hs[u], bit = bits[u];
      bool mine = mines[u];
      pfx_u64 todo = __ballot(mine);
      while (todo) {
        int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        long long he = __shfl(h, src);
        long long be = __shfl(bit, src);
        prefix_bucket_update(keys, masks, stamps, bucket_mask, he, be, lane, now, ttl, ev);
      }
    }
  }
  prefix_add_slot_events(counters, ev, lane);
}

// ---- replication across shards: export on the origin, apply on the rest ----
//
// Export is an ordered stream compaction of the insert list, judged against
// the table as it stands before the list is applied (PrefixTable.export).
// Two launches on one stream, no host sync:
//
// 1. prefix_export_flag_kernel, one wave per request (4 per workgroup) like
//    prefix_match_kernel and probing the same bucket: lane = block k decides
//    its entry's export flag; the wave's ballot is the request's flag word
//    for those 64 blocks, its popcount the request's count. Workgroup 0 also
//    snapshots log_n, so that the second launch never reads the word its
//    last workgroup writes.
// 2. prefix_export_write_kernel: workgroup b owns the ``per`` consecutive
//    requests from b * per. Its base is the sum of the counts of all
//    requests before them (one strided pass and a reduction); inside, four
//    requests at a time, one per wave, each offset by the counts before it.
//    An entry's log position is snapshot + offset + popcount of the flag
//    word below its lane: insert-list order whatever the grid. Entries at
//    or past cap are dropped, so the first ones that fit are kept. The last
//    workgroup ends with the grand total and publishes log_n and the
//    exported / dropped counters.
//
// scratch: flag_words uint64[n_req * 4], counts int32[n_req + 1] (the last
// entry is the log_n snapshot).

__global__ __launch_bounds__(256) void prefix_export_flag_kernel(
    const int64_t* __restrict__ keys, const int64_t* __restrict__ masks,
    const int32_t* __restrict__ stamps, unsigned bucket_mask,
    const int64_t* __restrict__ hashes, const int32_t* __restrict__ n_blocks,
    const int32_t* __restrict__ assign, const int64_t* __restrict__ bit_of, int n_rep,
    int n_req, int max_blocks, int now, int ttl, int refresh,
    const int32_t* __restrict__ log_n, pfx_u64* __restrict__ flag_words,
    int32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + wave;
  if (blockIdx.x == 0 && threadIdx.x == 0) counts[n_req] = log_n[0];
  if (r >= n_req) return;  // whole waves leave; there is no barrier below
  int nb = 0;
  pfx_u64 bit = 0;
  const int a = assign[r];
  if (a >= 0 && a < n_rep) {  // as prefix_insert: other requests produce nothing
    nb = n_blocks[r];
    if (nb > max_blocks) nb = max_blocks;
    bit = (pfx_u64)bit_of[a];
  }
  int total = 0;
  #pragma unroll
  for (int g = 0; g < PREFIX_MAX_BLOCKS / 64; ++g) {
    const int k = g * 64 + lane;
    bool flag = false;
    if (k < nb) {
      long long h = hashes[(long long)r * max_blocks + k];
      if (h != 0) {
        long long slot0 = (long long)((unsigned)(pfx_u64)h & bucket_mask) * PREFIX_SLOTS;
        int s = -1;  // the first slot holding h; apply keeps at most one
        #pragma unroll
        for (int j = PREFIX_SLOTS - 1; j >= 0; --j)
          if (keys[slot0 + j] == h) s = j;
        flag = true;
        if (s >= 0) {
          int stamp = stamps[slot0 + s];
          flag = !(prefix_live(h, stamp, now, ttl) &&
                   ((pfx_u64)masks[slot0 + s] & bit) != 0 &&
                   (long long)now - (long long)stamp < (long long)refresh);
        }
      }
    }
    pfx_u64 word = __ballot(flag);
    if (lane == 0) flag_words[(long long)r * 4 + g] = word;
    total += __popcll(word);
  }
  if (lane == 0) counts[r] = total;
}

__global__ __launch_bounds__(256) void prefix_export_write_kernel(
    const int64_t* __restrict__ hashes, const int32_t* __restrict__ assign,
    const int64_t* __restrict__ key_of, int n_req, int max_blocks, int per,
    const pfx_u64* __restrict__ flag_words, const int32_t* __restrict__ counts,
    int64_t* __restrict__ log, long long cap, int32_t* __restrict__ log_n,
    int32_t* __restrict__ repl_counters) {
  __shared__ long long part[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long r_lo = (long long)blockIdx.x * per;
  long long r_hi = r_lo + per;
  if (r_hi > n_req) r_hi = n_req;
  long long sum = 0;
  for (long long i = tid; i < r_lo; i += 256) sum += counts[i];
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
  if (lane == 0) part[wave] = sum;
  __syncthreads();
  long long running = part[0] + part[1] + part[2] + part[3];
  long long n0 = counts[n_req];  // log_n before this call, clamped to the log
  if (n0 < 0) n0 = 0;
  if (n0 > cap) n0 = cap;
  for (long long rg = r_lo; rg < r_hi; rg += 4) {
    // every lane reads the group's four counts (one broadcast load each)
    long long before = 0, group = 0;
    int mine = 0;
    #pragma unroll
    for (int w = 0; w < 4; ++w) {
      int c = rg + w < r_hi ? counts[rg + w] : 0;
      if (w < wave) before += c;
      if (w == wave) mine = c;
      group += c;
    }
    const long long r = rg + wave;
    if (mine > 0) {  // implies r < r_hi and a valid assign[r]
      const long long key = key_of[assign[r]];
      long long pos0 = n0 + running + before;
      #pragma unroll
      for (int g = 0; g < PREFIX_MAX_BLOCKS / 64; ++g) {
        pfx_u64 word = flag_words[r * 4 + g];
        long long pos = pos0 + __popcll(word & ((1ULL << lane) - 1ULL));
        if (((word >> lane) & 1ULL) && pos < cap) {
          log[2 * pos] = hashes[r * max_blocks + g * 64 + lane];
          log[2 * pos + 1] = key;
        }
        pos0 += __popcll(word);
      }
    }
    running += group;
  }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) {  // running is the grand total here
    long long kept = running < cap - n0 ? running : cap - n0;
    log_n[0] = (int)(n0 + kept);
    if (kept) atomicAdd(&repl_counters[0], (int)kept);
    if (running - kept) atomicAdd(&repl_counters[1], (int)(running - kept));
  }
}

// The flat-list sibling of prefix_insert_kernel, for records another shard
// exported: rec is (hash, member key) rows and the replica bit comes from
// looking the key up among this shard's at most 64 member keys (lane i
// holds member i; one compare and ballot per applied record), because every
// shard hands out bits in its own order. Same bucket ownership, same list
// order, same wait-free update. A record with hash 0 or an unknown key is
// skipped; the wave that would own its bucket counts it.
// repl_counters: [2] applied, [3] skipped.
__global__ __launch_bounds__(256) void prefix_apply_remote_kernel(
    int64_t* __restrict__ keys, int64_t* __restrict__ masks, int32_t* __restrict__ stamps,
    unsigned bucket_mask, int32_t* __restrict__ counters, const int64_t* __restrict__ rec,
    long long n_rec, const int64_t* __restrict__ member_keys,
    const int64_t* __restrict__ member_bits, int n_rep, int32_t* __restrict__ repl_counters,
    int now, int ttl) {
  const int lane = threadIdx.x & 63;
  const unsigned W = gridDim.x * 4;
  const unsigned w = blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool member_lane = lane < n_rep;
  const long long mkey = member_lane ? member_keys[lane] : 0;
  const long long mbit = member_lane ? member_bits[lane] : 0;
  PrefixSlotEvents ev = {0, 0, 0, 0};
  int c_applied = 0, c_skipped = 0;  // wave-uniform
  for (long long e0 = 0; e0 < n_rec; e0 += 4 * 64) {
    long long hs[4], ks[4];
    bool mines[4];
    #pragma unroll
    for (int u = 0; u < 4; ++u) {
      long long e = e0 + u * 64 + lane;
      hs[u] = 0;
      ks[u] = 0;
      mines[u] = false;
      if (e < n_rec) {
        hs[u] = rec[2 * e];
        ks[u] = rec[2 * e + 1];
        mines[u] = ((unsigned)(pfx_u64)hs[u] & bucket_mask) % W == w;
      }
    }
    #pragma unroll
    for (int u = 0; u < 4; ++u) {
      long long h = hs[u], k = ks[u];
      pfx_u64 todo = __ballot(mines[u]);
      while (todo) {
        int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        long long he = __shfl(h, src);
        long long ke = __shfl(k, src);
        pfx_u64 known = __ballot(member_lane && mkey == ke);
        if (he == 0 || known == 0) {
          c_skipped += 1;
          continue;
        }
        long long be = __shfl(mbit, __ffsll((long long)known) - 1);
        prefix_bucket_update(keys, masks, stamps, bucket_mask, he, be, lane, now, ttl, ev);
        c_applied += 1;
      }
    }
  }
  prefix_add_slot_events(counters, ev, lane);
  if (lane == 0) {
    if (c_applied) atomicAdd(&repl_counters[2], c_applied);
    if (c_skipped) atomicAdd(&repl_counters[3], c_skipped);
  }
}

// masks &= ~mask over the whole table: one streaming pass, run before a
// retired replica bit is handed to a new member.
__global__ __launch_bounds__(256) void prefix_clear_bits_kernel(int64_t* __restrict__ masks,
                                                                long long n, long long keep) {
  long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    masks[i] &= keep;
}

// kv_scorer_kernel with a prefix-hit term: hit = min(matched * B, p) tokens
// of the request are already cached on the replica, so only p - hit tokens
// are charged against its KV space, and w_p * hit / max(p, 1) is added to
// its score. With w_p = 0 and matched = 0 this is kv_scorer_kernel exactly.
__global__ void kv_scorer_prefix_kernel(const float* __restrict__ stats,  // R x 4
                                        int n_rep, const float* __restrict__ pred_tokens,
                                        int n_req, const int32_t* __restrict__ matched,
                                        int matched_stride, int block_tokens, float w_kv,
                                        float w_q, float w_a, float w_p,
                                        int32_t* __restrict__ assign) {
  int lane = threadIdx.x & 63;
  bool ok = lane < n_rep;
  float kv_used = ok ? stats[lane * 4 + 0] : 0.f;
  float kv_cap = ok ? stats[lane * 4 + 1] : 1.f;
  float kv_total = fmaxf(kv_cap, 1.f);
  float queue = ok ? stats[lane * 4 + 2] : 0.f;
  float active = ok ? stats[lane * 4 + 3] : 0.f;
  for (int i = 0; i < n_req; ++i) {
    float p = pred_tokens[i];
    int m = ok ? matched[(long long)i * matched_stride + lane] : 0;
    float hit = fminf((float)(m * block_tokens), p);
    float p_eff = p - hit;
    float score = ok ? (w_kv * (1.f - (kv_used + p_eff) / kv_total) - w_q * queue -
                        w_a * active + w_p * hit / fmaxf(p, 1.f))
                     : -1e30f;
    if (ok && kv_used + p_eff > kv_cap) score -= 1e6f;
    float best = score;
    int best_lane = lane;
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      float os = __shfl_xor(best, off);
      int ol = __shfl_xor(best_lane, off);
      if (os > best || (os == best && ol < best_lane)) { best = os; best_lane = ol; }
    }
    if (lane == 0) assign[i] = best_lane;
    if (lane == best_lane) {
      kv_used += p_eff;
      active += 1.f;
      queue += 1.f;
    }
  }
}
