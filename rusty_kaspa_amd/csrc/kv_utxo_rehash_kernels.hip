/* MI355X-native UTXO table maintenance (gfx950, PRODUCT code): occupancy
 * statistics, in-place rehash / grow / shrink / compaction, chunked export.
 *
 * All three walk the slot array of kv_utxo_kernels.hip and do something with
 * each live entry:
 *   kv_utxo_stats         counts it (and the arena bytes it owns);
 *   kv_utxo_rehash        re-inserts it into a fresh table and a fresh arena;
 *   kv_utxo_export_chunk  copies it out — the serving half of pruning-point
 *                         sync (get_pruning_point_utxos / get_virtual_utxos,
 *                         consensus/src/consensus/mod.rs:1067-1108), whose
 *                         receiving half is kv_utxo_import_chunk.
 * Rehash and export reuse kv_utxo_commit_compact_kernel and the commitment
 * scratch's index list and count word, one window of KV_COMMIT_WINDOW slots at
 * a time, and read each window's live count from device memory.
 *
 * utxo_value_export uses no wave intrinsics and no slot type:
 * tests/host_shim/utxo_export.cpp compiles it with g++.
 */
#ifndef KV_HOST_TEST
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>
#include <string.h>

#include "kaspa_engine_abi.h"

namespace kv {

/* a packed 64B table value → the record kv_utxo_upsert_spk /
 * kv_utxo_import_chunk take, in place. Inline values are left as stored. An
 * arena value loses KV_UTXO_F_SPK_ARENA and has its 36-byte spk field zeroed
 * (a covenant value: bytes 24..28 only, the flag and the id in 28..60 stay);
 * its script length and arena offset are reported and 1 is returned. */
__host__ __device__ inline int utxo_value_export(uint8_t *val64, uint32_t *spk_len,
                                                 uint32_t *arena_off) {
  uint16_t flags;
  memcpy(&flags, val64 + 16, 2);
  memcpy(spk_len, val64 + 20, 4);
  *arena_off = 0;
  if (!(flags & KV_UTXO_F_SPK_ARENA)) return 0;
  memcpy(arena_off, val64 + 24, 4);
  flags &= (uint16_t)~KV_UTXO_F_SPK_ARENA;
  memcpy(val64 + 16, &flags, 2);
  memset(val64 + 24, 0, (flags & KV_UTXO_F_COVENANT) ? 4 : 36);
  return 1;
}

#ifndef KV_HOST_TEST

/* the record kv_utxo_stats copies back (n_arena is internal: it sizes the
 * rehash job list) */
struct table_scan_rec {
  unsigned long long n_live, n_tomb, n_empty;
  unsigned long long arena_live_bytes;
  unsigned long long n_arena;
};

/* the record kv_utxo_rehash copies back */
struct rehash_rec {
  unsigned long long inserted;   /* slots published in the new table */
  unsigned long long arena_head; /* allocation cursor of the new arena */
  uint32_t n_jobs;               /* arena copy jobs appended */
  uint32_t fail;
};

#define KV_STATS_MAX_BLOCKS 4096u

/* export side record of one gathered entry: arena offset | script length << 32
 * for an arena entry, 0 for an inline one, all ones for a value whose script
 * reference fails utxo_value_spk_ok */
#define KV_EXPORT_REF_BAD (~0ULL)

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v; /* lane 0 holds the sum */
}

/* One pass over the slot array, grid-stride. States are counted by ballot +
 * popcount, arena bytes by a wave reduction; each wave issues one atomic per
 * counter at the end. n_slots is a power of two >= 64 and every wave starts at
 * a multiple of 64, so the lanes of a wave enter and leave the loop together
 * and every ballot sees the whole wave. */
extern "C" __global__ void kv_utxo_stats_kernel(const utxo_slot *__restrict__ table,
                                                uint64_t n_slots,
                                                table_scan_rec *rec) {
  const int lane = threadIdx.x & 63;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  uint32_t live = 0, tomb = 0, empty = 0, arena = 0;
  unsigned long long bytes = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots;
       i += stride) {
    const utxo_slot *s = &table[i];
    uint32_t st = s->state;
    int in_arena = 0;
    if (st == KV_SLOT_READY) {
      uint16_t flags;
      uint32_t spk_len;
      memcpy(&flags, s->value + 16, 2);
      memcpy(&spk_len, s->value + 20, 4);
      if (flags & KV_UTXO_F_SPK_ARENA) {
        in_arena = 1;
        bytes += spk_len;
      }
    }
    live += (uint32_t)__popcll(__ballot(st == KV_SLOT_READY));
    tomb += (uint32_t)__popcll(__ballot(st == KV_SLOT_TOMB));
    empty += (uint32_t)__popcll(__ballot(st == KV_SLOT_EMPTY));
    arena += (uint32_t)__popcll(__ballot(in_arena));
  }
  bytes = wave_sum_u64(bytes);
  if (lane != 0) return;
  if (live) atomicAdd(&rec->n_live, (unsigned long long)live);
  if (tomb) atomicAdd(&rec->n_tomb, (unsigned long long)tomb);
  if (empty) atomicAdd(&rec->n_empty, (unsigned long long)empty);
  if (arena) atomicAdd(&rec->n_arena, (unsigned long long)arena);
  if (bytes) atomicAdd(&rec->arena_live_bytes, bytes);
}

/* lane i < *count: source slot idx[i] → the new table.
 *
 * This is not the upsert kernel. The keys of one table are distinct and the
 * destination holds no tombstones, so a lane never compares keys, never waits
 * for a CLAIMED slot to publish and never restarts: any slot that is not EMPTY
 * is simply occupied, and the first EMPTY slot it wins by CAS is its own. The
 * probe is bounded by the slot count; running out sets the fail word.
 *
 * An arena entry allocates spk_len bytes at the new arena's cursor (one atomic
 * per such lane; they are rare), has its offset rewritten before the slot is
 * published, and appends a (src_off, len, dst_off) job for
 * kv_arena_copy_jobs_kernel. Nothing is written past new_arena_cap or
 * jobs_cap: an allocation that would not fit sets the fail word instead. */
extern "C" __global__ void kv_utxo_rehash_insert_kernel(
    const utxo_slot *__restrict__ src, uint64_t slot_base,
    const uint32_t *__restrict__ idx, const uint32_t *count, utxo_slot *dst,
    uint64_t dst_mask, uint64_t old_arena_len, uint64_t new_arena_cap,
    arena_gather_job *__restrict__ jobs, uint32_t jobs_cap, rehash_rec *rec) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  int done = 0;
  if (i < *count) {
    const utxo_slot *s = &src[slot_base + idx[i]];
    /* slots are 16-byte aligned: key at +8, value at +48 */
    uint64_t key[5];
    uint4 val[4];
#pragma unroll
    for (int k = 0; k < 5; k++) key[k] = ((const uint64_t *)s->key)[k];
#pragma unroll
    for (int k = 0; k < 4; k++) val[k] = ((const uint4 *)s->value)[k];
    int ok = utxo_value_spk_ok((const uint8_t *)val, old_arena_len);
    if (ok && (val[1].x & KV_UTXO_F_SPK_ARENA)) { /* flags: low half of word 4 */
      uint32_t spk_len = val[1].y, src_off = val[1].z;
      unsigned long long at = atomicAdd(&rec->arena_head, (unsigned long long)spk_len);
      uint32_t j = atomicAdd(&rec->n_jobs, 1u);
      if (at + spk_len > new_arena_cap || at + spk_len > 0xffffffffULL ||
          j >= jobs_cap) {
        ok = 0;
      } else {
        jobs[j] = arena_gather_job{src_off, spk_len, (uint32_t)at, 0};
        val[1].z = (uint32_t)at;
      }
    }
    if (ok) {
      uint64_t slot = op_hash((const uint8_t *)key) & dst_mask;
      for (uint64_t probe = 0; probe <= dst_mask; probe++, slot = (slot + 1) & dst_mask) {
        utxo_slot *t = &dst[slot];
        uint32_t expected = KV_SLOT_EMPTY;
        if (!__hip_atomic_compare_exchange_strong(&t->state, &expected, KV_SLOT_CLAIMED,
                                                  __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE,
                                                  __HIP_MEMORY_SCOPE_AGENT))
          continue; /* occupied, whatever its state */
#pragma unroll
        for (int k = 0; k < 5; k++) ((uint64_t *)t->key)[k] = key[k];
#pragma unroll
        for (int k = 0; k < 4; k++) ((uint4 *)t->value)[k] = val[k];
        __hip_atomic_store(&t->state, KV_SLOT_READY, __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_AGENT);
        done = 1;
        break;
      }
    }
    if (!done) rec->fail = 1;
  }
  /* no lane has returned: lane 0 of every wave is here to add its wave's count */
  unsigned long long mask = __ballot(done);
  if ((threadIdx.x & 63) == 0 && mask)
    atomicAdd(&rec->inserted, (unsigned long long)__popcll(mask));
}

/* kv_arena_gather_kernel with the job count in device memory: one job per
 * block, 256 threads striding the bytes. The grid is sized from the stats
 * pass's arena entry count, an upper bound of *n_jobs. */
extern "C" __global__ void kv_arena_copy_jobs_kernel(
    const uint8_t *__restrict__ arena, const arena_gather_job *__restrict__ jobs,
    const uint32_t *n_jobs, uint32_t jobs_cap, uint8_t *__restrict__ out) {
  uint32_t j = blockIdx.x;
  if (j >= *n_jobs || j >= jobs_cap) return;
  arena_gather_job job = jobs[j];
  for (uint32_t i = threadIdx.x; i < job.len; i += blockDim.x)
    out[job.dst_off + i] = arena[job.src_off + i];
}

/* lane i < *count: (key, exported value, script reference) of slot idx[i] to
 * staging row i. Rows are in compaction order; the host sorts them by idx. */
extern "C" __global__ void kv_utxo_export_gather_kernel(
    const utxo_slot *__restrict__ table, uint64_t slot_base,
    const uint32_t *__restrict__ idx, const uint32_t *count, uint64_t arena_len,
    uint8_t *__restrict__ keys_out, uint8_t *__restrict__ vals_out,
    unsigned long long *__restrict__ refs_out) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= *count) return;
  const utxo_slot *s = &table[slot_base + idx[i]];
  uint4 val[4];
#pragma unroll
  for (int k = 0; k < 4; k++) val[k] = ((const uint4 *)s->value)[k];
  unsigned long long ref = KV_EXPORT_REF_BAD;
  if (utxo_value_spk_ok((const uint8_t *)val, arena_len)) {
    uint32_t spk_len, off;
    ref = utxo_value_export((uint8_t *)val, &spk_len, &off)
              ? ((unsigned long long)spk_len << 32) | off
              : 0;
  }
  refs_out[i] = ref;
  uint32_t *ko = (uint32_t *)(keys_out + (size_t)i * 36);
#pragma unroll
  for (int k = 0; k < 9; k++) ko[k] = ((const uint32_t *)s->key)[k];
  uint4 *vo = (uint4 *)(vals_out + (size_t)i * 64);
#pragma unroll
  for (int k = 0; k < 4; k++) vo[k] = val[k];
}

#endif /* !KV_HOST_TEST */

} // namespace kv
