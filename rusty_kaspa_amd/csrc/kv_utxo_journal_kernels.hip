/* MI355X-native undo journal of the GPU-resident UTXO set (gfx950, PRODUCT
 * code).
 *
 * ⇔ the stored per-block diffs the virtual processor walks when the selected
 * chain changes (calculate_utxo_state_relatively, consensus/src/pipeline/
 * virtual_processor/processor.rs:393-437: with_diff_in_place(as_reversed) on
 * the way down, write_diff_batch on the way up; UtxoDiff::as_reversed,
 * consensus/core/src/utxo/utxo_diff.rs:71).
 *
 * kv_utxo_apply_diff captures, per outpoint of a diff, whether the table held
 * it and the 64-byte value it held, BEFORE the diff touches it; kv_utxo_revert
 * plays that record back. A record lives in device memory and is
 * self-contained: keys, values, a found bitmap and its own copy of the long
 * scripts. It names no slot and no offset into the live arena, so
 * kv_utxo_rehash may run between an apply and its revert.
 *
 * Record rows are the diff's outpoints, removed side first, then added side:
 *   row i <  n_removed : captured and tombstoned (the remove of the diff);
 *   row i >= n_removed : captured only (the upsert of the diff follows).
 * The two sides are one launch. The outpoints of a diff are distinct (the host
 * checks it), so no row looks for a key another row tombstones: a capture-only
 * row that meets a slot another row is tombstoning sees READY or TOMB with a
 * foreign key either way, and walks on.
 *
 * utxo_value_journal_rewrite uses no wave intrinsics and no slot type:
 * tests/host_shim/utxo_journal.cpp compiles it with g++.
 */
#ifndef KV_HOST_TEST
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>
#include <string.h>

#include "kaspa_engine_abi.h"

namespace kv {

#define KV_JOURNAL_SET 0    /* new reference = add            (capture) */
#define KV_JOURNAL_REBASE 1 /* new reference = old one + add  (revert)  */

/* The one place a journaled value's script reference is rewritten, in place.
 *   capture: live arena offset -> offset in the record's script blob
 *            (mode SET, add = the blob cursor, src_len = the arena's used
 *            prefix, dst_len = the u32 offset range);
 *   revert:  blob offset -> live arena offset (mode REBASE, add = where the
 *            blob was appended to the arena, src_len = the blob's bytes,
 *            dst_len = the arena's used prefix after the append).
 * An inline value (no KV_UTXO_F_SPK_ARENA) is left as stored: returns 0.
 * An arena value keeps its flag and every other byte and gets the new u32
 * reference: returns 1, with the old reference and the script length reported.
 * A reference that fails the rule of utxo_value_spk_ok against src_len, or
 * whose new span would end past dst_len or past a u32, is NOT rewritten and
 * returns -1: the caller sets its fail word and does not dereference. */
__host__ __device__ inline int utxo_value_journal_rewrite(uint8_t *val64, int mode,
                                                          uint64_t add, uint64_t src_len,
                                                          uint64_t dst_len,
                                                          uint32_t *old_off,
                                                          uint32_t *spk_len) {
  uint16_t flags;
  uint32_t len, off;
  memcpy(&flags, val64 + 16, 2);
  memcpy(&len, val64 + 20, 4);
  *spk_len = len;
  *old_off = 0;
  if (!(flags & KV_UTXO_F_SPK_ARENA)) return len <= 36 ? 0 : -1;
  memcpy(&off, val64 + 24, 4);
  *old_off = off;
  if (len > KV_UTXO_MAX_SPK || (uint64_t)off + len > src_len) return -1;
  uint64_t now = mode == KV_JOURNAL_REBASE ? add + off : add;
  if (now < add || now > 0xffffffffULL || now + len > dst_len ||
      now + len > 0xffffffffULL)
    return -1;
  uint32_t now32 = (uint32_t)now;
  memcpy(val64 + 24, &now32, 4);
  return 1;
}

#ifndef KV_HOST_TEST

/* the record kv_utxo_apply_diff copies back after the capture launch */
struct journal_rec {
  unsigned long long blob_bytes;       /* cursor of the record's script blob */
  unsigned long long n_removed_missing;
  unsigned long long n_added_overwrote;
  uint32_t n_jobs;                     /* script copy jobs appended */
  uint32_t fail;
};

/* the probe of kv_utxo_lookup_kernel / kv_utxo_remove_kernel: the READY slot
 * holding `key`, or NULL */
__device__ __forceinline__ utxo_slot *utxo_find(utxo_slot *table, uint64_t cap_mask,
                                                const uint8_t *key) {
  uint64_t slot = op_hash(key) & cap_mask;
  for (uint64_t probe = 0; probe <= cap_mask; probe++, slot = (slot + 1) & cap_mask) {
    utxo_slot *s = &table[slot];
    uint32_t st = s->state;
    if (st == KV_SLOT_EMPTY) return nullptr;
    if (st == KV_SLOT_READY && key_eq(s->key, key)) return s;
  }
  return nullptr;
}

/* row i of a diff (keys 36 B each, removed side first): one probe. On a hit
 * the 64-byte value goes to vals_out row i; an arena value takes spk_len bytes
 * at the record's blob cursor (one atomic per such lane; they are rare), is
 * stored with that blob offset, and appends a (src_off, len, dst_off) job for
 * kv_arena_copy_jobs_kernel. Only then does a removed-side row release-store
 * TOMB: tombstoning frees no arena bytes, so the copy job that follows on the
 * stream still finds the script. A value whose script reference fails
 * utxo_value_journal_rewrite sets the fail word, is recorded as not found and
 * is not tombstoned. found[] gets one word per wave by ballot; the two
 * consistency counters take one atomic per wave. */
extern "C" __global__ void kv_utxo_journal_capture_kernel(
    utxo_slot *table, uint64_t cap_mask, const uint8_t *__restrict__ keys,
    unsigned long long n, unsigned long long n_removed, uint64_t arena_len,
    uint8_t *__restrict__ vals_out, unsigned long long *__restrict__ found,
    arena_gather_job *__restrict__ jobs, uint32_t jobs_cap, journal_rec *rec) {
  unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int is_removed = i < n_removed;
  int hit = 0;
  if (i < n) {
    const uint8_t *key = keys + i * 36;
    utxo_slot *s = utxo_find(table, cap_mask, key);
    if (s) {
      /* slots are 16-byte aligned: value at +48 */
      uint4 val[4];
#pragma unroll
      for (int k = 0; k < 4; k++) val[k] = ((const uint4 *)s->value)[k];
      uint32_t len = val[1].y, src_off, j = 0;
      unsigned long long at = 0;
      /* flags: low half of word 4 */
      const int took_job = (val[1].x & KV_UTXO_F_SPK_ARENA) && len <= KV_UTXO_MAX_SPK;
      if (took_job) {
        at = atomicAdd(&rec->blob_bytes, (unsigned long long)len);
        j = atomicAdd(&rec->n_jobs, 1u);
      }
      int kind = j < jobs_cap
                     ? utxo_value_journal_rewrite((uint8_t *)val, KV_JOURNAL_SET, at,
                                                  arena_len, 0xffffffffULL, &src_off, &len)
                     : -1;
      /* every job index handed out is written: a refused reference leaves an
       * empty job, never a hole for kv_arena_copy_jobs_kernel to read */
      if (took_job && j < jobs_cap)
        jobs[j] = kind == 1 ? arena_gather_job{src_off, len, (uint32_t)at, 0}
                            : arena_gather_job{0, 0, 0, 0};
      if (kind >= 0) {
        uint4 *vo = (uint4 *)(vals_out + i * 64);
#pragma unroll
        for (int k = 0; k < 4; k++) vo[k] = val[k];
        if (is_removed)
          __hip_atomic_store(&s->state, KV_SLOT_TOMB, __ATOMIC_RELEASE,
                             __HIP_MEMORY_SCOPE_AGENT);
        hit = 1;
      } else {
        rec->fail = 1;
      }
    }
  }
  /* no lane has returned: every ballot sees the whole wave */
  unsigned long long mask = __ballot(hit);
  unsigned long long missing = __ballot(i < n && is_removed && !hit);
  unsigned long long overwrote = __ballot(i < n && !is_removed && hit);
  if ((threadIdx.x & 63) == 0 && i < n) {
    found[i / 64] = mask;
    if (missing)
      atomicAdd(&rec->n_removed_missing, (unsigned long long)__popcll(missing));
    if (overwrote)
      atomicAdd(&rec->n_added_overwrote, (unsigned long long)__popcll(overwrote));
  }
}

/* revert, first launch: added-side rows (first_row = n_removed) whose found
 * bit is OFF were absent before the diff and are removed again. Rows whose bit
 * is on do nothing here. */
extern "C" __global__ void kv_utxo_journal_unadd_kernel(
    utxo_slot *table, uint64_t cap_mask, const uint8_t *__restrict__ keys,
    const unsigned long long *__restrict__ found, unsigned long long first_row,
    unsigned long long n) {
  unsigned long long i =
      first_row + (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || ((found[i / 64] >> (i % 64)) & 1)) return;
  utxo_slot *s = utxo_find(table, cap_mask, keys + i * 36);
  if (s)
    __hip_atomic_store(&s->state, KV_SLOT_TOMB, __ATOMIC_RELEASE,
                       __HIP_MEMORY_SCOPE_AGENT);
}

/* revert, second launch (after the first: the upsert's tombstone discipline
 * assumes no concurrent remove): every row whose found bit is ON gets its
 * captured value back through the upsert of kv_utxo_upsert_kernel — removed
 * rows are re-inserted, overwritten added rows get the old value. The record's
 * script blob was appended to the live arena at arena_base; an arena value is
 * rebased to arena_base + its blob offset on the way. Rows whose bit is off do
 * nothing. The record itself is only read. */
extern "C" __global__ void kv_utxo_journal_restore_kernel(
    utxo_slot *table, uint64_t cap_mask, const uint8_t *__restrict__ keys,
    const uint8_t *__restrict__ vals, const unsigned long long *__restrict__ found,
    unsigned long long n, uint64_t arena_base, uint64_t blob_bytes,
    uint64_t arena_len, int *fail_flag) {
  unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !((found[i / 64] >> (i % 64)) & 1)) return;
  uint4 val[4];
#pragma unroll
  for (int k = 0; k < 4; k++) val[k] = ((const uint4 *)(vals + i * 64))[k];
  uint32_t off, len;
  if (utxo_value_journal_rewrite((uint8_t *)val, KV_JOURNAL_REBASE, arena_base,
                                 blob_bytes, arena_len, &off, &len) < 0 ||
      utxo_upsert_lane(table, cap_mask, keys + i * 36, (const uint8_t *)val))
    *fail_flag = 1;
}

#endif /* !KV_HOST_TEST */

} // namespace kv
