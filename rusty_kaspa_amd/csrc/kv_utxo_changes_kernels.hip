/* MI355X-native per-script UTXO changes of one journaled diff (gfx950, PRODUCT
 * code): what UtxosChanged notifications are made of, read from the device
 * undo journal and the live table.
 *
 * ⇔ UtxoIndexChanges::update_utxo_diff (indexes/utxoindex/src/
 * update_container.rs:29-51: the removed and the added entries of a diff,
 * grouped by script public key, and the supply change),
 * UtxosChangedNotification::apply_utxos_changed_subscription / filter_utxo_set
 * (indexes/core/src/notification.rs:81-127: keep the subscribed scripts) and
 * supply_change -> update_circulating_supply (indexes/utxoindex/src/
 * index.rs:98). The reference builds these on the host from a diff the host
 * holds. Here the removed side of a diff exists only in the journal record
 * (kv_utxo_journal_kernels.hip), so the join runs where the record lies.
 *
 * Change indices. A record with n_removed and n_added rows has
 * cursor_end = n_removed + 2·n_added of them, one lane each:
 *   c <  n_removed          removed row c: the captured value, found bit on
 *   c =  n_removed + 2k     added row k: the value the add overwrote, found
 *                           bit on
 *   c =  n_removed + 2k + 1 added row k: the value the table holds NOW
 *                           (utxo_find), script inline or in the live arena
 * The first two kinds left the set (KV_UTXO_CHANGE_F_REMOVED), the third
 * entered it; KV_UTXO_CHANGES_REVERSED swaps the labels and nothing else. The
 * added side is a probe of the live table and no second copy in the record:
 * the record stays what kv_utxo_apply_diff made it, and an added outpoint a
 * later diff removed is counted in n_added_gone.
 *
 * A record value's script reference is an offset into the record's own blob,
 * a live value's one into the arena: spk_query_match takes either as its
 * "arena" and routes the value to a subscribed script unchanged.
 *
 * utxo_change_locate and utxo_change_pack use no wave intrinsics and no slot
 * type: tests/host_shim/utxo_changes.cpp compiles them with g++.
 */
#ifndef KV_HOST_TEST
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>
#include <string.h>

#include "kaspa_engine_abi.h"

namespace kv {

#define KV_CHANGE_BYTES 96u
/* a staged record: the 96 bytes, then what the host needs to fetch the script
 * (words 24..35: script source, offset, the value's 36-byte inline field) */
#define KV_CHANGE_STAGED_WORDS 36u
#define KV_CHANGE_STAGED_BYTES (4u * KV_CHANGE_STAGED_WORDS)
#define KV_CHANGE_SPK_INLINE 0u /* in words 26..35 of the staged record */
#define KV_CHANGE_SPK_BLOB 1u   /* at `offset` in the record's script blob */
#define KV_CHANGE_SPK_ARENA 2u  /* at `offset` in the live arena */
/* a stored key: change index | spk_len << 48. A diff side has at most 2^30
 * rows, so an index is below 2^32; a length is at most KV_UTXO_MAX_SPK. */
#define KV_CHANGE_KEY_LEN_SHIFT 48

struct utxo_change_loc {
  uint64_t row; /* row of the record: removed side first */
  int live;     /* 1: the value comes from the table, 0: from the record */
  int removed;  /* the label under `flags` */
};

/* change index -> row, source and label. c < n_removed + 2·n_added. */
__host__ __device__ inline utxo_change_loc utxo_change_locate(uint64_t c,
                                                              uint64_t n_removed,
                                                              uint32_t flags) {
  utxo_change_loc loc;
  if (c < n_removed) {
    loc.row = c;
    loc.live = 0;
  } else {
    loc.row = n_removed + ((c - n_removed) >> 1);
    loc.live = (int)((c - n_removed) & 1);
  }
  loc.removed = (loc.live == 0) != ((flags & KV_UTXO_CHANGES_REVERSED) != 0);
  return loc;
}

/* The 96-byte change record, as 24 little-endian words, from the outpoint
 * (9 words), the packed 64-byte value (16 words), the query index and the
 * label. Byte layout as in kaspa_engine_abi.h: the match record of
 * kv_utxo_find_by_spk with spk_version in 58..60, spk_len in 60..64 and
 * KV_UTXO_CHANGE_F_REMOVED among the flags. */
__host__ __device__ inline void utxo_change_pack(uint32_t *out24, const uint32_t *key9,
                                                 const uint32_t *val16, uint32_t query_index,
                                                 int removed) {
#pragma unroll
  for (int w = 0; w < 9; w++) out24[w] = key9[w];
  out24[9] = query_index;
#pragma unroll
  for (int w = 0; w < 4; w++) out24[10 + w] = val16[w]; /* amount, daa_score */
  /* word 4 of the value: flags in the low half, spk_version in the high one */
  const uint32_t flags = val16[4] & (KV_UTXO_F_COINBASE | KV_UTXO_F_COVENANT);
  out24[14] = (val16[4] & 0xffff0000u) | flags |
              (removed ? KV_UTXO_CHANGE_F_REMOVED : 0u);
  out24[15] = val16[5]; /* spk_len */
#pragma unroll
  for (int w = 0; w < 8; w++) /* covenant id: bytes 28..60 of the value */
    out24[16 + w] = (flags & KV_UTXO_F_COVENANT) ? val16[7 + w] : 0u;
}

#ifndef KV_HOST_TEST

/* the record kv_utxo_changes_by_spk copies back. Index 0 of the pairs counts
 * the entries whose value came from the record (they left the set, read
 * forward), index 1 those found live (they entered it). */
struct changes_rec {
  unsigned long long amount[2];
  unsigned long long count[2];
  unsigned long long n_added_gone;
  uint32_t stored; /* matches with c >= cursor */
  uint32_t fail;   /* a value's script reference fails utxo_value_spk_ok */
};

/* One lane per change index over [0, total), total = n_removed + 2·n_added; the
 * grid is whole blocks and lanes past `total` only take part in the ballots.
 * Record rows are 64 B (values) and 36 B (keys) apart from allocation bases,
 * slot values 16-byte aligned: a value is four uint4 loads either way.
 * keys_out and staged_out hold out_cap entries; the host passes out_cap =
 * total - cursor, the number of lanes that can store. */
extern "C" __global__ void kv_utxo_changes_kernel(
    utxo_slot *table, uint64_t cap_mask, const uint8_t *__restrict__ keys,
    const uint8_t *__restrict__ vals, const unsigned long long *__restrict__ found,
    unsigned long long n_removed, unsigned long long total,
    const uint8_t *__restrict__ blob, uint64_t blob_bytes,
    const uint8_t *__restrict__ arena, uint64_t arena_len, spk_query_set S,
    uint32_t flags, unsigned long long cursor, uint32_t out_cap,
    unsigned long long *__restrict__ keys_out, uint8_t *__restrict__ staged_out,
    changes_rec *rec) {
  const unsigned long long c =
      (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  utxo_change_loc loc = {0, 0, 0};
  uint4 val[4] = {};
  const uint32_t *key = (const uint32_t *)keys;
  int present = 0, gone = 0;
  int32_t m = KV_SPK_MATCH_NONE;
  if (c < total) {
    loc = utxo_change_locate(c, n_removed, flags);
    key = (const uint32_t *)(keys + loc.row * 36);
    const uint4 *src = nullptr;
    if (!loc.live) {
      if ((found[loc.row / 64] >> (loc.row % 64)) & 1)
        src = (const uint4 *)(vals + loc.row * 64);
    } else {
      const utxo_slot *s = utxo_find(table, cap_mask, (const uint8_t *)key);
      if (s) src = (const uint4 *)s->value; /* value at +48 of a 16B-aligned slot */
      else gone = 1;
    }
    if (src) {
#pragma unroll
      for (int k = 0; k < 4; k++) val[k] = src[k];
      const uint8_t *spk_base = loc.live ? arena : blob;
      const uint64_t spk_bytes = loc.live ? arena_len : blob_bytes;
      if (flags & KV_UTXO_CHANGES_ALL)
        m = utxo_value_spk_ok((const uint8_t *)val, spk_bytes) ? 0 : KV_SPK_MATCH_BAD;
      else
        m = spk_query_match((const uint8_t *)val, spk_base, spk_bytes, S);
      present = m != KV_SPK_MATCH_BAD;
    }
  }
  /* no lane has returned: every ballot and wave sum sees the whole wave */
  const unsigned long long amount =
      present ? ((unsigned long long)val[0].y << 32) | val[0].x : 0ULL;
  const unsigned long long sum_rec = wave_sum_u64(present && !loc.live ? amount : 0ULL);
  const unsigned long long sum_live = wave_sum_u64(present && loc.live ? amount : 0ULL);
  const unsigned long long in_rec = __ballot(present && !loc.live);
  const unsigned long long in_live = __ballot(present && loc.live);
  const unsigned long long any_gone = __ballot(gone);
  const unsigned long long any_bad = __ballot(m == KV_SPK_MATCH_BAD);
  const int store = m >= 0 && c >= cursor;
  const unsigned long long hit = __ballot(store);
  uint32_t base = 0;
  if (lane == 0) {
    if (sum_rec) atomicAdd(&rec->amount[0], sum_rec);
    if (sum_live) atomicAdd(&rec->amount[1], sum_live);
    if (in_rec) atomicAdd(&rec->count[0], (unsigned long long)__popcll(in_rec));
    if (in_live) atomicAdd(&rec->count[1], (unsigned long long)__popcll(in_live));
    if (any_gone) atomicAdd(&rec->n_added_gone, (unsigned long long)__popcll(any_gone));
    if (any_bad) rec->fail = 1;
    if (hit) base = atomicAdd(&rec->stored, (uint32_t)__popcll(hit));
  }
  base = __shfl(base, 0);
  if (!store) return;
  const uint32_t pos = base + (uint32_t)__popcll(hit & ((1ULL << lane) - 1));
  if (pos >= out_cap) return; /* cannot happen: at most total - cursor lanes store */
  const uint32_t *v = (const uint32_t *)val;
  uint32_t st[KV_CHANGE_STAGED_WORDS];
  utxo_change_pack(st, key, v,
                   (flags & KV_UTXO_CHANGES_ALL) ? 0xffffffffu : (uint32_t)m, loc.removed);
  st[24] = !(v[4] & KV_UTXO_F_SPK_ARENA) ? KV_CHANGE_SPK_INLINE
           : loc.live                    ? KV_CHANGE_SPK_ARENA
                                         : KV_CHANGE_SPK_BLOB;
  st[25] = v[6]; /* the script offset of an out-of-line value */
#pragma unroll
  for (int w = 0; w < 9; w++) st[26 + w] = v[6 + w]; /* bytes 24..60 of the value */
  st[35] = 0;
  keys_out[pos] = c | ((unsigned long long)v[5] << KV_CHANGE_KEY_LEN_SHIFT);
  uint4 *o = (uint4 *)(staged_out + (size_t)pos * KV_CHANGE_STAGED_BYTES);
#pragma unroll
  for (int k = 0; k < (int)(KV_CHANGE_STAGED_WORDS / 4); k++)
    o[k] = make_uint4(st[4 * k], st[4 * k + 1], st[4 * k + 2], st[4 * k + 3]);
}

#endif /* !KV_HOST_TEST */

} // namespace kv
