/* MI355X-native UTXO-set queries by script public key (gfx950, PRODUCT code):
 * balances, entry counts, the circulating supply and the matching entries,
 * answered by a filtered scan of the one GPU-resident table.
 *
 * ⇔ UtxoIndexApi (indexes/utxoindex/src/core/api/mod.rs:23-30:
 * get_circulating_supply, get_utxos_by_script_public_keys,
 * get_balance_by_script_public_keys). The reference keeps a second database
 * for this, keyed version u16 ‖ len u64 ‖ script ‖ outpoint
 * (indexes/utxoindex/src/stores/indexed_utxos.rs:156-198), re-derived from
 * every virtual diff. Here nothing is kept in step: the set already sits in
 * HBM, and a query is one pass over it.
 *
 * The query set on the device (spk_query_set), one allocation:
 *   hash   u64[slots]   script hash of the query in that slot
 *   qidx   u32[slots]   query index + 1, 0 = free
 *   q      kv_spk_query[n_q]
 *   off    u32[n_q]     offset of query i's script in the blob
 *   blob                the scripts, concatenated in query order
 * slots = smallest power of two >= max(64, 2·n_q), open addressing, linear
 * probing. At KV_UTXO_QUERY_MAX queries that is 12 B × 131,072 + 12 B × 65,536
 * = 2.25 MiB plus the blob.
 *
 * spk_hash is over (version, length, the spk_len script bytes): never over the
 * zero-padded 36-byte inline field, or "abc" and "abc\0" would route alike.
 * The hash only routes; the compare of version, length and every byte decides.
 * With KV_SPK_HASH_CONST every hash is equal and every result must stay the
 * same (tests/host_shim/utxo_spk_query.cpp builds both ways).
 *
 * spk_hash, spk_query_check, spk_query_build and spk_query_match use no wave
 * intrinsics and no slot type: the host shim compiles them with g++, and the
 * engine's host side builds the table with the same spk_query_build, so host
 * and device cannot disagree on the hash. utxo_value_spk_ok comes from
 * kv_utxo_commit_kernels.hip, included before this file.
 *
 * Kernels:
 *   kv_utxo_balance_kernel  one grid-stride pass, the shape of
 *     kv_utxo_stats_kernel. READY lanes add their amount into a wave reduction
 *     for the supply (one atomic per wave per counter) and run the match; a
 *     wave whose ballot of matches is empty does nothing more. Matching lanes
 *     add into balances[q] / counts[q] with 64-bit atomics; when every
 *     matching lane of the wave has the same q (`combine`), the wave sums
 *     first and lane 0 issues the two atomics.
 *   kv_utxo_find_kernel     one launch per scan window. Matching lanes take
 *     positions by ballot + one atomic per wave and write their slot index and
 *     the 96-byte match record straight from the slot. Stop rule: before each
 *     window the host queues a 4-byte device-to-device copy of the match count
 *     into rec->seen; a window whose seen >= max_entries does nothing but
 *     record its index with atomicMin. The decision is the same for every wave
 *     of a launch, launches of one stream run in order, so the windows that
 *     ran are a prefix of the walk, each of them complete, and the count never
 *     passes max_entries - 1 + one window: the size of the output lists.
 */
#ifndef KV_HOST_TEST
#include <hip/hip_runtime.h>
#endif
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "kaspa_engine_abi.h"

namespace kv {

#define KV_SPK_MATCH_NONE (-1)
#define KV_SPK_MATCH_BAD (-2) /* the value fails utxo_value_spk_ok */

/* pointers into the one allocation described above (device side), or into the
 * host staging copy of it (spk_query_build, the host shim) */
struct spk_query_set {
  const uint64_t *hash;
  const uint32_t *qidx;
  const kv_spk_query *q;
  const uint32_t *off;
  const uint8_t *blob;
  uint32_t mask; /* slots - 1 */
  uint32_t n_q;
};

__host__ __device__ inline uint32_t spk_query_slots(size_t n_q) {
  uint32_t s = 64;
  while (s < 2 * n_q) s <<= 1;
  return s;
}

/* 64-bit hash of (version, length, script bytes): 8 bytes a step, the tail
 * assembled byte by byte so nothing past spk + len is read */
__host__ __device__ inline uint64_t spk_hash(uint16_t version, uint32_t len,
                                             const uint8_t *spk) {
#ifdef KV_SPK_HASH_CONST
  (void)version, (void)len, (void)spk;
  return 0;
#else
  uint64_t h = 0x9e3779b97f4a7c15ULL ^ (((uint64_t)len << 16) | version);
  h *= 0xff51afd7ed558ccdULL;
  h ^= h >> 32;
  uint32_t i = 0;
  for (; i + 8 <= len; i += 8) {
    uint64_t w;
    memcpy(&w, spk + i, 8);
    h = (h ^ w) * 0xff51afd7ed558ccdULL;
    h ^= h >> 32;
  }
  if (i < len) {
    uint64_t w = 0;
    for (uint32_t k = 0; i + k < len; k++) w |= (uint64_t)spk[i + k] << (8 * k);
    h = (h ^ w) * 0xff51afd7ed558ccdULL;
    h ^= h >> 32;
  }
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ULL;
  h ^= h >> 33;
  return h;
#endif
}

__host__ __device__ inline int spk_bytes_eq(const uint8_t *a, const uint8_t *b,
                                            uint32_t len) {
  uint32_t i = 0;
  for (; i + 8 <= len; i += 8) {
    uint64_t x, y;
    memcpy(&x, a + i, 8);
    memcpy(&y, b + i, 8);
    if (x != y) return 0;
  }
  for (; i < len; i++)
    if (a[i] != b[i]) return 0;
  return 1;
}

/* the argument rules of kv_utxo_balance_by_spk / kv_utxo_find_by_spk that need
 * no table: 0, or -1 for too many queries, a script longer than
 * KV_UTXO_MAX_SPK, a non-zero `zero` field, or a blob whose length is not the
 * sum of the script lengths */
__host__ __device__ inline int spk_query_check(const kv_spk_query *q, size_t n_q,
                                               size_t blob_len) {
  if (n_q > KV_UTXO_QUERY_MAX) return -1;
  uint64_t sum = 0;
  for (size_t i = 0; i < n_q; i++) {
    if (q[i].spk_len > KV_UTXO_MAX_SPK || q[i].zero != 0) return -1;
    sum += q[i].spk_len;
  }
  return sum == blob_len ? 0 : -1;
}

/* Fills off[n_q], hash[slots] and qidx[slots] (slots = spk_query_slots(n_q))
 * for queries that passed spk_query_check. Returns 0, or 1 when two queries are
 * equal in version, length and bytes (the reference takes a HashSet of
 * scripts); the arrays are then half built and must not be used. */
__host__ __device__ inline int spk_query_build(const kv_spk_query *q, size_t n_q,
                                               const uint8_t *blob, uint32_t *off,
                                               uint64_t *hash, uint32_t *qidx,
                                               uint32_t slots) {
  const uint32_t mask = slots - 1;
  for (uint32_t s = 0; s < slots; s++) hash[s] = 0, qidx[s] = 0;
  uint32_t at = 0;
  for (size_t i = 0; i < n_q; i++) {
    off[i] = at;
    const uint8_t *spk = blob + at;
    at += q[i].spk_len;
    const uint64_t h = spk_hash(q[i].spk_version, q[i].spk_len, spk);
    uint32_t s = (uint32_t)h & mask;
    for (; qidx[s]; s = (s + 1) & mask) { /* load <= 1/2: a free slot exists */
      const uint32_t j = qidx[s] - 1;
      if (hash[s] == h && q[j].spk_len == q[i].spk_len &&
          q[j].spk_version == q[i].spk_version &&
          spk_bytes_eq(blob + off[j], spk, q[i].spk_len))
        return 1;
    }
    hash[s] = h;
    qidx[s] = (uint32_t)i + 1;
  }
  return 0;
}

/* a packed 64B table value → the index of the query its script equals,
 * KV_SPK_MATCH_NONE, or KV_SPK_MATCH_BAD when its script reference fails
 * utxo_value_spk_ok (the reference is then not followed). Inline scripts are
 * read from the value, arena scripts in place from the arena; a covenant id
 * plays no part. */
__device__ inline int32_t spk_query_match(const uint8_t *val64, const uint8_t *arena,
                                          uint64_t arena_len, const spk_query_set &S) {
  if (!utxo_value_spk_ok(val64, arena_len)) return KV_SPK_MATCH_BAD;
  if (S.n_q == 0) return KV_SPK_MATCH_NONE;
  uint16_t flags, version;
  uint32_t len;
  memcpy(&flags, val64 + 16, 2);
  memcpy(&version, val64 + 18, 2);
  memcpy(&len, val64 + 20, 4);
  const uint8_t *spk = val64 + 24;
  if (flags & KV_UTXO_F_SPK_ARENA) {
    uint32_t off;
    memcpy(&off, val64 + 24, 4);
    spk = arena + off;
  }
  const uint64_t h = spk_hash(version, len, spk);
  uint32_t s = (uint32_t)h & S.mask;
  for (uint32_t probe = 0; probe <= S.mask; probe++, s = (s + 1) & S.mask) {
    const uint32_t qi = S.qidx[s];
    if (!qi) return KV_SPK_MATCH_NONE;
    if (S.hash[s] != h) continue;
    const kv_spk_query head = S.q[qi - 1];
    if (head.spk_len == len && head.spk_version == version &&
        spk_bytes_eq(S.blob + S.off[qi - 1], spk, len))
      return (int32_t)(qi - 1);
  }
  return KV_SPK_MATCH_NONE;
}

#ifndef KV_HOST_TEST

#define KV_QUERY_MATCH_BYTES 96u

/* the record both calls copy back; the find walk uses the last three words */
struct query_rec {
  unsigned long long total, n_live; /* over all READY entries */
  uint32_t fail;          /* a READY entry's script reference is out of range */
  uint32_t count;         /* matches stored so far (find) */
  uint32_t seen;          /* count as copied before the current window */
  uint32_t first_skipped; /* smallest window index that did nothing */
};

/* n_slots is a power of two >= 64 and every wave starts at a multiple of 64
 * (as kv_utxo_stats_kernel): the lanes of a wave enter and leave the loop
 * together, every ballot and wave sum sees the whole wave. */
extern "C" __global__ void kv_utxo_balance_kernel(
    const utxo_slot *__restrict__ table, uint64_t n_slots, spk_query_set S,
    const uint8_t *__restrict__ arena, uint64_t arena_len,
    unsigned long long *balances, unsigned long long *counts, int combine,
    query_rec *rec) {
  const int lane = threadIdx.x & 63;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  uint32_t live = 0;
  unsigned long long total = 0;
  int bad = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots;
       i += stride) {
    const utxo_slot *s = &table[i];
    const int ready = s->state == KV_SLOT_READY;
    int32_t m = KV_SPK_MATCH_NONE;
    unsigned long long amount = 0;
    if (ready) {
      amount = *(const unsigned long long *)s->value; /* value is 16B-aligned */
      m = spk_query_match(s->value, arena, arena_len, S);
      bad |= m == KV_SPK_MATCH_BAD;
    }
    live += (uint32_t)__popcll(__ballot(ready));
    total += amount;
    const unsigned long long hit = __ballot(m >= 0);
    if (hit == 0) continue; /* the common case */
    const int32_t m0 = __shfl(m, __ffsll((long long)hit) - 1);
    if (combine && __ballot(m == m0) == hit) {
      /* every matching lane pays into one query: one wave sum, two atomics */
      unsigned long long sum = wave_sum_u64(m >= 0 ? amount : 0);
      if (lane == 0) {
        atomicAdd(&balances[m0], sum);
        atomicAdd(&counts[m0], (unsigned long long)__popcll(hit));
      }
    } else if (m >= 0) {
      atomicAdd(&balances[m], amount);
      atomicAdd(&counts[m], 1ULL);
    }
  }
  total = wave_sum_u64(total);
  const unsigned long long any_bad = __ballot(bad);
  if (lane != 0) return;
  if (live) atomicAdd(&rec->n_live, (unsigned long long)live);
  if (total) atomicAdd(&rec->total, total);
  if (any_bad) rec->fail = 1;
}

/* slots [slot_base, slot_base + n_slots) of one window (n_slots need not be a
 * multiple of 64: the walk may start inside a window; the grid is whole waves
 * and lanes past n_slots only take part in the ballot). out_cap bounds both
 * output lists. */
extern "C" __global__ void kv_utxo_find_kernel(
    const utxo_slot *__restrict__ table, uint64_t slot_base, uint32_t n_slots,
    spk_query_set S, const uint8_t *__restrict__ arena, uint64_t arena_len,
    uint32_t max_entries, uint32_t window, uint32_t out_cap,
    unsigned long long *__restrict__ slots_out, uint8_t *__restrict__ recs_out,
    query_rec *rec) {
  if (rec->seen >= max_entries) { /* no launch writes `seen`: same for all */
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicMin(&rec->first_skipped, window);
    return;
  }
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const utxo_slot *s = &table[slot_base + (i < n_slots ? i : 0)];
  int32_t m = KV_SPK_MATCH_NONE;
  if (i < n_slots && s->state == KV_SLOT_READY) {
    m = spk_query_match(s->value, arena, arena_len, S);
    if (m == KV_SPK_MATCH_BAD) rec->fail = 1;
  }
  const unsigned long long hit = __ballot(m >= 0);
  if (hit == 0) return;
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(&rec->count, (uint32_t)__popcll(hit));
  base = __shfl(base, 0);
  if (m < 0) return;
  const uint32_t pos = base + (uint32_t)__popcll(hit & ((1ULL << lane) - 1));
  if (pos >= out_cap) return; /* cannot happen under the stop rule */
  slots_out[pos] = slot_base + i;
  /* key at +8 and value at +48 of a 16B-aligned slot; a record is 6 × 16 B */
  const uint32_t *k = (const uint32_t *)s->key;
  const uint32_t *v = (const uint32_t *)s->value;
  uint32_t *o = (uint32_t *)(recs_out + (size_t)pos * KV_QUERY_MATCH_BYTES);
#pragma unroll
  for (int w = 0; w < 9; w++) o[w] = k[w];
  o[9] = (uint32_t)m;
#pragma unroll
  for (int w = 0; w < 4; w++) o[10 + w] = v[w]; /* amount, daa_score */
  const uint32_t flags = v[4] & 0xffffu & ~KV_UTXO_F_SPK_ARENA;
  o[14] = flags;
  o[15] = 0;
#pragma unroll
  for (int w = 0; w < 8; w++) /* covenant id: bytes 28..60 of the value */
    o[16 + w] = (flags & KV_UTXO_F_COVENANT) ? v[7 + w] : 0u;
}

#endif /* !KV_HOST_TEST */

} // namespace kv
