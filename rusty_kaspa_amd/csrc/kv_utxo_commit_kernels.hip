/* MI355X-native UTXO-set MuHash commitment (gfx950, PRODUCT code).
 *
 * ⇔ the multiset a node builds when it imports a pruning-point UTXO set
 * (Consensus::append_imported_pruning_point_utxos, consensus/src/consensus/
 * mod.rs:1139-1152: MuHash::from_utxo of every entry, folded by a map-reduce)
 * and checks against the header (import_pruning_point_utxo_set,
 * consensus/src/pipeline/virtual_processor/processor.rs:1525-1538), and the
 * per-block invariant of verify_expected_utxo_state (utxo_validation.rs:188-195).
 *
 * utxo_entry_element: one table entry → its U3072 element, exactly
 * MuHash::from_utxo over write_utxo (consensus/core/src/muhash.rs:55-69):
 *   tx_id ‖ index u32 ‖ daa_score u64 ‖ amount u64 ‖ is_coinbase u8 ‖
 *   spk_version u16 ‖ spk_len u64 ‖ spk
 * hashed with keyed BLAKE2b-256("MuHashElement") and expanded by ChaCha20 to
 * 384 bytes = 48 LE limbs (crypto/muhash/src/lib.rs:148-169). The script is
 * read inline when spk_len ≤ 36 and IN PLACE from the arena when the entry
 * carries KV_UTXO_F_SPK_ARENA — no gather copy. An entry with
 * KV_UTXO_F_COVENANT appends the 32-byte covenant id held in bytes 28..60 of
 * its value (muhash.rs:66-67); such a value always has its script in the
 * arena. The function uses no wave intrinsics: tests/host_shim/
 * utxo_element.cpp compiles it with g++.
 *
 * Whole-table commitment (kv_utxo_commitment), per window of
 * KV_COMMIT_WINDOW slots, all on one stream with no host round trip:
 *   1. kv_utxo_commit_compact_kernel — wave ballot + one atomic per wave packs
 *      the window's READY slot indices; the live count stays on the device.
 *   2. kv_utxo_commit_element_kernel — lane i < count hashes slot idx[i], so
 *      EMPTY and TOMB slots never reach BLAKE2b/ChaCha.
 *   3. kv_u3072_reduce_wave_acc_kernel — the device-count sibling of
 *      kv_u3072_reduce_wave_kernel: wave w multiplies elements w, w+stride, …
 *      (count read from device memory) INTO running accumulator w. The
 *      accumulators start at one, so a wave that finds nothing leaves the
 *      identity in place.
 * After the last window the KV_COMMIT_LANES accumulators reduce to one value
 * with the existing kv_u3072_reduce_wave_kernel (host-known counts).
 * Multiplication order is free: the group is commutative.
 *
 * Scratch is a function of the compiled window only, never of table capacity:
 *   idx        KV_COMMIT_WINDOW × 4 B
 *   elements   KV_COMMIT_WINDOW × 384 B
 *   acc        KV_COMMIT_LANES × 384 B
 *   partials   2 × 1024 × 384 B (final reduce ping-pong)
 *   out        one commit_out record (the single copy back)
 */
#ifndef KV_HOST_TEST
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>
#include <string.h>

#include "kaspa_engine_abi.h"
#include "kv_hash_device.h"
#include "kv_u3072.h"

#ifndef KV_COMMIT_WINDOW
#define KV_COMMIT_WINDOW (1u << 17) /* slots per scan window (power of two) */
#endif
#define KV_COMMIT_LANES 4096u /* running accumulators = first-pass stride */

namespace kv {

__device__ __constant__ static const uint8_t KEY_UTXO_ELEM[13] = {
    'M', 'u', 'H', 'a', 's', 'h', 'E', 'l', 'e', 'm', 'e', 'n', 't'};

/* keyed-hash output → 48 LE limbs: ChaCha20 (key = hash, zero nonce), blocks
 * 0..5 — the same tail as kv_muhash_element_kernel */
__device__ inline void muhash_expand_element(const uint8_t hash[32], uint64_t *out) {
  uint32_t key[8];
#pragma unroll
  for (int i = 0; i < 8; i++)
    key[i] = (uint32_t)hash[4 * i] | ((uint32_t)hash[4 * i + 1] << 8) |
             ((uint32_t)hash[4 * i + 2] << 16) | ((uint32_t)hash[4 * i + 3] << 24);
  uint8_t stream[64];
  for (int blk = 0; blk < 6; blk++) {
    chacha20_block(key, blk, stream);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      uint64_t w = 0;
#pragma unroll
      for (int j = 0; j < 8; j++) w |= (uint64_t)stream[8 * i + j] << (8 * j);
      out[blk * 8 + i] = w;
    }
  }
}

/* a packed 64B value whose script this code may read: inline scripts fit the
 * slot, arena scripts lie inside the arena's used prefix. A covenant id takes
 * the inline field, so KV_UTXO_F_COVENANT without the arena flag is refused. */
__device__ inline int utxo_value_spk_ok(const uint8_t *val64, uint64_t arena_len) {
  uint16_t flags;
  uint32_t spk_len, off;
  memcpy(&flags, val64 + 16, 2);
  memcpy(&spk_len, val64 + 20, 4);
  if (!(flags & KV_UTXO_F_SPK_ARENA))
    return spk_len <= 36 && !(flags & KV_UTXO_F_COVENANT);
  memcpy(&off, val64 + 24, 4);
  return spk_len <= KV_UTXO_MAX_SPK && (uint64_t)off + spk_len <= arena_len;
}

/* (outpoint 36B, packed table value 64B, arena base) → 48-limb element */
__device__ inline void utxo_entry_element(const uint8_t *op36, const uint8_t *val64,
                                          const uint8_t *arena, uint64_t *out) {
  uint64_t amount, daa;
  uint16_t flags, spk_version;
  uint32_t spk_len;
  memcpy(&amount, val64, 8);
  memcpy(&daa, val64 + 8, 8);
  memcpy(&flags, val64 + 16, 2);
  memcpy(&spk_version, val64 + 18, 2);
  memcpy(&spk_len, val64 + 20, 4);
  const uint8_t *spk = val64 + 24;
  if (flags & KV_UTXO_F_SPK_ARENA) {
    uint32_t off;
    memcpy(&off, val64 + 24, 4);
    spk = arena + off;
  }
  b2b_state S;
  b2b_init_keyed(S, KEY_UTXO_ELEM, 13);
  b2b_update(S, op36, 36); /* tx_id ‖ index u32 LE, as stored */
  b2b_update_u64(S, daa);
  b2b_update_u64(S, amount);
  uint8_t cb = (flags & KV_UTXO_F_COINBASE) ? 1 : 0;
  b2b_update(S, &cb, 1);
  b2b_update_u16(S, spk_version);
  b2b_update_u64(S, spk_len);
  b2b_update(S, spk, spk_len);
  if (flags & KV_UTXO_F_COVENANT) b2b_update(S, val64 + 28, 32);
  uint8_t hash[32];
  b2b_final(S, hash);
  muhash_expand_element(hash, out);
}

#ifndef KV_HOST_TEST

/* the one record copied back at the end of a chain */
struct commit_out {
  uint64_t limbs[KVU_LIMBS];
  unsigned long long n_live;
  uint32_t fail; /* a READY slot whose script reference is out of range */
  uint32_t _pad;
};

__device__ __forceinline__ void u3072_store_one(uint64_t *out) {
  for (int k = 0; k < KVU_LIMBS; k++) out[k] = k == 0;
}

/* READY slots of [slot_base, slot_base + n_slots) → idx[0..*count), window-
 * relative. *count is zeroed by the host's memset node before each window. */
extern "C" __global__ void kv_utxo_commit_compact_kernel(
    const utxo_slot *__restrict__ table, uint64_t slot_base, uint32_t n_slots,
    uint32_t *__restrict__ idx, uint32_t *count) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  int lane = threadIdx.x & 63;
  int ready = i < n_slots && table[slot_base + i].state == KV_SLOT_READY;
  unsigned long long mask = __ballot(ready);
  if (mask == 0) return;
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(count, (uint32_t)__popcll(mask));
  base = __shfl(base, 0);
  if (ready) idx[base + __popcll(mask & ((1ULL << lane) - 1))] = i;
}

/* lane i < *count: element of slot idx[i] → elements[i] */
extern "C" __global__ void kv_utxo_commit_element_kernel(
    const utxo_slot *__restrict__ table, uint64_t slot_base,
    const uint32_t *__restrict__ idx, const uint32_t *count,
    const uint8_t *__restrict__ arena, uint64_t arena_len,
    uint64_t *__restrict__ elements, commit_out *out) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= *count) return;
  const utxo_slot *s = &table[slot_base + idx[i]];
  uint64_t *e = elements + (size_t)i * KVU_LIMBS;
  if (!utxo_value_spk_ok(s->value, arena_len)) {
    out->fail = 1;
    u3072_store_one(e);
    return;
  }
  utxo_entry_element(s->key, s->value, arena, e);
}

/* the import path: entry i of a chunk as staged on the device (values already
 * rewritten to their arena offsets) → elements[i] */
extern "C" __global__ void kv_utxo_chunk_element_kernel(
    const uint8_t *__restrict__ outpoints, const uint8_t *__restrict__ values,
    uint32_t n, const uint8_t *__restrict__ arena, uint64_t arena_len,
    uint64_t *__restrict__ elements, commit_out *out) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t *val = values + (size_t)i * 64;
  uint64_t *e = elements + (size_t)i * KVU_LIMBS;
  if (!utxo_value_spk_ok(val, arena_len)) {
    out->fail = 1;
    u3072_store_one(e);
    return;
  }
  utxo_entry_element(outpoints + (size_t)i * 36, val, arena, e);
}

extern "C" __global__ void kv_u3072_fill_one_kernel(uint64_t *__restrict__ vals,
                                                    uint32_t n) {
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n * KVU_LIMBS) vals[t] = (t % KVU_LIMBS) == 0;
}

/* single wave: the final value into the copy-back record */
extern "C" __global__ void kv_u3072_commit_out_kernel(const uint64_t *__restrict__ src,
                                                      commit_out *out) {
  if (threadIdx.x < KVU_LIMBS) out->limbs[threadIdx.x] = src[threadIdx.x];
}

#endif /* !KV_HOST_TEST */

} // namespace kv

#ifndef KV_HOST_TEST
/* one WAVE per running accumulator: acc[w] *= elements[w] · elements[w+stride] · …
 * The element count comes from device memory (count_dev) when given, else from
 * n_host; it is also added to out->n_live. A wave with no element returns
 * before touching its accumulator. */
extern "C" __global__ void kv_u3072_reduce_wave_acc_kernel(
    const uint64_t *__restrict__ elements, const uint32_t *count_dev, uint32_t n_host,
    uint32_t stride, uint64_t *acc, kv::commit_out *out) {
  uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) / 64;
  int lane = threadIdx.x & 63;
  if (wave >= stride) return;
  uint32_t n = count_dev ? *count_dev : n_host;
  if (wave == 0 && lane == 0) out->n_live += n;
  if (wave >= n) return;
  uint64_t a = lane < 48 ? acc[(size_t)wave * KVU_LIMBS + lane] : 0;
  for (uint32_t i = wave; i < n; i += stride) {
    uint64_t e = lane < 48 ? elements[(size_t)i * KVU_LIMBS + lane] : 0;
    a = u3072_wave_mulmod(a, e);
  }
  if (lane < 48) acc[(size_t)wave * KVU_LIMBS + lane] = a;
}
#endif /* !KV_HOST_TEST */
