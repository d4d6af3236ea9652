/* kaspa_engine_abi.h — the C-ABI drop-in boundary of the MI355X-native
 * transaction-validation engine.
 *
 * This header declares exactly what a Rust host (rusty-kaspa) would bind over FFI
 * to replace its validation hot path. Each entry point cites the reference
 * interface it replaces (kaspanet/rusty-kaspa v2.0.1, paths relative to the
 * reference root):
 *
 *   kv_validate_block       ⇔ TransactionValidator::validate_populated_transaction_and_get_fee
 *                             fanned out per tx, plus the muhash monoid reduce
 *                             (consensus/src/processes/transaction_validator/
 *                              tx_validation_in_utxo_context.rs:37-67;
 *                              consensus/src/pipeline/virtual_processor/
 *                              utxo_validation.rs:319-348)
 *   kv_check_scripts        ⇔ check_scripts (tx_validation_in_utxo_context.rs:181-218)
 *                             for a single tx of the batch
 *   kv_verify_schnorr_batch ⇔ batched secp256k1::schnorr::Signature::verify
 *                             (crypto/txscript/src/lib.rs:869)
 *   kv_verify_ecdsa_batch   ⇔ batched secp256k1::ecdsa::Signature::verify
 *                             (crypto/txscript/src/lib.rs:899)
 *   kv_sighash_batch        ⇔ calc_schnorr_signature_hash / calc_ecdsa_signature_hash
 *                             (consensus/core/src/hashing/sighash.rs:245-292)
 *   kv_muhash_finalize      ⇔ MuHash::finalize (crypto/muhash/src/lib.rs:93)
 *   kv_utxo_commitment      ⇔ the multiset of the whole UTXO set that
 *                             import_pruning_point_utxo_set checks against the
 *                             header (consensus/src/pipeline/virtual_processor/
 *                             processor.rs:1525-1538) and that
 *                             verify_expected_utxo_state implies per block
 *                             (utxo_validation.rs:188-195)
 *   kv_utxo_commitment_window  slots per scan window of kv_utxo_commitment
 *   kv_utxo_import_chunk    ⇔ Consensus::append_imported_pruning_point_utxos
 *                             (consensus/src/consensus/mod.rs:1139-1152)
 *   kv_utxo_apply_diff      ⇔ write_diff_batch (consensus/src/model/stores/
 *                             utxo_set.rs:107-112), keeping the diff's inverse
 *   kv_utxo_revert          ⇔ with_diff_in_place(as_reversed) of one chain
 *                             block (processor.rs:410, utxo_diff.rs:71)
 *   kv_utxo_journal_drop    ⇔ the stored diffs of blocks past finality depth
 *                             going away
 *   kv_utxo_journal_stats   what the undo journal holds
 *   kv_validate_block_utxo_undo  kv_validate_block_utxo(apply_diff = 1) with a
 *                             revertible diff
 *   kv_utxo_balance_by_spk  ⇔ UtxoIndexApi::get_balance_by_script_public_keys
 *                             and get_circulating_supply
 *                             (indexes/utxoindex/src/core/api/mod.rs:23-30)
 *   kv_utxo_find_by_spk     ⇔ UtxoIndexApi::get_utxos_by_script_public_keys
 *                             (same place), paginated
 *
 * No torch types cross this boundary: plain pointers and sizes only.
 * See INTEGRATION.md for the Rust-side binding a maintainer would add.
 */
#ifndef KASPA_ENGINE_ABI_H
#define KASPA_ENGINE_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ======================================================================
 * Transaction batch blob format (little-endian throughout)
 *
 * The host (Rust over FFI, or the C++/Python harness here) flattens a block's
 * transactions WITH their populated UTXO entries into one contiguous buffer —
 * the borrow-only contract of validate_populated_transaction_and_get_fee
 * (caller owns everything, engine retains nothing).
 *
 *   Blob     := u32 n_txs, u32 tx_offset[n_txs], Tx...
 *   Tx       := u16 version, u16 n_inputs, u16 n_outputs, u16 _pad,
 *               u64 lock_time, u8 subnetwork_id[20], u32 payload_len, u64 gas,
 *               u64 storage_mass, u8 tx_id[32],   // id is carried AND re-derivable
 *               u8 payload[payload_len],
 *               Input[n_inputs], Output[n_outputs]
 *   Input    := u8 prev_tx_id[32], u32 prev_index, u64 sequence,
 *               u8 commit_kind (0 = sigop_count, 1 = compute_budget),
 *               u8 _pad, u16 commit_value,
 *               u32 sig_script_len, u8 sig_script[...],
 *               // populated UtxoEntry (consensus/core/src/utxo/utxo_entry.rs:20)
 *               u64 utxo_amount, u64 utxo_daa_score, u8 utxo_is_coinbase,
 *               u8 utxo_has_covenant_id, u16 utxo_spk_version,
 *               u32 utxo_spk_len, u8 utxo_spk[...],
 *               u8 utxo_covenant_id[32 if utxo_has_covenant_id else 0]
 *   Output   := u64 value, u16 spk_version, u16 _pad, u32 spk_len, u8 spk[...],
 *               u8 has_covenant, (u16 cov_authorizing_input, u8 cov_id[32] if has)
 * ====================================================================== */

/* ---- validation flags (TxValidationFlags, tx_validation_in_utxo_context.rs:24-34) */
#define KV_FLAGS_FULL 0u
#define KV_FLAGS_SKIP_SCRIPT_CHECKS 1u
#define KV_FLAGS_SKIP_MASS_CHECK 2u

/* ---- per-tx result codes ----
 * 0 = valid. 1..99 mirror TxRuleError variants on the non-script path
 * (consensus/src/processes/transaction_validator/errors.rs).
 * 100+s = SignatureInvalid(script error s); 200+s = SignatureEmpty(script error s)
 * (the map_script_err convention, tx_validation_in_utxo_context.rs:220-222). */
#define KV_OK 0
#define KV_ERR_IMMATURE_COINBASE 1
#define KV_ERR_INPUT_AMOUNT_OVERFLOW 2
#define KV_ERR_INPUT_AMOUNT_TOO_HIGH 3
#define KV_ERR_SPEND_TOO_HIGH 4
#define KV_ERR_WRONG_MASS 5
#define KV_ERR_SEQUENCE_LOCK 6
#define KV_ERR_FEERATE_TOO_LOW 7
#define KV_ERR_MASS_INCOMPUTABLE 8
#define KV_ERR_MISSING_OUTPOINT 9   /* populate failure: outpoint not in the UTXO set
                                       (ruleerrors::RuleError::MissingTxOutpoints) */
/* body-in-isolation rule codes (RuleError::{DuplicateTransactions,
 * DoubleSpendInSameBlock, ChainedTransaction}) */
#define KV_ERR_BODY_DUP_TX 10
#define KV_ERR_BODY_DOUBLE_SPEND 11
#define KV_ERR_BODY_CHAINED 12
/* covenant bindings (TxRuleError::CovenantsError ⇔ CovenantsContext::from_tx,
 * crypto/txscript/src/covenants.rs:101-163), checked after the sequence lock
 * and before any script work (tx_validation_in_utxo_context.rs:58) */
#define KV_ERR_COVENANT_AUTH_INPUT 13 /* AuthInputOutOfBounds: an output's
                                         authorizing_input >= input count */
#define KV_ERR_COVENANT_GENESIS_ID 14 /* WrongGenesisCovenantId: a genesis group's
                                         id is not hashing::covenant_id of it */
#define KV_ERR_BAD_BLOB 90
#define KV_ERR_SIGNATURE_INVALID_BASE 100
#define KV_ERR_SIGNATURE_EMPTY_BASE 200

/* TxScriptError variants (kaspa-txscript-errors crate) used as s above */
#define KV_SCRIPT_EVAL_FALSE 1
#define KV_SCRIPT_EMPTY_STACK 2
#define KV_SCRIPT_CLEAN_STACK 3
#define KV_SCRIPT_NULL_FAIL 4
#define KV_SCRIPT_NOT_PUSH_ONLY 5
#define KV_SCRIPT_INVALID_SIG_HASH_TYPE 6
#define KV_SCRIPT_INVALID_PUBKEY 7
#define KV_SCRIPT_INVALID_SIGNATURE 8
#define KV_SCRIPT_VERIFY_ERROR 9
#define KV_SCRIPT_EARLY_RETURN 10
#define KV_SCRIPT_OPCODE_RESERVED 11
#define KV_SCRIPT_OPCODE_DISABLED 12
#define KV_SCRIPT_INVALID_OPCODE 13
#define KV_SCRIPT_MALFORMED_PUSH 14
#define KV_SCRIPT_STACK_SIZE_EXCEEDED 15
#define KV_SCRIPT_TOO_MANY_OPERATIONS 16
#define KV_SCRIPT_ELEMENT_TOO_BIG 17
#define KV_SCRIPT_INVALID_STACK_OPERATION 18
#define KV_SCRIPT_UNBALANCED_CONDITIONAL 19
#define KV_SCRIPT_INVALID_STATE 20
#define KV_SCRIPT_NUMBER_TOO_BIG 21
#define KV_SCRIPT_NOT_MINIMAL_DATA 22
#define KV_SCRIPT_INVALID_PUBKEY_COUNT 23
#define KV_SCRIPT_INVALID_SIGNATURE_COUNT 24
#define KV_SCRIPT_PUBKEY_FORMAT 25
#define KV_SCRIPT_SCRIPT_SIZE 26
#define KV_SCRIPT_NO_SCRIPTS 27
#define KV_SCRIPT_EXCEEDED_SCRIPT_UNITS 28
#define KV_SCRIPT_UNSATISFIED_LOCKTIME 29
#define KV_SCRIPT_INVALID_INPUT_INDEX 30
#define KV_SCRIPT_INVALID_SOURCE 31
#define KV_SCRIPT_INVALID_INDEX 32
#define KV_SCRIPT_INVALID_RANGE 33
#define KV_SCRIPT_UNSUPPORTED_OPCODE 63 /* engine-only: routed to CPU fallback */

/* Structurally-distinct "route this tx back to the reference CPU interpreter"
 * signal: an engine per-tx code that is NEGATIVE, so no binder can fold it
 * into the reject path by accident (every reject code is >= 1; 0 is accept).
 * Emitted when a script's execution reaches an opcode the engine does not
 * decide (currently only OpZkPrecompile, 0xa6). The legacy 1xx/2xx+63 codes
 * are no longer produced by the engine. */
#define KV_TX_DEFER_TO_CPU (-63)

/* ---- engine lifecycle ---- */

typedef struct kv_ctx kv_ctx; /* opaque; thread-safe (Sync), internally synchronized */

typedef struct {
  uint64_t coinbase_maturity;   /* params.coinbase_maturity(): mainnet 1000 (Crescendo) */
  uint64_t mass_per_sig_op;     /* params.mass_per_sig_op: mainnet 1000 grams */
  uint64_t sig_cache_size;      /* TransactionValidator sig_cache entries (10_000) */
  int device;                   /* HIP device ordinal, -1 = default */
} kv_params;

/* Create / destroy an engine context. Fails (returns NULL) if no HIP device is
 * available — there is NO CPU fallback in the product path. */
kv_ctx *kv_create(const kv_params *params);
void kv_destroy(kv_ctx *ctx);
/* Human-readable description of the last error on this thread. */
const char *kv_last_error(void);

/* ---- the drop-in entry points ---- */

/* Validate a block's transactions (blob format above) against their populated
 * entries. Writes per-tx result codes and fees, and the muhash partial
 * (numerator 384B ‖ denominator 384B LE) over the txs that validated OK —
 * mirroring validate_transactions_with_muhash_in_parallel
 * (utxo_validation.rs:319-348; coinbase txs are skipped by the caller there,
 * so the blob should not contain them — if it does, pass their index in
 * skip_mask). Returns 0 on success (even when some txs are invalid), <0 on
 * malformed blob / device error. Blocking; callable from multiple threads. */
int kv_validate_block(kv_ctx *ctx, const uint8_t *blob, size_t blob_len,
                      uint64_t pov_daa_score, uint64_t block_daa_score, uint32_t flags,
                      int32_t *tx_codes_out /*[n_txs]*/, uint64_t *fees_out /*[n_txs]*/,
                      uint8_t *muhash_partial_out /*[768] or NULL*/);

/* Batched BIP-340 Schnorr verify — the "verify_schnorr batch API" of the north
 * star. tuples = n × 128 bytes: r(32) ‖ s(32) ‖ pk_xonly(32) ‖ msg(32), SoA-major
 * not required (the engine re-lays-out on device). bitmap_out: bit i set ⇔ tuple
 * i valid. Returns 0, or <0 on device error. */
int kv_verify_schnorr_batch(kv_ctx *ctx, const uint8_t *tuples, size_t n,
                            uint64_t *bitmap_out /*[ceil(n/64)]*/);

/* Batched ECDSA verify. tuples = n × 129 bytes: r(32) ‖ s(32) ‖ pk33(33) ‖ msg(32). */
int kv_verify_ecdsa_batch(kv_ctx *ctx, const uint8_t *tuples, size_t n,
                          uint64_t *bitmap_out);

/* Batched sighash: for each (tx_index, input_index, hash_type, ecdsa) job, compute
 * the 32-byte signing hash of the blob's tx input. */
typedef struct {
  uint32_t tx_index;
  uint32_t input_index;
  uint8_t hash_type;
  uint8_t ecdsa;
  uint16_t _pad;
} kv_sighash_job;
int kv_sighash_batch(kv_ctx *ctx, const uint8_t *blob, size_t blob_len,
                     const kv_sighash_job *jobs, size_t n, uint8_t *hashes_out /*[32n]*/);

/* Finalize a muhash partial (num‖den, 768B LE) into the 32-byte commitment. */
int kv_muhash_finalize(kv_ctx *ctx, const uint8_t *partial768, uint8_t *hash32_out);

/* Fold another partial into an accumulator partial: acc *= other (num and den
 * multiplied mod 2^3072-1103717) — MuHash::combine (crypto/muhash/src/lib.rs:87). */
int kv_muhash_combine(kv_ctx *ctx, uint8_t *acc_partial768, const uint8_t *other_partial768);

/* Batched verifies with per-signature status bytes (0 valid / 1 invalid /
 * 2 pubkey-parse-error / 3 sig-parse-error) — the validate path uses these to
 * distinguish TxScriptError::InvalidPubkey/InvalidSignature from boolean false. */
int kv_verify_schnorr_batch_status(kv_ctx *ctx, const uint8_t *tuples, size_t n,
                                   uint64_t *bitmap_out, uint8_t *status_out);
int kv_verify_ecdsa_batch_status(kv_ctx *ctx, const uint8_t *tuples, size_t n,
                                 uint64_t *bitmap_out, uint8_t *status_out);

/* Staged mode: stage a batch into HBM once, then time repeated launches with
 * inputs resident (bench harness; kernel_ms from hipEvents on the engine stream). */
int kv_stage_tuples(kv_ctx *ctx, const uint8_t *tuples, size_t n, int ecdsa);
int kv_verify_staged(kv_ctx *ctx, size_t n, int ecdsa, double *kernel_ms);
int kv_fetch_bitmap(kv_ctx *ctx, size_t n, uint64_t *bitmap_out);

/* Schnorr batches of at least KV_SCHNORR_SPLIT_MIN signatures (environment,
 * read once in kv_create; a built-in default otherwise) run as a ladder kernel
 * plus a finish kernel that inverts K signatures per lane in one batch. Same
 * outputs as the fused kernel. Returns K as compiled. */
int kv_schnorr_finish_batch(void);

/* Introspection: copies `count` 64-byte entries of the verify ladder's joint
 * fixed-base table, from entry `first`, to out64. Entry hi<<8|lo is the affine
 * point lo·G + hi·2^128·G (entry 0 is G) as x then y, each 8 little-endian
 * 32-bit words of the canonical value. Returns -1 if first + count > 65536. */
int kv_g_comb_fetch(kv_ctx *ctx, uint32_t first, uint32_t count, uint8_t *out64);

/* ---- GPU-resident UTXO set ----
 * ⇔ UtxoCollection (consensus/core/src/utxo/utxo_collection.rs:5) + the
 * populate/diff steps (utxo_validation.rs:351-390, utxo_diff.rs:224).
 * Outpoints are 36B (tx_id‖index LE); entries are packed 64B records:
 * amount u64 ‖ daa_score u64 ‖ flags u16 ‖ spk_version u16 ‖
 * spk_len u32 ‖ spk[36] inline when spk_len ≤ 36.
 * Scripts larger than 36B (the reference allows spk up to
 * max_script_public_key_len = 10,000B, utxo_entry.rs:20 / params.rs) live in
 * a device-side ARENA: the entry carries flags bit1
 * (KV_UTXO_F_SPK_ARENA) and its spk field's first 4 bytes are the u32 arena
 * byte offset. Arena space is bump-allocated; removing an entry leaks its
 * arena span until the next kv_utxo_reset or kv_utxo_rehash (documented trade:
 * non-standard outputs are rare; the arena compacts on reset and on rehash,
 * and kv_utxo_stats reports the leaked bytes).
 *
 * Covenant ids (UtxoEntry::covenant_id): an entry that carries one has flags
 * bit2 (KV_UTXO_F_COVENANT) and the 32-byte id in bytes 28..60 of the record.
 * Its script ALWAYS travels out of line, whatever its length (an empty one
 * included): in every spk blob below (kv_utxo_upsert_spk, kv_utxo_import_chunk,
 * kv_utxo_apply_diff in; kv_utxo_export_chunk, kv_utxo_lookup_spk out) it sits
 * in entry order among the scripts longer than 36 bytes. On input bytes 24..28
 * of such a record are ignored. In the table the value also has
 * KV_UTXO_F_SPK_ARENA, the arena offset in bytes 24..28 and zeros in 60..64;
 * the arena span is exactly spk_len bytes. kv_utxo_upsert (inline only)
 * refuses the flag with -1. */
#define KV_UTXO_F_COINBASE 1u
#define KV_UTXO_F_SPK_ARENA 2u
#define KV_UTXO_F_COVENANT 4u
#define KV_UTXO_MAX_SPK 10000u
int kv_utxo_reset(kv_ctx *ctx, uint64_t capacity);
/* inline-only upsert: every entry's spk_len must be ≤ 36 */
int kv_utxo_upsert(kv_ctx *ctx, const uint8_t *outpoints, const uint8_t *entries64,
                   size_t n);
/* general upsert: entries with spk_len > 36, and covenant entries of any
 * length, take their script bytes from spk_blob, concatenated in entry order
 * (total = sum of those spk_lens);
 * the engine stores them in the arena and rewrites the entry in the table
 * with KV_UTXO_F_SPK_ARENA + the arena offset. */
int kv_utxo_upsert_spk(kv_ctx *ctx, const uint8_t *outpoints,
                       const uint8_t *entries64, const uint8_t *spk_blob,
                       size_t spk_blob_len, size_t n);
int kv_utxo_remove(kv_ctx *ctx, const uint8_t *outpoints, size_t n);
int kv_utxo_lookup(kv_ctx *ctx, const uint8_t *outpoints, size_t n,
                   uint8_t *entries_out /*[64n] or NULL*/, uint64_t *found_bitmap,
                   double *kernel_ms /*optional*/);
/* lookup that also returns out-of-line scripts: arena entries' bytes are
 * gathered (device-side) into spk_out in entry order and each such returned
 * entry's spk field is rewritten to the u32 offset INTO spk_out. *spk_used
 * receives the total bytes (call with spk_cap 0 to size). Returns -3 when
 * spk_cap is too small (entries_out/bitmap still valid, *spk_used = needed). */
int kv_utxo_lookup_spk(kv_ctx *ctx, const uint8_t *outpoints, size_t n,
                       uint8_t *entries_out, uint64_t *found_bitmap,
                       uint8_t *spk_out, size_t spk_cap, size_t *spk_used);

/* ---- UTXO-set MuHash commitment ----
 * An entry's element is MuHash::from_utxo over write_utxo
 * (consensus/core/src/muhash.rs:55-69): tx_id ‖ index u32 ‖ daa_score u64 ‖
 * amount u64 ‖ is_coinbase u8 ‖ spk_version u16 ‖ spk_len u64 ‖ spk. Arena
 * scripts are hashed in place. An entry with KV_UTXO_F_COVENANT appends its
 * 32-byte covenant id after the script (muhash.rs:66-67). */

/* ⇔ MuHash over every live entry of the GPU-resident set
 *   (import_pruning_point_utxo_set's multiset, consensus/src/pipeline/
 *   virtual_processor/processor.rs:1525-1538; verify_expected_utxo_state,
 *   utxo_validation.rs:188-195).
 * partial768_out: numerator = product of every READY slot's element mod
 * 2^3072-1103717 (not necessarily canonical), denominator = 1. An empty or
 * never-reset table gives the identity partial and n_live = 0. Read-only on
 * the table; takes the context lock and is stream-ordered after earlier
 * upserts and removes. kernel_ms is hipEvent time over the whole chain.
 *  - Bounded scratch: the table is scanned in windows of
 *    kv_utxo_commitment_window() slots. Device scratch is 4 B + 384 B per
 *    window slot (index list, elements), 4096 × 384 B of running accumulators
 *    and under 1 MB for the final reduce — a function of the compiled window,
 *    never of table capacity.
 *  - No per-window host round trip: every window's compact → hash → fold
 *    kernels read the window's live count from device memory; the whole chain
 *    enqueues on the stream, is synchronised once at the end, and one 400 B
 *    record (384 B value, count, status) is copied back.
 *  - Only live slots cost hashing: READY slots are compacted first (wave
 *    ballot + one atomic per wave), so EMPTY and TOMB slots never reach
 *    BLAKE2b/ChaCha or the multiply chain.
 * Returns -3 if a READY entry's script reference lies outside the arena. */
int kv_utxo_commitment(kv_ctx *ctx, uint8_t partial768_out[768],
                       uint64_t *n_live_out /*optional*/, double *kernel_ms /*optional*/);
int kv_utxo_commitment_window(void); /* slots per scan window, as compiled */

/* ⇔ Consensus::append_imported_pruning_point_utxos
 *   (consensus/src/consensus/mod.rs:1139-1152): store the chunk AND fold
 *   MuHash::from_utxo of each of its entries into a running multiset.
 * Inputs and table effect are exactly those of kv_utxo_upsert_spk. In
 * addition the product of the chunk's n elements is multiplied into the
 * numerator half of acc_partial768; the denominator half is untouched. The
 * elements are computed from the chunk as staged on the device, after the
 * arena rewrite (long scripts are read from the arena), not from a table
 * scan. n == 0 is a no-op returning 0; on any error the accumulator is
 * unchanged. Start from the identity partial (num = den = 1) and compare
 * kv_muhash_finalize of the accumulator with the header's utxo_commitment.
 * Duplicates: an outpoint that occurs twice across chunks (or within one) is
 * counted twice in the multiset but stored once in the table — as in the
 * reference, where write_many overwrites while the multiset keeps both. With
 * distinct outpoints imported into a fresh table, kv_utxo_commitment equals
 * the accumulator. */
int kv_utxo_import_chunk(kv_ctx *ctx, const uint8_t *outpoints, const uint8_t *entries64,
                         const uint8_t *spk_blob, size_t spk_blob_len, size_t n,
                         uint8_t acc_partial768[768] /* in/out */);

/* ---- UTXO table maintenance: stats, rehash, export ----
 * The table's capacity is fixed at kv_utxo_reset, removes leave tombstones
 * that only an upsert probing through them reuses, and the arena only grows.
 * These three calls let a host watch that and repair it without losing the
 * set. Nothing is automatic: kv_utxo_upsert still returns -3 on a full table,
 * and the host decides when to rehash. */

typedef struct kv_utxo_table_stats {
  uint64_t slots;            /* slot count (power of two), 0 if never reset */
  uint64_t n_live, n_tomb, n_empty; /* sum == slots */
  uint64_t arena_used;       /* bump head, bytes */
  uint64_t arena_live_bytes; /* sum of spk_len over READY entries with KV_UTXO_F_SPK_ARENA */
  uint64_t arena_cap;
} kv_utxo_table_stats;

/* One pass over the slot array: slot states are counted per wave by ballot +
 * popcount, arena bytes by a wave reduction, one atomic per wave per counter;
 * one 40 B record is copied back after one stream synchronisation. Read-only,
 * takes the context lock, stream-ordered after earlier mutations. A
 * never-reset context gives all zeros and returns 0. arena_used -
 * arena_live_bytes is the arena garbage a kv_utxo_rehash would reclaim; lookup,
 * remove and upsert probe until the first EMPTY slot, so a falling n_empty is
 * the signal that probe chains are growing. */
int kv_utxo_stats(kv_ctx *ctx, kv_utxo_table_stats *out);

/* Rebuild the set into a fresh table and a fresh arena: grows a full table,
 * shrinks a sparse one, and compacts tombstones and arena garbage.
 * capacity means what it means for kv_utxo_reset (entries; slots = smallest
 * power of two >= max(64, 2*capacity)); capacity == 0 keeps the current slot
 * count, a pure compaction. If the resulting slot count is < 2*n_live the call
 * fails, except for capacity == 0, which keeps whatever load the table has.
 *  - Device chain, all on the context's stream: the kv_utxo_stats pass gives
 *    n_live and arena_live_bytes, from which the new table and arena are
 *    allocated (arena: 1 MiB doubled until it holds arena_live_bytes, the
 *    rounding of the growing arena). Then, per window of
 *    kv_utxo_commitment_window() source slots, the commitment's compaction
 *    kernel packs the READY slot indices and an insert kernel places each in
 *    the new table, reading the window's live count from device memory — no
 *    per-window host round trip. Long scripts are re-allocated back to back in
 *    the new arena by a 64-bit device cursor and moved by a block-per-script
 *    copy kernel. One record (inserted count, new arena head, status) is
 *    copied back after one synchronisation.
 *  - Atomic: the table, its capacity, the arena, its capacity and its head are
 *    swapped only after the device work has completed and reported no failure,
 *    and the old allocations are freed after the swap. On ANY error the old
 *    table and arena are still in place and unchanged.
 *  - Transient device memory is therefore old + new: both tables (112 B per
 *    slot) and both arenas are alive until the swap.
 * After a successful call n_tomb == 0, n_live is unchanged, arena_used ==
 * arena_live_bytes, every entry is retrievable with identical bytes and
 * kv_utxo_commitment is unchanged mod P.
 * kernel_ms is hipEvent time over the stats pass plus the rebuild chain.
 * Returns -1 never reset, -2 allocation failure, -3 capacity too small for the
 * live set, a READY entry whose script reference is out of range, or a
 * compacted arena beyond what a u32 offset addresses. */
int kv_utxo_rehash(kv_ctx *ctx, uint64_t capacity, double *kernel_ms /*optional*/);

/* ⇔ get_pruning_point_utxos / get_virtual_utxos (consensus/src/consensus/
 *   mod.rs:1067-1108, seek_iterator(from_outpoint, chunk_size, skip_first)):
 *   the serving half of pruning-point sync, of which kv_utxo_import_chunk is
 *   the receiving half. A slot cursor stands in for from_outpoint +
 *   skip_first.
 * Walk: start with *cursor = 0 and call until *cursor == stats.slots with
 * *n_out == 0. Entries come out in ascending slot order and *cursor is
 * advanced to one past the last slot consumed; a full walk with no mutation in
 * between yields every live entry exactly once. The reference iterates in DB
 * key order; order carries no consensus meaning here, because the receiver
 * folds a commutative multiset (kv_utxo_import_chunk).
 * Output is exactly the input format of kv_utxo_upsert_spk /
 * kv_utxo_import_chunk, so a chunk can be fed straight back: inline entries
 * are copied as stored; an arena entry has KV_UTXO_F_SPK_ARENA cleared and its
 * 36-byte spk field zeroed (a covenant entry: bytes 24..28 zeroed,
 * KV_UTXO_F_COVENANT and the id in 28..60 kept), and its script bytes are
 * appended to spk_out in entry order (*spk_used = total).
 * spk_cap must be >= KV_UTXO_MAX_SPK (else -1), so one entry always fits. A
 * chunk ends early, with the cursor before the next entry, when that entry's
 * script would not fit; it may also come back short of max_entries — empty
 * even — at the end of the span of slots one call scans (sized from
 * max_entries, at most one commitment window and never across a window
 * boundary). Callers loop until the end condition.
 * Read-only on the table, under the context lock. Returns -3 if an entry's
 * script reference lies outside the arena. */
int kv_utxo_export_chunk(kv_ctx *ctx, uint64_t *cursor /* in/out, slot index; start at 0 */,
                         size_t max_entries,
                         uint8_t *outpoints_out /*[36*max]*/, uint8_t *entries_out /*[64*max]*/,
                         uint8_t *spk_out, size_t spk_cap, size_t *spk_used,
                         size_t *n_out);

/* ---- queries by script public key: balances, supply, entries ----
 * ⇔ the utxoindex (indexes/utxoindex/src/core/api/mod.rs:23-30), which in the
 *   reference is a second database keyed version u16 ‖ len u64 ‖ script ‖
 *   outpoint (indexes/utxoindex/src/stores/indexed_utxos.rs:156-198),
 *   re-derived from every virtual diff and rebuilt by resync. Here both calls
 *   are a filtered scan of the one GPU-resident table: there is no secondary
 *   index to keep in step with reorgs.
 * A query is one script public key: kv_spk_query gives its version and length
 * (`zero` must be 0), and the scripts of all queries lie concatenated in query
 * order in spk_blob. At most KV_UTXO_QUERY_MAX queries per call.
 * What matches: a READY entry matches query i when its spk_version, its
 * spk_len and its spk_len script bytes all equal the query's. Inline scripts
 * are read from the slot, scripts of KV_UTXO_F_SPK_ARENA values (every
 * covenant entry among them, however short its script) in place from the
 * arena. The covenant id plays no part in matching.
 * Both calls are read-only on the table, take the context lock and run on the
 * context's stream, ordered after earlier mutations. The queries are hashed on
 * the host into an open-addressing table of at least 2·n_q slots (64-bit hash
 * over version, length and the script bytes; the full compare decides), which
 * is uploaded with the blob: device scratch is bounded by KV_UTXO_QUERY_MAX
 * (and the scripts handed in) and by the compiled scan window, never by table
 * capacity.
 * Both return -1, with nothing written to any output, for n_q >
 * KV_UTXO_QUERY_MAX, a spk_len > KV_UTXO_MAX_SPK, a non-zero `zero` field,
 * spk_blob_len != the sum of the lengths, or two identical queries (the
 * reference takes a HashSet); and -3 when a READY entry the scan met has a
 * script reference outside the arena (the reference is not followed). */
#define KV_UTXO_QUERY_MAX 65536u
typedef struct kv_spk_query {
  uint32_t spk_len;
  uint16_t spk_version;
  uint16_t zero;
} kv_spk_query;

/* ⇔ get_balance_by_script_public_keys + get_circulating_supply
 *   (indexes/utxoindex/src/core/api/mod.rs:23-30).
 * balances_out[i] / counts_out[i]: sum of amount / number of the entries that
 * match query i. total_amount_out / n_live_out: the same over ALL READY
 * entries (the circulating supply as this table holds it, and kv_utxo_stats'
 * n_live). Arithmetic is mod 2^64. n_q == 0 is legal (q, spk_blob and
 * balances_out may be NULL) and gives the supply alone. A never-reset context
 * gives zeros.
 * One grid-stride pass over the slot array; per-query sums by 64-bit atomics,
 * the supply by a wave reduction and one atomic per wave per counter. One
 * stream synchronisation, one copy back of 16·n_q + 32 bytes. kernel_ms is
 * hipEvent time over the pass (the upload of the query table is outside). */
int kv_utxo_balance_by_spk(kv_ctx *ctx, const kv_spk_query *q, size_t n_q,
                           const uint8_t *spk_blob, size_t spk_blob_len,
                           uint64_t *balances_out /*[n_q]*/,
                           uint64_t *counts_out /*[n_q], optional*/,
                           uint64_t *total_amount_out /*optional*/,
                           uint64_t *n_live_out /*optional*/,
                           double *kernel_ms /*optional*/);

/* ⇔ get_utxos_by_script_public_keys, paginated (the reference's own TODO at
 *   indexes/utxoindex/src/stores/indexed_utxos.rs:158-159).
 * 96-byte match record (⇔ CompactUtxoEntry, indexes/core/src/
 * indexed_utxos.rs:24-29, with its outpoint and script):
 *    0..36 outpoint | 36..40 query index u32 | 40..48 amount | 48..56 daa_score |
 *   56..58 flags (KV_UTXO_F_COINBASE, KV_UTXO_F_COVENANT; arena bit cleared) |
 *   58..64 zero | 64..96 covenant id, zeros without the flag
 * Walk, in the shape of kv_utxo_export_chunk: start with *cursor = 0 and call
 * until *cursor == stats.slots with *n_out == 0. Records come out in ascending
 * slot order; a call may return fewer than max_entries, or none, and one that
 * returns none has advanced the cursor unless it was at the end already. A
 * full walk with no mutation in between yields every matching entry exactly
 * once. max_entries above one scan window (kv_utxo_commitment_window()) is
 * clamped to the window; max_entries == 0 is refused with -1. A never-reset
 * context gives *n_out = 0 and leaves the cursor alone.
 * One call enqueues every remaining window from *cursor (which may lie inside
 * a window) in one go, with no host round trip per window: a window that
 * starts when max_entries matches are already stored does nothing, so the
 * windows that ran are a prefix of the walk. After the one stream
 * synchronisation of the chain (a 32 B record comes back with it), the slot
 * indices and records that were stored — fewer than max_entries + one window
 * — are copied back, sorted by slot, and the first max_entries are returned;
 * the cursor goes one past the last slot returned, or to the start of the
 * first window that did nothing, or to the end. Device scratch: 104 B per
 * stored match, (max_entries + one window) of them at most. */
int kv_utxo_find_by_spk(kv_ctx *ctx, uint64_t *cursor /* in/out, slot index; start at 0 */,
                        const kv_spk_query *q, size_t n_q, const uint8_t *spk_blob,
                        size_t spk_blob_len, size_t max_entries,
                        uint8_t *matches_out /*[96*max_entries]*/, size_t *n_out);

/* ---- undo journal: a reorg reverts diffs on the device ----
 * ⇔ calculate_utxo_state_relatively (consensus/src/pipeline/virtual_processor/
 *   processor.rs:393-437): down the old chain each block's stored diff is
 *   applied reversed (with_diff_in_place(&mergeset_diff.as_reversed()), :410;
 *   UtxoDiff::as_reversed, consensus/core/src/utxo/utxo_diff.rs:71), up the
 *   new chain diffs are committed with write_diff_batch
 *   (consensus/src/model/stores/utxo_set.rs:107-112).
 * The reference keeps every chain block's diff in a store; here each journaled
 * apply pushes one undo record onto a per-context journal in device memory.
 * A record holds the diff's outpoints, the 64-byte value each one had (and
 * whether it had one) before the diff, and its own copy of the long scripts
 * among them: about 100 B per outpoint plus those scripts. It holds no slot
 * index and no offset into the live arena, so kv_utxo_rehash leaves the
 * journal valid. kv_utxo_reset clears the journal, kv_destroy frees it.
 * Tokens are per context, start at 1 and only grow (also across resets). */
typedef struct kv_utxo_diff_result {
  uint64_t n_removed_missing; /* removed outpoints that were not in the set */
  uint64_t n_added_overwrote; /* added outpoints that were already in the set */
  uint64_t journal_bytes;     /* device bytes of the record this call pushed */
  double kernel_ms;           /* capture + script copy + upsert kernels */
} kv_utxo_diff_result;

/* ⇔ write_diff_batch (utxo_set.rs:107-112: delete the removed keys, write the
 *   added ones), with the inverse kept.
 * removed_ops has the input format of kv_utxo_remove (n_removed × 36 B); the
 * added side that of kv_utxo_upsert_spk. The table effect is exactly "remove,
 * then upsert_spk". One record is pushed even when both sides are empty, so
 * one block is always one token (*undo_token_out, required).
 * The reference unwrap()s on a removed key that is missing and on an added key
 * that exists; the engine applies and journals both faithfully and counts them
 * in res_out, so a host can treat a non-zero count as a consistency alarm.
 * Outpoints must be distinct across removed ∪ added: otherwise -1, nothing
 * changed. Device chain on the context's stream: one launch probes every
 * outpoint once, copies what it finds into the record and tombstones the
 * removed side; one synchronisation brings back a 32 B record (counts, script
 * bytes); a block-per-script copy fills the record's script blob; then the
 * upsert of kv_utxo_upsert_spk runs.
 * Failure atomicity: if the call fails after it began to mutate (-3: table
 * full, or a stored script reference out of range), the engine reverts what
 * it did from the record it just captured, drops that record and returns the
 * error with the set unchanged (arena bytes spent on the attempt stay spent
 * until the next kv_utxo_rehash). Should that internal revert itself fail (-2,
 * out of device memory), the record stays the newest one. */
int kv_utxo_apply_diff(kv_ctx *ctx, const uint8_t *removed_ops, size_t n_removed,
                       const uint8_t *added_ops, const uint8_t *added_entries64,
                       const uint8_t *spk_blob, size_t spk_blob_len, size_t n_added,
                       kv_utxo_diff_result *res_out /*optional*/,
                       uint64_t *undo_token_out);

/* ⇔ with_diff_in_place(as_reversed) of one chain block (processor.rs:410).
 * Applies the exact inverse of the record `token` names and pops it: added
 * outpoints that were absent before are removed; added outpoints that
 * overwrote an entry get the old entry back; removed outpoints that were
 * present are re-inserted with their original 64 bytes (and script, for arena
 * entries: the record's scripts are appended to the arena); removed outpoints
 * that were missing are left alone.
 * Strictly last-in-first-out: a token that is not the newest unreverted
 * record returns -1 and changes nothing.
 * Contract: the revert is exact if the set is in the state the matching apply
 * left it in. Non-journaled mutations in between (kv_utxo_upsert[_spk],
 * kv_utxo_remove, kv_utxo_import_chunk, kv_validate_block_utxo with
 * apply_diff) are the caller's business; kv_utxo_rehash is not a mutation.
 * Returns -3, with the record kept, if the table is too full to take the
 * entries back. */
int kv_utxo_revert(kv_ctx *ctx, uint64_t token);

/* Frees every record with token <= upto_token: blocks past finality depth,
 * which no reorg can reach. Returns 0 also when there is none. */
int kv_utxo_journal_drop(kv_ctx *ctx, uint64_t upto_token);

typedef struct kv_utxo_journal_info {
  uint64_t n_records;
  uint64_t oldest_token; /* 0 when the journal is empty */
  uint64_t newest_token; /* 0 when the journal is empty */
  uint64_t device_bytes; /* device memory the records hold */
  double last_revert_kernel_ms; /* of the last kv_utxo_revert: the blob append
                                   and its two launches */
} kv_utxo_journal_info;
int kv_utxo_journal_stats(kv_ctx *ctx, kv_utxo_journal_info *out);

/* ---- per-script changes of one journaled diff ----
 * ⇔ the UtxoChanges behind UtxosChanged notifications:
 *   UtxoIndexChanges::update_utxo_diff (indexes/utxoindex/src/
 *   update_container.rs:29-51), UtxosChangedNotification::
 *   apply_utxos_changed_subscription / filter_utxo_set (indexes/core/src/
 *   notification.rs:81-127) and supply_change -> update_circulating_supply
 *   (indexes/utxoindex/src/index.rs:98).
 * The removed side of a journaled diff (amount, daa score, script and covenant
 * id of every spent entry) exists only in the device record, and a block that
 * went through kv_validate_block_utxo_undo never showed its diff to the host:
 * this call reads the record `token` names and the live table, and reports the
 * entries that left and entered the set, filtered by script public key.
 *
 * Change index. A record with n_removed and n_added rows has
 * cursor_end = n_removed + 2·n_added change indices:
 *   c <  n_removed           removed row c; value and script from the record;
 *                            reported when the row was found at apply time
 *   c == n_removed + 2k      added row k; the value the add overwrote, from
 *                            the record; reported when there was one
 *   c == n_removed + 2k + 1  added row k; the value the table holds NOW, script
 *                            inline or from the live arena; reported when the
 *                            outpoint is still in the table, else counted in
 *                            n_added_gone
 * The first two kinds are entries that left the set and carry
 * KV_UTXO_CHANGE_F_REMOVED; the third kind entered it. With
 * KV_UTXO_CHANGES_REVERSED the labels swap and nothing else does (⇔
 * as_reversed: what a host needs before kv_utxo_revert of that token);
 * added_amount / removed_amount and n_added / n_removed swap with them.
 * Any token still in the journal is legal, not only the newest: the added side
 * of an older record reflects the table as it is now.
 *
 * 96-byte change record, the match record of kv_utxo_find_by_spk with the zero
 * bytes put to use:
 *    0..36 outpoint | 36..40 query index u32 (0xffffffff with
 *   KV_UTXO_CHANGES_ALL) | 40..48 amount | 48..56 daa_score |
 *   56..58 flags (KV_UTXO_F_COINBASE, KV_UTXO_F_COVENANT,
 *   KV_UTXO_CHANGE_F_REMOVED; arena bit cleared) | 58..60 spk_version |
 *   60..64 spk_len | 64..96 covenant id, zeros without the flag
 * Queries are those of kv_utxo_find_by_spk, matched the same way. n_q == 0
 * without KV_UTXO_CHANGES_ALL is legal: the totals and no record.
 *
 * Walk: start with *cursor = 0 and call until *cursor == res_out->cursor_end.
 * Records come out in ascending change index; the cursor goes one past the
 * last index returned, or to cursor_end when nothing is left. A walk with no
 * mutation in between yields each change exactly once; with spk_out == NULL it
 * takes at most matches / max_entries + 1 calls. The totals in res_out are
 * over the WHOLE record, whatever the filter and the cursor.
 * Scripts: with spk_out non-NULL the script of every returned record, of any
 * length, is appended to it in record order (*spk_used = total). spk_cap must
 * be >= KV_UTXO_MAX_SPK, so one entry always fits; a chunk ends early, with
 * the cursor before the next record, when that record's script would not fit
 * (the rule of kv_utxo_export_chunk). With spk_out == NULL, spk_cap and
 * spk_used are ignored.
 *
 * One launch with a lane per change index, one synchronisation with a 48 B
 * record back (counts, totals, status); then the stored indices are copied
 * back and sorted, the prefix that fits is cut and its records are copied
 * back; long scripts are gathered once per source (record blob, live arena).
 * Device scratch: 152 B × (cursor_end - *cursor) plus the query table; never a
 * function of table capacity. Read-only on table and journal, under the
 * context lock, on the context's stream; kv_utxo_rehash between the apply and
 * this call changes nothing in the answer.
 * Returns -1, with nothing written to any output and the cursor left alone,
 * for a null cursor, n_out, res_out or changes_out, max_entries == 0, unknown
 * flag bits, KV_UTXO_CHANGES_ALL with n_q != 0, a token that is not in the
 * journal (never issued, reverted, dropped, or cleared by kv_utxo_reset),
 * *cursor > cursor_end, spk_out with spk_cap < KV_UTXO_MAX_SPK, and every
 * refusal of the queries listed at kv_utxo_find_by_spk; -3 when a value the
 * kernel met has a script reference out of range (it is not followed). */
#define KV_UTXO_CHANGES_REVERSED 1u   /* report the record as its REVERT would change the set */
#define KV_UTXO_CHANGES_ALL      2u   /* no filter (⇔ subscription.to_all()); n_q must be 0 */
#define KV_UTXO_CHANGE_F_REMOVED 0x8000u /* in a change record's flags: the entry left the set */

typedef struct kv_utxo_changes_result {
  uint64_t cursor_end;      /* n_removed + 2*n_added of the record: the walk ends here */
  uint64_t added_amount;    /* sum of amount over ALL entries the record adds, mod 2^64 */
  uint64_t removed_amount;  /* same for removed; supply_change = added - removed */
  uint64_t n_added, n_removed;   /* the entries counted in those sums */
  uint64_t n_added_gone;    /* added-side outpoints that are no longer READY in the table */
  double kernel_ms;         /* hipEvents over the launch(es) of this call */
} kv_utxo_changes_result;

int kv_utxo_changes_by_spk(kv_ctx *ctx, uint64_t token, uint32_t flags,
                           uint64_t *cursor /* in/out, change index; start at 0 */,
                           const kv_spk_query *q, size_t n_q,
                           const uint8_t *spk_blob, size_t spk_blob_len,
                           size_t max_entries, uint8_t *changes_out /*[96*max_entries]*/,
                           uint8_t *spk_out /*optional*/, size_t spk_cap, size_t *spk_used,
                           size_t *n_out, kv_utxo_changes_result *res_out /*required*/);

/* Populate + validate + (optionally) apply the UTXO diff — the full virtual
 * processor step for one block (utxo_validation.rs:351-390 populate, then
 * validation, then utxo_diff.rs:224 add_transaction per accepted tx).
 * Blob format as kv_validate_block, but each input's UtxoEntry fields are
 * IGNORED (builders write zeros with utxo_spk_len = 0); entries resolve from
 * the GPU-resident table. A missing outpoint pre-fails that tx with
 * KV_ERR_MISSING_OUTPOINT (it is skipped by validation and muhash). When
 * apply_diff != 0, accepted txs' spent outpoints are removed and their created
 * outputs upserted with block_daa_score (coinbase txs never enter this path). */
int kv_validate_block_utxo(kv_ctx *ctx, const uint8_t *blob, size_t blob_len,
                           uint64_t pov_daa_score, uint64_t block_daa_score,
                           uint32_t flags, int apply_diff, int32_t *tx_codes_out,
                           uint64_t *fees_out, uint8_t *muhash_partial_out);

/* kv_validate_block_utxo with apply_diff = 1 whose diff can be reverted ⇔ the
 * same virtual processor step, with the block's diff kept as the reference
 * keeps it for calculate_utxo_state_relatively (processor.rs:393-437).
 * Codes, fees and the muhash partial are those of apply_diff = 1; the accepted
 * txs' diff goes through kv_utxo_apply_diff's path and *undo_token_out
 * (required) names its record for kv_utxo_revert. A block of which no tx is
 * accepted still pushes an (empty) record. If two accepted txs spend one
 * outpoint, or the diff fails to apply, the error of kv_utxo_apply_diff is
 * returned with the set unchanged and no record pushed (the outputs are
 * already filled in): run kv_block_body_check first. */
int kv_validate_block_utxo_undo(kv_ctx *ctx, const uint8_t *blob, size_t blob_len,
                                uint64_t pov_daa_score, uint64_t block_daa_score,
                                uint32_t flags, int32_t *tx_codes_out,
                                uint64_t *fees_out, uint8_t *muhash_partial_out,
                                uint64_t *undo_token_out);

/* Mempool batch validation ⇔ validate_mempool_transaction_in_utxo_context
 * (utxo_validation.rs:418-457) fanned over independent txs: SkipMassCheck +
 * per-tx COMPUTED contextual storage mass + optional feerate threshold
 * (<= 0 disables; fee / normalized_max(mass) <= threshold →
 * KV_ERR_FEERATE_TOO_LOW). from_utxo_table = 1 resolves entries from the
 * GPU-resident table (missing outpoint → KV_ERR_MISSING_OUTPOINT), 0 takes
 * them inline from the blob. */
int kv_validate_mempool(kv_ctx *ctx, const uint8_t *blob, size_t blob_len,
                        uint64_t pov_daa_score, double feerate_threshold,
                        int from_utxo_table, int32_t *tx_codes_out,
                        uint64_t *fees_out);

/* Block-body-in-isolation batch (body_validation_in_isolation.rs):
 * merkle_root_out ← calc_hash_merkle_root over the txs (GPU leaf hashes,
 * caller compares against the header commitment); rule_code_out ← 0 or the
 * first KV_ERR_BODY_* violation (duplicate tx / in-block double spend /
 * chained tx). Either out-pointer may be NULL. */
int kv_block_body_check(kv_ctx *ctx, const uint8_t *blob, size_t blob_len,
                        uint8_t merkle_root_out[32], int32_t *rule_code_out);

/* ---- KIP-21 sequencing-commitment accessor ----
 * ⇔ SeqCommitAccessor consulted by OpChainblockSeqCommit
 * (crypto/txscript/src/opcodes/mod.rs:1389-1405; threaded through
 * tx_validation_in_utxo_context.rs:44,170). The host (Rust over FFI) supplies
 * a callback so DAG reachability stays on the node side. Contract:
 *   return 0  → block is a chain ancestor within depth; write the 32-byte
 *               commitment to commitment_out32
 *   return nonzero → not an ancestor / pruned / too deep (the script fails
 *               with the InvalidSource class, matching the reference's
 *               BlockNotSelected/BlockAlreadyPruned/BlockIsTooDeep rejects)
 * A NULL accessor (the default) disables the opcode: executing it fails with
 * InvalidOpcode, matching a None accessor in the reference.
 * The callback may be invoked concurrently from engine worker threads. */
typedef int (*kv_seq_commit_accessor_fn)(void *user, const uint8_t block_hash32[32],
                                         uint8_t commitment_out32[32]);
int kv_set_seq_commit_accessor(kv_ctx *ctx, kv_seq_commit_accessor_fn fn, void *user);

/* Per-kernel GPU timings (hipEvents on the engine stream) and job counts of
 * the LAST kv_validate_block/kv_validate_block_utxo call on this context —
 * the bench harness derives the block-path kernel roofline from these.
 * A kernel that did not launch reports 0. */
typedef struct {
  double subhash_ms;   /* kv_tx_subhash_kernel */
  double s_assemble_ms; /* sighash+tuple assembly, schnorr jobs */
  double e_assemble_ms; /* sighash+tuple assembly, ecdsa jobs */
  double schnorr_ms;   /* kv_schnorr_verify_kernel */
  double ecdsa_ms;     /* kv_ecdsa_verify_kernel */
  double muhash_ms;    /* element + reduce kernels */
  uint64_t n_schnorr;  /* schnorr verify lane-jobs (cache misses only) */
  uint64_t n_ecdsa;    /* ecdsa verify lane-jobs */
} kv_validate_timings;
int kv_get_validate_timings(kv_ctx *ctx, kv_validate_timings *out);

/* Sig-cache statistics (crypto/txscript/src/caches.rs:57-82 counters). */
typedef struct {
  uint64_t insertions;
  uint64_t hits;
  uint64_t misses;
} kv_cache_stats;
int kv_sig_cache_stats(kv_ctx *ctx, kv_cache_stats *out);

#ifdef __cplusplus
}
#endif

#endif /* KASPA_ENGINE_ABI_H */
