"""ctypes host wrapper over the MI355X-native engine C-ABI (libkaspa_gpu.so).

This is plumbing over include/kaspa_engine_abi.h — the same surface a Rust host
would bind over FFI. The engine has NO CPU fallback:
constructing an Engine raises if the shared library is missing or no HIP
device is present.
"""
from __future__ import annotations

import ctypes
import os

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB_PATH = os.path.join(_REPO, "rusty_kaspa_amd", "libkaspa_gpu.so")

# UTXO entry flags (bytes 16..18 of a 64-byte record) and the covenant-binding
# result codes, as in include/kaspa_engine_abi.h
KV_UTXO_F_COINBASE = 1
KV_UTXO_F_SPK_ARENA = 2
KV_UTXO_F_COVENANT = 4
KV_ERR_COVENANT_AUTH_INPUT = 13
KV_ERR_COVENANT_GENESIS_ID = 14
KV_UTXO_QUERY_MAX = 65536
KV_UTXO_MATCH_BYTES = 96  # one record of utxo_find_by_spk
KV_UTXO_MAX_SPK = 10000
KV_UTXO_CHANGES_REVERSED = 1  # flags of utxo_changes_by_spk
KV_UTXO_CHANGES_ALL = 2
KV_UTXO_CHANGE_F_REMOVED = 0x8000  # in a change record's flags
KV_UTXO_CHANGE_BYTES = 96  # one record of utxo_changes_by_spk


class KvParams(ctypes.Structure):
    _fields_ = [("coinbase_maturity", ctypes.c_uint64),
                ("mass_per_sig_op", ctypes.c_uint64),
                ("sig_cache_size", ctypes.c_uint64),
                ("device", ctypes.c_int)]


class KvCacheStats(ctypes.Structure):
    _fields_ = [("insertions", ctypes.c_uint64), ("hits", ctypes.c_uint64),
                ("misses", ctypes.c_uint64)]


class KvUtxoTableStats(ctypes.Structure):
    _fields_ = [("slots", ctypes.c_uint64), ("n_live", ctypes.c_uint64),
                ("n_tomb", ctypes.c_uint64), ("n_empty", ctypes.c_uint64),
                ("arena_used", ctypes.c_uint64),
                ("arena_live_bytes", ctypes.c_uint64),
                ("arena_cap", ctypes.c_uint64)]


class KvUtxoDiffResult(ctypes.Structure):
    _fields_ = [("n_removed_missing", ctypes.c_uint64),
                ("n_added_overwrote", ctypes.c_uint64),
                ("journal_bytes", ctypes.c_uint64),
                ("kernel_ms", ctypes.c_double)]


class KvUtxoJournalInfo(ctypes.Structure):
    _fields_ = [("n_records", ctypes.c_uint64),
                ("oldest_token", ctypes.c_uint64),
                ("newest_token", ctypes.c_uint64),
                ("device_bytes", ctypes.c_uint64),
                ("last_revert_kernel_ms", ctypes.c_double)]


class KvUtxoChangesResult(ctypes.Structure):
    _fields_ = [("cursor_end", ctypes.c_uint64),
                ("added_amount", ctypes.c_uint64),
                ("removed_amount", ctypes.c_uint64),
                ("n_added", ctypes.c_uint64),
                ("n_removed", ctypes.c_uint64),
                ("n_added_gone", ctypes.c_uint64),
                ("kernel_ms", ctypes.c_double)]


class KvSpkQuery(ctypes.Structure):
    _fields_ = [("spk_len", ctypes.c_uint32), ("spk_version", ctypes.c_uint16),
                ("zero", ctypes.c_uint16)]


def pack_spk_queries(queries):
    """[(version, script_bytes)] -> (kv_spk_query array, blob, n) as
    kv_utxo_balance_by_spk / kv_utxo_find_by_spk take them."""
    heads = (KvSpkQuery * max(len(queries), 1))()
    for i, (version, script) in enumerate(queries):
        heads[i] = KvSpkQuery(len(script), version, 0)
    return heads, b"".join(bytes(s) for _, s in queries), len(queries)


def load_library() -> ctypes.CDLL:
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(
            f"libkaspa_gpu.so not built at {_LIB_PATH} — run __graft_entry__.build()")
    lib = ctypes.CDLL(_LIB_PATH)
    lib.kv_create.restype = ctypes.c_void_p
    lib.kv_create.argtypes = [ctypes.POINTER(KvParams)]
    lib.kv_last_error.restype = ctypes.c_char_p
    return lib


class Engine:
    """One engine context == one GPU (⇔ TransactionValidator instance,
    consensus/src/processes/transaction_validator/mod.rs:15)."""

    def __init__(self, device: int = -1, coinbase_maturity: int = 1000,
                 mass_per_sig_op: int = 1000, sig_cache_size: int = 10_000):
        self.lib = load_library()
        params = KvParams(coinbase_maturity, mass_per_sig_op, sig_cache_size,
                          device)
        self.ctx = self.lib.kv_create(ctypes.byref(params))
        if not self.ctx:
            err = self.lib.kv_last_error().decode()
            raise RuntimeError(f"kv_create failed: {err}")

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.kv_destroy(ctypes.c_void_p(self.ctx))
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != 0:
            raise RuntimeError(
                f"engine call failed rc={rc}: {self.lib.kv_last_error().decode()}")

    def verify_schnorr_batch(self, tuples: bytes, n: int, with_status=False):
        words = (n + 63) // 64
        bitmap = (ctypes.c_uint64 * words)()
        status = (ctypes.c_uint8 * n)() if with_status else None
        if with_status:
            rc = self.lib.kv_verify_schnorr_batch_status(
                ctypes.c_void_p(self.ctx), tuples, ctypes.c_size_t(n), bitmap, status)
        else:
            rc = self.lib.kv_verify_schnorr_batch(
                ctypes.c_void_p(self.ctx), tuples, ctypes.c_size_t(n), bitmap)
        self._check(rc)
        return (list(bitmap), bytes(status) if with_status else None)

    def verify_ecdsa_batch(self, tuples: bytes, n: int, with_status=False):
        words = (n + 63) // 64
        bitmap = (ctypes.c_uint64 * words)()
        status = (ctypes.c_uint8 * n)() if with_status else None
        if with_status:
            rc = self.lib.kv_verify_ecdsa_batch_status(
                ctypes.c_void_p(self.ctx), tuples, ctypes.c_size_t(n), bitmap, status)
        else:
            rc = self.lib.kv_verify_ecdsa_batch(
                ctypes.c_void_p(self.ctx), tuples, ctypes.c_size_t(n), bitmap)
        self._check(rc)
        return (list(bitmap), bytes(status) if with_status else None)

    def g_comb_fetch(self, first: int, count: int) -> bytes:
        """`count` 64-byte entries of the joint fixed-base table from `first`."""
        out = (ctypes.c_uint8 * (64 * count))()
        rc = self.lib.kv_g_comb_fetch(ctypes.c_void_p(self.ctx),
                                      ctypes.c_uint32(first),
                                      ctypes.c_uint32(count), out)
        self._check(rc)
        return bytes(out)

    def muhash_finalize(self, partial768: bytes) -> bytes:
        out = (ctypes.c_uint8 * 32)()
        rc = self.lib.kv_muhash_finalize(ctypes.c_void_p(self.ctx), partial768, out)
        self._check(rc)
        return bytes(out)

    def muhash_combine(self, acc768: bytearray, other768: bytes) -> None:
        buf = (ctypes.c_uint8 * 768).from_buffer(acc768)
        rc = self.lib.kv_muhash_combine(ctypes.c_void_p(self.ctx), buf, other768)
        self._check(rc)

    def u3072_reduce_hook(self, elements: bytes, n: int, stride: int,
                          acc: bytes | None = None):
        """Test hook (kv_test_u3072_reduce): one launch of the wave U3072
        reduce over `n` 384-byte LE elements. Without `acc`, wave w returns
        elements[w]·elements[w+stride]·… (one for an idle wave); with `acc`
        (stride × 384 bytes) each wave multiplies its chain into its own
        accumulator. Returns (stride × 384 result bytes, counted elements)."""
        assert len(elements) == 384 * n
        assert acc is None or len(acc) == 384 * stride
        out = (ctypes.c_uint8 * (384 * stride))()
        n_live = ctypes.c_uint64()
        rc = self.lib.kv_test_u3072_reduce(
            ctypes.c_void_p(self.ctx), elements if n else None,
            ctypes.c_uint32(n), ctypes.c_uint32(stride), acc, out,
            ctypes.byref(n_live))
        self._check(rc)
        return bytes(out), n_live.value

    def validate_block(self, blob: bytes, n_txs: int, pov_daa: int, block_daa: int,
                       flags: int = 2, want_muhash: bool = True, raw: bool = False):
        codes = (ctypes.c_int32 * n_txs)()
        fees = (ctypes.c_uint64 * n_txs)()
        partial = (ctypes.c_uint8 * 768)() if want_muhash else None
        rc = self.lib.kv_validate_block(
            ctypes.c_void_p(self.ctx), blob, ctypes.c_size_t(len(blob)),
            ctypes.c_uint64(pov_daa), ctypes.c_uint64(block_daa),
            ctypes.c_uint32(flags), codes, fees, partial)
        self._check(rc)
        if raw:  # bench hot loop: skip the O(n) ctypes->list conversions
            return codes, fees, partial
        return list(codes), list(fees), bytes(partial) if want_muhash else None

    def validate_block_utxo(self, blob: bytes, n_txs: int, pov_daa: int,
                            block_daa: int, flags: int = 2, apply_diff: bool = True,
                            want_muhash: bool = True):
        """Populate from the GPU-resident UTXO table, validate, apply diff."""
        codes = (ctypes.c_int32 * n_txs)()
        fees = (ctypes.c_uint64 * n_txs)()
        partial = (ctypes.c_uint8 * 768)() if want_muhash else None
        rc = self.lib.kv_validate_block_utxo(
            ctypes.c_void_p(self.ctx), blob, ctypes.c_size_t(len(blob)),
            ctypes.c_uint64(pov_daa), ctypes.c_uint64(block_daa),
            ctypes.c_uint32(flags), ctypes.c_int(1 if apply_diff else 0),
            codes, fees, partial)
        self._check(rc)
        return list(codes), list(fees), bytes(partial) if want_muhash else None

    def utxo_commitment(self):
        """MuHash partial over every live entry of the GPU-resident UTXO set:
        (partial768, n_live, kernel_ms). The denominator half is one."""
        partial = (ctypes.c_uint8 * 768)()
        n_live = ctypes.c_uint64()
        ms = ctypes.c_double()
        rc = self.lib.kv_utxo_commitment(
            ctypes.c_void_p(self.ctx), partial, ctypes.byref(n_live),
            ctypes.byref(ms))
        self._check(rc)
        return bytes(partial), n_live.value, ms.value

    def utxo_commitment_window(self) -> int:
        """Slots per scan window of utxo_commitment, as compiled."""
        return self.lib.kv_utxo_commitment_window()

    def utxo_import_chunk(self, outpoints: bytes, entries64: bytes,
                          spk_blob: bytes, n: int, acc: bytearray) -> None:
        """kv_utxo_upsert_spk of the chunk, and its n elements multiplied into
        the numerator half of the 768-byte accumulator `acc` (in place)."""
        buf = (ctypes.c_uint8 * 768).from_buffer(acc)
        rc = self.lib.kv_utxo_import_chunk(
            ctypes.c_void_p(self.ctx), outpoints, entries64, spk_blob,
            ctypes.c_size_t(len(spk_blob)), ctypes.c_size_t(n), buf)
        self._check(rc)

    def utxo_stats(self) -> dict:
        """Occupancy of the GPU-resident UTXO table and its script arena
        (kv_utxo_stats): slots, n_live, n_tomb, n_empty, arena_used,
        arena_live_bytes, arena_cap. All zeros before the first reset."""
        out = KvUtxoTableStats()
        self._check(self.lib.kv_utxo_stats(ctypes.c_void_p(self.ctx),
                                           ctypes.byref(out)))
        return {name: getattr(out, name) for name, _ in out._fields_}

    def utxo_rehash(self, capacity: int = 0) -> float:
        """Rebuild the table and arena in place (kv_utxo_rehash): grow or
        shrink to `capacity` entries, or compact tombstones and arena garbage
        at the current size with capacity=0. Returns kernel_ms. Raises, with
        the old table untouched, if the call fails."""
        ms = ctypes.c_double()
        rc = self.lib.kv_utxo_rehash(ctypes.c_void_p(self.ctx),
                                     ctypes.c_uint64(capacity), ctypes.byref(ms))
        self._check(rc)
        return ms.value

    def utxo_export_chunk(self, cursor: int, max_entries: int,
                          spk_cap: int = 1 << 20):
        """One step of the export walk (kv_utxo_export_chunk), from slot
        `cursor`: (cursor, outpoints, entries, spk_blob, n), in the input
        format of utxo_import_chunk. The walk is over when the returned cursor
        equals utxo_stats()["slots"] and n == 0."""
        cur = ctypes.c_uint64(cursor)
        ops = (ctypes.c_uint8 * (36 * max(max_entries, 1)))()
        ents = (ctypes.c_uint8 * (64 * max(max_entries, 1)))()
        spk = (ctypes.c_uint8 * max(spk_cap, 1))()
        used, n = ctypes.c_size_t(), ctypes.c_size_t()
        rc = self.lib.kv_utxo_export_chunk(
            ctypes.c_void_p(self.ctx), ctypes.byref(cur),
            ctypes.c_size_t(max_entries), ops, ents, spk,
            ctypes.c_size_t(spk_cap), ctypes.byref(used), ctypes.byref(n))
        self._check(rc)
        return (cur.value, ctypes.string_at(ops, 36 * n.value),
                ctypes.string_at(ents, 64 * n.value),
                ctypes.string_at(spk, used.value), n.value)

    def utxo_balance_by_spk(self, queries):
        """Balances by script public key and the circulating supply, from one
        scan of the GPU-resident set (kv_utxo_balance_by_spk). `queries` is a
        list of distinct (version, script_bytes); returns (balances, counts,
        total, n_live, kernel_ms): per query the sum of amounts and the number
        of matching entries, then the same over every live entry, all mod
        2^64. An empty list gives the supply alone."""
        heads, blob, n = pack_spk_queries(queries)
        bal = (ctypes.c_uint64 * max(n, 1))()
        cnt = (ctypes.c_uint64 * max(n, 1))()
        total, n_live = ctypes.c_uint64(), ctypes.c_uint64()
        ms = ctypes.c_double()
        rc = self.lib.kv_utxo_balance_by_spk(
            ctypes.c_void_p(self.ctx), heads, ctypes.c_size_t(n), blob,
            ctypes.c_size_t(len(blob)), bal, cnt, ctypes.byref(total),
            ctypes.byref(n_live), ctypes.byref(ms))
        self._check(rc)
        return list(bal[:n]), list(cnt[:n]), total.value, n_live.value, ms.value

    def utxo_find_by_spk(self, cursor: int, queries, max_entries: int):
        """One step of the walk over the entries whose script public key is
        one of `queries` (kv_utxo_find_by_spk), from slot `cursor`: (cursor,
        records, n), records being n 96-byte match records (outpoint 36 ‖
        query index u32 ‖ amount u64 ‖ daa_score u64 ‖ flags u16 ‖ 6 zero
        bytes ‖ covenant id 32) in slot order. The walk is over when the
        returned cursor equals utxo_stats()["slots"] and n == 0."""
        heads, blob, n = pack_spk_queries(queries)
        cur = ctypes.c_uint64(cursor)
        out = (ctypes.c_uint8 * (KV_UTXO_MATCH_BYTES * max(max_entries, 1)))()
        n_out = ctypes.c_size_t()
        rc = self.lib.kv_utxo_find_by_spk(
            ctypes.c_void_p(self.ctx), ctypes.byref(cur), heads,
            ctypes.c_size_t(n), blob, ctypes.c_size_t(len(blob)),
            ctypes.c_size_t(max_entries), out, ctypes.byref(n_out))
        self._check(rc)
        return (cur.value,
                ctypes.string_at(out, KV_UTXO_MATCH_BYTES * n_out.value),
                n_out.value)

    def utxo_apply_diff(self, removed_ops: bytes, added_ops: bytes = b"",
                        added_entries64: bytes = b"", spk_blob: bytes = b""):
        """Remove, then upsert_spk, with the inverse pushed onto the device
        undo journal (kv_utxo_apply_diff): (token, result), result a dict of
        n_removed_missing, n_added_overwrote, journal_bytes, kernel_ms.
        Raises, with the set unchanged, if the call fails."""
        assert len(removed_ops) % 36 == 0 and len(added_ops) % 36 == 0
        assert len(added_entries64) == len(added_ops) // 36 * 64
        res = KvUtxoDiffResult()
        token = ctypes.c_uint64()
        rc = self.lib.kv_utxo_apply_diff(
            ctypes.c_void_p(self.ctx), removed_ops,
            ctypes.c_size_t(len(removed_ops) // 36), added_ops, added_entries64,
            spk_blob, ctypes.c_size_t(len(spk_blob)),
            ctypes.c_size_t(len(added_ops) // 36), ctypes.byref(res),
            ctypes.byref(token))
        self._check(rc)
        return token.value, {name: getattr(res, name) for name, _ in res._fields_}

    def utxo_revert(self, token: int) -> None:
        """Undo the newest journaled diff and pop its record (kv_utxo_revert).
        Raises if `token` is not the newest unreverted record."""
        self._check(self.lib.kv_utxo_revert(ctypes.c_void_p(self.ctx),
                                            ctypes.c_uint64(token)))

    def utxo_journal_drop(self, upto_token: int) -> None:
        """Free every undo record with token <= upto_token."""
        self._check(self.lib.kv_utxo_journal_drop(ctypes.c_void_p(self.ctx),
                                                  ctypes.c_uint64(upto_token)))

    def utxo_journal_stats(self) -> dict:
        """What the undo journal holds (kv_utxo_journal_stats): n_records,
        oldest_token, newest_token (0 when empty), device_bytes, and the
        kernel_ms of the last revert."""
        out = KvUtxoJournalInfo()
        self._check(self.lib.kv_utxo_journal_stats(ctypes.c_void_p(self.ctx),
                                                   ctypes.byref(out)))
        return {name: getattr(out, name) for name, _ in out._fields_}

    def utxo_changes_by_spk(self, token: int, queries, max_entries: int,
                            cursor: int = 0, flags: int = 0, spk_cap: int = 0):
        """One step of the walk over the entries the journaled diff `token`
        removed from and added to the set, filtered by script public key
        (kv_utxo_changes_by_spk), from change index `cursor`: (records,
        scripts, cursor, result). records are 96-byte change records (outpoint
        36 ‖ query index u32 ‖ amount u64 ‖ daa_score u64 ‖ flags u16 ‖
        spk_version u16 ‖ spk_len u32 ‖ covenant id 32) in ascending change
        index, KV_UTXO_CHANGE_F_REMOVED set on those that left the set.
        scripts is None with spk_cap == 0, else the records' scripts
        concatenated in record order (spk_cap >= KV_UTXO_MAX_SPK). result is a
        dict of cursor_end, added_amount, removed_amount, n_added, n_removed,
        n_added_gone, kernel_ms, over the whole record; the walk is over when
        the returned cursor equals result["cursor_end"]. With
        KV_UTXO_CHANGES_ALL in flags `queries` must be empty."""
        heads, blob, n = pack_spk_queries(queries)
        cur = ctypes.c_uint64(cursor)
        out = (ctypes.c_uint8 * (KV_UTXO_CHANGE_BYTES * max(max_entries, 1)))()
        spk = (ctypes.c_uint8 * spk_cap)() if spk_cap else None
        used, n_out = ctypes.c_size_t(), ctypes.c_size_t()
        res = KvUtxoChangesResult()
        rc = self.lib.kv_utxo_changes_by_spk(
            ctypes.c_void_p(self.ctx), ctypes.c_uint64(token),
            ctypes.c_uint32(flags), ctypes.byref(cur), heads, ctypes.c_size_t(n),
            blob, ctypes.c_size_t(len(blob)), ctypes.c_size_t(max_entries), out,
            spk, ctypes.c_size_t(spk_cap), ctypes.byref(used),
            ctypes.byref(n_out), ctypes.byref(res))
        self._check(rc)
        return (ctypes.string_at(out, KV_UTXO_CHANGE_BYTES * n_out.value),
                ctypes.string_at(spk, used.value) if spk_cap else None,
                cur.value,
                {name: getattr(res, name) for name, _ in res._fields_})

    def validate_block_utxo_undo(self, blob: bytes, n_txs: int, pov_daa: int,
                                 block_daa: int, flags: int = 2,
                                 want_muhash: bool = True):
        """validate_block_utxo(apply_diff=True) whose diff can be reverted:
        (codes, fees, partial, token)."""
        codes = (ctypes.c_int32 * n_txs)()
        fees = (ctypes.c_uint64 * n_txs)()
        partial = (ctypes.c_uint8 * 768)() if want_muhash else None
        token = ctypes.c_uint64()
        rc = self.lib.kv_validate_block_utxo_undo(
            ctypes.c_void_p(self.ctx), blob, ctypes.c_size_t(len(blob)),
            ctypes.c_uint64(pov_daa), ctypes.c_uint64(block_daa),
            ctypes.c_uint32(flags), codes, fees, partial, ctypes.byref(token))
        self._check(rc)
        return (list(codes), list(fees),
                bytes(partial) if want_muhash else None, token.value)

    def sig_cache_stats(self):
        out = KvCacheStats()
        self._check(self.lib.kv_sig_cache_stats(ctypes.c_void_p(self.ctx),
                                                ctypes.byref(out)))
        return out.insertions, out.hits, out.misses

    def block_body_check(self, blob: bytes):
        """Merkle root over tx hashes + duplicate/double-spend/chained checks."""
        root = (ctypes.c_uint8 * 32)()
        code = ctypes.c_int32()
        rc = self.lib.kv_block_body_check(
            ctypes.c_void_p(self.ctx), blob, ctypes.c_size_t(len(blob)),
            root, ctypes.byref(code))
        self._check(rc)
        return bytes(root), code.value

    def validate_mempool(self, blob: bytes, n_txs: int, pov_daa: int,
                         feerate_threshold: float = 0.0,
                         from_utxo_table: bool = False):
        codes = (ctypes.c_int32 * n_txs)()
        fees = (ctypes.c_uint64 * n_txs)()
        rc = self.lib.kv_validate_mempool(
            ctypes.c_void_p(self.ctx), blob, ctypes.c_size_t(len(blob)),
            ctypes.c_uint64(pov_daa), ctypes.c_double(feerate_threshold),
            ctypes.c_int(1 if from_utxo_table else 0), codes, fees)
        self._check(rc)
        return list(codes), list(fees)
