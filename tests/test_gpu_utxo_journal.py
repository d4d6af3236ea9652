"""The device-resident undo journal of the GPU UTXO table: kv_utxo_apply_diff
⇔ write_diff_batch (consensus/src/model/stores/utxo_set.rs:107-112) with the
inverse kept, kv_utxo_revert ⇔ with_diff_in_place(as_reversed) of one chain
block (consensus/src/pipeline/virtual_processor/processor.rs:410), plus
kv_utxo_journal_drop / kv_utxo_journal_stats and kv_validate_block_utxo_undo.

The model is a Python dict of Entry, independent of the engine, as in
test_gpu_utxo_rehash.py (whose small helpers are copied here). "The same set"
is checked entry by entry through kv_utxo_lookup_spk, by count through
kv_utxo_stats, and as a whole through kv_utxo_commitment against the oracle's
product. Tables have 64 to 8,192 slots."""
import ctypes
import os
import random
import struct
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))
from workload import gen_block  # noqa: E402

from rusty_kaspa_amd.blob import strip_utxo_entries  # noqa: E402

pytestmark = pytest.mark.gpu

P = 2**3072 - 1103717
U = ctypes.c_uint64 * 48
SKIP_MASS = 2
F_COINBASE, F_ARENA = 1, 2
U64_MAX = 2**64 - 1
MAX_SPK = 10000


@pytest.fixture(scope="module")
def engine():
    from rusty_kaspa_amd.engine import Engine
    eng = Engine()
    yield eng
    eng.close()


# ---------------- the independent model (as test_gpu_utxo_rehash.py) ----------------

class Entry:
    __slots__ = ("amount", "daa", "coinbase", "spk_version", "spk")

    def __init__(self, amount, daa, coinbase, spk, spk_version=0):
        self.amount, self.daa, self.coinbase = amount, daa, coinbase
        self.spk, self.spk_version = spk, spk_version

    def pack(self):
        """the 64-byte record handed to kv_utxo_upsert_spk"""
        head = struct.pack("<QQHHI", self.amount, self.daa,
                           F_COINBASE if self.coinbase else 0,
                           self.spk_version, len(self.spk))
        inline = self.spk.ljust(36, b"\0") if len(self.spk) <= 36 else bytes(36)
        return head + inline + bytes(4)


def write_utxo(op36, e):
    """muhash.rs:55-69, byte for byte (the table stores no covenant id)."""
    index, = struct.unpack("<I", op36[32:])
    return (op36[:32] + struct.pack("<I", index) + struct.pack("<Q", e.daa)
            + struct.pack("<Q", e.amount) + bytes([1 if e.coinbase else 0])
            + struct.pack("<H", e.spk_version) + struct.pack("<Q", len(e.spk))
            + e.spk)


_elements = {}  # serialisation -> element as an integer; computed once


def element(oracle, op36, e):
    data = write_utxo(op36, e)
    v = _elements.get(data)
    if v is None:
        out = U()
        oracle.ok_muhash_element(data, ctypes.c_size_t(len(data)), out)
        v = _elements[data] = sum(int(out[i]) << (64 * i) for i in range(48))
    return v


def product(oracle, model):
    acc = 1
    for op, e in model.items():
        acc = acc * element(oracle, op, e) % P
    return acc


def num(partial):
    return int.from_bytes(partial[:384], "little")


def den(partial):
    return int.from_bytes(partial[384:768], "little")


def oracle_finalize(oracle, value):
    n = U(*[(value >> (64 * i)) & U64_MAX for i in range(48)])
    d = U()
    oracle.ok_u3072_one(d)
    out = (ctypes.c_uint8 * 32)()
    oracle.ok_muhash_finalize(n, d, out)
    return bytes(out)


def check_commitment(engine, oracle, model):
    partial, n_live, ms = engine.utxo_commitment()
    want = product(oracle, model)
    assert n_live == len(model)
    assert num(partial) % P == want
    assert den(partial) == 1
    assert engine.muhash_finalize(partial) == oracle_finalize(oracle, want)
    assert ms >= 0.0
    return partial


def arena_bytes(model):
    return sum(len(e.spk) for e in model.values() if len(e.spk) > 36)


# ---------------- table helpers ----------------

def reset(engine, capacity):
    assert engine.lib.kv_utxo_reset(ctypes.c_void_p(engine.ctx),
                                    ctypes.c_uint64(capacity)) == 0


def chunk_args(items):
    ops = b"".join(op for op, _ in items)
    ents = b"".join(e.pack() for _, e in items)
    blob = b"".join(e.spk for _, e in items if len(e.spk) > 36)
    return ops, ents, blob


def upsert(engine, items):
    ops, ents, blob = chunk_args(items)
    rc = engine.lib.kv_utxo_upsert_spk(
        ctypes.c_void_p(engine.ctx), ops, ents, blob,
        ctypes.c_size_t(len(blob)), ctypes.c_size_t(len(items)))
    assert rc == 0, engine.lib.kv_last_error().decode()


def lookup_spk(engine, ops, spk_cap):
    n = len(ops)
    out = (ctypes.c_uint8 * (64 * n))()
    bm = (ctypes.c_uint64 * ((n + 63) // 64))()
    spk = (ctypes.c_uint8 * spk_cap)()
    used = ctypes.c_size_t()
    rc = engine.lib.kv_utxo_lookup_spk(
        ctypes.c_void_p(engine.ctx), b"".join(ops), ctypes.c_size_t(n), out,
        bm, spk, ctypes.c_size_t(spk_cap), ctypes.byref(used))
    assert rc == 0, engine.lib.kv_last_error().decode()
    return ([(bm[i // 64] >> (i % 64)) & 1 for i in range(n)], bytes(out),
            bytes(spk[:used.value]))


def check_contents(engine, model, absent=()):
    """every model key is found with the model's amount, daa, coinbase,
    version, length and script bytes; none of `absent` (keys outside the
    model) is found"""
    ops = list(model)
    if ops:
        found, ents, spks = lookup_spk(engine, ops, max(1, arena_bytes(model)))
        assert found == [1] * len(ops)
        for i, op in enumerate(ops):
            e, rec = model[op], ents[64 * i:64 * (i + 1)]
            amount, daa, flags, ver, ln = struct.unpack_from("<QQHHI", rec)
            assert (amount, daa, flags & 1, ver, ln) == (
                e.amount, e.daa, int(e.coinbase), e.spk_version, len(e.spk))
            if ln <= 36:
                assert not flags & F_ARENA and rec[24:24 + ln] == e.spk
            else:
                off, = struct.unpack_from("<I", rec, 24)
                assert flags & F_ARENA and spks[off:off + ln] == e.spk
    absent = [op for op in absent if op not in model]
    if absent:
        found, _, _ = lookup_spk(engine, absent, 1)
        assert found == [0] * len(absent)
    assert engine.utxo_stats()["n_live"] == len(model)


def snapshot(engine, model):
    """what kv_utxo_lookup_spk returns for the model's keys, byte for byte.
    Scripts come back in key order with gathered-buffer offsets, so two
    snapshots of equal sets are equal whatever the arena looks like."""
    return lookup_spk(engine, list(model), max(1, arena_bytes(model)))


def rand_op(rng):
    return rng.randbytes(32) + struct.pack("<I", rng.randrange(8))


def rand_entry(rng, spk_len=None):
    if spk_len is None:
        # mostly standard 34/35-byte scripts, a few short, a few in the arena
        spk_len = rng.choice([34] * 10 + [35] * 5 + [0, 20, 36, 37, 150, 400])
    return Entry(rng.randrange(1 << 50), rng.randrange(1 << 40),
                 rng.random() < 0.1, rng.randbytes(spk_len))


def rand_items(rng, n, spk_lens=()):
    """n random entries, the first len(spk_lens) with those script lengths"""
    items = [(rand_op(rng), rand_entry(rng, ln)) for ln in spk_lens]
    items += [(rand_op(rng), rand_entry(rng)) for _ in range(n - len(spk_lens))]
    assert len({op for op, _ in items}) == n
    return items


# ---------------- journal helpers ----------------

def apply_rc(engine, removed, added):
    """(rc, token, result) of kv_utxo_apply_diff"""
    from rusty_kaspa_amd.engine import KvUtxoDiffResult
    ops, ents, blob = chunk_args(added)
    res = KvUtxoDiffResult()
    token = ctypes.c_uint64()
    rc = engine.lib.kv_utxo_apply_diff(
        ctypes.c_void_p(engine.ctx), b"".join(removed),
        ctypes.c_size_t(len(removed)), ops, ents, blob,
        ctypes.c_size_t(len(blob)), ctypes.c_size_t(len(added)),
        ctypes.byref(res), ctypes.byref(token))
    return rc, token.value, res


def apply(engine, model, removed, added):
    """the diff through the engine wrapper and on the model: (token, result)"""
    ops, ents, blob = chunk_args(added)
    token, res = engine.utxo_apply_diff(b"".join(removed), ops, ents, blob)
    assert res["n_removed_missing"] == sum(op not in model for op in removed)
    assert res["n_added_overwrote"] == sum(op in model for op, _ in added)
    assert res["journal_bytes"] > 0 or not (removed or added)
    assert res["kernel_ms"] >= 0.0
    for op in removed:
        model.pop(op, None)
    model.update(added)
    return token, res


def revert_rc(engine, token):
    return engine.lib.kv_utxo_revert(ctypes.c_void_p(engine.ctx),
                                     ctypes.c_uint64(token))


def load(engine, capacity, items):
    reset(engine, capacity)
    upsert(engine, items)
    assert engine.utxo_journal_stats()["n_records"] == 0
    return dict(items)


# ---------------- 1. round trip ----------------

def test_round_trip(engine, oracle):
    rng = random.Random(101)
    items = rand_items(rng, 1003, (37, 200, 10000))
    model = load(engine, 2048, items)
    original = dict(model)
    snap0 = snapshot(engine, original)
    c0 = check_commitment(engine, oracle, model)
    st0 = engine.utxo_stats()
    # 300 out, the three special arena entries among them; 300 in, arena too
    removed = [op for op, _ in items[:3]] + \
        [op for op, _ in rng.sample(items[3:], 297)]
    assert sum(len(original[op].spk) > 36 for op in removed) >= 3
    added = rand_items(rng, 300, (37, 200, 10000, 400))
    token, res = apply(engine, model, removed, added)
    assert (res["n_removed_missing"], res["n_added_overwrote"]) == (0, 0)
    js = engine.utxo_journal_stats()
    assert (js["n_records"], js["oldest_token"], js["newest_token"]) == (1, token, token)
    assert js["device_bytes"] == res["journal_bytes"]
    # keys, values, bitmap, and the scripts of the removed arena entries
    captured = sum(len(original[op].spk) for op in removed
                   if len(original[op].spk) > 36)
    assert res["journal_bytes"] >= 600 * 100 + captured
    check_contents(engine, model, removed)
    check_commitment(engine, oracle, model)
    engine.utxo_revert(token)
    assert engine.utxo_journal_stats()["n_records"] == 0
    check_contents(engine, original, [op for op, _ in added])
    assert snapshot(engine, original) == snap0  # byte-identical
    st = engine.utxo_stats()
    assert st["n_live"] == st0["n_live"] == len(original)
    c1 = check_commitment(engine, oracle, original)  # the oracle product
    assert num(c1) % P == num(c0) % P
    assert engine.muhash_finalize(c1) == engine.muhash_finalize(c0)


# ---------------- 2. wave edges ----------------

EDGES = [0, 1, 63, 64, 65, 257]


@pytest.fixture(scope="module")
def edge_items():
    rng = random.Random(102)
    return rand_items(rng, 600, (37, 200, 10000)), rand_items(rng, 257, (37, 10000))


@pytest.mark.parametrize("n_added", EDGES)
@pytest.mark.parametrize("n_removed", EDGES)
def test_wave_edges(engine, edge_items, n_removed, n_added):
    base, fresh = edge_items
    model = load(engine, 1024, base)
    original = dict(model)
    snap0 = snapshot(engine, original)
    removed = [op for op, _ in base[:n_removed]]
    added = fresh[:n_added]
    token, res = apply(engine, model, removed, added)
    assert (res["n_removed_missing"], res["n_added_overwrote"]) == (0, 0)
    assert engine.utxo_journal_stats()["n_records"] == 1  # also for 0 + 0
    check_contents(engine, model, removed)
    engine.utxo_revert(token)
    check_contents(engine, original, [op for op, _ in added])
    assert snapshot(engine, original) == snap0
    assert engine.utxo_journal_stats()["n_records"] == 0


def test_duplicate_outpoints_refused(engine):
    rng = random.Random(103)
    items = rand_items(rng, 100)
    model = load(engine, 128, items)
    snap0 = snapshot(engine, model)
    a, b = items[0][0], items[1][0]
    fresh = rand_items(rng, 2)
    for removed, added in (([a, b, a], []),
                           ([a], [(a, rand_entry(rng))]),
                           ([], [fresh[0], fresh[1], (fresh[0][0], rand_entry(rng))])):
        rc, _, _ = apply_rc(engine, removed, added)
        assert rc == -1
        assert b"distinct" in engine.lib.kv_last_error()
    assert snapshot(engine, model) == snap0
    check_contents(engine, model, [op for op, _ in fresh])
    assert engine.utxo_journal_stats()["n_records"] == 0


# ---------------- 3. non-canonical diffs ----------------

def test_non_canonical_diffs(engine, oracle):
    rng = random.Random(104)
    items = rand_items(rng, 200, (34, 400, 35, 10000, 37))
    model = load(engine, 256, items)
    original = dict(model)
    snap0 = snapshot(engine, original)
    c0 = check_commitment(engine, oracle, model)
    inline_a, arena_a, inline_b, arena_b, arena_c = (op for op, _ in items[:5])
    ghosts = [rand_op(rng) for _ in range(3)]  # removed, but never in the set
    removed = ghosts[:2] + [items[10][0], items[11][0]] + ghosts[2:]
    added = [(inline_a, rand_entry(rng, 5000)),   # inline -> arena
             (arena_a, rand_entry(rng, 20)),      # arena -> inline
             (inline_b, rand_entry(rng, 34)),     # inline -> inline
             (arena_b, rand_entry(rng, 300)),     # arena -> arena
             (arena_c, rand_entry(rng, 37))] + rand_items(rng, 70, (150,))
    token, res = apply(engine, model, removed, added)
    assert (res["n_removed_missing"], res["n_added_overwrote"]) == (3, 5)
    check_contents(engine, model, removed)
    check_commitment(engine, oracle, model)
    engine.utxo_revert(token)
    # the old values are back; the absent ones were not invented
    check_contents(engine, original, ghosts + [op for op, _ in added[5:]])
    assert snapshot(engine, original) == snap0
    c1 = check_commitment(engine, oracle, original)
    assert num(c1) % P == num(c0) % P


# ---------------- 4. stack of three ----------------

def test_stack_of_three(engine, oracle):
    rng = random.Random(105)
    items = rand_items(rng, 400, (37, 10000))
    model = load(engine, 1024, items)
    states = [dict(model)]
    # diff 1 removes 50 (an arena entry among them) and creates 60
    removed1 = [op for op, _ in items[:50]]
    added1 = rand_items(rng, 60, (200, 36))
    t1, _ = apply(engine, model, removed1, added1)
    states.append(dict(model))
    # diff 2 spends outputs diff 1 created and re-creates an outpoint diff 1
    # removed (with another value)
    removed2 = [op for op, _ in added1[:20]] + [op for op, _ in items[60:70]]
    added2 = [(removed1[0], rand_entry(rng, 34)), (removed1[1], rand_entry(rng, 500))] \
        + rand_items(rng, 30, (37,))
    t2, res2 = apply(engine, model, removed2, added2)
    assert (res2["n_removed_missing"], res2["n_added_overwrote"]) == (0, 0)
    states.append(dict(model))
    removed3 = [op for op, _ in added2[:10]] + [op for op, _ in items[100:140]]
    added3 = rand_items(rng, 45, (10000,))
    t3, _ = apply(engine, model, removed3, added3)
    assert t1 < t2 < t3
    js = engine.utxo_journal_stats()
    assert (js["n_records"], js["oldest_token"], js["newest_token"]) == (3, t1, t3)
    check_contents(engine, model, removed3)
    # out of order: refused, nothing changes
    snap3 = snapshot(engine, model)
    for stale in (t1, t2, t3 + 1, 0):
        assert revert_rc(engine, stale) == -1
    assert snapshot(engine, model) == snap3
    assert engine.utxo_journal_stats() == js
    check_contents(engine, model, removed3)
    everything = set().union(*states, model)
    for token, state in ((t3, states[2]), (t2, states[1]), (t1, states[0])):
        engine.utxo_revert(token)
        check_contents(engine, state, [op for op in everything if op not in state])
        check_commitment(engine, oracle, state)
    assert engine.utxo_journal_stats()["n_records"] == 0
    assert revert_rc(engine, t1) == -1


# ---------------- 5. probe chains ----------------

def test_probe_chains(engine):
    """ten keys with one home slot in a 64-slot table: op_hash reads only the
    first eight bytes of the tx id and the index"""
    rng = random.Random(106)
    head = rng.randbytes(8)
    keys = [head + rng.randbytes(24) + struct.pack("<I", 3) for _ in range(10)]
    chain = [(op, rand_entry(rng, ln))
             for op, ln in zip(keys[:8], (34, 35, 0, 36, 400, 34, 37, 35))]
    reset(engine, 32)
    for item in chain:  # one at a time: slots home .. home + 7, in this order
        upsert(engine, [item])
    model = dict(chain)
    snap0 = snapshot(engine, model)
    st = engine.utxo_stats()
    assert (st["slots"], st["n_live"], st["n_tomb"]) == (64, 8, 0)
    removed = [keys[1], keys[4]]  # the second and the fifth; the fifth in the arena
    added = [(keys[8], rand_entry(rng, 34)), (keys[9], rand_entry(rng, 150))]
    token, res = apply(engine, dict(model), removed, added)
    after = {op: e for op, e in model.items() if op not in removed}
    after.update(added)
    check_contents(engine, after, removed)
    st = engine.utxo_stats()
    assert (st["n_live"], st["n_tomb"]) == (8, 0)  # the new keys took the tombstones
    engine.utxo_revert(token)
    check_contents(engine, model, keys[8:])
    assert snapshot(engine, model) == snap0
    st = engine.utxo_stats()
    assert (st["n_live"], st["n_tomb"], st["n_empty"]) == (8, 0, 56)


# ---------------- 6. a rehash between apply and revert ----------------

@pytest.mark.parametrize("grow", [False, True])
def test_rehash_in_between(engine, oracle, grow):
    rng = random.Random(107)
    items = rand_items(rng, 500, (37, 200, 10000, 400))
    model = load(engine, 512, items)
    original = dict(model)
    snap0 = snapshot(engine, original)
    c0 = check_commitment(engine, oracle, model)
    slots0 = engine.utxo_stats()["slots"]
    removed = [op for op, _ in items[:120]]  # four arena entries at least
    added = rand_items(rng, 100, (37, 10000, 150)) + \
        [(items[200][0], rand_entry(rng, 600))]  # one overwrite
    captured = sum(len(original[op].spk) for op in removed + [items[200][0]]
                   if len(original[op].spk) > 36)
    assert captured >= 37 + 200 + 10000 + 400
    token, res = apply(engine, model, removed, added)
    assert res["n_added_overwrote"] == 1
    engine.utxo_rehash(2 * 512 if grow else 0)
    st = engine.utxo_stats()
    assert st["slots"] == (2 * slots0 if grow else slots0) and st["n_tomb"] == 0
    assert st["arena_used"] == st["arena_live_bytes"] == arena_bytes(model)
    check_contents(engine, model, removed)
    js = engine.utxo_journal_stats()
    assert (js["n_records"], js["newest_token"]) == (1, token)  # still valid
    engine.utxo_revert(token)
    check_contents(engine, original, [op for op, _ in added])
    assert snapshot(engine, original) == snap0
    c1 = check_commitment(engine, oracle, original)
    assert num(c1) % P == num(c0) % P
    st = engine.utxo_stats()
    assert st["n_live"] + st["n_tomb"] + st["n_empty"] == st["slots"]
    assert st["arena_live_bytes"] == arena_bytes(original)
    # the compacted arena of the applied set, plus the record's scripts
    assert st["arena_used"] == arena_bytes(model) + captured
    assert st["arena_used"] - st["arena_live_bytes"] >= 0
    assert st["arena_used"] <= st["arena_cap"]


# ---------------- 7. atomic failure ----------------

def test_atomic_failure(engine):
    rng = random.Random(108)
    items = rand_items(rng, 60, (37, 10000))
    model = load(engine, 32, items)
    assert engine.utxo_stats()["slots"] == 64
    snap0 = snapshot(engine, model)
    added = rand_items(rng, 10, (200,))
    rc, _, _ = apply_rc(engine, [], added)
    assert rc == -3
    assert b"table full" in engine.lib.kv_last_error()
    check_contents(engine, model, [op for op, _ in added])
    assert snapshot(engine, model) == snap0
    assert engine.utxo_stats()["n_live"] == 60
    js = engine.utxo_journal_stats()
    assert (js["n_records"], js["device_bytes"]) == (0, 0)
    # with removes in the same diff: they are put back too
    rc, _, _ = apply_rc(engine, [op for op, _ in items[:3]], rand_items(rng, 10))
    assert rc == -3
    check_contents(engine, model)
    assert snapshot(engine, model) == snap0
    assert engine.utxo_journal_stats()["n_records"] == 0
    with pytest.raises(RuntimeError):
        engine.utxo_apply_diff(b"", *chunk_args(added))
    # a diff that fits still goes through, and back
    token, _ = apply(engine, dict(model), [items[0][0]], added[:4])
    engine.utxo_revert(token)
    assert snapshot(engine, model) == snap0


# ---------------- 8. drop, reset, stats ----------------

def test_drop_reset_stats(engine):
    rng = random.Random(109)
    items = rand_items(rng, 300, (37, 10000))
    model = load(engine, 512, items)
    js = engine.utxo_journal_stats()
    assert (js["n_records"], js["oldest_token"], js["newest_token"],
            js["device_bytes"]) == (0, 0, 0, 0)
    tokens, sizes = [], []
    for k in range(3):
        removed = [op for op, _ in items[40 * k:40 * k + 40]]
        token, res = apply(engine, model, removed, rand_items(rng, 30, (150,)))
        tokens.append(token)
        sizes.append(res["journal_bytes"])
        if k == 1:
            after_two = dict(model)
    js3 = engine.utxo_journal_stats()
    assert js3["n_records"] == 3 and js3["device_bytes"] == sum(sizes)
    assert sizes[0] > 10037  # the first diff removed both special arena entries
    engine.utxo_journal_drop(tokens[1])
    js1 = engine.utxo_journal_stats()
    assert (js1["n_records"], js1["oldest_token"], js1["newest_token"]) == (
        1, tokens[2], tokens[2])
    assert js1["device_bytes"] == sizes[2] < js3["device_bytes"]
    assert revert_rc(engine, tokens[0]) == -1 and revert_rc(engine, tokens[1]) == -1
    check_contents(engine, model)
    engine.utxo_journal_drop(tokens[1])  # nothing left to drop: still fine
    engine.utxo_revert(tokens[2])  # the newest one is still revertible
    check_contents(engine, after_two, [op for op in model if op not in after_two])
    assert engine.utxo_journal_stats()["n_records"] == 0
    assert revert_rc(engine, tokens[1]) == -1
    # kv_utxo_reset empties the journal; tokens keep growing
    token, _ = apply(engine, dict(after_two), [items[299][0]], [])
    assert token > tokens[2]
    assert engine.utxo_journal_stats()["n_records"] == 1
    reset(engine, 512)
    js = engine.utxo_journal_stats()
    assert (js["n_records"], js["device_bytes"]) == (0, 0)
    assert revert_rc(engine, token) == -1
    assert engine.utxo_stats()["n_live"] == 0
    # a context that never had a table refuses the apply
    from rusty_kaspa_amd.engine import Engine
    fresh = Engine()
    try:
        rc, _, _ = apply_rc(fresh, [items[0][0]], [])
        assert rc == -1
        assert fresh.utxo_journal_stats()["n_records"] == 0
    finally:
        fresh.close()


# ---------------- 9. the block path ----------------

def test_block_path(engine, oracle):
    n = 40
    blob, _ = gen_block(oracle, seed=23, n_txs=n, pct_multi_input=25,
                        pct_ecdsa=10, pct_multisig=10, pct_invalid=15)
    stripped, seeds = strip_utxo_entries(blob)
    offs = struct.unpack_from(f"<{n}I", blob, 4)
    n_in = [struct.unpack_from("<H", blob, off + 2)[0] for off in offs]
    bounds = [sum(n_in[:t]) for t in range(n + 1)]
    assert bounds[n] == len(seeds)

    def seed_table(eng):
        reset(eng, max(64, 2 * len(seeds)))
        rc = eng.lib.kv_utxo_upsert(
            ctypes.c_void_p(eng.ctx), b"".join(op for op, _ in seeds),
            b"".join(e for _, e in seeds), ctypes.c_size_t(len(seeds)))
        assert rc == 0, eng.lib.kv_last_error().decode()

    from rusty_kaspa_amd.engine import Engine
    other = Engine()
    try:
        seed_table(engine)
        seed_table(other)
        c0, n0, _ = engine.utxo_commitment()
        codes, fees, partial, token = engine.validate_block_utxo_undo(
            stripped, n, 10**9, 10**9, SKIP_MASS)
        codes2, fees2, partial2 = other.validate_block_utxo(
            stripped, n, 10**9, 10**9, SKIP_MASS, apply_diff=True)
        assert any(c != 0 for c in codes) and any(c == 0 for c in codes)
        assert codes == codes2 and fees == fees2 and partial == partial2
        c1, n1, _ = engine.utxo_commitment()
        c2, n2, _ = other.utxo_commitment()
        assert n1 == n2 and num(c1) % P == num(c2) % P
        assert num(c1) % P != num(c0) % P
        js = engine.utxo_journal_stats()
        assert (js["n_records"], js["newest_token"]) == (1, token)
        # a rejected tx's inputs were never touched; an accepted tx's are gone
        spent = {seeds[i][0] for t in range(n) if codes[t] == 0
                 for i in range(bounds[t], bounds[t + 1])}
        kept = [seeds[i] for t in range(n) if codes[t] != 0
                for i in range(bounds[t], bounds[t + 1]) if seeds[i][0] not in spent]
        assert kept and spent
        found, ents, _ = lookup_spk(engine, [op for op, _ in kept], 1)
        assert found == [1] * len(kept)
        assert ents == b"".join(e for _, e in kept)
        found, _, _ = lookup_spk(engine, sorted(spent), 1)
        assert found == [0] * len(spent)
        # revert: the pre-block set, so the same block validates the same way
        engine.utxo_revert(token)
        c3, n3, _ = engine.utxo_commitment()
        assert n3 == n0 and num(c3) % P == num(c0) % P
        assert engine.muhash_finalize(c3) == engine.muhash_finalize(c0)
        found, ents, _ = lookup_spk(engine, [op for op, _ in seeds], 1)
        assert found == [1] * len(seeds)
        assert ents == b"".join(e for _, e in seeds)
        codes3, fees3, partial3 = engine.validate_block_utxo(
            stripped, n, 10**9, 10**9, SKIP_MASS, apply_diff=False)
        assert codes3 == codes and fees3 == fees
        assert engine.muhash_finalize(partial3) == engine.muhash_finalize(partial)
        assert engine.utxo_journal_stats()["n_records"] == 0
    finally:
        other.close()
