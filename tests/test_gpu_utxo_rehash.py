"""GPU UTXO table maintenance: kv_utxo_stats, kv_utxo_rehash (grow, shrink,
tombstone and arena compaction) and the export walk kv_utxo_export_chunk ⇔
get_pruning_point_utxos / get_virtual_utxos (consensus/src/consensus/
mod.rs:1067-1108), the serving half of kv_utxo_import_chunk.

The model is independent of the engine, as in test_gpu_utxo_commitment.py: a
Python dict of Entry, each element the oracle's ok_muhash_element over the
write_utxo serialisation written out here, products Python integers mod P.
A rehash must not change the set: "same contents" is checked entry by entry
through kv_utxo_lookup_spk and as a whole through kv_utxo_commitment."""
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
# 63 fixed bytes + script: 64/65/66 give 127/128/129-byte messages, 193 gives
# 256; 37 is the first arena length, 10,000 the longest script
SPK_LENS = [0, 1, 35, 36, 37, 64, 65, 66, 193, 10000]


@pytest.fixture(scope="module")
def engine():
    from rusty_kaspa_amd.engine import Engine
    eng = Engine()
    yield eng
    eng.close()


# ---------------- the independent model ----------------

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
        v = _elements[data] = limbs_int(out)
    return v


def limbs_int(limbs):
    return sum(int(limbs[i]) << (64 * i) for i in range(48))


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


def upsert_rc(engine, items):
    ops, ents, blob = chunk_args(items)
    return engine.lib.kv_utxo_upsert_spk(
        ctypes.c_void_p(engine.ctx), ops, ents, blob,
        ctypes.c_size_t(len(blob)), ctypes.c_size_t(len(items)))


def upsert(engine, items):
    assert upsert_rc(engine, items) == 0, engine.lib.kv_last_error().decode()


def remove(engine, ops):
    rc = engine.lib.kv_utxo_remove(ctypes.c_void_p(engine.ctx), b"".join(ops),
                                   ctypes.c_size_t(len(ops)))
    assert rc == 0, engine.lib.kv_last_error().decode()


def lookup(engine, ops):
    n = len(ops)
    out = (ctypes.c_uint8 * (64 * n))()
    bm = (ctypes.c_uint64 * ((n + 63) // 64))()
    rc = engine.lib.kv_utxo_lookup(ctypes.c_void_p(engine.ctx), b"".join(ops),
                                   ctypes.c_size_t(n), out, bm, None)
    assert rc == 0, engine.lib.kv_last_error().decode()
    return [(bm[i // 64] >> (i % 64)) & 1 for i in range(n)], bytes(out)


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


def rehash_rc(engine, capacity):
    return engine.lib.kv_utxo_rehash(ctypes.c_void_p(engine.ctx),
                                     ctypes.c_uint64(capacity), None)


def check_stats_sum(st):
    assert st["n_live"] + st["n_tomb"] + st["n_empty"] == st["slots"]
    assert st["arena_live_bytes"] <= st["arena_used"] <= st["arena_cap"] \
        or st["arena_used"] == 0
    return st


def check_contents(engine, model, removed=()):
    """every model key is found with the model's amount, daa, coinbase,
    version, length and script bytes; a sample of removed keys is not found"""
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
    removed = [op for op in removed if op not in model]
    if removed:
        found, _ = lookup(engine, removed)
        assert found == [0] * len(removed)


def rand_op(rng):
    return rng.randbytes(32) + struct.pack("<I", rng.randrange(8))


def rand_entry(rng, spk_len=None):
    if spk_len is None:
        # mostly standard 34/35-byte scripts, a few short, a few in the arena
        spk_len = rng.choice([34] * 10 + [35] * 5 + [0, 20, 36, 37, 150, 400])
    return Entry(rng.randrange(1 << 50), rng.randrange(1 << 40),
                 rng.random() < 0.1, rng.randbytes(spk_len))


def special_items(rng):
    """one entry for each script length of SPK_LENS"""
    return [(rand_op(rng), rand_entry(rng, ln)) for ln in SPK_LENS]


def mixed_items(seed=11, n_random=5000):
    rng = random.Random(seed)
    items = [(rand_op(rng), rand_entry(rng)) for _ in range(n_random)]
    items += special_items(rng)
    assert len({op for op, _ in items}) == len(items)
    return items


def load_mixed(engine):
    """4 scan windows of slots, ~5,000 entries spread over them"""
    window = engine.utxo_commitment_window()
    reset(engine, 2 * window)  # capacity doubles into slots: 4 windows
    items = mixed_items()
    upsert(engine, items)
    return items, dict(items)


def load_churned(engine):
    """the case-3 table: load_mixed, every third key removed, 200 live keys
    overwritten, 100 removed keys re-inserted. Returns (model, removed keys)."""
    items, model = load_mixed(engine)
    rng = random.Random(12)
    ops = [op for op, _ in items]
    removed = ops[::3]
    remove(engine, removed)
    for op in removed:
        del model[op]
    live = [op for op in ops if op in model]
    rewrites = [(op, rand_entry(rng)) for op in rng.sample(live, 200)]
    upsert(engine, rewrites)
    model.update(rewrites)
    back = [(op, rand_entry(rng)) for op in rng.sample(removed, 100)]
    upsert(engine, back)
    model.update(back)
    return model, [op for op in removed if op not in model]


def identity_partial():
    one = (1).to_bytes(384, "little")
    return bytearray(one + one)


# ---------------- stats and rehash ----------------

def test_stats_basics(engine):
    from rusty_kaspa_amd.engine import Engine
    fresh = Engine()
    try:
        st = fresh.utxo_stats()
        assert set(st) == {"slots", "n_live", "n_tomb", "n_empty", "arena_used",
                           "arena_live_bytes", "arena_cap"}
        assert all(v == 0 for v in st.values())
    finally:
        fresh.close()
    reset(engine, 32)
    st = check_stats_sum(engine.utxo_stats())
    assert (st["slots"], st["n_empty"], st["n_live"], st["n_tomb"]) == (64, 64, 0, 0)
    assert st["arena_used"] == 0 and st["arena_live_bytes"] == 0
    rng = random.Random(31)
    specials = special_items(rng)
    items = specials + [(rand_op(rng), rand_entry(rng)) for _ in range(20)]
    model = dict(items)
    assert len(model) == 30
    upsert(engine, items)
    st = check_stats_sum(engine.utxo_stats())
    assert (st["slots"], st["n_live"], st["n_tomb"], st["n_empty"]) == (64, 30, 0, 34)
    assert st["arena_live_bytes"] == st["arena_used"] == arena_bytes(model)
    assert st["arena_cap"] >= st["arena_used"]
    # remove the 10,000-byte entry, overwrite the 193-byte one with 400 bytes
    by_len = {len(e.spk): op for op, e in specials}
    used_before = st["arena_used"]
    remove(engine, [by_len[10000]])
    del model[by_len[10000]]
    model[by_len[193]] = rand_entry(rng, 400)
    upsert(engine, [(by_len[193], model[by_len[193]])])
    st = check_stats_sum(engine.utxo_stats())
    assert (st["n_live"], st["n_tomb"], st["n_empty"]) == (29, 1, 34)
    assert st["arena_live_bytes"] == arena_bytes(model)
    assert st["arena_used"] == used_before + 400
    assert st["arena_used"] > st["arena_live_bytes"]
    # stats is read-only
    assert engine.utxo_stats() == st
    check_contents(engine, model, [by_len[10000]])


def test_grow_full_table(engine, oracle):
    rng = random.Random(32)
    reset(engine, 32)
    items = [(rand_op(rng), rand_entry(rng)) for _ in range(64)]
    model = dict(items)
    assert len(model) == 64
    upsert(engine, items)  # every slot taken: probes wrap past the last slot
    st = check_stats_sum(engine.utxo_stats())
    assert (st["slots"], st["n_live"], st["n_empty"], st["n_tomb"]) == (64, 64, 0, 0)
    extra = (rand_op(rng), rand_entry(rng, 34))
    assert upsert_rc(engine, [extra]) == -3  # the table really is full
    check_contents(engine, model, [extra[0]])
    assert rehash_rc(engine, 65) == 0, engine.lib.kv_last_error().decode()
    st = check_stats_sum(engine.utxo_stats())
    assert (st["slots"], st["n_live"], st["n_tomb"]) == (256, 64, 0)
    assert st["arena_used"] == st["arena_live_bytes"] == arena_bytes(model)
    check_contents(engine, model, [extra[0]])
    upsert(engine, [extra])
    model[extra[0]] = extra[1]
    check_contents(engine, model)
    assert engine.utxo_stats()["n_live"] == 65
    check_commitment(engine, oracle, model)


def test_compaction_several_windows(engine, oracle):
    model, removed = load_churned(engine)
    st0 = check_stats_sum(engine.utxo_stats())
    window = engine.utxo_commitment_window()
    assert st0["slots"] == 4 * window
    assert st0["n_live"] == len(model) and st0["n_tomb"] > 0
    assert st0["arena_live_bytes"] == arena_bytes(model) < st0["arena_used"]
    c0 = check_commitment(engine, oracle, model)
    ms = engine.utxo_rehash(0)
    assert ms >= 0.0
    st = check_stats_sum(engine.utxo_stats())
    assert st["slots"] == st0["slots"]
    assert st["n_tomb"] == 0 and st["n_live"] == st0["n_live"]
    assert st["arena_used"] == st["arena_live_bytes"] == arena_bytes(model)
    check_contents(engine, model, removed[:200])
    c1 = check_commitment(engine, oracle, model)  # equals the oracle product
    assert num(c1) % P == num(c0) % P
    assert engine.muhash_finalize(c1) == engine.muhash_finalize(c0)
    # the rebuilt table takes further mutations
    rng = random.Random(33)
    gone = rng.sample(list(model), 50)
    remove(engine, gone)
    for op in gone:
        del model[op]
    more = [(rand_op(rng), rand_entry(rng, rng.choice([34, 35, 37, 400, 10000])))
            for _ in range(50)]
    assert any(len(e.spk) > 36 for _, e in more)
    upsert(engine, more)
    model.update(more)
    check_commitment(engine, oracle, model)
    check_contents(engine, model, gone)
    st = check_stats_sum(engine.utxo_stats())
    assert st["n_live"] == len(model)
    assert st["arena_live_bytes"] == arena_bytes(model)


def ensure_entry(engine, model, rng, spk_len):
    """a live key whose script has this length (upserting one if need be)"""
    for op, e in model.items():
        if len(e.spk) == spk_len:
            return op
    op, e = rand_op(rng), rand_entry(rng, spk_len)
    upsert(engine, [(op, e)])
    model[op] = e
    return op


def test_shrink(engine, oracle):
    model, _ = load_churned(engine)
    rng = random.Random(34)
    keep = [ensure_entry(engine, model, rng, 37),
            ensure_entry(engine, model, rng, MAX_SPK)]
    keep += rng.sample([op for op in model if op not in keep], 18)
    gone = [op for op in model if op not in keep]
    remove(engine, gone)
    model = {op: model[op] for op in keep}
    assert len(model) == 20
    assert engine.utxo_stats()["slots"] == 4 * engine.utxo_commitment_window()
    assert rehash_rc(engine, 20) == 0, engine.lib.kv_last_error().decode()
    st = check_stats_sum(engine.utxo_stats())
    assert (st["slots"], st["n_live"], st["n_tomb"], st["n_empty"]) == (64, 20, 0, 44)
    assert st["arena_used"] == st["arena_live_bytes"] == arena_bytes(model)
    check_contents(engine, model, gone[:200])
    check_commitment(engine, oracle, model)


def test_refusal_leaves_table_alone(engine, oracle):
    rng = random.Random(35)
    reset(engine, 100)
    items = [(rand_op(rng), rand_entry(rng)) for _ in range(110)]
    upsert(engine, items)
    model = dict(items)
    gone = [op for op, _ in items[:10]]  # leave tombstones and arena garbage
    remove(engine, gone)
    for op in gone:
        del model[op]
    assert len(model) == 100
    st0 = check_stats_sum(engine.utxo_stats())
    c0 = check_commitment(engine, oracle, model)
    assert rehash_rc(engine, 10) == -3  # 64 slots < 2 x 100 live
    assert engine.lib.kv_last_error()
    assert engine.utxo_stats() == st0
    c1, n_live, _ = engine.utxo_commitment()
    assert c1 == c0 and n_live == 100
    check_contents(engine, model, gone)
    with pytest.raises(RuntimeError):
        engine.utxo_rehash(49)  # 128 slots: still < 200
    assert engine.utxo_stats() == st0
    from rusty_kaspa_amd.engine import Engine
    fresh = Engine()
    try:
        assert rehash_rc(fresh, 0) == -1
        assert rehash_rc(fresh, 100) == -1
        assert all(v == 0 for v in fresh.utxo_stats().values())
    finally:
        fresh.close()


def test_rehash_empty_table(engine, golden):
    empty = bytes(golden("muhash.json")["empty_muhash"])
    reset(engine, 64)
    for capacity, slots in ((0, 128), (1000, 2048)):
        assert rehash_rc(engine, capacity) == 0
        st = check_stats_sum(engine.utxo_stats())
        assert (st["slots"], st["n_live"], st["n_tomb"]) == (slots, 0, 0)
        assert st["arena_used"] == 0
        partial, n_live, _ = engine.utxo_commitment()
        assert n_live == 0
        assert engine.muhash_finalize(partial) == empty


def test_tombstone_saturation(engine):
    rng = random.Random(36)
    reset(engine, 32)
    permanent = [(rand_op(rng), rand_entry(rng, 34)) for _ in range(8)]
    model = dict(permanent)
    upsert(engine, permanent)
    churned = []
    for _ in range(30):
        batch = [(rand_op(rng), rand_entry(rng, 34)) for _ in range(16)]
        upsert(engine, batch)
        remove(engine, [op for op, _ in batch])
        churned += [op for op, _ in batch]
    st = check_stats_sum(engine.utxo_stats())
    assert st["slots"] == 64 and st["n_live"] == 8
    assert st["n_tomb"] > 0 and st["n_empty"] < 56
    check_contents(engine, model, churned[-64:])
    engine.utxo_rehash(0)
    st = check_stats_sum(engine.utxo_stats())
    assert (st["slots"], st["n_live"], st["n_tomb"], st["n_empty"]) == (64, 8, 0, 56)
    check_contents(engine, model, churned[-64:])


def test_block_path_after_rehash(engine, oracle):
    """validate_block_utxo(apply_diff) on a rebuilt table gives what it gives
    on the table as seeded, and the per-block commitment invariant holds."""
    n = 60
    blob, _ = gen_block(oracle, seed=22, n_txs=n, pct_multi_input=25,
                        pct_ecdsa=10, pct_multisig=10, pct_invalid=15)
    stripped, seeds = strip_utxo_entries(blob)

    def seed_table():
        reset(engine, max(64, 2 * len(seeds)))
        rc = engine.lib.kv_utxo_upsert(
            ctypes.c_void_p(engine.ctx), b"".join(op for op, _ in seeds),
            b"".join(e for _, e in seeds), ctypes.c_size_t(len(seeds)))
        assert rc == 0, engine.lib.kv_last_error().decode()

    seed_table()
    c0, n0, _ = engine.utxo_commitment()
    engine.utxo_rehash(0)
    assert engine.utxo_stats()["n_live"] == n0
    codes, fees, block_partial = engine.validate_block_utxo(
        stripped, n, 10**9, 10**9, SKIP_MASS, apply_diff=True)
    c1, n1, _ = engine.utxo_commitment()
    assert any(c != 0 for c in codes) and any(c == 0 for c in codes)
    acc = bytearray(c0)
    engine.muhash_combine(acc, block_partial)
    assert c1 != c0 and n1 > 0
    assert engine.muhash_finalize(bytes(acc)) == engine.muhash_finalize(c1)
    # the same block on the table as seeded, no rehash
    seed_table()
    codes2, fees2, block_partial2 = engine.validate_block_utxo(
        stripped, n, 10**9, 10**9, SKIP_MASS, apply_diff=True)
    c2, n2, _ = engine.utxo_commitment()
    assert codes == codes2 and fees == fees2
    assert num(block_partial) * den(block_partial2) % P == \
        num(block_partial2) * den(block_partial) % P
    assert engine.muhash_finalize(block_partial) == \
        engine.muhash_finalize(block_partial2)
    assert n1 == n2 and num(c1) % P == num(c2) % P


# ---------------- the export walk ----------------

def export_rc(engine, cursor, max_entries, spk_cap):
    cur = ctypes.c_uint64(cursor)
    ops = (ctypes.c_uint8 * (36 * max_entries))()
    ents = (ctypes.c_uint8 * (64 * max_entries))()
    spk = (ctypes.c_uint8 * max(spk_cap, 1))()
    used, n = ctypes.c_size_t(), ctypes.c_size_t()
    rc = engine.lib.kv_utxo_export_chunk(
        ctypes.c_void_p(engine.ctx), ctypes.byref(cur),
        ctypes.c_size_t(max_entries), ops, ents, spk, ctypes.c_size_t(spk_cap),
        ctypes.byref(used), ctypes.byref(n))
    return rc, cur.value, n.value


def walk(engine, max_entries, spk_cap):
    """every chunk of a full walk, as (outpoints, entries, spk_blob, n); the
    end is *cursor == slots with n == 0, and only there"""
    slots = engine.utxo_stats()["slots"]
    cursor, chunks = 0, []
    for _ in range(slots + 2):
        nxt, ops, ents, spk, n = engine.utxo_export_chunk(cursor, max_entries,
                                                          spk_cap)
        assert n <= max_entries and cursor <= nxt <= slots
        assert len(ops) == 36 * n and len(ents) == 64 * n
        assert nxt > cursor or (n == 0 and nxt == slots)
        if n == 0 and nxt == slots:
            # the end is stable
            assert engine.utxo_export_chunk(nxt, max_entries, spk_cap) == (
                slots, b"", b"", b"", 0)
            return chunks
        chunks.append((ops, ents, spk, n))
        cursor = nxt
    raise AssertionError("the walk did not end")


def check_walk(chunks, model, spk_cap):
    seen = set()
    for ops, ents, spk, n in chunks:
        pos = 0
        for i in range(n):
            op, rec = ops[36 * i:36 * (i + 1)], ents[64 * i:64 * (i + 1)]
            assert op in model and op not in seen
            seen.add(op)
            e = model[op]
            assert rec == e.pack()
            if len(e.spk) > 36:  # scripts sit in spk_out in entry order
                assert spk[pos:pos + len(e.spk)] == e.spk
                pos += len(e.spk)
        assert pos == len(spk) <= spk_cap
    assert seen == set(model)


@pytest.mark.parametrize("max_entries", [1, 63, 64, 65, 1000])
def test_export_walk(engine, max_entries):
    model, _ = load_churned(engine)  # the walk crosses tombstones
    st = engine.utxo_stats()
    assert st["n_tomb"] > 0
    chunks = walk(engine, max_entries, 1 << 16)
    check_walk(chunks, model, 1 << 16)
    assert sum(c[3] for c in chunks) == len(model)
    if max_entries != 1:  # slot order is stable: the same byte streams again
        assert walk(engine, max_entries, 1 << 16) == chunks
    assert engine.utxo_stats() == st  # read-only


def test_export_splits_on_spk_cap(engine):
    rng = random.Random(37)
    reset(engine, 32)
    items = [(rand_op(rng), rand_entry(rng, 6000)) for _ in range(3)]
    items += [(rand_op(rng), rand_entry(rng, ln)) for ln in (0, 34, 35, 36, 37)]
    upsert(engine, items)
    model = dict(items)
    chunks = walk(engine, 64, MAX_SPK)  # two 6,000-byte scripts never share
    check_walk(chunks, model, MAX_SPK)
    assert len(chunks) >= 3
    for _, _, spk, _ in chunks:
        assert len(spk) < 12000
    rc, cursor, n = export_rc(engine, 0, 64, MAX_SPK - 1)
    assert (rc, cursor, n) == (-1, 0, 0)
    assert b"spk_cap" in engine.lib.kv_last_error()


def test_export_empty_and_never_reset(engine):
    reset(engine, 32)
    assert engine.utxo_export_chunk(0, 10, MAX_SPK) == (64, b"", b"", b"", 0)
    assert walk(engine, 10, MAX_SPK) == []
    from rusty_kaspa_amd.engine import Engine
    fresh = Engine()
    try:
        assert fresh.utxo_export_chunk(0, 10, MAX_SPK) == (0, b"", b"", b"", 0)
    finally:
        fresh.close()


def test_export_import_round_trip(engine, oracle):
    model, _ = load_churned(engine)
    want = product(oracle, model)
    source = check_commitment(engine, oracle, model)
    chunks = walk(engine, 1000, 1 << 16)
    from rusty_kaspa_amd.engine import Engine
    other = Engine()
    try:
        reset(other, 8192)
        acc = identity_partial()
        for ops, ents, spk, n in chunks:  # fed back unchanged
            other.utxo_import_chunk(ops, ents, spk, n, acc)
        final = oracle_finalize(oracle, want)
        assert other.muhash_finalize(bytes(acc)) == final
        assert engine.muhash_finalize(source) == final
        assert num(bytes(acc)) % P == num(source) % P and den(bytes(acc)) == 1
        imported = check_commitment(other, oracle, model)
        assert num(imported) % P == num(source) % P
        check_contents(other, model)
    finally:
        other.close()
