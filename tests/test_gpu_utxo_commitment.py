"""GPU UTXO-set MuHash commitment (kv_utxo_commitment) and verified chunk
import (kv_utxo_import_chunk) ⇔ the pruning-point import multiset
(consensus/src/consensus/mod.rs:1139-1152, processor.rs:1525-1538) and the
per-block invariant of verify_expected_utxo_state (utxo_validation.rs:188-195).

The reference is independent of the engine: each element is the oracle's
ok_muhash_element over the write_utxo serialisation written out here
(consensus/core/src/muhash.rs:55-69), products are Python integers mod P.
Partials are compared as integers mod P (a partial need not be canonical), and
the 32-byte kv_muhash_finalize result against ok_muhash_finalize."""
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


def rand_op(rng):
    return rng.randbytes(32) + struct.pack("<I", rng.randrange(8))


def rand_entry(rng, spk_len=None):
    if spk_len is None:
        # mostly standard 34/35-byte scripts, a few short, a few in the arena
        spk_len = rng.choice([34] * 10 + [35] * 5 + [0, 20, 36, 37, 150, 400])
    return Entry(rng.randrange(1 << 50), rng.randrange(1 << 40),
                 rng.random() < 0.1, rng.randbytes(spk_len))


def special_items(rng):
    """one entry for each script length of the issue's list"""
    return [(rand_op(rng), rand_entry(rng, ln)) for ln in SPK_LENS]


def mixed_items(seed=11, n_random=5000):
    rng = random.Random(seed)
    items = [(rand_op(rng), rand_entry(rng)) for _ in range(n_random)]
    items += special_items(rng)
    assert len({op for op, _ in items}) == len(items)
    return items


def load_mixed(engine):
    """case-3 table: 4 scan windows of slots, ~5,000 entries spread over them"""
    window = engine.utxo_commitment_window()
    reset(engine, 2 * window)  # capacity doubles into slots: 4 windows
    items = mixed_items()
    upsert(engine, items)
    return items, dict(items)


# ---------------- the cases ----------------

def test_empty_table(engine, oracle, golden):
    reset(engine, 64)
    partial, n_live, _ = engine.utxo_commitment()
    assert n_live == 0
    assert num(partial) == 1 and den(partial) == 1
    assert engine.muhash_finalize(partial) == bytes(
        golden("muhash.json")["empty_muhash"])


def test_never_reset_table(oracle, golden):
    from rusty_kaspa_amd.engine import Engine
    eng = Engine()
    try:
        partial, n_live, _ = eng.utxo_commitment()
        assert n_live == 0 and num(partial) == 1 and den(partial) == 1
    finally:
        eng.close()


@pytest.mark.parametrize("spk_len", [34, 10000])
def test_single_entry(engine, oracle, spk_len):
    rng = random.Random(spk_len)
    op, e = rand_op(rng), rand_entry(rng, spk_len)
    reset(engine, 64)
    upsert(engine, [(op, e)])
    partial = check_commitment(engine, oracle, {op: e})
    assert num(partial) % P == element(oracle, op, e) % P


def test_mixed_set_several_windows(engine, oracle):
    items, model = load_mixed(engine)
    sample = [op for op, e in items if len(e.spk) <= 36][:64]
    found0, ents0 = lookup(engine, sample)
    first = check_commitment(engine, oracle, model)
    second, n_live, _ = engine.utxo_commitment()
    assert second == first and n_live == len(model)
    # the scan is read-only
    found1, ents1 = lookup(engine, sample)
    assert found0 == found1 == [1] * len(sample)
    assert ents0 == ents1 == b"".join(model[op].pack() for op in sample)


def test_tombstones_and_overwrites(engine, oracle):
    items, model = load_mixed(engine)
    rng = random.Random(12)
    ops = [op for op, _ in items]
    removed = ops[::3]
    remove(engine, removed)
    for op in removed:
        del model[op]
    # overwrite 200 live keys with new values (some move to or from the arena)
    live = [op for op in ops if op in model]
    rewrites = [(op, rand_entry(rng)) for op in rng.sample(live, 200)]
    upsert(engine, rewrites)
    model.update(rewrites)
    # re-insert 100 removed keys
    back = [(op, rand_entry(rng)) for op in rng.sample(removed, 100)]
    upsert(engine, back)
    model.update(back)
    # remove one arena entry
    arena_op = next(op for op, e in model.items() if len(e.spk) > 36)
    remove(engine, [arena_op])
    del model[arena_op]
    check_commitment(engine, oracle, model)


def test_block_invariant(engine, oracle):
    """C(after block) == combine(C(before), block partial), the invariant of
    verify_expected_utxo_state, on a block that includes invalid txs."""
    n = 60
    blob, _ = gen_block(oracle, seed=22, n_txs=n, pct_multi_input=25,
                        pct_ecdsa=10, pct_multisig=10, pct_invalid=15)
    stripped, seeds = strip_utxo_entries(blob)
    reset(engine, max(64, 2 * len(seeds)))
    rc = engine.lib.kv_utxo_upsert(
        ctypes.c_void_p(engine.ctx), b"".join(op for op, _ in seeds),
        b"".join(e for _, e in seeds), ctypes.c_size_t(len(seeds)))
    assert rc == 0, engine.lib.kv_last_error().decode()
    c0, n0, _ = engine.utxo_commitment()
    assert n0 == len({op for op, _ in seeds})
    codes, _, block_partial = engine.validate_block_utxo(
        stripped, n, 10**9, 10**9, SKIP_MASS, apply_diff=True)
    assert any(c != 0 for c in codes) and any(c == 0 for c in codes)
    acc = bytearray(c0)
    engine.muhash_combine(acc, block_partial)
    c1, n1, _ = engine.utxo_commitment()
    assert c1 != c0 and n1 > 0
    assert engine.muhash_finalize(bytes(acc)) == engine.muhash_finalize(c1)
    assert num(bytes(acc)) * den(c1) % P == num(c1) * den(bytes(acc)) % P


def identity_partial():
    one = (1).to_bytes(384, "little")
    return bytearray(one + one)


def test_import_chunks(engine, oracle):
    rng = random.Random(13)
    reset(engine, 4096)
    acc = identity_partial()
    model, want = {}, 1
    chunks = [[(rand_op(rng), rand_entry(rng, rng.choice([0, 34, 35, 36])))
               for _ in range(size)] for size in (1, 63, 64, 65, 1000, 0)]
    chunks.append(special_items(rng) + [(rand_op(rng), rand_entry(rng))
                                        for _ in range(30)])
    for chunk in chunks:
        ops, ents, blob = chunk_args(chunk)
        engine.utxo_import_chunk(ops, ents, blob, len(chunk), acc)
        for op, e in chunk:
            assert op not in model
            model[op] = e
            want = want * element(oracle, op, e) % P
        assert num(bytes(acc)) % P == want, len(chunk)
        assert den(bytes(acc)) == 1
    partial = check_commitment(engine, oracle, model)
    assert num(partial) % P == num(bytes(acc)) % P
    assert engine.muhash_finalize(bytes(acc)) == oracle_finalize(oracle, want)
    # every imported outpoint is in the table with its script
    ops = list(model)
    found, ents, spks = lookup_spk(engine, ops, spk_cap=1 << 16)
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


def test_import_leaves_denominator_and_counts_duplicates(engine, oracle):
    """The denominator half passes through untouched; an outpoint imported
    twice is counted twice in the multiset and stored once (write_many
    overwrites in the reference too)."""
    rng = random.Random(14)
    reset(engine, 64)
    op = rand_op(rng)
    e1, e2 = rand_entry(rng, 34), rand_entry(rng, 100)
    d0 = rng.getrandbits(3000)
    n0 = rng.getrandbits(3000)
    acc = bytearray(n0.to_bytes(384, "little") + d0.to_bytes(384, "little"))
    for e in (e1, e2):
        ops, ents, blob = chunk_args([(op, e)])
        engine.utxo_import_chunk(ops, ents, blob, 1, acc)
    want = n0 * element(oracle, op, e1) * element(oracle, op, e2) % P
    assert num(bytes(acc)) % P == want
    assert den(bytes(acc)) == d0
    check_commitment(engine, oracle, {op: e2})
