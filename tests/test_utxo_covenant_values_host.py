"""The table-value functions on values that carry a covenant id
(KV_UTXO_F_COVENANT: id in bytes 28..60, script always in the arena), run ON
CPU from the device sources through the existing shims utxo_element.cpp,
utxo_export.cpp and utxo_journal.cpp.

The element reference is covenant_model.utxo_element: write_utxo with the id
appended (consensus/core/src/muhash.rs:55-69), keyed BLAKE2b and ChaCha20
restated in Python. The model is itself pinned to the oracle's
ok_muhash_element on the serialisation, which knows nothing of covenants."""
import ctypes
import os
import random
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import covenant_model as M  # noqa: E402
from covenant_model import B, F_ARENA, F_COINBASE, F_COVENANT  # noqa: E402
from test_utxo_element_host import build_element_shim  # noqa: E402
from test_utxo_export_host import build_export_shim  # noqa: E402
from test_utxo_journal_host import build_journal_shim  # noqa: E402

U = ctypes.c_uint64 * 48
SPK_LENS = [0, 1, 36, 37, 300]
SET, REBASE = 0, 1


@pytest.fixture(scope="module")
def elem():
    return build_element_shim()


@pytest.fixture(scope="module")
def exp():
    return build_export_shim()


@pytest.fixture(scope="module")
def jrn():
    return build_journal_shim()


def covenant_value(u, arena_off):
    """The 64-byte value as the table holds a covenant entry."""
    flags = (F_COINBASE if u["is_coinbase"] else 0) | F_ARENA | F_COVENANT
    return struct.pack("<QQHHII", u["amount"], u["daa_score"], flags,
                       u["spk_version"], len(u["spk"]), arena_off) \
        + u["covenant_id"] + bytes(4)


def plain_value(u, arena_off):
    """The same entry without the id, as the table holds it."""
    flags = F_COINBASE if u["is_coinbase"] else 0
    head = struct.pack("<QQHH", u["amount"], u["daa_score"],
                       flags | (F_ARENA if len(u["spk"]) > 36 else 0),
                       u["spk_version"]) + struct.pack("<I", len(u["spk"]))
    if len(u["spk"]) <= 36:
        return head + u["spk"].ljust(36, b"\0") + bytes(4)
    return head + struct.pack("<I", arena_off) + bytes(36)


def shim_element(elem, op, val, arena):
    out = U()
    elem.host_utxo_entry_element(op, val, arena, out)
    return sum(int(out[i]) << (64 * i) for i in range(48))


def test_model_element_matches_oracle(oracle):
    rng = random.Random(11)
    for n in (0, 65, 200):
        data = rng.randbytes(n)
        out = U()
        oracle.ok_muhash_element(data, ctypes.c_size_t(n), out)
        assert M.element_of(data) == sum(int(out[i]) << (64 * i) for i in range(48))


@pytest.mark.parametrize("spk_len", SPK_LENS)
def test_element_appends_the_id(elem, spk_len):
    rng = random.Random(100 + spk_len)
    for coinbase in (False, True):
        op = rng.randbytes(36)
        u = B.utxo_entry(rng.getrandbits(64), rng.randbytes(spk_len),
                         rng.getrandbits(64), coinbase, rng.getrandbits(16),
                         rng.randbytes(32))
        # the script sits at an unaligned arena offset between other bytes
        arena = rng.randbytes(13) + u["spk"] + rng.randbytes(7)
        val = covenant_value(u, 13)
        assert elem.host_utxo_value_spk_ok(val, ctypes.c_uint64(len(arena))) == 1
        got = shim_element(elem, op, val, arena)
        assert got == M.utxo_element(op, u)
        # and it is not the element of the entry without the id
        bare = dict(u, covenant_id=None)
        assert M.utxo_element(op, bare) != got
        assert shim_element(elem, op, plain_value(bare, 13), arena) \
            == M.utxo_element(op, bare)


def test_spk_ok_refuses_the_flag_without_the_arena(elem):
    ok = lambda v, n: elem.host_utxo_value_spk_ok(v, ctypes.c_uint64(n))
    rng = random.Random(12)
    for spk_len in (0, 1, 36):
        u = B.utxo_entry(5, rng.randbytes(spk_len), 6, covenant_id=rng.randbytes(32))
        good = bytearray(covenant_value(u, 0))
        assert ok(bytes(good), spk_len) == 1
        assert ok(bytes(good), 1 << 20) == 1
        bad = bytearray(good)
        struct.pack_into("<H", bad, 16, F_COVENANT)
        assert ok(bytes(bad), 1 << 20) == 0
    # an arena reference is still checked against the used prefix
    u = B.utxo_entry(5, bytes(10), 6, covenant_id=bytes(32))
    assert ok(covenant_value(u, 50), 60) == 1
    assert ok(covenant_value(u, 50), 59) == 0


@pytest.mark.parametrize("spk_len", SPK_LENS)
def test_export_keeps_flag_and_id(exp, spk_len):
    rng = random.Random(200 + spk_len)
    for coinbase in (False, True):
        for arena_off in (0, 13, 0xFFFFFFFF - spk_len):
            u = B.utxo_entry(rng.getrandbits(64), rng.randbytes(spk_len),
                             rng.getrandbits(64), coinbase, rng.getrandbits(16),
                             rng.randbytes(32))
            buf = (ctypes.c_uint8 * 64).from_buffer_copy(covenant_value(u, arena_off))
            ln, off = ctypes.c_uint32(0xdeadbeef), ctypes.c_uint32(0xdeadbeef)
            assert exp.host_utxo_value_export(buf, ctypes.byref(ln),
                                              ctypes.byref(off)) == 1
            assert (ln.value, off.value) == (spk_len, arena_off)
            # exactly the record pack_utxo_entries makes for upsert_spk
            ents, spk_blob = B.pack_utxo_entries([u])
            assert bytes(buf) == ents and spk_blob == u["spk"]
            flags, = struct.unpack_from("<H", ents, 16)
            assert flags == F_COVENANT | (F_COINBASE if coinbase else 0)
            assert ents[24:28] == bytes(4) and ents[28:60] == u["covenant_id"]


@pytest.mark.parametrize("spk_len", SPK_LENS)
def test_journal_rewrite_leaves_the_id(jrn, spk_len):
    rng = random.Random(300 + spk_len)
    u = B.utxo_entry(rng.getrandbits(64), rng.randbytes(spk_len),
                     rng.getrandbits(64), False, 3, rng.randbytes(32))
    val = covenant_value(u, 1000)

    def rewrite(v, mode, add, src_len, dst_len):
        buf = (ctypes.c_uint8 * 64).from_buffer_copy(v)
        off, ln = ctypes.c_uint32(), ctypes.c_uint32()
        rc = jrn.host_utxo_value_journal_rewrite(
            buf, ctypes.c_int(mode), ctypes.c_uint64(add), ctypes.c_uint64(src_len),
            ctypes.c_uint64(dst_len), ctypes.byref(off), ctypes.byref(ln))
        return rc, bytes(buf), off.value, ln.value

    # capture: arena offset 1000 -> blob cursor 77
    rc, cap, off, ln = rewrite(val, SET, 77, 1000 + spk_len, 0xFFFFFFFF)
    assert (rc, off, ln) == (1, 1000, spk_len)
    assert cap == val[:24] + struct.pack("<I", 77) + val[28:]
    # revert: blob offset 77 -> 5000 + 77 in the live arena
    rc, back, off, ln = rewrite(cap, REBASE, 5000, 77 + spk_len, 5077 + spk_len)
    assert (rc, off, ln) == (1, 77, spk_len)
    assert back == val[:24] + struct.pack("<I", 5077) + val[28:]
    assert back[28:60] == u["covenant_id"]
