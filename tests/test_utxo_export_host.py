"""utxo_value_export (kv_utxo_rehash_kernels.hip), run ON CPU from the device
source (tests/host_shim/utxo_export.cpp, g++): a packed 64-byte table value
becomes the record kv_utxo_upsert_spk / kv_utxo_import_chunk take. Inline
values pass through unchanged; an arena value loses KV_UTXO_F_SPK_ARENA and has
its 36-byte script field zeroed, with its length and arena offset reported."""
import ctypes
import os
import random
import struct
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_DIR = os.path.join(REPO, "tests", "host_shim")
CSRC = os.path.join(REPO, "rusty_kaspa_amd", "csrc")
INCLUDE = os.path.join(REPO, "include")
LIB = os.path.join(SHIM_DIR, "libutxoexportshim.so")

F_COINBASE, F_ARENA = 1, 2
SPK_LENS = [0, 1, 35, 36, 37, 64, 65, 66, 193, 10000]


def build_export_shim():
    srcs = [os.path.join(SHIM_DIR, f) for f in ("utxo_export.cpp", "shim.h")]
    srcs.append(os.path.join(CSRC, "kv_utxo_rehash_kernels.hip"))
    srcs.append(os.path.join(INCLUDE, "kaspa_engine_abi.h"))
    if (not os.path.exists(LIB)
            or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in srcs)):
        tmp = f"{LIB}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O1", "-fPIC", "-shared", "-I", CSRC,
                        "-I", SHIM_DIR, "-I", INCLUDE, srcs[0], "-o", tmp],
                       check=True)
        os.replace(tmp, LIB)
    return ctypes.CDLL(LIB)


@pytest.fixture(scope="module")
def shim():
    return build_export_shim()


def entry_pack(amount, daa, coinbase, spk_version, spk):
    """the 64-byte record handed to kv_utxo_upsert_spk (Entry.pack() of the
    GPU tests)"""
    head = struct.pack("<QQHHI", amount, daa, F_COINBASE if coinbase else 0,
                       spk_version, len(spk))
    inline = spk.ljust(36, b"\0") if len(spk) <= 36 else bytes(36)
    return head + inline + bytes(4)


def table_value(amount, daa, coinbase, spk_version, spk, arena_off, tail):
    """the packed 64-byte value as utxo_upsert_spk_nolock stores it: a long
    script's field is the u32 arena offset followed by zeros"""
    flags = F_COINBASE if coinbase else 0
    if len(spk) <= 36:
        field = spk.ljust(36, b"\0")
    else:
        flags |= F_ARENA
        field = struct.pack("<I", arena_off) + tail
    return struct.pack("<QQHHI", amount, daa, flags, spk_version, len(spk)) \
        + field + bytes(4)


def export(shim, value64):
    buf = (ctypes.c_uint8 * 64).from_buffer_copy(value64)
    ln, off = ctypes.c_uint32(0xdeadbeef), ctypes.c_uint32(0xdeadbeef)
    is_arena = shim.host_utxo_value_export(buf, ctypes.byref(ln), ctypes.byref(off))
    return is_arena, bytes(buf), ln.value, off.value


@pytest.mark.parametrize("spk_len", [n for n in SPK_LENS if n <= 36])
def test_inline_values_unchanged(shim, spk_len):
    rng = random.Random(spk_len)
    for coinbase in (False, True):
        val = table_value(rng.getrandbits(64), rng.getrandbits(64), coinbase,
                          rng.getrandbits(16), rng.randbytes(spk_len), 0, b"")
        is_arena, out, ln, off = export(shim, val)
        assert is_arena == 0 and out == val
        assert ln == spk_len and off == 0


@pytest.mark.parametrize("spk_len", [n for n in SPK_LENS if n > 36])
def test_arena_values(shim, spk_len):
    rng = random.Random(spk_len)
    for coinbase in (False, True):
        for arena_off in (0, 1, 13, 65537, 0xFFFFFFFF - spk_len):
            amount, daa = rng.getrandbits(64), rng.getrandbits(64)
            ver, spk = rng.getrandbits(16), rng.randbytes(spk_len)
            # the bytes after the offset are zero as stored; the conversion
            # must zero the field even if they were not
            for tail in (bytes(32), rng.randbytes(32)):
                val = table_value(amount, daa, coinbase, ver, spk, arena_off, tail)
                is_arena, out, ln, off = export(shim, val)
                assert is_arena == 1
                assert (ln, off) == (spk_len, arena_off)
                flags, = struct.unpack_from("<H", out, 16)
                assert not flags & F_ARENA
                assert flags & F_COINBASE == (F_COINBASE if coinbase else 0)
                assert out[24:60] == bytes(36)
                assert out == entry_pack(amount, daa, coinbase, ver, spk)


def test_random_entries_equal_entry_pack(shim):
    rng = random.Random(77)
    for _ in range(500):
        spk_len = rng.choice([34] * 10 + [35] * 5 + SPK_LENS + [150, 400])
        amount, daa = rng.randrange(1 << 50), rng.randrange(1 << 40)
        coinbase, spk = rng.random() < 0.1, rng.randbytes(spk_len)
        arena_off = rng.randrange(1 << 32)
        val = table_value(amount, daa, coinbase, 0, spk, arena_off, bytes(32))
        is_arena, out, ln, off = export(shim, val)
        assert out == entry_pack(amount, daa, coinbase, 0, spk)
        assert ln == spk_len
        assert is_arena == (spk_len > 36)
        assert off == (arena_off if spk_len > 36 else 0)


def test_unknown_flag_bits_survive(shim):
    """only KV_UTXO_F_SPK_ARENA is cleared"""
    val = bytearray(table_value(1, 2, True, 3, bytes(100), 40, bytes(32)))
    struct.pack_into("<H", val, 16, 0xFFFF)
    _, out, _, _ = export(shim, bytes(val))
    assert struct.unpack_from("<H", out, 16)[0] == 0xFFFF & ~F_ARENA
