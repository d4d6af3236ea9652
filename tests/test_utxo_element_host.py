"""utxo_entry_element (kv_utxo_commit_kernels.hip), run ON CPU from the device
source (tests/host_shim/utxo_element.cpp, g++): a 36-byte outpoint, a packed
64-byte table value and the arena base must give exactly MuHash::from_utxo of
the entry (consensus/core/src/muhash.rs:55-69). The reference is the oracle's
ok_muhash_element over the write_utxo serialisation written out here."""
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
LIB = os.path.join(SHIM_DIR, "libutxoelemshim.so")

U = ctypes.c_uint64 * 48
F_COINBASE, F_ARENA = 1, 2
U64_MAX = 2**64 - 1


def build_element_shim():
    srcs = [os.path.join(SHIM_DIR, f) for f in ("utxo_element.cpp", "shim.h")]
    srcs += [os.path.join(CSRC, f) for f in ("kv_utxo_commit_kernels.hip",
                                             "kv_hash_device.h", "kv_u3072.h")]
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
    return build_element_shim()


def write_utxo(outpoint36, amount, daa, coinbase, spk_version, spk):
    """muhash.rs:55-69, byte for byte (no covenant id: the table stores none)."""
    tx_id, index = outpoint36[:32], struct.unpack("<I", outpoint36[32:])[0]
    return (tx_id + struct.pack("<I", index) + struct.pack("<Q", daa)
            + struct.pack("<Q", amount) + bytes([1 if coinbase else 0])
            + struct.pack("<H", spk_version) + struct.pack("<Q", len(spk)) + spk)


def oracle_element(oracle, data):
    out = U()
    oracle.ok_muhash_element(data, ctypes.c_size_t(len(data)), out)
    return list(out)


def table_value(amount, daa, coinbase, spk_version, spk, arena_off=None):
    """The packed 64-byte value as the table holds it."""
    flags = F_COINBASE if coinbase else 0
    if len(spk) <= 36:
        field = spk.ljust(36, b"\0")
    else:
        flags |= F_ARENA
        field = struct.pack("<I", arena_off) + bytes(32)
    return struct.pack("<QQHHI", amount, daa, flags, spk_version, len(spk)) \
        + field + bytes(4)


def shim_element(shim, outpoint36, value64, arena=b""):
    out = U()
    shim.host_utxo_entry_element(outpoint36, value64, arena, out)
    return list(out)


def check(shim, oracle, rng, spk_len, amount=12345, daa=678, coinbase=False,
          spk_version=0, index=1, arena_off=13):
    tx_id = bytes(rng.randrange(256) for _ in range(32))
    op = tx_id + struct.pack("<I", index)
    spk = bytes(rng.randrange(256) for _ in range(spk_len))
    # arena scripts sit at a non-zero offset that is not 16-byte aligned,
    # between unrelated bytes
    arena = b""
    if spk_len > 36:
        assert arena_off % 16 != 0
        arena = bytes(rng.randrange(256) for _ in range(arena_off)) + spk \
            + bytes(rng.randrange(256) for _ in range(7))
    val = table_value(amount, daa, coinbase, spk_version, spk, arena_off)
    assert len(val) == 64
    assert shim.host_utxo_value_spk_ok(val, ctypes.c_uint64(len(arena))) == 1
    want = oracle_element(
        oracle, write_utxo(op, amount, daa, coinbase, spk_version, spk))
    assert shim_element(shim, op, val, arena) == want, \
        (spk_len, amount, daa, coinbase, spk_version, index)


# 63 fixed bytes + script: 64/65/66 make 127/128/129-byte messages (one exact
# BLAKE2b block, where compressing a full final block early goes wrong), 193
# makes 256; 37 is the first arena length, 10,000 the longest script.
SPK_LENS = [0, 1, 35, 36, 37, 64, 65, 66, 193, 10000]


@pytest.mark.parametrize("spk_len", SPK_LENS)
def test_script_lengths(shim, oracle, spk_len):
    rng = random.Random(1000 + spk_len)
    assert len(write_utxo(bytes(36), 0, 0, False, 0, bytes(65))) == 128
    check(shim, oracle, rng, spk_len)


@pytest.mark.parametrize("spk_len", [34, 100])
def test_field_values(shim, oracle, spk_len):
    rng = random.Random(7 + spk_len)
    for coinbase in (False, True):
        check(shim, oracle, rng, spk_len, coinbase=coinbase)
    check(shim, oracle, rng, spk_len, spk_version=0x0102)
    for index in (0, 0xFFFFFFFF):
        check(shim, oracle, rng, spk_len, index=index)
    for amount in (0, U64_MAX):
        for daa in (0, U64_MAX):
            check(shim, oracle, rng, spk_len, amount=amount, daa=daa)
    # amount and daa_score are not interchangeable
    check(shim, oracle, rng, spk_len, amount=1, daa=2)
    check(shim, oracle, rng, spk_len, amount=2, daa=1)


def test_arena_offsets(shim, oracle):
    rng = random.Random(99)
    for off in (1, 7, 13, 4099, 65537):
        check(shim, oracle, rng, 300, arena_off=off)


def test_inline_padding_is_not_hashed(shim, oracle):
    """Bytes of the 36-byte slot beyond spk_len never reach the hash."""
    rng = random.Random(5)
    op = bytes(rng.randrange(256) for _ in range(36))
    spk = bytes(rng.randrange(256) for _ in range(20))
    val = bytearray(table_value(5, 6, False, 0, spk))
    val[24 + 20:24 + 36] = b"\xaa" * 16
    want = oracle_element(oracle, write_utxo(op, 5, 6, False, 0, spk))
    assert shim_element(shim, op, bytes(val)) == want


def test_script_reference_check(shim):
    """utxo_value_spk_ok: what the kernels refuse to dereference."""
    ok = lambda v, n: shim.host_utxo_value_spk_ok(v, ctypes.c_uint64(n))
    inline_bad = struct.pack("<QQHHI", 1, 1, 0, 0, 37) + bytes(40)
    assert ok(inline_bad, 1 << 20) == 0
    arena = table_value(1, 1, False, 0, bytes(100), arena_off=50)
    assert ok(arena, 150) == 1
    assert ok(arena, 149) == 0
    assert ok(arena, 0) == 0
    too_long = struct.pack("<QQHHI", 1, 1, F_ARENA, 0, 10001) + bytes(40)
    assert ok(too_long, 1 << 20) == 0
