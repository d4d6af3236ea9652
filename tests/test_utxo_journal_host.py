"""utxo_value_journal_rewrite (kv_utxo_journal_kernels.hip), run ON CPU from the
device source (tests/host_shim/utxo_journal.cpp, g++): the one rule by which an
undo record's copy of a table value has its script reference rewritten — live
arena offset to record-blob offset when kv_utxo_apply_diff captures it, and
back to an arena offset when kv_utxo_revert restores it. Checked against a
Python restatement: inline values are untouched, arena values map there and
back with the flag and every other byte preserved, and a reference outside its
source is refused (fail word set, nothing rewritten, nothing dereferenced)."""
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
LIB = os.path.join(SHIM_DIR, "libutxojournalshim.so")

F_COINBASE, F_ARENA = 1, 2
MAX_SPK = 10000
U32_MAX = 0xFFFFFFFF
U64_MAX = 2**64 - 1
SET, REBASE = 0, 1
SPK_LENS = [0, 1, 35, 36, 37, 64, 200, 10000]
OFFSETS = [0, 1, 2**32 - 10001]


def build_journal_shim():
    srcs = [os.path.join(SHIM_DIR, f) for f in ("utxo_journal.cpp", "shim.h")]
    srcs.append(os.path.join(CSRC, "kv_utxo_journal_kernels.hip"))
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
    return build_journal_shim()


def table_value(rng, spk_len, arena_off=0, coinbase=False, tail=bytes(32)):
    """the packed 64-byte value as the table stores it"""
    flags = F_COINBASE if coinbase else 0
    if spk_len <= 36:
        field = rng.randbytes(spk_len).ljust(36, b"\0")
    else:
        flags |= F_ARENA
        field = struct.pack("<I", arena_off) + tail
    return struct.pack("<QQHHI", rng.getrandbits(64), rng.getrandbits(64), flags,
                       rng.getrandbits(16), spk_len) + field + rng.randbytes(4)


def model_rewrite(val, mode, add, src_len, dst_len):
    """the rule restated: (return code, value after, old offset, length)"""
    flags, = struct.unpack_from("<H", val, 16)
    ln, = struct.unpack_from("<I", val, 20)
    if not flags & F_ARENA:
        return (0 if ln <= 36 else -1), val, 0, ln
    off, = struct.unpack_from("<I", val, 24)
    if ln > MAX_SPK or off + ln > src_len:
        return -1, val, off, ln
    now = add + off if mode == REBASE else add
    if now >= 2**64 or now + ln > dst_len or now + ln > U32_MAX:
        return -1, val, off, ln
    return 1, val[:24] + struct.pack("<I", now) + val[28:], off, ln


def rewrite(shim, val, mode, add, src_len, dst_len):
    buf = (ctypes.c_uint8 * 64).from_buffer_copy(val)
    off, ln = ctypes.c_uint32(0xdeadbeef), ctypes.c_uint32(0xdeadbeef)
    rc = shim.host_utxo_value_journal_rewrite(
        buf, ctypes.c_int(mode), ctypes.c_uint64(add), ctypes.c_uint64(src_len),
        ctypes.c_uint64(dst_len), ctypes.byref(off), ctypes.byref(ln))
    return rc, bytes(buf), off.value, ln.value


@pytest.mark.parametrize("spk_len", [n for n in SPK_LENS if n <= 36])
def test_inline_values_untouched(shim, spk_len):
    rng = random.Random(spk_len)
    for coinbase in (False, True):
        for mode in (SET, REBASE):
            val = table_value(rng, spk_len, coinbase=coinbase)
            # no bound matters for an inline value, not even empty ones
            rc, out, off, ln = rewrite(shim, val, mode, 12345, 0, 0)
            assert (rc, out, off, ln) == (0, val, 0, spk_len)
            assert (rc, out, off, ln) == model_rewrite(val, mode, 12345, 0, 0)


@pytest.mark.parametrize("arena_off", OFFSETS)
@pytest.mark.parametrize("spk_len", [n for n in SPK_LENS if n > 36])
def test_arena_values_there_and_back(shim, spk_len, arena_off):
    """capture to each blob offset, then revert onto each arena base: the
    value that comes back is the captured one with base + blob offset, and
    when the base puts it where it was, the original byte for byte"""
    rng = random.Random(spk_len * 7 + arena_off % 1000)
    for coinbase in (False, True):
        val = table_value(rng, spk_len, arena_off, coinbase)
        arena_len = arena_off + spk_len  # the entry ends the used prefix
        for blob_off in OFFSETS:
            rc, rec, off, ln = rewrite(shim, val, SET, blob_off, arena_len, U32_MAX)
            assert (rc, rec, off, ln) == model_rewrite(val, SET, blob_off, arena_len,
                                                       U32_MAX)
            if blob_off + spk_len > U32_MAX:
                assert rc == -1 and rec == val
                continue
            assert rc == 1 and (off, ln) == (arena_off, spk_len)
            flags, = struct.unpack_from("<H", rec, 16)
            assert flags & F_ARENA  # the flag is preserved
            assert flags & F_COINBASE == (F_COINBASE if coinbase else 0)
            assert struct.unpack_from("<I", rec, 24)[0] == blob_off
            assert rec[:24] == val[:24] and rec[28:] == val[28:]
            blob_bytes = blob_off + spk_len
            for base in OFFSETS + [arena_off - blob_off]:
                if base < 0:
                    continue
                new_len = base + blob_bytes
                got = rewrite(shim, rec, REBASE, base, blob_bytes, new_len)
                assert got == model_rewrite(rec, REBASE, base, blob_bytes, new_len)
                rc2, back, off2, ln2 = got
                if base + blob_off + spk_len > U32_MAX:
                    assert rc2 == -1 and back == rec
                    continue
                assert rc2 == 1 and (off2, ln2) == (blob_off, spk_len)
                assert struct.unpack_from("<I", back, 24)[0] == base + blob_off
                assert back[:24] == val[:24] and back[28:] == val[28:]
                if base + blob_off == arena_off:
                    assert back == val


def test_random_values_match_the_model(shim):
    rng = random.Random(91)
    for _ in range(2000):
        spk_len = rng.choice([34] * 5 + SPK_LENS + [150, 400, 10001, 70000])
        off = rng.choice([0, 1, rng.randrange(1 << 20), rng.randrange(1 << 32)])
        val = table_value(rng, spk_len, off, rng.random() < 0.1, rng.randbytes(32))
        if rng.random() < 0.05:  # a long length without the flag, a short one with
            flags, = struct.unpack_from("<H", val, 16)
            val = val[:16] + struct.pack("<H", flags ^ F_ARENA) + val[18:]
        mode = rng.choice([SET, REBASE])
        add = rng.choice([0, 1, rng.randrange(1 << 32), 2**64 - 5])
        src_len = rng.choice([0, off + spk_len, off + spk_len - 1, 1 << 33])
        dst_len = rng.choice([0, U32_MAX, 1 << 33, min(add + off + spk_len, U64_MAX)])
        assert rewrite(shim, val, mode, add, max(src_len, 0), dst_len) == \
            model_rewrite(val, mode, add, max(src_len, 0), dst_len)


def test_out_of_range_reference_sets_the_fail_word(shim):
    """the capture kernel's guard: a script reference outside the arena's used
    prefix (the rule of utxo_value_spk_ok) sets the fail word and leaves the
    value as it was; one inside does neither"""
    rng = random.Random(92)

    def capture(val, cursor, arena_len):
        buf = (ctypes.c_uint8 * 64).from_buffer_copy(val)
        fail = ctypes.c_uint32(0)
        shim.host_journal_capture_value(buf, ctypes.c_uint64(cursor),
                                        ctypes.c_uint64(arena_len), ctypes.byref(fail))
        return fail.value, bytes(buf)

    good = table_value(rng, 200, 1000)
    fail, out = capture(good, 77, 1200)  # ends exactly at the used prefix
    assert fail == 0 and struct.unpack_from("<I", out, 24)[0] == 77
    assert capture(good, 77, 1199) == (1, good)  # one byte past it
    wild = table_value(rng, 200, U32_MAX)
    assert capture(wild, 0, 1 << 20) == (1, wild)
    too_long = table_value(rng, MAX_SPK + 1, 0)
    assert capture(too_long, 0, 1 << 20) == (1, too_long)
    # an inline value whose length does not fit the field
    bad_inline = bytearray(table_value(rng, 36))
    struct.pack_into("<I", bad_inline, 20, 37)
    assert capture(bytes(bad_inline), 0, 1 << 20) == (1, bytes(bad_inline))
    # a blob cursor that would push the span past a u32
    assert capture(good, U32_MAX - 100, 1200) == (1, good)
    inline = table_value(rng, 34)
    assert capture(inline, 0, 0) == (0, inline)
