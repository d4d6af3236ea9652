"""The host-compilable functions of kv_utxo_changes_kernels.hip, run ON CPU
from the device source (tests/host_shim/utxo_changes.cpp, g++):
utxo_change_locate maps a change index of a journal record to (row, source,
label), utxo_change_pack makes the 96-byte change record of
kv_utxo_changes_by_spk from an outpoint and a packed 64-byte value. Both are
checked against restatements in Python. The same kinds of cases run once more
as a stand-alone program under -fsanitize=address,undefined."""
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

F_COINBASE, F_ARENA, F_COVENANT, F_REMOVED = 1, 2, 4, 0x8000
REVERSED, ALL = 1, 2
SIZES = [0, 1, 2, 63, 64, 65]


def _build(out, extra):
    srcs = [os.path.join(SHIM_DIR, "utxo_changes.cpp"),
            os.path.join(SHIM_DIR, "shim.h"),
            os.path.join(CSRC, "kv_utxo_changes_kernels.hip"),
            os.path.join(INCLUDE, "kaspa_engine_abi.h")]
    if (not os.path.exists(out)
            or os.path.getmtime(out) < max(os.path.getmtime(p) for p in srcs)):
        tmp = f"{out}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O1", *extra, "-I", CSRC, "-I", SHIM_DIR,
                        "-I", INCLUDE, srcs[0], "-o", tmp], check=True)
        os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def shim():
    return ctypes.CDLL(_build(os.path.join(SHIM_DIR, "libutxochangesshim.so"),
                              ["-fPIC", "-shared"]))


# ---------------- the change-index mapping ----------------

def model_locate(c, n_removed, n_added, flags):
    """(row, live, removed) of change index c, from the table in
    kaspa_engine_abi.h"""
    assert 0 <= c < n_removed + 2 * n_added
    if c < n_removed:
        row, live = c, 0
    else:
        row, live = n_removed + (c - n_removed) // 2, (c - n_removed) % 2
    left_the_set = not live  # record-sourced values are what the diff took out
    if flags & REVERSED:
        left_the_set = not left_the_set
    return row, live, int(left_the_set)


@pytest.mark.parametrize("flags", [0, REVERSED, ALL, REVERSED | ALL])
def test_locate_equals_restatement(shim, flags):
    out = (ctypes.c_uint64 * 3)()
    checked = 0
    for n_removed in SIZES:
        for n_added in SIZES:
            end = n_removed + 2 * n_added
            rows = []
            for c in range(end):  # every index, cursor_end - 1 included
                shim.host_utxo_change_locate(ctypes.c_uint64(c),
                                             ctypes.c_uint64(n_removed),
                                             ctypes.c_uint32(flags), out)
                assert tuple(out) == model_locate(c, n_removed, n_added, flags), \
                    (c, n_removed, n_added)
                rows.append((out[0], out[1]))
                checked += 1
            # every removed row once, every added row once per source
            want = [(i, 0) for i in range(n_removed)]
            want += [(n_removed + k, s) for k in range(n_added) for s in (0, 1)]
            assert rows == want
    assert checked == sum(r + 2 * a for r in SIZES for a in SIZES)


def test_labels_forward_and_reversed(shim):
    out = (ctypes.c_uint64 * 3)()

    def label(c, flags):
        shim.host_utxo_change_locate(ctypes.c_uint64(c), ctypes.c_uint64(3),
                                     ctypes.c_uint32(flags), out)
        return out[2]
    # 3 removed rows, then added rows: overwritten value, live value
    assert [label(c, 0) for c in range(7)] == [1, 1, 1, 1, 0, 1, 0]
    assert [label(c, REVERSED) for c in range(7)] == [0, 0, 0, 0, 1, 0, 1]
    # indices far above 2^32 stay exact
    big = (1 << 40) + 5
    shim.host_utxo_change_locate(ctypes.c_uint64(big + 2 * 9 + 1),
                                 ctypes.c_uint64(big), ctypes.c_uint32(0), out)
    assert tuple(out) == (big + 9, 1, 0)


# ---------------- the 96-byte record ----------------

def table_value(rng, spk_len, version=0, coinbase=False, arena=False, covenant=False):
    """a packed 64-byte value as the table or a journal record holds it; the
    script field, the id and the tail are random bytes"""
    flags = (F_COINBASE if coinbase else 0) | (F_ARENA if arena or covenant else 0) \
        | (F_COVENANT if covenant else 0)
    return struct.pack("<QQHHI", rng.randrange(1 << 64), rng.randrange(1 << 64),
                       flags, version, spk_len) + rng.randbytes(40)


def model_record(op36, val64, query_index, removed):
    amount, daa, flags, version, spk_len = struct.unpack_from("<QQHHI", val64)
    out_flags = (flags & (F_COINBASE | F_COVENANT)) | (F_REMOVED if removed else 0)
    cov = val64[28:60] if flags & F_COVENANT else bytes(32)
    return op36 + struct.pack("<IQQHHI", query_index, amount, daa, out_flags,
                              version, spk_len) + cov


CASES = [
    dict(spk_len=0), dict(spk_len=1), dict(spk_len=35), dict(spk_len=36),
    dict(spk_len=37, arena=True), dict(spk_len=10000, arena=True, version=3),
    dict(spk_len=5, covenant=True), dict(spk_len=0, covenant=True, coinbase=True),
    dict(spk_len=34, coinbase=True), dict(spk_len=34, version=0xfffe),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_pack_equals_python_packer(shim, case):
    rng = random.Random(5100 + case)
    for removed in (0, 1):
        for query_index in (0, 1, 65535, 0xFFFFFFFF):
            op = rng.randbytes(36)
            val = table_value(rng, **CASES[case])
            out = (ctypes.c_uint8 * 96)(*[0xA5] * 96)
            shim.host_utxo_change_pack(op, val, ctypes.c_uint32(query_index),
                                       ctypes.c_int(removed), out)
            got = bytes(out)
            assert got == model_record(op, val, query_index, removed)
            flags, = struct.unpack_from("<H", got, 56)
            assert not flags & F_ARENA  # the arena bit is cleared
            assert bool(flags & F_REMOVED) == bool(removed)
            assert bool(flags & F_COINBASE) == bool(CASES[case].get("coinbase"))
            if CASES[case].get("covenant"):
                assert flags & F_COVENANT and got[64:] == val[28:60]
            else:
                assert got[64:] == bytes(32)


def test_record_extends_the_find_record(shim):
    """bytes 0..58 and 64..96 are the match record of kv_utxo_find_by_spk for
    an entry that is not labelled removed"""
    rng = random.Random(52)
    op, val = rng.randbytes(36), table_value(rng, 20, covenant=True, coinbase=True)
    out = (ctypes.c_uint8 * 96)()
    shim.host_utxo_change_pack(op, val, ctypes.c_uint32(9), ctypes.c_int(0), out)
    amount, daa = struct.unpack_from("<QQ", val)
    find = op + struct.pack("<IQQH", 9, amount, daa, F_COINBASE | F_COVENANT) \
        + bytes(6) + val[28:60]
    got = bytes(out)
    assert got[:58] == find[:58] and got[64:] == find[64:]
    assert got[58:64] == struct.pack("<HI", 0, 20)


def test_standalone_program_under_host_sanitizers():
    prog = _build(os.path.join(SHIM_DIR, "utxo_changes_san"),
                  ["-g", "-fsanitize=address,undefined",
                   "-fno-sanitize-recover=undefined", "-DKV_UTXO_CHANGES_MAIN"])
    out = subprocess.run([prog], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 bad" in out.stdout
