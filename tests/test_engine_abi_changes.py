"""CPU-side check that the built engine library exports
kv_utxo_changes_by_spk (include/kaspa_engine_abi.h), with its flags and
kv_utxo_changes_result declared as the Python wrapper mirrors them. No compute
calls here; the behaviour is tested on the GPU in test_gpu_utxo_changes.py."""
import ctypes
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(REPO, "rusty_kaspa_amd", "libkaspa_gpu.so")
HEADER = os.path.join(REPO, "include", "kaspa_engine_abi.h")

FIELDS = ["cursor_end", "added_amount", "removed_amount", "n_added", "n_removed",
          "n_added_gone", "kernel_ms"]


@pytest.fixture(scope="module")
def engine_lib():
    import __graft_entry__
    __graft_entry__.build()
    return ctypes.CDLL(SO)


def test_changes_symbol_exported(engine_lib):
    assert hasattr(engine_lib, "kv_utxo_changes_by_spk"), \
        "kv_utxo_changes_by_spk missing from libkaspa_gpu.so"


def test_changes_items_declared():
    hdr = open(HEADER).read()
    assert re.search(r"^int kv_utxo_changes_by_spk\(kv_ctx \*ctx, uint64_t token, "
                     r"uint32_t flags,$", hdr, re.M)
    assert re.search(r"^#define KV_UTXO_CHANGES_REVERSED 1u\b", hdr, re.M)
    assert re.search(r"^#define KV_UTXO_CHANGES_ALL +2u\b", hdr, re.M)
    assert re.search(r"^#define KV_UTXO_CHANGE_F_REMOVED 0x8000u\b", hdr, re.M)
    assert re.search(r"^typedef struct kv_utxo_changes_result \{", hdr, re.M)
    assert re.search(r"^\} kv_utxo_changes_result;", hdr, re.M)
    # declared after the journal section it reads
    assert hdr.index("int kv_utxo_journal_stats(") < \
        hdr.index("int kv_utxo_changes_by_spk(") < \
        hdr.index("int kv_validate_block_utxo(")


def test_struct_and_flags_as_compiled(tmp_path):
    """the header through a C compiler: sizeof and the field offsets of
    kv_utxo_changes_result and the three macros are what the ctypes mirror
    assumes"""
    offsets = ",\n  ".join(f"offsetof(kv_utxo_changes_result, {f})" for f in FIELDS)
    src = tmp_path / "c.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "kaspa_engine_abi.h"\n'
        'int main(void) { printf("%zu' + " %zu" * len(FIELDS) + ' %u %u %u\\n",\n'
        "  sizeof(kv_utxo_changes_result),\n  " + offsets + ",\n"
        "  KV_UTXO_CHANGES_REVERSED, KV_UTXO_CHANGES_ALL, KV_UTXO_CHANGE_F_REMOVED);\n"
        "  return 0; }\n")
    exe = tmp_path / "c"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o",
                    str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True)
    got = [int(x) for x in out.stdout.split()]
    from rusty_kaspa_amd import engine as E
    R = E.KvUtxoChangesResult
    assert [name for name, _ in R._fields_] == FIELDS
    assert got[0] == ctypes.sizeof(R) == 56
    assert got[1:1 + len(FIELDS)] == [getattr(R, f).offset for f in FIELDS] \
        == [8 * i for i in range(len(FIELDS))]
    assert got[-3:] == [E.KV_UTXO_CHANGES_REVERSED, E.KV_UTXO_CHANGES_ALL,
                        E.KV_UTXO_CHANGE_F_REMOVED] == [1, 2, 0x8000]
    assert E.KV_UTXO_CHANGE_BYTES == 96


def test_changes_call_refuses_a_null_context(engine_lib):
    """the context is checked before anything else: nothing is written"""
    from rusty_kaspa_amd.engine import KvUtxoChangesResult
    engine_lib.kv_last_error.restype = ctypes.c_char_p
    z = ctypes.c_size_t(0)
    cur, n = ctypes.c_uint64(5), ctypes.c_size_t(9)
    res = KvUtxoChangesResult(11, 12, 13, 14, 15, 16, -1.0)
    out = (ctypes.c_uint8 * 96)(*[0xA5] * 96)
    rc = engine_lib.kv_utxo_changes_by_spk(
        None, ctypes.c_uint64(1), ctypes.c_uint32(0), ctypes.byref(cur), None, z,
        None, z, ctypes.c_size_t(1), out, None, z, None, ctypes.byref(n),
        ctypes.byref(res))
    assert rc == -1
    assert b"null ctx" in engine_lib.kv_last_error()
    assert (cur.value, n.value) == (5, 9)
    assert [getattr(res, f) for f in FIELDS] == [11, 12, 13, 14, 15, 16, -1.0]
    assert bytes(out) == b"\xa5" * 96
