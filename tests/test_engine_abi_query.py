"""CPU-side check that the built engine library exports the queries by script
public key (include/kaspa_engine_abi.h): kv_utxo_balance_by_spk and
kv_utxo_find_by_spk, with kv_spk_query and KV_UTXO_QUERY_MAX declared as the
Python wrapper mirrors them. No compute calls here; the behaviour is tested on
the GPU in test_gpu_utxo_query.py."""
import ctypes
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(REPO, "rusty_kaspa_amd", "libkaspa_gpu.so")
HEADER = os.path.join(REPO, "include", "kaspa_engine_abi.h")

QUERY_SYMBOLS = ["kv_utxo_balance_by_spk", "kv_utxo_find_by_spk"]


@pytest.fixture(scope="module")
def engine_lib():
    import __graft_entry__
    __graft_entry__.build()
    return ctypes.CDLL(SO)


@pytest.mark.parametrize("sym", QUERY_SYMBOLS)
def test_query_symbol_exported(engine_lib, sym):
    assert hasattr(engine_lib, sym), f"{sym} missing from libkaspa_gpu.so"


def test_query_items_declared():
    hdr = open(HEADER).read()
    for sym in QUERY_SYMBOLS:
        assert re.search(r"^int %s\(kv_ctx \*ctx" % sym, hdr, re.M), sym
    assert re.search(r"^#define KV_UTXO_QUERY_MAX 65536u$", hdr, re.M)
    assert re.search(r"^typedef struct kv_spk_query \{", hdr, re.M)
    assert re.search(r"^\} kv_spk_query;", hdr, re.M)


def test_struct_size_and_limit_as_compiled(tmp_path):
    """the header through a C compiler: sizeof(kv_spk_query) == 8, the field
    offsets and the limit are what the Python wrapper assumes"""
    src = tmp_path / "q.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "kaspa_engine_abi.h"\n'
        'int main(void) { printf("%zu %zu %zu %zu %u\\n", sizeof(kv_spk_query),\n'
        '  offsetof(kv_spk_query, spk_len), offsetof(kv_spk_query, spk_version),\n'
        '  offsetof(kv_spk_query, zero), KV_UTXO_QUERY_MAX); return 0; }\n')
    exe = tmp_path / "q"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o",
                    str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True)
    assert out.stdout.split() == ["8", "0", "4", "6", "65536"]
    from rusty_kaspa_amd.engine import KV_UTXO_QUERY_MAX, KvSpkQuery
    assert ctypes.sizeof(KvSpkQuery) == 8 and KV_UTXO_QUERY_MAX == 65536
    assert (KvSpkQuery.spk_len.offset, KvSpkQuery.spk_version.offset,
            KvSpkQuery.zero.offset) == (0, 4, 6)


def test_query_calls_refuse_a_null_context(engine_lib):
    """every entry point checks its context before anything else"""
    engine_lib.kv_last_error.restype = ctypes.c_char_p
    z = ctypes.c_size_t(0)
    assert engine_lib.kv_utxo_balance_by_spk(None, None, z, None, z, None, None,
                                             None, None, None) == -1
    assert b"null ctx" in engine_lib.kv_last_error()
    cur, n = ctypes.c_uint64(5), ctypes.c_size_t(9)
    assert engine_lib.kv_utxo_find_by_spk(None, ctypes.byref(cur), None, z, None, z,
                                          ctypes.c_size_t(1), None,
                                          ctypes.byref(n)) == -1
    assert b"null ctx" in engine_lib.kv_last_error()
    assert (cur.value, n.value) == (5, 9)
