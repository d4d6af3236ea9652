"""CPU-side check that the built engine library exports the undo journal's
entry points (include/kaspa_engine_abi.h): kv_utxo_apply_diff, kv_utxo_revert,
kv_utxo_journal_drop, kv_utxo_journal_stats, kv_validate_block_utxo_undo. No
compute calls here; the behaviour is tested on the GPU in
test_gpu_utxo_journal.py."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(REPO, "rusty_kaspa_amd", "libkaspa_gpu.so")

JOURNAL_SYMBOLS = ["kv_utxo_apply_diff", "kv_utxo_revert", "kv_utxo_journal_drop",
                   "kv_utxo_journal_stats", "kv_validate_block_utxo_undo"]


@pytest.fixture(scope="module")
def engine_lib():
    import __graft_entry__
    __graft_entry__.build()
    return ctypes.CDLL(SO)


@pytest.mark.parametrize("sym", JOURNAL_SYMBOLS)
def test_journal_symbol_exported(engine_lib, sym):
    assert hasattr(engine_lib, sym), f"{sym} missing from libkaspa_gpu.so"


def test_journal_symbols_declared():
    hdr = open(os.path.join(REPO, "include", "kaspa_engine_abi.h")).read()
    for sym in JOURNAL_SYMBOLS:
        assert re.search(r"^int %s\(kv_ctx \*ctx" % sym, hdr, re.M), sym


def test_journal_calls_refuse_a_null_context(engine_lib):
    """every entry point checks its context before anything else"""
    engine_lib.kv_last_error.restype = ctypes.c_char_p
    token = ctypes.c_uint64()
    assert engine_lib.kv_utxo_apply_diff(None, None, ctypes.c_size_t(0), None, None,
                                         None, ctypes.c_size_t(0), ctypes.c_size_t(0),
                                         None, ctypes.byref(token)) == -1
    assert b"null ctx" in engine_lib.kv_last_error()
    assert engine_lib.kv_utxo_revert(None, ctypes.c_uint64(1)) == -1
    assert engine_lib.kv_utxo_journal_drop(None, ctypes.c_uint64(1)) == -1
    assert engine_lib.kv_utxo_journal_stats(None, None) == -1
    assert engine_lib.kv_validate_block_utxo_undo(
        None, None, ctypes.c_size_t(0), ctypes.c_uint64(0), ctypes.c_uint64(0),
        ctypes.c_uint32(0), None, None, None, ctypes.byref(token)) == -1
