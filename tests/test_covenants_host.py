"""check_covenant_info of phase 1 (kvh_check_covenant_info,
kv_validate_host.inc) and the covenant opcodes of the host interpreter
(kvs_exec_introspection, kv_script_host.inc), run ON CPU through g++ shims.

⇔ CovenantsContext::from_tx (crypto/txscript/src/covenants.rs:101-163) and its
accessors (:66-94). The scenarios are those of covenants.rs:277-451 rebuilt as
blobs; expected ids come from covenant_model.covenant_id, a restatement of
consensus/core/src/hashing/covenant_id.rs over hashlib. The oracle rejects
covenant outputs and is not consulted."""
import ctypes
import hashlib
import os
import random
import subprocess
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import covenant_model as M  # noqa: E402
from covenant_model import B  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_DIR = os.path.join(REPO, "tests", "host_shim")
CSRC = os.path.join(REPO, "rusty_kaspa_amd", "csrc")
INCLUDE = os.path.join(REPO, "include")

# TxScriptError codes of include/kaspa_engine_abi.h
SCRIPT_EVAL_FALSE = 1
SCRIPT_INVALID_SOURCE = 31  # the k-th index of a context does not exist


def build_shim(src_name, lib_name):
    src = os.path.join(SHIM_DIR, src_name)
    lib = os.path.join(SHIM_DIR, lib_name)
    deps = [src, os.path.join(CSRC, "kv_script_host.inc"),
            os.path.join(CSRC, "kv_validate_host.inc"),
            os.path.join(INCLUDE, "kaspa_engine_abi.h")]
    if (not os.path.exists(lib)
            or os.path.getmtime(lib) < max(os.path.getmtime(p) for p in deps)):
        tmp = f"{lib}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O1", "-fPIC", "-shared", "-I", INCLUDE,
                        "-I", CSRC, src, "-o", tmp], check=True)
        os.replace(tmp, lib)
    return ctypes.CDLL(lib)


@pytest.fixture(scope="module")
def cov():
    return build_shim("covenants.cpp", "libcovenantshim.so")


@pytest.fixture(scope="module")
def script():
    # the same build as test_host_interpreter.py's, of the unchanged shim
    return build_shim("script_main.cpp", "libscriptshim.so")


def check_code(cov, tx):
    blob = B.build_blob([tx])
    return cov.host_check_covenant_info(blob, ctypes.c_size_t(len(blob)), 0)


def test_covenant_id_restatement():
    """The model's id against the construction written out longhand, so a slip
    in the struct formats cannot hide in both the test and the engine."""
    tx_id, spk = bytes(range(32)), bytes(range(5))
    h = hashlib.blake2b(key=b"CovenantID", digest_size=32)
    h.update(tx_id)
    h.update((7).to_bytes(4, "little"))       # outpoint index u32
    h.update((1).to_bytes(8, "little"))       # number of outputs u64
    h.update((3).to_bytes(4, "little"))       # output index u32
    h.update((1000).to_bytes(8, "little"))    # value u64
    h.update((2).to_bytes(2, "little"))       # spk version u16
    h.update((5).to_bytes(8, "little"))       # spk length u64
    h.update(spk)
    assert M.covenant_id(tx_id, 7, [(3, 1000, 2, spk)]) == h.digest()


@pytest.mark.parametrize("name", sorted(M.SCENARIOS))
def test_scenarios(cov, name):
    tx, want = M.scenario_tx(random.Random(zlib.crc32(name.encode())), name)
    assert check_code(cov, tx) == want


def test_continuation_classes(cov):
    tx, _ = M.scenario_tx(random.Random(1), "continuation_with_genesis")
    blob = B.build_blob([tx])
    got = [cov.host_cov_is_continuation(blob, ctypes.c_size_t(len(blob)), 0, k)
           for k in range(4)]
    assert got == [1, 0, 0, 0]


def test_genesis_id_covers_every_field(cov):
    """Each hashed field of a genesis group changes the id: a transaction that
    is valid stops being so when one is altered after the id was computed."""
    rng = random.Random(2)

    def fresh():
        return M.cov_tx(rng, [None, None], [(1, 1), None, (1, 1)],
                        out_spk_lens=[5, 5, 40])

    assert check_code(cov, fresh()) == 0
    tx = fresh()
    tx["outputs"][2]["value"] += 1
    assert check_code(cov, tx) == M.ERR_GENESIS_ID
    tx = fresh()
    tx["outputs"][0]["spk_version"] ^= 1
    assert check_code(cov, tx) == M.ERR_GENESIS_ID
    tx = fresh()
    tx["outputs"][2]["spk"] = tx["outputs"][2]["spk"][:-1] + b"\0\0"
    assert check_code(cov, tx) == M.ERR_GENESIS_ID
    tx = fresh()
    tx["inputs"][1]["prev_index"] += 1
    assert check_code(cov, tx) == M.ERR_GENESIS_ID
    tx = fresh()
    tx["inputs"][1]["prev_tx_id"] = bytes(32)
    assert check_code(cov, tx) == M.ERR_GENESIS_ID
    # the other input's outpoint is not hashed
    tx = fresh()
    tx["inputs"][0]["prev_index"] += 1
    assert check_code(cov, tx) == 0
    # the output between the two members moves neither index
    tx = fresh()
    tx["outputs"][1]["value"] += 1
    assert check_code(cov, tx) == 0
    # the same outputs authorized by the other input form another group
    tx = fresh()
    for k in (0, 2):
        tx["outputs"][k]["covenant"] = (0, tx["outputs"][k]["covenant"][1])
    assert check_code(cov, tx) == M.ERR_GENESIS_ID


def test_out_of_bounds_wins_over_wrong_id(cov):
    rng = random.Random(3)
    for order in ([(0, 1), (2, 2)], [(2, 2), (0, 1)]):
        tx = M.cov_tx(rng, [None, None], order, correct=False)
        assert check_code(cov, tx) == M.ERR_AUTH_INPUT


def test_different_id_on_input_is_genesis(cov):
    """An authorizing input that carries ANOTHER id makes the output a genesis
    output (covenants.rs:137): valid with the recomputed id, 14 without."""
    rng = random.Random(4)
    assert check_code(cov, M.cov_tx(rng, [M.X], [(0, 7)])) == 0
    assert check_code(cov, M.cov_tx(rng, [M.X], [(0, 7)], correct=False)) \
        == M.ERR_GENESIS_ID


def test_second_failing_group_is_found(cov):
    """Groups are checked one by one: a wrong id in the last group fails."""
    rng = random.Random(5)
    tx = M.cov_tx(rng, [None, None], [(0, 1), (1, 2), (0, 1), (1, 3)])
    assert check_code(cov, tx) == 0
    auth, cid = tx["outputs"][3]["covenant"]
    tx["outputs"][3]["covenant"] = (auth, bytes([cid[0] ^ 1]) + cid[1:])
    assert check_code(cov, tx) == M.ERR_GENESIS_ID


# ---------------- interpreter opcodes ----------------

OP_0, OP_1, OP_4 = 0x00, 0x51, 0x54
OP_NUMEQUAL, OP_NUMEQUALVERIFY = 0x9c, 0x9d
OP_AUTH_OUT_COUNT, OP_AUTH_OUT_IDX = 0xcb, 0xcc
OP_COV_IN_COUNT, OP_COV_OUT_COUNT, OP_COV_OUT_IDX = 0xd0, 0xd2, 0xd3


def push32(b):
    assert len(b) == 32
    return bytes([0x20]) + b


def run_spk(script, spk):
    """The continuation-plus-genesis transaction with `spk` as the version-0
    script of the entry input 0 spends; the code of that input's script."""
    tx, _ = M.scenario_tx(random.Random(6), "continuation_with_genesis",
                          in_spk_version=0, in_spks=[spk])
    blob = B.build_blob([tx])
    rc = script.host_run_input_script(blob, ctypes.c_size_t(len(blob)), 0, 0,
                                      ctypes.c_uint64(1000))
    return rc, tx


def test_auth_output_count_counts_continuations_only(script):
    rc, _ = run_spk(script, bytes([OP_0, OP_AUTH_OUT_COUNT, OP_1, OP_NUMEQUAL]))
    assert rc == 0
    # not 4, the number of outputs that name input 0
    rc, _ = run_spk(script, bytes([OP_0, OP_AUTH_OUT_COUNT, OP_4, OP_NUMEQUAL]))
    assert rc == SCRIPT_EVAL_FALSE


def test_auth_output_idx(script):
    rc, _ = run_spk(script, bytes([OP_0, OP_0, OP_AUTH_OUT_IDX, OP_0, OP_NUMEQUAL]))
    assert rc == 0
    # (0, 1): input 0 has one authorized output only
    rc, _ = run_spk(script, bytes([OP_0, OP_1, OP_AUTH_OUT_IDX, OP_1, OP_NUMEQUAL]))
    assert rc == SCRIPT_INVALID_SOURCE


def test_covenant_output_and_input_counts(script):
    x = push32(M.X)
    rc, tx = run_spk(script, x + bytes([OP_COV_OUT_COUNT, OP_1, OP_NUMEQUAL]))
    assert rc == 0
    rc, _ = run_spk(script, x + bytes([OP_COV_IN_COUNT, OP_1, OP_NUMEQUAL]))
    assert rc == 0
    rc, _ = run_spk(script, bytes([OP_0]) + x
                    + bytes([OP_COV_OUT_IDX, OP_0, OP_NUMEQUAL]))
    assert rc == 0
    # a genesis id has no shared context: no outputs, no inputs. The ids do
    # not depend on the spent script, so those of this run serve the next.
    gen_a = tx["outputs"][1]["covenant"][1]
    assert gen_a == tx["outputs"][3]["covenant"][1] != M.X
    g = push32(gen_a)
    rc, tx2 = run_spk(script, g + bytes([OP_COV_OUT_COUNT, OP_0, OP_NUMEQUAL]))
    assert tx2["outputs"][1]["covenant"][1] == gen_a
    assert rc == 0
    rc, _ = run_spk(script, g + bytes([OP_COV_IN_COUNT, OP_0, OP_NUMEQUAL]))
    assert rc == 0
    rc, _ = run_spk(script, bytes([OP_0]) + g
                    + bytes([OP_COV_OUT_IDX, OP_0, OP_NUMEQUAL]))
    assert rc == SCRIPT_INVALID_SOURCE
