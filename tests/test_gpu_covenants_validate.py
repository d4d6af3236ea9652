"""Covenant transactions through kv_validate_block under KV_FLAGS_FULL:
check_covenant_info in phase 1 (codes 13 and 14), fees, the covenant opcodes
end to end, and the block's MuHash partial with covenant ids in both halves.

⇔ tx_validation_in_utxo_context.rs:46-66 with CovenantsContext::from_tx
(crypto/txscript/src/covenants.rs:101-163) and muhash.rs:55-69. Expected
values come from tests/covenant_model.py (hashlib and Python integers); the
oracle rejects covenant outputs and is not consulted. Spent entries have
script version 1, which the script engine accepts unseen, so nothing here
needs a signature."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))
import covenant_model as M  # noqa: E402
from covenant_model import B, P  # noqa: E402
from workload import storage_mass  # noqa: E402

pytestmark = pytest.mark.gpu

FULL, SKIP_MASS = 0, 2
POV_DAA = BLOCK_DAA = 10**9
ERR_FEERATE_TOO_LOW, ERR_BAD_BLOB = 7, 90
# a failing OpNumEqualVerify is TxScriptError::VerifyError; the signature
# script is empty, so the code is SignatureEmpty(VerifyError)
SIGNATURE_EMPTY_BASE, SCRIPT_VERIFY_ERROR = 200, 9

OP_0, OP_1, OP_4 = 0x00, 0x51, 0x54
OP_NUMEQUAL, OP_NUMEQUALVERIFY = 0x9c, 0x9d
OP_AUTH_OUT_COUNT, OP_COV_OUT_COUNT = 0xcb, 0xd2


@pytest.fixture(scope="module")
def engine():
    from rusty_kaspa_amd.engine import Engine
    eng = Engine()
    yield eng
    eng.close()


def opcode_spk(auth_count):
    """auth output count of input 0 == auth_count, and one covenant output of
    id X: true on the continuation-plus-genesis transaction for 1 only."""
    return bytes([OP_0, OP_AUTH_OUT_COUNT, auth_count, OP_NUMEQUALVERIFY, 0x20]) \
        + M.X + bytes([OP_COV_OUT_COUNT, OP_1, OP_NUMEQUAL])


def scenario_block():
    """(txs, expected codes): every scenario, then the opcode transactions."""
    rng = random.Random(2024)
    txs, want = [], []
    for name in sorted(M.SCENARIOS):
        tx, code = M.scenario_tx(rng, name)
        txs.append(tx)
        want.append(code)
    for auth_count, code in ((OP_1, 0),
                             (OP_4, SIGNATURE_EMPTY_BASE + SCRIPT_VERIFY_ERROR)):
        tx, _ = M.scenario_tx(rng, "continuation_with_genesis", in_spk_version=0,
                              in_spks=[opcode_spk(auth_count)])
        txs.append(tx)
        want.append(code)
    for tx in txs:
        tx["storage_mass"] = storage_mass(tx)
    return txs, want


def want_fees(txs, codes):
    return [0 if c else sum(i["utxo"]["amount"] for i in tx["inputs"])
            - sum(o["value"] for o in tx["outputs"]) for tx, c in zip(txs, codes)]


def check_partial(partial, txs, codes):
    """numerator / denominator == created / spent (mod P), halves non-trivial"""
    num = int.from_bytes(partial[:384], "little") % P
    den = int.from_bytes(partial[384:], "little") % P
    want_num, want_den = M.block_partial(txs, codes, BLOCK_DAA)
    assert want_num != 1 and want_den != 1
    assert num * want_den % P == want_num * den % P


def test_scenarios_full_validation(engine):
    txs, want = scenario_block()
    assert sorted(set(want)) == [0, 13, 14, 209]
    blob = B.build_blob(txs)
    codes, fees, partial = engine.validate_block(blob, len(txs), POV_DAA, BLOCK_DAA,
                                                 FULL)
    assert codes == want
    assert fees == want_fees(txs, want)
    # covenant outputs are in the numerator, spent covenant entries in the
    # denominator; the same block without the ids hashes to something else
    assert any(o["covenant"] for tx, c in zip(txs, want) if not c
               for o in tx["outputs"])
    assert any(i["utxo"]["covenant_id"] for tx, c in zip(txs, want) if not c
               for i in tx["inputs"])
    check_partial(partial, txs, want)


def test_version_0_binding_is_a_bad_blob(engine):
    """The version-0 wire form has no binding field."""
    rng = random.Random(7)
    tx, _ = M.scenario_tx(rng, "genesis_single_output", version=0)
    plain = M.cov_tx(rng, [None], [None], version=0)
    blob = B.build_blob([tx, plain])
    codes, fees, _ = engine.validate_block(blob, 2, POV_DAA, BLOCK_DAA, SKIP_MASS)
    assert codes == [ERR_BAD_BLOB, 0]
    assert fees == want_fees([tx, plain], codes)


def test_mempool_feerate_wins_over_covenant_errors(engine):
    """check_feerate_threshold (:57) runs before check_covenant_info (:58)."""
    rng = random.Random(8)
    txs = [M.scenario_tx(rng, n)[0] for n in
           ("wrong_genesis_id", "auth_input_out_of_bounds", "genesis_single_output")]
    blob = B.build_blob(txs)
    codes, fees = engine.validate_mempool(blob, 3, POV_DAA, 0.0)
    assert codes == [M.ERR_GENESIS_ID, M.ERR_AUTH_INPUT, 0]
    assert fees == want_fees(txs, codes)
    # fee ~ 1e10 over a mass of tens of thousands: 1e9 is out of reach, 1.0 is not
    codes, fees = engine.validate_mempool(blob, 3, POV_DAA, 1e9)
    assert codes == [ERR_FEERATE_TOO_LOW] * 3 and fees == [0, 0, 0]
    codes, fees = engine.validate_mempool(blob, 3, POV_DAA, 1.0)
    assert codes == [M.ERR_GENESIS_ID, M.ERR_AUTH_INPUT, 0]
