"""GPU: the sighash, transaction-hash and MuHash-element kernels
(kv_sighash_kernels.hip, kv_hash_device.h) on shapes the workload generator
never builds: version 1, covenants, non-native subnetworks with an empty
payload, storage mass, and BLAKE2b streams that end on, one short of and one
past every 128-byte block boundary (length sweeps 0..300, input counts around
multiples of 16 and 128).

Blobs are crafted with rusty_kaspa_amd.blob; nothing here verifies a signature,
so nothing is signed. Results are compared byte for byte with the reference's
recorded vectors where they exist (tests/golden/sighash.json, txid.json) and
with the oracle otherwise."""
import ctypes
import random

import pytest

from conftest import oracle_tx_id
from rusty_kaspa_amd import blob as B
from test_oracle_sighash import apply_action, base_txs
from test_oracle_txid import tx_from_case

pytestmark = pytest.mark.gpu

HASH_TYPES = (0x01, 0x02, 0x04, 0x81, 0x82, 0x84)
N_IN_LIST = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129)
NON_NATIVE = bytes([7, 0, 3] + [0] * 16 + [9])
MAX_SOMPI = 29_000_000_000 * 100_000_000
U64 = 2**64 - 1
SKIP_MASS = 2


class Job(ctypes.Structure):
    _fields_ = [("tx_index", ctypes.c_uint32), ("input_index", ctypes.c_uint32),
                ("hash_type", ctypes.c_uint8), ("ecdsa", ctypes.c_uint8),
                ("_pad", ctypes.c_uint16)]


@pytest.fixture(scope="module")
def engine():
    from rusty_kaspa_amd.engine import Engine
    eng = Engine()
    yield eng
    eng.close()


# ---------------------------------------------------------------- builders

def rb(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


def mk_input(rng, index, version, sig_len=0, spk_len=34, spk_version=0, cov=False,
             amount=None, daa=None, coinbase=False, sequence=None):
    """An input with its spent entry. Outpoints are distinct (random 32-byte
    previous id); the commit field follows the version: a sigop count for
    version 0, a compute budget for version 1."""
    return B.tx_input(
        rb(rng, 32), (index * 2654435761 + 17) & 0xFFFFFFFF,
        sequence=rng.getrandbits(64) if sequence is None else sequence,
        sig_script=rb(rng, sig_len),
        commit_kind=0 if version == 0 else 1,
        commit_value=(index * 37 + 1) % 251 if version == 0
        else (index * 997 + 1) & 0xFFFF,
        utxo=B.utxo_entry(rng.getrandbits(63) if amount is None else amount,
                          rb(rng, spk_len),
                          daa_score=rng.getrandbits(64) if daa is None else daa,
                          is_coinbase=coinbase, spk_version=spk_version,
                          covenant_id=rb(rng, 32) if cov else None))


def mk_output(rng, spk_len=34, spk_version=0, cov=False, value=None):
    return B.tx_output(rng.getrandbits(64) if value is None else value,
                       rb(rng, spk_len), spk_version,
                       (rng.randrange(1, 1 << 16), rb(rng, 32)) if cov else None)


def mk_tx(rng, version, inputs, outputs, **kw):
    kw.setdefault("lock_time", rng.getrandbits(64))
    return B.tx_dict(version, inputs, outputs, **kw)


def varied_inputs(rng, version, n_in):
    """Inputs of unequal record sizes, so that a wrong record end cannot
    cancel out over a walk."""
    return [mk_input(rng, i, version, sig_len=rng.randrange(0, 90),
                     spk_len=rng.randrange(0, 70),
                     spk_version=rng.choice((0, 0, 1, 0xFFFF)),
                     cov=version >= 1 and rng.random() < 0.3)
            for i in range(n_in)]


def n_out_choices(n_in):
    return sorted({n for n in (1, n_in - 1, n_in, n_in + 1) if n >= 1})


def input_count_txs(rng):
    txs = []
    for n_in in N_IN_LIST:
        for version in (0, 1):
            for n_out in n_out_choices(n_in):
                outs = [mk_output(rng, spk_len=rng.randrange(0, 70),
                                  cov=version >= 1 and rng.random() < 0.3)
                        for _ in range(n_out)]
                txs.append(mk_tx(rng, version, varied_inputs(rng, version, n_in),
                                 outs))
    return txs


# ---------------------------------------------------------------- sighash

def gpu_sighashes(engine, blob, jobs):
    arr = (Job * len(jobs))(*[Job(t, i, ht, ec, 0) for t, i, ht, ec in jobs])
    out = (ctypes.c_uint8 * (32 * len(jobs)))()
    rc = engine.lib.kv_sighash_batch(ctypes.c_void_p(engine.ctx), blob,
                                     ctypes.c_size_t(len(blob)), arr,
                                     ctypes.c_size_t(len(jobs)), out)
    assert rc == 0, engine.lib.kv_last_error().decode()
    raw = bytes(out)
    return [raw[32 * k:32 * k + 32] for k in range(len(jobs))]


def check_sighash_sweep(oracle, engine, txs, describe):
    """One blob, one kv_sighash_batch call: every input × six hash types ×
    Schnorr and ECDSA, against ok_sighash."""
    blob = B.build_blob(txs)
    jobs = [(t, i, ht, ec) for t, tx in enumerate(txs)
            for i in range(len(tx["inputs"])) for ht in HASH_TYPES
            for ec in (0, 1)]
    got = gpu_sighashes(engine, blob, jobs)
    exp = (ctypes.c_uint8 * 32)()
    blen = ctypes.c_size_t(len(blob))
    for k, (t, i, ht, ec) in enumerate(jobs):
        assert oracle.ok_sighash(blob, blen, t, i, ht, ec, exp) == 0
        assert got[k] == bytes(exp), (describe(t), "input", i, hex(ht),
                                      "ecdsa" if ec else "schnorr")


def test_golden_sighash_vectors(engine, golden):
    """All recorded cases of sighash.json (version-1 budget and sigop cases
    among them) in one blob, against the reference's own expected hashes."""
    g = golden("sighash.json")
    txs, jobs, names = [], [], []
    for name, txkey, hash_type, input_index, action, aidx, expected in g["tests"]:
        tx = base_txs(g)[txkey]
        apply_action(g, tx, action, aidx)
        jobs.append((len(txs), input_index, hash_type, 0))
        txs.append(tx)
        names.append((name, expected))
    assert len(txs) >= 33
    got = gpu_sighashes(engine, B.build_blob(txs), jobs)
    for h, (name, expected) in zip(got, names):
        assert h.hex() == expected, name


def test_golden_tx_hash_vectors(oracle, engine, golden):
    """Every recorded transaction hash of txid.json as a one-transaction blob:
    the root of a one-leaf tree over the recorded hash."""
    g = golden("txid.json")
    root = (ctypes.c_uint8 * 32)()
    for case in g["cases"]:
        blob = B.build_blob([tx_from_case(case)])
        oracle.ok_merkle_root(bytes.fromhex(case["hash"]), ctypes.c_size_t(1), root)
        got, _ = engine.block_body_check(blob)
        assert got == bytes(root), case["name"]


def test_sighash_utxo_spk_len(oracle, engine):
    rng = random.Random(101)
    txs = [mk_tx(rng, version, [mk_input(rng, 0, version, spk_len=n)],
                 [mk_output(rng)])
           for n in range(301) for version in (0, 1)]
    check_sighash_sweep(oracle, engine, txs,
                        lambda t: f"utxo spk_len {t // 2} version {t % 2}")


def test_sighash_output_spk_len(oracle, engine):
    rng = random.Random(102)
    kinds = ((0, False), (1, False), (1, True))
    txs = [mk_tx(rng, version, [mk_input(rng, 0, version)],
                 [mk_output(rng, spk_len=n, cov=cov)])
           for n in range(301) for version, cov in kinds]
    check_sighash_sweep(oracle, engine, txs,
                        lambda t: f"output spk_len {t // 3} (version, cov) {kinds[t % 3]}")


def test_sighash_payload_len(oracle, engine):
    """payload_len 0..300 on the native and on a non-native subnetwork; length
    0 differs between the two (zero hash vs the hash of an empty payload)."""
    rng = random.Random(103)
    txs = [mk_tx(rng, n & 1, [mk_input(rng, 0, n & 1)], [mk_output(rng)],
                 subnetwork_id=sub, payload=rb(rng, n), gas=rng.getrandbits(64))
           for n in range(301) for sub in (B.SUBNETWORK_NATIVE, NON_NATIVE)]
    assert txs[0]["payload"] == txs[1]["payload"] == b""
    check_sighash_sweep(oracle, engine, txs,
                        lambda t: f"payload_len {t // 2} non-native {t % 2}")


def test_sighash_input_counts(oracle, engine):
    rng = random.Random(104)
    txs = input_count_txs(rng)
    check_sighash_sweep(
        oracle, engine, txs,
        lambda t: (f"version {txs[t]['version']} n_in {len(txs[t]['inputs'])} "
                   f"n_out {len(txs[t]['outputs'])}"))


def test_sighash_covenants_versions_high_bits(oracle, engine):
    """Version-1 output covenants and spent-entry covenant ids, script
    versions other than 0, and lock_time / gas / sequence / amount with their
    high bits set."""
    rng = random.Random(105)
    txs = []
    for k in range(48):
        version = 1 if k % 3 else 0
        n_in, n_out = rng.randrange(1, 5), rng.randrange(1, 5)
        ins = [mk_input(rng, i, version, sig_len=rng.randrange(0, 40),
                        spk_len=rng.randrange(0, 140),
                        spk_version=rng.choice((0, 1, 0x8000, 0xFFFF)),
                        cov=version == 1 and rng.random() < 0.5,
                        amount=rng.choice((U64, 1 << 63, rng.getrandbits(64))),
                        sequence=rng.choice((U64, 1 << 63, rng.getrandbits(64))))
               for i in range(n_in)]
        outs = [mk_output(rng, spk_len=rng.randrange(0, 140),
                          spk_version=rng.choice((0, 1, 0x8000, 0xFFFF)),
                          cov=version == 1 and rng.random() < 0.6,
                          value=rng.choice((U64, 1 << 63, rng.getrandbits(64))))
                for _ in range(n_out)]
        txs.append(mk_tx(rng, version, ins, outs,
                         lock_time=rng.choice((U64, 1 << 63)),
                         gas=rng.choice((U64, 1 << 63)),
                         subnetwork_id=rng.choice((B.SUBNETWORK_NATIVE, NON_NATIVE))))
    assert any(o["covenant"] for tx in txs for o in tx["outputs"])
    assert any(i["utxo"]["covenant_id"] for tx in txs for i in tx["inputs"])
    check_sighash_sweep(oracle, engine, txs, lambda t: f"tx {t}")


# ---------------------------------------------------------------- tx hash

def check_body(oracle, engine, txs, describe):
    """Root and rule code of kv_block_body_check vs the oracle; on a wrong
    root, the transactions go through again one per blob to name the first
    culprit."""
    B.finalize_tx_ids(txs, lambda blob, i: oracle_tx_id(oracle, blob, i))
    blob = B.build_blob(txs)
    expect = (ctypes.c_uint8 * 32)()
    assert oracle.ok_blob_merkle_root(blob, ctypes.c_size_t(len(blob)), expect) == 0
    root, code = engine.block_body_check(blob)
    if root != bytes(expect):
        for t, tx in enumerate(txs):
            one = B.build_blob([tx])
            assert oracle.ok_blob_merkle_root(one, ctypes.c_size_t(len(one)),
                                              expect) == 0
            assert engine.block_body_check(one)[0] == bytes(expect), describe(t)
        raise AssertionError("root differs, yet every transaction alone agrees")
    assert code == oracle.ok_body_check(blob, ctypes.c_size_t(len(blob))) == 0


def test_tx_hash_sig_script_len(oracle, engine):
    rng = random.Random(201)
    txs = [mk_tx(rng, n & 1, [mk_input(rng, 0, n & 1, sig_len=n)],
                 [mk_output(rng)]) for n in range(301)]
    check_body(oracle, engine, txs, lambda t: f"sig_script_len {t}")


def test_tx_hash_payload_len(oracle, engine):
    rng = random.Random(202)
    txs = [mk_tx(rng, n & 1, [mk_input(rng, 0, n & 1)], [mk_output(rng)],
                 payload=rb(rng, n),
                 subnetwork_id=NON_NATIVE if n % 3 == 0 else B.SUBNETWORK_NATIVE)
           for n in range(301)]
    check_body(oracle, engine, txs, lambda t: f"payload_len {t}")


def test_tx_hash_storage_mass_budgets_covenants(oracle, engine):
    """storage_mass {0, 1, 2^64-1} × version {0, 1} (version 0 hashes the mass
    only when non-zero, version 1 always); commit_kind=1 budgets and output
    covenants on version 1."""
    rng = random.Random(203)
    txs, names = [], []
    for mass in (0, 1, U64):
        for version in (0, 1):
            txs.append(mk_tx(rng, version, [mk_input(rng, 0, version)],
                             [mk_output(rng)], storage_mass=mass))
            names.append(f"storage_mass {mass} version {version}")
    for k in range(24):
        n_in, n_out = rng.randrange(1, 6), rng.randrange(1, 6)
        ins = [mk_input(rng, i, 1, sig_len=rng.randrange(0, 70)) for i in range(n_in)]
        for i in ins:  # budgets over the whole u16 range, and kind 0 on version 1
            i["commit_value"] = rng.choice((0, 1, 0xFF, 0x100, 0xFFFF,
                                            rng.getrandbits(16)))
            i["commit_kind"] = 0 if rng.random() < 0.2 else 1
        outs = [mk_output(rng, spk_len=rng.randrange(0, 140), cov=rng.random() < 0.6,
                          spk_version=rng.choice((0, 0xFFFF))) for _ in range(n_out)]
        txs.append(mk_tx(rng, 1, ins, outs, storage_mass=rng.getrandbits(64),
                         gas=rng.getrandbits(64)))
        names.append(f"version-1 budgets/covenants tx {k}")
    # a version-0 input whose commit field is a budget hashes a zero sigop count
    tx = mk_tx(rng, 0, [mk_input(rng, 0, 0)], [mk_output(rng)])
    tx["inputs"][0]["commit_kind"], tx["inputs"][0]["commit_value"] = 1, 0x1234
    txs.append(tx)
    names.append("version 0 with commit_kind 1")
    assert any(o["covenant"] for tx in txs for o in tx["outputs"])
    check_body(oracle, engine, txs, lambda t: names[t])


def test_tx_hash_input_counts(oracle, engine):
    rng = random.Random(204)
    txs = input_count_txs(rng)
    check_body(
        oracle, engine, txs,
        lambda t: (f"version {txs[t]['version']} n_in {len(txs[t]['inputs'])} "
                   f"n_out {len(txs[t]['outputs'])}"))


# ---------------------------------------------------------------- muhash

# the sequence-lock rule compares DAA scores as signed 64-bit values, so the
# point-of-view score stays below 2^63; the block's own score is only hashed
POV_DAA = (1 << 62) + 10**9
BLOCK_DAA = (1 << 63) + 123_456_789
# (numerator count, denominator count): created outputs and spent inputs of
# the accepted transactions. Each list walks 1, 2, 63, 64, 65, 128, 129, 4097,
# the steps of the reduce schedule stride = ceil(n / 64).
MUHASH_COUNTS = ((1, 2), (2, 1), (63, 65), (64, 64), (65, 63), (128, 129),
                 (129, 128), (4097, 4097))


def spread(rng, total, parts):
    """`parts` positive integers summing to `total`."""
    cuts = sorted(rng.sample(range(1, total), parts - 1)) if parts > 1 else []
    return [b - a for a, b in zip([0] + cuts, cuts + [total])]


def muhash_block(n_num, n_den):
    """A block of transactions that are valid without a signature: every spent
    entry has a script version above 0, which the script engine accepts
    unseen. Script lengths walk 0..300 (and wrap), versions reach 0xFFFF, some
    entries are mature coinbase outputs, some carry a covenant id, and amounts
    and DAA scores have high bits set, with Σin >= Σout per transaction."""
    rng = random.Random(n_num * 10007 + n_den)
    n_txs = min(n_num, n_den, 700)
    ins_per, outs_per = spread(rng, n_den, n_txs), spread(rng, n_num, n_txs)
    txs, ki, ko = [], 0, 0
    for t in range(n_txs):
        n_in, n_out = ins_per[t], outs_per[t]
        cap = MAX_SOMPI // n_in
        ins = []
        for i in range(n_in):
            coinbase = ki % 5 == 0
            # a sequence either disables the relative lock (bit 63) or is 0
            seq = 0 if ki % 4 == 1 else (1 << 63) | rng.getrandbits(63)
            if coinbase:
                daa = rng.randrange(0, POV_DAA - 10**6)
            elif seq == 0:
                daa = rng.randrange(1 << 61, POV_DAA - 10)
            else:
                daa = rng.getrandbits(64)
            amount = cap if i == 0 else rng.randrange(cap // 2, cap + 1)
            ins.append(mk_input(
                rng, ki, 0, sig_len=rng.randrange(0, 6), spk_len=ki % 301,
                spk_version=(1, 2, 0x100, 0x8000, 0xFFFF)[ki % 5] if ki % 7
                else rng.randrange(1, 1 << 16),
                cov=ki % 3 == 0, amount=amount, daa=daa, coinbase=coinbase,
                sequence=seq))
            ki += 1
        total_in = sum(i["utxo"]["amount"] for i in ins)
        assert total_in <= MAX_SOMPI
        # spend all of it in the first transaction, most of it otherwise
        budget = total_in if t == 0 else total_in - rng.randrange(0, 1 << 40)
        vals = spread(rng, budget, n_out) if budget > n_out else [0] * n_out
        outs = []
        for v in vals:
            outs.append(mk_output(rng, spk_len=ko % 301, value=v,
                                  spk_version=(0, 1, 0xFFFF)[ko % 3]))
            ko += 1
        txs.append(mk_tx(rng, 0, ins, outs, lock_time=0))
    assert ki == n_den and ko == n_num
    return txs


def test_muhash_small_then_large_block(oracle):
    """A context of its own, so that the second block is sure to outgrow the
    pinned upload staging that the first one sized: the landing pad of the
    MuHash partial must survive that growth (it used to be freed with it)."""
    from rusty_kaspa_amd.engine import Engine
    eng = Engine()
    try:
        for n_num, n_den in ((1, 2), (129, 128), (2, 1)):
            test_muhash_elements_and_reduce(oracle, eng, n_num, n_den)
    finally:
        eng.close()


@pytest.mark.parametrize("n_num,n_den", MUHASH_COUNTS)
def test_muhash_elements_and_reduce(oracle, engine, n_num, n_den):
    txs = muhash_block(n_num, n_den)
    B.finalize_tx_ids(txs, lambda blob, i: oracle_tx_id(oracle, blob, i))
    blob, n = B.build_blob(txs), len(txs)
    ocodes, ofees = (ctypes.c_int32 * n)(), (ctypes.c_uint64 * n)()
    omh = (ctypes.c_uint8 * 32)()
    assert oracle.ok_validate_block_parallel(
        blob, ctypes.c_size_t(len(blob)), ctypes.c_uint64(POV_DAA),
        ctypes.c_uint64(BLOCK_DAA), SKIP_MASS, 8, ocodes, ofees, omh) == 0
    # the condition: a rejected transaction contributes no element, and the
    # comparison below would then pass without testing what it is here for
    assert list(ocodes) == [0] * n, [(t, c) for t, c in enumerate(ocodes) if c][:5]
    assert sum(len(tx["outputs"]) for tx in txs) == n_num
    assert sum(len(tx["inputs"]) for tx in txs) == n_den
    codes, fees, partial = engine.validate_block(blob, n, POV_DAA, BLOCK_DAA,
                                                 SKIP_MASS)
    assert codes == list(ocodes)
    assert fees == list(ofees)
    assert engine.muhash_finalize(partial) == bytes(omh)
