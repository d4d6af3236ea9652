"""Covenant ids in the GPU-resident UTXO table (KV_UTXO_F_COVENANT): the
commitment and the chunk import hash them (muhash.rs:66-67), lookup, export,
rehash, grow and the undo journal carry them, and kv_validate_block_utxo
populates them from the table and writes them back with its diff.

Expected values come from tests/covenant_model.py: write_utxo with the id
appended, keyed BLAKE2b and ChaCha20 in Python, products mod 2^3072 - 1103717.
The table is the smallest that holds the entries."""
import ctypes
import os
import random
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))
import covenant_model as M  # noqa: E402
from covenant_model import B, P, F_ARENA, F_COINBASE, F_COVENANT  # noqa: E402
from workload import storage_mass  # noqa: E402

pytestmark = pytest.mark.gpu

FULL = 0
POV_DAA = BLOCK_DAA = 10**9
MAX_SPK = 10000
CAPACITY = 64  # entries; 128 slots


@pytest.fixture(scope="module")
def engine():
    from rusty_kaspa_amd.engine import Engine
    eng = Engine()
    yield eng
    eng.close()


# ---------------- the entries ----------------

COV_SPK_LENS = [0, 1, 34, 36, 37, 300]


def build_model():
    """40 entries: plain inline, plain long, and covenant entries of every
    script length class, some coinbase, several script versions."""
    rng = random.Random(4040)
    model = {}

    def add(spk_len, cov, coinbase=False):
        op = rng.randbytes(32) + struct.pack("<I", rng.randrange(4))
        model[op] = B.utxo_entry(
            rng.randrange(1, 1 << 50), rng.randbytes(spk_len), rng.randrange(1 << 40),
            coinbase, rng.choice((0, 1, 0xFFFF)), rng.randbytes(32) if cov else None)

    for rep in range(3):
        for n in COV_SPK_LENS:
            add(n, True, coinbase=rep == 2 and n in (0, 37))
    for n in (0, 20, 34, 34, 34, 35, 36, 34, 34, 34, 34, 34):
        add(n, False, coinbase=n == 35)
    for n in (37, 64, 300, 1000, 37, 65, 129, 200, 2000, MAX_SPK):
        add(n, False)
    assert len(model) == 40
    return model


MODEL = build_model()


# ---------------- table helpers ----------------

def ctx(engine):
    return ctypes.c_void_p(engine.ctx)


def err(engine):
    return engine.lib.kv_last_error().decode()


def reset(engine, capacity=CAPACITY):
    assert engine.lib.kv_utxo_reset(ctx(engine), ctypes.c_uint64(capacity)) == 0


def upsert_spk(engine, items):
    ops = b"".join(op for op, _ in items)
    ents, spk_blob = B.pack_utxo_entries([u for _, u in items])
    rc = engine.lib.kv_utxo_upsert_spk(ctx(engine), ops, ents, spk_blob,
                                       ctypes.c_size_t(len(spk_blob)),
                                       ctypes.c_size_t(len(items)))
    assert rc == 0, err(engine)


def load(engine, model=MODEL):
    reset(engine)
    upsert_spk(engine, list(model.items()))


def read_entries(engine, ops):
    """kv_utxo_lookup_spk decoded: a utxo_entry dict per outpoint, or None"""
    n = len(ops)
    out = (ctypes.c_uint8 * (64 * n))()
    bm = (ctypes.c_uint64 * ((n + 63) // 64))()
    cap = 1 << 16
    spk = (ctypes.c_uint8 * cap)()
    used = ctypes.c_size_t()
    rc = engine.lib.kv_utxo_lookup_spk(ctx(engine), b"".join(ops), ctypes.c_size_t(n),
                                       out, bm, spk, ctypes.c_size_t(cap),
                                       ctypes.byref(used))
    assert rc == 0, err(engine)
    out, spk = bytes(out), bytes(spk[:used.value])
    got, expect_off = [], 0
    for i in range(n):
        if not (bm[i // 64] >> (i % 64)) & 1:
            got.append(None)
            continue
        rec = out[64 * i:64 * (i + 1)]
        amount, daa, flags, ver, ln = struct.unpack_from("<QQHHI", rec, 0)
        cid = None
        if flags & F_COVENANT:
            assert flags & F_ARENA and rec[60:64] == bytes(4)
            cid = rec[28:60]
        if flags & F_ARENA:
            off, = struct.unpack_from("<I", rec, 24)
            assert off == expect_off  # scripts come out in entry order
            script = spk[off:off + ln]
            expect_off += ln
            assert len(script) == ln
        else:
            assert ln <= 36
            script = rec[24:24 + ln]
        got.append(B.utxo_entry(amount, script, daa, bool(flags & F_COINBASE), ver,
                                cid))
    assert expect_off == used.value
    return got


def check_table(engine, model, gone=()):
    """commitment, live count and every entry equal the model"""
    partial, n_live, _ = engine.utxo_commitment()
    assert n_live == len(model)
    assert int.from_bytes(partial[:384], "little") % P == M.product(model.items())
    assert int.from_bytes(partial[384:], "little") == 1
    ops = list(model)
    assert read_entries(engine, ops) == [model[op] for op in ops]
    if gone:
        assert read_entries(engine, list(gone)) == [None] * len(gone)
    return partial


def walk(engine, max_entries):
    slots = engine.utxo_stats()["slots"]
    cursor, chunks = 0, []
    for _ in range(slots + 2):
        nxt, ops, ents, spk, n = engine.utxo_export_chunk(cursor, max_entries,
                                                          1 << 16)
        if n == 0 and nxt == slots:
            return chunks
        assert nxt > cursor
        chunks.append((ops, ents, spk, n))
        cursor = nxt
    raise AssertionError("the walk did not end")


def identity_partial():
    return bytearray((1).to_bytes(384, "little") * 2)


# ---------------- tests ----------------

def test_commitment_import_and_lookup(engine):
    """kv_utxo_commitment == the Python product == the import accumulator, and
    kv_utxo_lookup_spk returns every id and script."""
    reset(engine)
    items = list(MODEL.items())
    acc = identity_partial()
    for lo in range(0, len(items), 16):  # three chunks: 16, 16, 8
        part = items[lo:lo + 16]
        ents, spk_blob = B.pack_utxo_entries([u for _, u in part])
        engine.utxo_import_chunk(b"".join(op for op, _ in part), ents, spk_blob,
                                 len(part), acc)
    want = M.product(items)
    assert int.from_bytes(acc[:384], "little") % P == want
    partial = check_table(engine, MODEL)
    assert engine.muhash_finalize(bytes(acc)) == engine.muhash_finalize(partial)
    # the ids are hashed: without them the product is another number
    bare = [(op, dict(u, covenant_id=None)) for op, u in items]
    assert M.product(bare) != want


def test_chunk_of_empty_covenant_scripts_only(engine):
    """No entry brings script bytes, yet every entry needs the arena form."""
    rng = random.Random(5)
    model = {rng.randbytes(36): B.utxo_entry(7 + k, b"", 9, covenant_id=rng.randbytes(32))
             for k in range(3)}
    reset(engine)
    acc = identity_partial()
    ents, spk_blob = B.pack_utxo_entries(list(model.values()))
    assert spk_blob == b""
    engine.utxo_import_chunk(b"".join(model), ents, spk_blob, 3, acc)
    assert int.from_bytes(acc[:384], "little") % P == M.product(model.items())
    check_table(engine, model)
    engine.utxo_rehash(0)
    check_table(engine, model)


def test_export_into_a_fresh_table(engine):
    load(engine)
    chunks = walk(engine, 16)
    assert sum(n for _, _, _, n in chunks) == len(MODEL)
    for ops, ents, spk, n in chunks:
        for i in range(n):
            op, rec = ops[36 * i:36 * (i + 1)], ents[64 * i:64 * (i + 1)]
            # exactly the record pack_utxo_entries makes: a valid upsert input
            assert rec == B.pack_utxo_entries([MODEL[op]])[0]
    reset(engine)
    acc = identity_partial()
    for ops, ents, spk, n in chunks:
        engine.utxo_import_chunk(ops, ents, spk, n, acc)
    assert int.from_bytes(acc[:384], "little") % P == M.product(MODEL.items())
    check_table(engine, MODEL)


def test_rehash_and_grow_keep_ids(engine):
    load(engine)
    engine.utxo_rehash(0)
    check_table(engine, MODEL)
    engine.utxo_rehash(4 * CAPACITY)
    assert engine.utxo_stats()["slots"] == 8 * CAPACITY
    check_table(engine, MODEL)


def test_journaled_diff_and_revert_across_a_rehash(engine):
    """Covenant entries on the removed side, on the added side and
    overwritten, in both directions; a rehash between apply and revert."""
    load(engine)
    rng = random.Random(6)
    ops = list(MODEL)
    cov_ops = [op for op in ops if MODEL[op]["covenant_id"]]
    plain_ops = [op for op in ops if not MODEL[op]["covenant_id"]]
    removed = cov_ops[0:6] + plain_ops[0:3] + plain_ops[-2:]
    added = {}
    for n in COV_SPK_LENS:  # new covenant entries
        added[rng.randbytes(36)] = B.utxo_entry(rng.randrange(1, 1 << 40),
                                                rng.randbytes(n), 77, False, 1,
                                                rng.randbytes(32))
    added[rng.randbytes(36)] = B.utxo_entry(5, rng.randbytes(50), 77)
    # overwrites: covenant by covenant (another id, another script length),
    # covenant by plain, plain inline by covenant, plain long by covenant
    added[cov_ops[6]] = B.utxo_entry(11, rng.randbytes(40), 78,
                                     covenant_id=rng.randbytes(32))
    added[cov_ops[7]] = B.utxo_entry(12, rng.randbytes(34), 78)
    added[plain_ops[3]] = B.utxo_entry(13, b"", 78, covenant_id=rng.randbytes(32))
    added[plain_ops[-3]] = B.utxo_entry(14, rng.randbytes(3), 78,
                                        covenant_id=rng.randbytes(32))
    assert not set(removed) & set(added)
    after = {op: u for op, u in MODEL.items() if op not in removed}
    after.update(added)

    ents, spk_blob = B.pack_utxo_entries(list(added.values()))
    token, res = engine.utxo_apply_diff(b"".join(removed), b"".join(added), ents,
                                        spk_blob)
    assert res["n_removed_missing"] == 0 and res["n_added_overwrote"] == 4
    check_table(engine, after, gone=removed)
    engine.utxo_rehash(0)
    check_table(engine, after, gone=removed)
    engine.utxo_revert(token)
    check_table(engine, MODEL, gone=[op for op in added if op not in MODEL])


def test_inline_upsert_refuses_the_flag(engine):
    load(engine)
    op = bytes(36)
    rec = struct.pack("<QQHHI", 1, 2, F_COVENANT, 0, 0) + bytes(40)
    rc = engine.lib.kv_utxo_upsert(ctx(engine), op + op[:35] + b"\1",
                                   struct.pack("<QQHHI", 1, 2, 0, 0, 0) + bytes(40) + rec,
                                   ctypes.c_size_t(2))
    assert rc == -1 and "KV_UTXO_F_COVENANT" in err(engine)
    check_table(engine, MODEL, gone=[op])  # nothing was written


def test_validate_block_utxo_spends_and_creates_covenant_entries(engine):
    rng = random.Random(9)
    y = rng.randbytes(32)
    txs = [
        # continuation of X (and two genesis groups), from a 20-byte script
        M.cov_tx(rng, [M.X, None], [(0, M.X), (0, 100), (1, 200), (0, 100), None],
                 in_spks=[rng.randbytes(20), rng.randbytes(300)],
                 out_spk_lens=[34, 0, 37, 300, 34]),
        # continuation of Y from an empty script; one plain output
        M.cov_tx(rng, [y], [(0, y), None], in_spks=[b""], out_spk_lens=[36, 50]),
        # a wrong genesis id: rejected, so its input stays and nothing is added
        M.cov_tx(rng, [None], [(0, 1)], correct=False),
    ]
    for tx in txs:
        tx["storage_mass"] = storage_mass(tx)
    want_codes = [0, 0, M.ERR_GENESIS_ID]
    blob = B.build_blob(txs)
    stripped, ops, ents, spk_blob = B.strip_utxo_entries_spk(blob)
    spent = {i["prev_tx_id"] + struct.pack("<I", i["prev_index"]): i["utxo"]
             for tx in txs for i in tx["inputs"]}
    assert ops == b"".join(spent)

    ic, if_, ip = engine.validate_block(blob, 3, POV_DAA, BLOCK_DAA, FULL)
    assert ic == want_codes

    model = dict(MODEL)
    model.update(spent)
    reset(engine)
    upsert_spk(engine, list(model.items()))
    uc, uf, up = engine.validate_block_utxo(stripped, 3, POV_DAA, BLOCK_DAA, FULL,
                                            apply_diff=True)
    assert (uc, uf) == (ic, if_)
    assert up == ip
    num, den = M.block_partial(txs, want_codes, BLOCK_DAA)
    assert int.from_bytes(up[:384], "little") * den % P \
        == int.from_bytes(up[384:], "little") * num % P

    gone = []
    for tx, code in zip(txs, want_codes):
        if code:
            continue
        for i in tx["inputs"]:
            op = i["prev_tx_id"] + struct.pack("<I", i["prev_index"])
            del model[op]
            gone.append(op)
        for k, o in enumerate(tx["outputs"]):
            model[tx["tx_id"] + struct.pack("<I", k)] = M.output_entry(o, BLOCK_DAA)
    assert sum(1 for u in model.values() if u["covenant_id"]) \
        == sum(1 for u in MODEL.values() if u["covenant_id"]) + 5
    check_table(engine, model, gone=gone)
