"""Independent model for the covenant tests, written from the reference
source and sharing no code with the engine or the oracle:

- covenant_id: consensus/core/src/hashing/covenant_id.rs (keyed BLAKE2b-256,
  key "CovenantID", the construction tests/golden/hashers.json pins for the
  other domains);
- utxo_element: MuHash::from_utxo over write_utxo with the covenant id
  appended (consensus/core/src/muhash.rs:55-69), expanded by ChaCha20 to 384
  bytes (crypto/muhash/src/lib.rs:148-169), as an integer; products are taken
  mod P = 2^3072 - 1103717;
- scenario transactions: those of crypto/txscript/src/covenants.rs:277-451,
  rebuilt as blob dicts (version 1: the version-0 wire form has no binding).
"""
import hashlib
import os
import struct
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from rusty_kaspa_amd import blob as B  # noqa: E402

P = 2**3072 - 1103717
ERR_AUTH_INPUT, ERR_GENESIS_ID = 13, 14
F_COINBASE, F_ARENA, F_COVENANT = 1, 2, 4


def covenant_id(prev_tx_id, prev_index, auth_outputs):
    """auth_outputs: (out_index, value, spk_version, spk) in ascending index."""
    h = hashlib.blake2b(key=b"CovenantID", digest_size=32)
    h.update(prev_tx_id + struct.pack("<IQ", prev_index, len(auth_outputs)))
    for index, value, spk_version, spk in auth_outputs:
        h.update(struct.pack("<IQHQ", index, value, spk_version, len(spk)) + spk)
    return h.digest()


# ---------------- MuHash element ----------------

def _chacha20_block(key_words, counter):
    def rotl(x, n):
        return ((x << n) | (x >> (32 - n))) & 0xFFFFFFFF

    init = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574] + key_words \
        + [counter & 0xFFFFFFFF, counter >> 32, 0, 0]
    x = list(init)

    def qr(a, b, c, d):
        x[a] = (x[a] + x[b]) & 0xFFFFFFFF
        x[d] = rotl(x[d] ^ x[a], 16)
        x[c] = (x[c] + x[d]) & 0xFFFFFFFF
        x[b] = rotl(x[b] ^ x[c], 12)
        x[a] = (x[a] + x[b]) & 0xFFFFFFFF
        x[d] = rotl(x[d] ^ x[a], 8)
        x[c] = (x[c] + x[d]) & 0xFFFFFFFF
        x[b] = rotl(x[b] ^ x[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12), qr(1, 5, 9, 13), qr(2, 6, 10, 14), qr(3, 7, 11, 15)
        qr(0, 5, 10, 15), qr(1, 6, 11, 12), qr(2, 7, 8, 13), qr(3, 4, 9, 14)
    return struct.pack("<16I", *[(a + b) & 0xFFFFFFFF for a, b in zip(x, init)])


def element_of(data):
    """keyed BLAKE2b-256("MuHashElement") -> ChaCha20 key, zero nonce, 384
    bytes of keystream read as one little-endian integer."""
    key = hashlib.blake2b(data, key=b"MuHashElement", digest_size=32).digest()
    words = list(struct.unpack("<8I", key))
    stream = b"".join(_chacha20_block(words, c) for c in range(6))
    return int.from_bytes(stream, "little")


def write_utxo(op36, u):
    """muhash.rs:55-69 over an outpoint and a blob.utxo_entry dict."""
    data = (op36 + struct.pack("<QQ", u["daa_score"], u["amount"])
            + bytes([1 if u["is_coinbase"] else 0])
            + struct.pack("<HQ", u["spk_version"], len(u["spk"])) + u["spk"])
    if u["covenant_id"]:
        data += u["covenant_id"]
    return data


_elements = {}


def utxo_element(op36, u):
    data = write_utxo(op36, u)
    v = _elements.get(data)
    if v is None:
        v = _elements[data] = element_of(data)
    return v


def product(items):
    """items: iterable of (op36, utxo_entry dict)."""
    acc = 1
    for op, u in items:
        acc = acc * utxo_element(op, u) % P
    return acc


def block_partial(txs, codes, block_daa):
    """(numerator, denominator) of a validated block: the created outputs and
    the spent entries of its accepted transactions (muhash.rs add_transaction)."""
    created, spent = [], []
    for tx, code in zip(txs, codes):
        if code:
            continue
        for i in tx["inputs"]:
            spent.append((i["prev_tx_id"] + struct.pack("<I", i["prev_index"]),
                          i["utxo"]))
        for k, o in enumerate(tx["outputs"]):
            created.append((tx["tx_id"] + struct.pack("<I", k),
                            output_entry(o, block_daa)))
    return product(created), product(spent)


def output_entry(o, block_daa):
    return B.utxo_entry(o["value"], o["spk"], block_daa, False, o["spk_version"],
                        o["covenant"][1] if o["covenant"] else None)


# ---------------- scenario transactions ----------------

def rand_bytes(rng, n):
    return bytes(rng.randrange(256) for _ in range(n))


def cov_tx(rng, input_cov_ids, outputs, *, correct=True, in_spk_version=1,
           in_spks=None, out_spk_lens=None, version=1):
    """A transaction in the shape of create_genesis_tx (covenants.rs:190).

    input_cov_ids: per input, a 32-byte id or None.
    outputs: per output, None (no binding) or (authorizing_input, group).
      A group that is a 32-byte id equal to that input's id is a continuation
      and is used as is. Any other group is a genesis label: outputs sharing
      (authorizing_input, label) get the id recomputed over them, or, with
      correct=False, a random id.
    Spent entries have script version >= 1 by default, which the script engine
    accepts unseen, so no signature is needed.
    """
    ins = []
    for i, cid in enumerate(input_cov_ids):
        spk = in_spks[i] if in_spks else rand_bytes(rng, 34)
        ins.append(B.tx_input(
            rand_bytes(rng, 32), i, sequence=1 << 63,
            utxo=B.utxo_entry(10**10 + i, spk, daa_score=5, spk_version=in_spk_version,
                              covenant_id=cid)))
    outs = []
    for k, cfg in enumerate(outputs):
        n = out_spk_lens[k] if out_spk_lens else 34
        outs.append(B.tx_output(10**8 + k, rand_bytes(rng, n), spk_version=k % 2))
    groups = {}
    for k, cfg in enumerate(outputs):
        if cfg is None:
            continue
        auth, group = cfg
        if auth < len(ins) and group == input_cov_ids[auth]:
            outs[k]["covenant"] = (auth, group)
        else:
            groups.setdefault((auth, group), []).append(k)
    for (auth, _), members in groups.items():
        if correct and auth < len(ins):
            cid = covenant_id(ins[auth]["prev_tx_id"], ins[auth]["prev_index"],
                              [(k, outs[k]["value"], outs[k]["spk_version"],
                                outs[k]["spk"]) for k in members])
        else:
            cid = rand_bytes(rng, 32)
        for k in members:
            outs[k]["covenant"] = (auth, cid)
    return B.tx_dict(version=version, inputs=ins, outputs=outs,
                     tx_id=rand_bytes(rng, 32))


X = bytes([42]) + bytes(31)  # the carried covenant id of the scenarios

# name -> (input_cov_ids, outputs, kwargs, expected code)
SCENARIOS = {
    "genesis_single_output": ([None], [(0, 1)], {}, 0),
    "genesis_two_outputs_one_group": ([None], [(0, 1), (0, 1)], {}, 0),
    "two_groups_interleaved": ([None], [(0, 1), (0, 2), (0, 1)], {}, 0),
    "two_inputs_one_group_each": ([None, None], [(0, 1), (1, 2)], {}, 0),
    "continuation_with_genesis":
        ([X], [(0, X), (0, 100), (0, 200), (0, 100)], {}, 0),
    "wrong_genesis_id": ([None], [(0, 1)], {"correct": False}, ERR_GENESIS_ID),
    "auth_input_out_of_bounds": ([None], [(1, 1)], {}, ERR_AUTH_INPUT),
    "input_id_no_covenant_outputs": ([X], [None, None], {}, 0),
    "genesis_group_script_lengths":
        ([None], [(0, 1)] * 4, {"out_spk_lens": [0, 36, 37, 300]}, 0),
}


def scenario_tx(rng, name, **over):
    ids, outs, kw, code = SCENARIOS[name]
    return cov_tx(rng, ids, outs, **{**kw, **over}), code
