"""GPU parity for the verify ladder (inversion-free P table, first-window frame,
cheap zero tests): per-tuple verdict bit AND status vs the oracle, on batches of
1 and 65 tuples (one full wave plus one lane).

Keys are 1..8 and n-8..n-1, so the P tables are small multiples of ±G: 2G..8G
also sit in the shared G table. Every valid tuple travels with a copy that has
one flipped bit in s and one that has one flipped bit in msg. The crafted
equal-x ladder cases cannot be reached through valid signatures; they are
covered on the same source by test_ladder_host.py.
"""
import ctypes
import random

import pytest

pytestmark = pytest.mark.gpu

N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
KEYS = list(range(1, 9)) + list(range(N - 8, N))
# oracle verdict -> kernel status (KVS_VALID / INVALID / BAD_PUBKEY / BAD_SIG)
STATUS_OF = {1: 0, 0: 1, -1: 2, -2: 3}
BATCHES = (1, 65)


@pytest.fixture(scope="module")
def engine():
    from rusty_kaspa_amd.engine import Engine
    eng = Engine()
    yield eng
    eng.close()


def flip(b, rng):
    bit = rng.randrange(256)
    out = bytearray(b)
    out[bit // 8] ^= 1 << (bit % 8)
    return bytes(out)


def triples(rng, sign, pubkey, pk_len):
    """(sig, pk, msg) triples: valid, s-flipped, msg-flipped, per key."""
    out = []
    for j in range(22):  # 66 tuples; keys wrap so each of the 16 gets a triple
        key = KEYS[j % len(KEYS)].to_bytes(32, "big")
        msg = bytes(rng.randrange(256) for _ in range(32))
        sig = (ctypes.c_uint8 * 64)()
        pk = (ctypes.c_uint8 * pk_len)()
        assert sign(key, msg, sig) == 1
        assert pubkey(key, pk) == 1
        sig, pk = bytes(sig), bytes(pk)
        out.append((sig, pk, msg))
        out.append((sig[:32] + flip(sig[32:], rng), pk, msg))
        out.append((sig, pk, flip(msg, rng)))
    return out


def check(bitmap, status, expect):
    for i, e in enumerate(expect):
        assert (bitmap[i // 64] >> (i % 64)) & 1 == (1 if e == 1 else 0), i
        assert status[i] == STATUS_OF[e], (i, status[i], e)


@pytest.fixture(scope="module")
def schnorr_cases(oracle):
    rng = random.Random(301)
    ts = triples(rng, lambda k, m, s: oracle.ok_schnorr_sign(k, m, None, s),
                 oracle.ok_pubkey_xonly, 32)
    expect = [oracle.ok_schnorr_verify(pk, msg, sig) for sig, pk, msg in ts]
    assert expect[0::3] == [1] * 22 and 1 not in expect[1::3] + expect[2::3]
    return [sig + pk + msg for sig, pk, msg in ts], expect


@pytest.fixture(scope="module")
def ecdsa_cases(oracle):
    rng = random.Random(302)
    ts = triples(rng, oracle.ok_ecdsa_sign, oracle.ok_pubkey_compressed, 33)
    expect = [oracle.ok_ecdsa_verify(pk, msg, sig) for sig, pk, msg in ts]
    assert expect[0::3] == [1] * 22 and 1 not in expect[1::3] + expect[2::3]
    return [sig + pk + msg + bytes(3) for sig, pk, msg in ts], expect


@pytest.mark.parametrize("n", BATCHES)
def test_schnorr_ladder_parity(engine, schnorr_cases, n):
    tuples, expect = schnorr_cases
    bitmap, status = engine.verify_schnorr_batch(b"".join(tuples[:n]), n,
                                                 with_status=True)
    check(bitmap, status, expect[:n])


@pytest.mark.parametrize("n", BATCHES)
def test_ecdsa_ladder_parity(engine, ecdsa_cases, n):
    tuples, expect = ecdsa_cases
    bitmap, status = engine.verify_ecdsa_batch(b"".join(tuples[:n]), n,
                                               with_status=True)
    check(bitmap, status, expect[:n])
