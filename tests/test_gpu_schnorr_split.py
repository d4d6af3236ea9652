"""GPU parity of the split Schnorr verify (ladder kernel + batched finish) with
the fused kernel and with the oracle: one engine with KV_SCHNORR_SPLIT_MIN=1,
one with the fused path forced, the same batches through both with status.

Batch sizes 1, 65 and 64*K + 65 (K = signatures per finish lane, as compiled):
the last one gives several rows per lane, a partial last bitmap word and lanes
with fewer than K entries. Each batch cycles through valid tuples, s-flipped and
msg-flipped copies, a public key x that is not on the curve, r >= p and s >= n.
"""
import ctypes
import os
import random

import pytest

pytestmark = pytest.mark.gpu

P = 2**256 - 0x1000003D1
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
# oracle verdict -> kernel status (KVS_VALID / INVALID / BAD_PUBKEY / BAD_SIG)
STATUS_OF = {1: 0, 0: 1, -1: 2, -2: 3}
ENV = "KV_SCHNORR_SPLIT_MIN"


def engine_with(split_min):
    from rusty_kaspa_amd.engine import Engine
    saved = os.environ.get(ENV)
    os.environ[ENV] = str(split_min)
    try:
        return Engine()  # the variable is read once, in kv_create
    finally:
        if saved is None:
            del os.environ[ENV]
        else:
            os.environ[ENV] = saved


@pytest.fixture(scope="module")
def engines():
    split, fused = engine_with(1), engine_with(1 << 62)
    yield split, fused
    split.close()
    fused.close()


@pytest.fixture(scope="module")
def finish_k(engines):
    k = engines[0].lib.kv_schnorr_finish_batch()
    assert k in (8, 16, 32)
    return k


def flip(b, rng):
    bit = rng.randrange(256)
    out = bytearray(b)
    out[bit // 8] ^= 1 << (bit % 8)
    return bytes(out)


def off_curve_x(rng):
    while True:
        x = rng.randrange(1, P)
        if pow((x * x * x + 7) % P, (P - 1) // 2, P) != 1:
            return x.to_bytes(32, "big")


@pytest.fixture(scope="module")
def cases(oracle, finish_k):
    """(tuples, oracle verdicts) for the largest batch; smaller ones are
    prefixes. Built once."""
    rng = random.Random(401)
    n = 64 * finish_k + 65
    tuples = []
    while len(tuples) < n:
        key = rng.randrange(1, N).to_bytes(32, "big")
        msg = bytes(rng.randrange(256) for _ in range(32))
        sig = (ctypes.c_uint8 * 64)()
        pk = (ctypes.c_uint8 * 32)()
        assert oracle.ok_schnorr_sign(key, msg, None, sig) == 1
        assert oracle.ok_pubkey_xonly(key, pk) == 1
        sig, pk = bytes(sig), bytes(pk)
        r_big = (P + rng.randrange(0x1000003D1)).to_bytes(32, "big")
        s_big = (N + rng.randrange(2**256 - N)).to_bytes(32, "big")
        tuples += [
            (sig, pk, msg),
            (sig[:32] + flip(sig[32:], rng), pk, msg),
            (sig, pk, flip(msg, rng)),
            (sig, off_curve_x(rng), msg),
            (r_big + sig[32:], pk, msg),
            (sig[:32] + s_big, pk, msg),
        ]
    tuples = tuples[:n]
    expect = [oracle.ok_schnorr_verify(pk, msg, sig) for sig, pk, msg in tuples]
    assert expect[0::6] == [1] * len(expect[0::6])
    assert set(expect[3::6]) == {-1}
    assert 1 not in [e for i, e in enumerate(expect) if i % 6]
    return [sig + pk + msg for sig, pk, msg in tuples], expect


@pytest.mark.parametrize("size", ["1", "65", "64K+65"])
def test_split_matches_fused_and_oracle(engines, cases, finish_k, size):
    n = {"1": 1, "65": 65, "64K+65": 64 * finish_k + 65}[size]
    tuples, expect = cases
    raw = b"".join(tuples[:n])
    split, fused = engines
    bm_s, st_s = split.verify_schnorr_batch(raw, n, with_status=True)
    bm_f, st_f = fused.verify_schnorr_batch(raw, n, with_status=True)
    assert bm_s == bm_f
    assert st_s == st_f
    assert len(bm_s) == (n + 63) // 64
    for i, e in enumerate(expect[:n]):
        assert (bm_s[i // 64] >> (i % 64)) & 1 == (1 if e == 1 else 0), i
        assert st_s[i] == STATUS_OF[e], (i, st_s[i], e)
    # bits past n in the last word are zero
    assert bm_s[-1] >> ((n - 1) % 64 + 1) == 0
