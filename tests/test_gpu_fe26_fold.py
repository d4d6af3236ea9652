"""GPU parity of the verify kernels over the half-word field reduction
(fe26_reduce19): the device build differs from the host-test build in its
opaque fold multipliers and in how the compiler picks multiply-adds, so the
host tests do not cover its code generation.

Schnorr batches of 1, 64, 65 and 257 tuples through the fused kernel and
through the split path (ladder + batched finish, an engine created with
KV_SCHNORR_SPLIT_MIN=1), ECDSA batches of 1 and 65. About a third of the
tuples carry one flipped bit in s, in r or in the message. Status bytes and
bitmap must equal the oracle's verdicts tuple by tuple.
"""
import ctypes
import os
import random

import pytest

pytestmark = pytest.mark.gpu

# oracle verdict -> kernel status (KVS_VALID / INVALID / BAD_PUBKEY / BAD_SIG)
STATUS_OF = {1: 0, 0: 1, -1: 2, -2: 3}
ENV = "KV_SCHNORR_SPLIT_MIN"
N_MAX = 257


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
    yield {"split": split, "fused": fused}
    split.close()
    fused.close()


def spoil(tuples, size, msg_at, rng):
    """Every third tuple gets one flipped bit: in s, in r, in the message."""
    out = []
    for i in range(len(tuples) // size):
        t = bytearray(tuples[i * size:(i + 1) * size])
        if i % 3 == 1:
            start = (32, 0, msg_at)[(i // 3) % 3]
            bit = rng.randrange(256)
            t[start + bit // 8] ^= 1 << (bit % 8)
        out.append(bytes(t))
    return out


@pytest.fixture(scope="module")
def schnorr_cases(oracle):
    buf = ctypes.create_string_buffer(N_MAX * 128)
    oracle.ok_gen_schnorr_tuples(ctypes.c_uint64(601), ctypes.c_size_t(N_MAX), 0, buf, 4)
    tuples = spoil(buf.raw[: N_MAX * 128], 128, 96, random.Random(602))
    expect = [oracle.ok_schnorr_verify(t[64:96], t[96:128], t[0:64]) for t in tuples]
    assert expect[0::3] == [1] * len(expect[0::3])
    assert 1 not in expect[1::3]
    return tuples, expect


@pytest.fixture(scope="module")
def ecdsa_cases(oracle):
    n = 65
    buf = ctypes.create_string_buffer(n * 132)
    oracle.ok_gen_ecdsa_tuples(ctypes.c_uint64(603), ctypes.c_size_t(n), 0, buf, 4)
    tuples = spoil(buf.raw[: n * 132], 132, 97, random.Random(604))
    expect = [oracle.ok_ecdsa_verify(t[64:97], t[97:129], t[0:64]) for t in tuples]
    assert expect[0::3] == [1] * len(expect[0::3])
    assert 1 not in expect[1::3]
    return tuples, expect


def compare(bitmap, status, expect, n):
    assert len(bitmap) == (n + 63) // 64
    for i, e in enumerate(expect[:n]):
        assert (bitmap[i // 64] >> (i % 64)) & 1 == (1 if e == 1 else 0), i
        assert status[i] == STATUS_OF[e], (i, status[i], e)
    assert bitmap[-1] >> ((n - 1) % 64 + 1) == 0


@pytest.mark.parametrize("n", [1, 64, 65, 257])
@pytest.mark.parametrize("path", ["fused", "split"])
def test_schnorr_matches_oracle(engines, schnorr_cases, path, n):
    tuples, expect = schnorr_cases
    bitmap, status = engines[path].verify_schnorr_batch(b"".join(tuples[:n]), n,
                                                        with_status=True)
    compare(bitmap, status, expect, n)


@pytest.mark.parametrize("n", [1, 65])
def test_ecdsa_matches_oracle(engines, ecdsa_cases, n):
    tuples, expect = ecdsa_cases
    bitmap, status = engines["fused"].verify_ecdsa_batch(b"".join(tuples[:n]), n,
                                                         with_status=True)
    compare(bitmap, status, expect, n)
