"""GPU checks of the joint 16-bit fixed-base table: every entry as the device
built it against Python big-ints, ECDSA tuples crafted so that the G scalar u1
walks the table's edges, and Schnorr tuples of the same keys through the fused
and the split verify path, all against the oracle's verdicts."""
import ctypes
import os
import random

import pytest

from secp_bigint import (G, N, P, crafted_g_scalars, ec_mul, multiples)

pytestmark = pytest.mark.gpu

# oracle verdict -> kernel status (KVS_VALID / INVALID / BAD_PUBKEY / BAD_SIG)
STATUS_OF = {1: 0, 0: 1, -1: 2, -2: 3}
ENV = "KV_SCHNORR_SPLIT_MIN"
N_KEYS = 22  # 22 valid tuples + two siblings each = 66 >= 65


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
def keys():
    rng = random.Random(601)
    return tuple(rng.randrange(1, N) for _ in range(N_KEYS))


def flip(b, rng):
    bit = rng.randrange(256)
    out = bytearray(b)
    out[bit // 8] ^= 1 << (bit % 8)
    return bytes(out)


def b32(v):
    return v.to_bytes(32, "big")


# ---------- (a) the whole table ----------

def reference_table():
    """All 65,536 entries as (x, y): two 255-step chains, then the 65,025 sums
    lo·G + hi·H as affine adds sharing one batch inversion."""
    gmul = multiples(G, 255)
    hmul = multiples(ec_mul(1 << 128, G), 255)
    table = [None] * 65536
    table[0] = G
    for d in range(1, 256):
        table[d] = gmul[d - 1]
        table[d << 8] = hmul[d - 1]
    pairs = [(lo, hi) for hi in range(1, 256) for lo in range(1, 256)]
    dx = [(hmul[hi - 1][0] - gmul[lo - 1][0]) % P for lo, hi in pairs]
    assert all(dx)  # lo·G and hi·H never share an x
    pref, acc = [], 1
    for v in dx:
        pref.append(acc)
        acc = acc * v % P
    inv = pow(acc, -1, P)
    for k in range(len(pairs) - 1, -1, -1):
        lo, hi = pairs[k]
        a, b = gmul[lo - 1], hmul[hi - 1]
        lam = (b[1] - a[1]) * (inv * pref[k] % P) % P
        inv = inv * dx[k] % P
        x = (lam * lam - a[0] - b[0]) % P
        table[hi << 8 | lo] = (x, (lam * (a[0] - x) - a[1]) % P)
    return table


def test_every_entry_matches_bigint(engines):
    eng = engines[0]
    raw = eng.g_comb_fetch(0, 65536)
    assert len(raw) == 65536 * 64
    want = reference_table()
    for idx in range(65536):
        e = raw[64 * idx:64 * idx + 64]
        got = (int.from_bytes(e[0:32], "little"), int.from_bytes(e[32:64], "little"))
        assert got == want[idx], hex(idx)
    # partial fetches address the same entries; out-of-range ones are refused
    assert eng.g_comb_fetch(0xFFFF, 1) == raw[-64:]
    assert eng.g_comb_fetch(0x0100, 3) == raw[64 * 0x100:64 * 0x103]
    buf = (ctypes.c_uint8 * 128)()
    ctx = ctypes.c_void_p(eng.ctx)
    assert eng.lib.kv_g_comb_fetch(ctx, ctypes.c_uint32(65535),
                                   ctypes.c_uint32(2), buf) == -1
    assert eng.lib.kv_g_comb_fetch(ctx, ctypes.c_uint32(65537),
                                   ctypes.c_uint32(0), buf) == -1


# ---------- (b) ECDSA with a chosen u1 ----------

@pytest.fixture(scope="module")
def ecdsa_cases(oracle, keys):
    """(132-byte tuples, oracle verdicts): per key one valid tuple whose G
    scalar is a crafted u1, then its s-flipped and msg-flipped siblings. The
    tuple's msg is the digest z itself, so z = u1·s fixes u1 = z/s."""
    rng = random.Random(602)
    crafted = crafted_g_scalars()
    tuples = []
    for k, d in enumerate(keys):
        u1 = crafted[k % len(crafted)]
        pk = (ctypes.c_uint8 * 33)()
        assert oracle.ok_pubkey_compressed(b32(d), pk) == 1
        pk = bytes(pk)
        while True:
            u2 = rng.randrange(1, N)
            pt = ec_mul((u1 + u2 * d) % N, G)
            if pt is None:
                continue
            r = pt[0] % N
            s = r * pow(u2, -1, N) % N
            if r == 0 or s == 0 or s > N // 2:
                continue
            break
        z = u1 * s % N
        sig, msg = b32(r) + b32(s), b32(z)
        tuples += [(sig, pk, msg),
                   (sig[:32] + flip(sig[32:], rng), pk, msg),
                   (sig, pk, flip(msg, rng))]
    expect = [oracle.ok_ecdsa_verify(pk, msg, sig) for sig, pk, msg in tuples]
    assert expect[0::3] == [1] * N_KEYS
    assert 1 not in [e for i, e in enumerate(expect) if i % 3]
    return [sig + pk + msg + b"\0\0\0" for sig, pk, msg in tuples], expect


@pytest.mark.parametrize("n", [1, 65])
def test_ecdsa_chosen_g_scalar(engines, ecdsa_cases, n):
    tuples, expect = ecdsa_cases
    bitmap, status = engines[0].verify_ecdsa_batch(b"".join(tuples[:n]), n,
                                                   with_status=True)
    for i, e in enumerate(expect[:n]):
        assert (bitmap[i // 64] >> (i % 64)) & 1 == (1 if e == 1 else 0), i
        assert status[i] == STATUS_OF[e], (i, status[i], e)
    assert bitmap[-1] >> ((n - 1) % 64 + 1) == 0


# ---------- (c) Schnorr, fused and split ----------

@pytest.fixture(scope="module")
def schnorr_cases(oracle, keys):
    rng = random.Random(603)
    tuples = []
    for d in keys:
        msg = bytes(rng.randrange(256) for _ in range(32))
        sig = (ctypes.c_uint8 * 64)()
        pk = (ctypes.c_uint8 * 32)()
        assert oracle.ok_schnorr_sign(b32(d), msg, None, sig) == 1
        assert oracle.ok_pubkey_xonly(b32(d), pk) == 1
        sig, pk = bytes(sig), bytes(pk)
        tuples += [(sig, pk, msg),
                   (sig[:32] + flip(sig[32:], rng), pk, msg),
                   (sig, pk, flip(msg, rng))]
    expect = [oracle.ok_schnorr_verify(pk, msg, sig) for sig, pk, msg in tuples]
    assert expect[0::3] == [1] * N_KEYS
    assert 1 not in [e for i, e in enumerate(expect) if i % 3]
    return [sig + pk + msg for sig, pk, msg in tuples], expect


def test_schnorr_fused_and_split(engines, schnorr_cases):
    n = 65
    tuples, expect = schnorr_cases
    raw = b"".join(tuples[:n])
    split, fused = engines
    bm_s, st_s = split.verify_schnorr_batch(raw, n, with_status=True)
    bm_f, st_f = fused.verify_schnorr_batch(raw, n, with_status=True)
    assert bm_s == bm_f and st_s == st_f
    for i, e in enumerate(expect[:n]):
        assert (bm_s[i // 64] >> (i % 64)) & 1 == (1 if e == 1 else 0), i
        assert st_s[i] == STATUS_OF[e], (i, st_s[i], e)
    assert bm_s[-1] >> ((n - 1) % 64 + 1) == 0
