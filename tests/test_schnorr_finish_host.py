"""The batched Schnorr finish (schnorr_finish_lane: Montgomery's trick over the
K entries of one lane), run ON CPU from the device sources through
tests/host_shim/finish.cpp with K as compiled, against affine checks built on
pow(z, -1, p). Entries are random curve points in random Jacobian scalings;
non-pending and infinity entries must be neutral for their neighbours."""
import ctypes
import random

import pytest

from test_fe26_reduce_host import P, build_finish_shim, to26

VALID, INVALID, BAD_PUBKEY = 0, 1, 2
GARBAGE = [0xFFFFFFFF] * 10  # limbs of a non-pending entry: never to be used


@pytest.fixture(scope="module")
def shim():
    return build_finish_shim()


def random_affine(rng, odd):
    while True:
        x = rng.randrange(1, P)
        y2 = (x * x * x + 7) % P
        y = pow(y2, (P + 1) // 4, P)
        if y * y % P == y2:
            return x, (y if (y & 1) == odd else P - y)


def entry(rng, kind):
    """(pre, X, Y, Z limbs, r, expected code)"""
    if kind == "nonpending":
        code = rng.choice((INVALID, BAD_PUBKEY))
        return code, GARBAGE, GARBAGE, GARBAGE, rng.randrange(P), code
    x, y = random_affine(rng, odd=int(kind == "odd"))
    lam = rng.randrange(1, P)
    X, Y, Z = x * lam * lam % P, y * pow(lam, 3, P) % P, lam
    if rng.random() < 0.3:  # same residues, not canonical (value + p)
        X, Y, Z = X + P, Y + P, Z + P
    # nine 26-bit digits and whatever is left on top (23 bits for value + p)
    limbs = lambda v: to26(v)[:9] + [v >> 234]
    lx, ly, lz = limbs(X), limbs(Y), limbs(Z)
    r = x
    if kind == "differ":
        r = (x + 1 + rng.randrange(P - 1)) % P
    if kind == "inf0":
        lz = [0] * 10
    if kind == "infp":
        lz = to26(P)
    # the reference verdict, from the affine coordinates
    z = sum(l << (26 * i) for i, l in enumerate(lz)) % P
    if z == 0:
        want = INVALID
    else:
        zi = pow(z, -1, P)
        xa, ya = X * zi * zi % P, Y * pow(zi, 3, P) % P
        assert (xa, ya) == (x, y)
        want = VALID if (ya & 1) == 0 and xa == r else INVALID
    assert want == (VALID if kind == "match" else INVALID)
    return 0, lx, ly, lz, r, want


def run_lanes(shim, entries, lanes):
    """Lay the entries out as the ladder kernel does and finish them with
    `lanes` lanes (lane t takes entries m*lanes + t). Returns the codes."""
    k = shim.host_finish_k()
    n = len(entries)
    assert lanes * k >= n
    limbs = (ctypes.c_uint32 * (30 * n))()
    pre = (ctypes.c_uint8 * n)()
    tuples = (ctypes.c_uint8 * (128 * n))()
    for i, (p, lx, ly, lz, r, _) in enumerate(entries):
        pre[i] = p
        for j in range(10):
            limbs[j * n + i] = lx[j]
            limbs[(10 + j) * n + i] = ly[j]
            limbs[(20 + j) * n + i] = lz[j]
        tuples[128 * i:128 * i + 32] = list(r.to_bytes(32, "big"))
    got = [None] * n
    for t in range(lanes):
        st = (ctypes.c_uint8 * k)()
        shim.host_schnorr_finish_lane(limbs, pre, tuples,
                                      ctypes.c_ulonglong(n), ctypes.c_ulonglong(t),
                                      ctypes.c_ulonglong(lanes), st)
        for m in range(k):
            if m * lanes + t < n:
                got[m * lanes + t] = st[m]
    return got


def check(shim, entries, lanes=1):
    got = run_lanes(shim, entries, lanes)
    assert got == [e[5] for e in entries]


REGULAR = ("match", "differ", "odd")
NEUTRAL = ("nonpending", "inf0", "infp")


def test_k_is_a_supported_batch(shim):
    assert shim.host_finish_k() in (8, 16, 32)


def test_regular_entries(shim):
    rng = random.Random(51)
    k = shim.host_finish_k()
    check(shim, [entry(rng, REGULAR[i % 3]) for i in range(k)])
    check(shim, [entry(rng, "match") for _ in range(k)])
    check(shim, [entry(rng, rng.choice(REGULAR)) for _ in range(k)])


@pytest.mark.parametrize("kind", NEUTRAL)
def test_neutral_entry_at_each_position(shim, kind):
    rng = random.Random(52)
    k = shim.host_finish_k()
    for pos in (0, k // 2, k - 1):
        es = [entry(rng, REGULAR[i % 3]) for i in range(k)]
        es[pos] = entry(rng, kind)
        # the neighbours keep their verdicts, valid ones included
        for nb in (pos - 1, pos + 1):
            if 0 <= nb < k:
                es[nb] = entry(rng, "match")
        check(shim, es)


def test_neutral_entries_together(shim):
    rng = random.Random(53)
    k = shim.host_finish_k()
    es = [entry(rng, "match") for _ in range(k)]
    es[0] = entry(rng, "inf0")
    es[k // 2] = entry(rng, "nonpending")
    es[k - 1] = entry(rng, "infp")
    check(shim, es)


def test_batch_of_neutral_entries_only(shim):
    rng = random.Random(54)
    k = shim.host_finish_k()
    check(shim, [entry(rng, NEUTRAL[i % 3]) for i in range(k)])
    check(shim, [entry(rng, "nonpending") for _ in range(k)])
    check(shim, [entry(rng, "inf0") for _ in range(k)])


def test_strided_lanes_with_short_last_rows(shim):
    """Three lanes over 3K-2 entries: lane t takes m*3 + t, the last lane has
    an entry past n, which must stay out of its product."""
    rng = random.Random(55)
    k = shim.host_finish_k()
    n = 3 * k - 2
    es = [entry(rng, rng.choice(REGULAR + ("match",))) for _ in range(n)]
    for pos, kind in ((0, "nonpending"), (n // 2, "inf0"), (n - 1, "infp"),
                      (n - 2, "nonpending")):
        es[pos] = entry(rng, kind)
    check(shim, es, lanes=3)
    # one entry only: every other row of the lane is out of range
    check(shim, [entry(rng, "match")], lanes=1)
    check(shim, [entry(rng, "odd")], lanes=1)
