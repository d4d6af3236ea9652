"""The verify ladder's building blocks, run ON CPU from the device sources
(tests/host_shim/ladder.cpp, g++, KV_HOST_TEST magnitude asserts live) against
Python bigint and affine EC arithmetic: the doubled-operand squaring, the cheap
zero predicate, the inversion-free P table and ecmult_double with the crafted
scalars and points that valid signatures never reach."""
import ctypes
import os
import random
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_DIR = os.path.join(REPO, "tests", "host_shim")
CSRC = os.path.join(REPO, "rusty_kaspa_amd", "csrc")
LIB = os.path.join(SHIM_DIR, "libladdershim.so")

P = 2**256 - 0x1000003D1
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
     0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A6855419 << 64
     | 0x9C47D08FFB10D4B8)
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
M26 = (1 << 26) - 1


@pytest.fixture(scope="module")
def shim():
    srcs = [os.path.join(SHIM_DIR, f) for f in ("ladder.cpp", "main.cpp", "shim.h")]
    srcs += [os.path.join(CSRC, f) for f in ("kv_secp_device.h", "kv_hash_device.h",
                                             "kv_secp_kernels.hip")]
    if (not os.path.exists(LIB)
            or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in srcs)):
        subprocess.run(["g++", "-O1", "-fPIC", "-shared", "-I", CSRC,
                        "-I", SHIM_DIR, srcs[0], "-o", LIB], check=True)
    lib = ctypes.CDLL(LIB)
    lib.host_init_gtable()
    return lib


# ---------- python reference: field limbs and affine EC ----------

def arr(limbs):
    return (ctypes.c_uint32 * 10)(*limbs)


def val(a):
    return sum(int(a[i]) << (26 * i) for i in range(10))


def to26(v):
    return [(v >> (26 * i)) & M26 for i in range(10)]


def ec_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return (x, (lam * (a[0] - x) - a[1]) % P)


def ec_mul(k, pt):
    k %= N
    acc = None
    while k:
        if k & 1:
            acc = ec_add(acc, pt)
        pt = ec_add(pt, pt)
        k >>= 1
    return acc


# ---------- fe26_sqr ----------

def test_fe26_sqr_vs_bigint(shim):
    rng = random.Random(31)
    cases = [[1 << 30] * 10, [0] * 10]
    for m in (1, 2, 4, 8):
        for _ in range(1500):
            cases.append([rng.randrange(m << 26) for _ in range(9)]
                         + [rng.randrange(m << 22)])
        # limbs at the top of the magnitude's range
        cases.append([(m << 26) - 1] * 9 + [(m << 22) - 1])
    for a in cases:
        r = (ctypes.c_uint32 * 10)()
        shim.host_fe26_sqr(arr(a), r)
        assert val(r) % P == val(a) ** 2 % P, a
        assert all(r[i] <= 2 << 26 for i in range(10)), a  # output magnitude


# ---------- zero predicate ----------

NTZ_LIMB_BOUND = (1 << 31) - 1  # the predicate's stated domain: limbs < 2^31
NTZ_MAGNITUDES = (1, 2, 3, 5, 8, 15)


def limb_bound(m):
    """Largest limb at magnitude m (negate convention: limb <= 2m*2^26)."""
    return min(2 * m << 26, NTZ_LIMB_BOUND)


def decompose(v, bound, rng, greedy):
    """Limbs <= bound with value v, pushed away from the canonical digits:
    walking down from the top, limb i lends t units to limb i-1 (t*2^26 there),
    so lower limbs (l0/l1 included) carry overflow bits. None if v does not
    fit."""
    l = to26(v)
    l[9] = v >> 234
    for i in range(9, 0, -1):
        need = max(0, l[i] - bound)  # must lend at least this much to fit
        room = min(l[i], (bound - l[i - 1]) >> 26)
        if need > room:
            return None
        t = room if greedy else rng.choice((need, room, rng.randint(need, room)))
        l[i] -= t
        l[i - 1] += t << 26
    assert val(l) == v and max(l) <= bound
    return l


def test_normalizes_to_zero_vs_bigint(shim):
    rng = random.Random(32)
    ntz = lambda l: shim.host_fe26_normalizes_to_zero(arr(l))
    for m in NTZ_MAGNITUDES:
        bound = limb_bound(m)
        top = sum(bound << (26 * i) for i in range(10))
        k, hits = 0, 0
        while k * P - 1 <= top:
            for v in (k * P - 1, k * P, k * P + 1):
                if v < 0:
                    continue
                forms = [decompose(v, bound, rng, True)]
                forms += [decompose(v, bound, rng, False) for _ in range(4)]
                for l in forms:
                    if l is None:
                        continue
                    assert ntz(l) == (v % P == 0), (m, k, v - k * P, l)
                    hits += v == k * P
            k += 1
        # the multiples were really tried (the last few fit only some forms)
        assert k >= 32 * m and hits >= 5 * (k - 2)
        for _ in range(3000):
            l = [rng.randrange(bound + 1) for _ in range(10)]
            assert ntz(l) == (val(l) % P == 0), (m, l)
    # canonical 0 and p, and p with the overflow pushed into l0/l1 only
    assert ntz([0] * 10) == 1
    assert ntz(to26(P)) == 1
    pl = to26(P)
    assert ntz([pl[0] + (1 << 26), pl[1] - 1] + pl[2:]) == 1
    assert ntz([pl[0] + (1 << 26), pl[1]] + pl[2:]) == 0


# ---------- rescaled P table ----------

def random_point(rng):
    return ec_mul(rng.randrange(1, N), G)


def test_ptab_is_k_times_p_over_zg(shim):
    rng = random.Random(33)
    for pt in [G] + [random_point(rng) for _ in range(12)]:
        out = (ctypes.c_uint32 * 160)()
        zg = (ctypes.c_uint32 * 10)()
        assert shim.host_ptab_build(arr(to26(pt[0])), arr(to26(pt[1])), out, zg) == 8
        z = val(zg)
        assert z % P != 0
        zi = pow(z, -1, P)
        kp = None
        for k in range(1, 9):
            kp = ec_add(kp, pt)
            x = val(out[20 * (k - 1):20 * (k - 1) + 10])
            y = val(out[20 * (k - 1) + 10:20 * k])
            assert (x * zi * zi % P, y * zi ** 3 % P) == kp, k


# ---------- ecmult_double ----------

def glv_halves(shim, k):
    out = (ctypes.c_uint64 * 8)()
    shim.host_glv_split((ctypes.c_uint64 * 4)(*[(k >> (64 * i)) & (2**64 - 1)
                                                for i in range(4)]), out)
    h = lambda o: out[o] | (out[o + 1] << 64) | (out[o + 2] << 128)
    return h(0), h(4)


def recode(h):
    """The kernel's signed 4-bit recode (33 digits, LSB first)."""
    dig, carry = [], 0
    for w in range(33):
        v = ((h >> (4 * w)) & 15) + carry
        carry = int(v > 8)
        dig.append(v - 16 * carry)
    return dig


def check_ecmult(shim, gs, ps, pt):
    out = (ctypes.c_uint32 * 30)()
    u = lambda k: (ctypes.c_uint64 * 4)(*[(k >> (64 * i)) & (2**64 - 1)
                                          for i in range(4)])
    inf = shim.host_ecmult_double(u(gs), u(ps), arr(to26(pt[0])),
                                  arr(to26(pt[1])), out)
    want = ec_add(ec_mul(gs, G), ec_mul(ps, pt))
    x, y, z = val(out[0:10]), val(out[10:20]), val(out[20:30])
    assert bool(inf) == (want is None) == (z == 0), (gs, ps, pt)
    if want is not None:
        zi = pow(z, -1, P)
        assert (x * zi * zi % P, y * zi ** 3 % P) == want, (gs, ps, pt)


def test_ecmult_double_random(shim):
    rng = random.Random(34)
    for _ in range(24):
        check_ecmult(shim, rng.randrange(N), rng.randrange(N), random_point(rng))


def test_ecmult_double_zero_scalars(shim):
    rng = random.Random(35)
    pt = random_point(rng)
    k = rng.randrange(1, N)
    check_ecmult(shim, 0, k, pt)
    check_ecmult(shim, k, 0, pt)
    check_ecmult(shim, 0, 0, pt)  # every digit zero: infinity


def test_ecmult_double_extreme_digits(shim):
    rng = random.Random(36)
    pt = random_point(rng)
    # k = e - e·λ with e = 0x88..8: the split returns the halves (+e, -e), so
    # every recoded digit below the top window is 8 and the streams add
    # +8·P and -8·φP (the split never returns a negative first half)
    for nibbles in (32, 31):
        eights = int("8" * nibbles, 16)
        k = (eights - eights * LAMBDA) % N
        h1, h2 = glv_halves(shim, k)
        assert h1 == eights and h2 == eights
        assert recode(h1)[:nibbles] == [8] * nibbles
        check_ecmult(shim, k, k, pt)
        check_ecmult(shim, k, rng.randrange(N), pt)
        check_ecmult(shim, rng.randrange(N), k, pt)
    # bit 128 of a half-scalar set: the top window (first frame) is non-zero
    found = 0
    for t in range(1 << 12):
        k = ((1 << 128) + rng.getrandbits(120)
             + rng.choice((1, -1)) * rng.getrandbits(127) * LAMBDA) % N
        if any(h >> 128 for h in glv_halves(shim, k)):
            found += 1
            check_ecmult(shim, k, k, pt)
            check_ecmult(shim, rng.randrange(N), k, pt)
            if found == 4:
                break
    assert found == 4


def test_ecmult_double_same_and_opposite_points(shim):
    rng = random.Random(37)
    for _ in range(6):
        ps = rng.randrange(1, N)
        check_ecmult(shim, ps, ps, G)      # same-x doubling in every window
        check_ecmult(shim, N - ps, ps, G)  # opposite points: infinity
    check_ecmult(shim, 1, 1, G)
    check_ecmult(shim, N - 1, 1, G)


def test_ecmult_double_p_table_collides_with_g_table(shim):
    rng = random.Random(38)
    for k in range(2, 9):
        pt = ec_mul(k, G)
        check_ecmult(shim, rng.randrange(N), rng.randrange(N), pt)
        ps = rng.randrange(1, N)
        check_ecmult(shim, k * ps % N, ps, pt)        # gs·G == ps·P
        check_ecmult(shim, (N - k * ps) % N, ps, pt)  # gs·G == -ps·P
        check_ecmult(shim, rng.randrange(256), rng.randrange(16), pt)
