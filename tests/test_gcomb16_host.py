"""The joint 16-bit fixed-base table, run ON CPU from the device sources
(tests/host_shim/gcomb16.cpp, g++, KV_HOST_TEST magnitude asserts live) against
Python big-int secp256k1: the per-entry build routine and the unpack, the
2^128·G multiples, and ecmult_double over the G scalars that walk the table's
edges, alone and beside a P stream."""
import ctypes
import os
import random
import subprocess

import pytest

from secp_bigint import (G, N, P, crafted_g_scalars, ec_add, ec_mul,
                         joint_entry, multiples)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_DIR = os.path.join(REPO, "tests", "host_shim")
CSRC = os.path.join(REPO, "rusty_kaspa_amd", "csrc")
LIB = os.path.join(SHIM_DIR, "libgcomb16shim.so")
M26 = (1 << 26) - 1


@pytest.fixture(scope="module")
def shim():
    srcs = [os.path.join(SHIM_DIR, f) for f in ("gcomb16.cpp", "main.cpp", "shim.h")]
    srcs += [os.path.join(CSRC, f) for f in ("kv_secp_device.h", "kv_hash_device.h",
                                             "kv_secp_kernels.hip")]
    if (not os.path.exists(LIB)
            or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in srcs)):
        subprocess.run(["g++", "-O1", "-fPIC", "-shared", "-I", CSRC,
                        "-I", SHIM_DIR, srcs[0], "-o", LIB], check=True)
    lib = ctypes.CDLL(LIB)
    lib.host_init_gtable()
    assert lib.host_g16_joint_ladder() == 1  # the default build's ladder
    return lib


@pytest.fixture(scope="module")
def ref():
    """(multiples of G, multiples of H), computed once and never modified."""
    h = ec_mul(1 << 128, G)
    return tuple(multiples(G, 255)), tuple(multiples(h, 255))


def val(a):
    return sum(int(a[i]) << (26 * i) for i in range(10))


def to26(v):
    return [(v >> (26 * i)) & M26 for i in range(10)]


def arr(limbs):
    return (ctypes.c_uint32 * 10)(*limbs)


def u256(k):
    return (ctypes.c_uint64 * 4)(*[(k >> (64 * i)) & (2**64 - 1) for i in range(4)])


# ---------- per-entry build and unpack ----------

def test_entry_build_and_unpack(shim, ref):
    rng = random.Random(51)
    idxs = [0x0000, 0x0001, 0x00FF, 0x0100, 0xFF00, 0x0101, 0xFFFF]
    idxs += [rng.randrange(1 << 16) for _ in range(64)]
    for idx in idxs:
        raw = (ctypes.c_uint32 * 16)()
        xy = (ctypes.c_uint32 * 20)()
        assert shim.host_g16_entry(idx, raw, xy) == 0, hex(idx)
        want = joint_entry(idx, *ref)
        # packed form: canonical x then y, 8 little-endian words each
        x = sum(int(raw[i]) << (32 * i) for i in range(8))
        y = sum(int(raw[8 + i]) << (32 * i) for i in range(8))
        assert (x, y) == want, hex(idx)
        # the unpack gives the canonical limbs themselves (magnitude 1)
        assert list(xy[0:10]) == to26(want[0]), hex(idx)
        assert list(xy[10:20]) == to26(want[1]), hex(idx)
    assert shim.host_g16_entry(1 << 16, raw, xy) == -1


def test_entry_zero_is_g(shim, ref):
    assert joint_entry(0, *ref) == G  # the reference's own convention
    raw = (ctypes.c_uint32 * 16)()
    xy = (ctypes.c_uint32 * 20)()
    assert shim.host_g16_entry(0, raw, xy) == 0
    assert (val(xy[0:10]), val(xy[10:20])) == G


def test_h_multiples(shim, ref):
    out = (ctypes.c_uint32 * (256 * 20))()
    assert shim.host_h_table(out) == 256
    hmul = ref[1]
    for d in range(256):
        want = hmul[max(d, 1) - 1]  # entry 0 is H itself
        assert list(out[20 * d:20 * d + 10]) == to26(want[0]), d
        assert list(out[20 * d + 10:20 * d + 20]) == to26(want[1]), d


# ---------- ecmult_double ----------

def check_ecmult(shim, gs, ps, pt):
    out = (ctypes.c_uint32 * 30)()
    inf = shim.host_g16_ecmult_double(u256(gs), u256(ps), arr(to26(pt[0])),
                                      arr(to26(pt[1])), out)
    want = ec_add(ec_mul(gs, G), ec_mul(ps, pt))
    x, y, z = val(out[0:10]), val(out[10:20]), val(out[20:30])
    assert bool(inf) == (want is None) == (z == 0), (hex(gs), hex(ps), pt)
    if want is not None:
        zi = pow(z, -1, P)
        assert (x * zi * zi % P, y * zi ** 3 % P) == want, (hex(gs), hex(ps), pt)


def test_ecmult_g_alone(shim):
    pt = ec_mul(0x1234567, G)
    for gs in crafted_g_scalars():
        check_ecmult(shim, gs, 0, pt)  # R = gs·G (gs == 0: infinity)


def test_ecmult_crafted_g_with_random_p(shim):
    rng = random.Random(52)
    pt = ec_mul(rng.randrange(1, N), G)
    for gs in crafted_g_scalars():
        check_ecmult(shim, gs, rng.randrange(1, N), pt)


def test_ecmult_crafted_g_with_p_equal_g(shim):
    # P = G: the P table's entries collide with the G table's partial sums
    rng = random.Random(53)
    for gs in crafted_g_scalars():
        check_ecmult(shim, gs, rng.randrange(1, N), G)
        check_ecmult(shim, gs, (N - gs) % N, G)  # gs·G + (-gs)·G: infinity
        check_ecmult(shim, gs, gs, G)


def test_ecmult_random(shim):
    rng = random.Random(54)
    for _ in range(200):
        check_ecmult(shim, rng.randrange(N), rng.randrange(N),
                     ec_mul(rng.randrange(1, N), G))
