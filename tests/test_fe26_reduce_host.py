"""fe26_mul / fe26_sqr through the digit-first fe26_reduce19, run ON CPU from
the device sources (tests/host_shim/finish.cpp, g++, KV_HOST_TEST asserts live)
against Python bigints mod p. Every result is checked for its value and for the
output bound the header states: l0..l8 <= 2^26 and l9 < 2^22."""
import ctypes
import os
import random
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_DIR = os.path.join(REPO, "tests", "host_shim")
CSRC = os.path.join(REPO, "rusty_kaspa_amd", "csrc")
LIB = os.path.join(SHIM_DIR, "libfinishshim.so")

P = 2**256 - 0x1000003D1
M26 = (1 << 26) - 1
BOUND = 1 << 30  # the mul/sqr input bound: every limb <= 2^30


def build_finish_shim():
    srcs = [os.path.join(SHIM_DIR, f) for f in ("finish.cpp", "main.cpp", "shim.h")]
    srcs += [os.path.join(CSRC, f) for f in ("kv_secp_device.h", "kv_hash_device.h",
                                             "kv_secp_kernels.hip")]
    if (not os.path.exists(LIB)
            or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in srcs)):
        tmp = f"{LIB}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O1", "-fPIC", "-shared", "-I", CSRC,
                        "-I", SHIM_DIR, srcs[0], "-o", tmp], check=True)
        os.replace(tmp, LIB)
    return ctypes.CDLL(LIB)


@pytest.fixture(scope="module")
def shim():
    return build_finish_shim()


def arr(limbs):
    return (ctypes.c_uint32 * 10)(*limbs)


def val(a):
    return sum(int(a[i]) << (26 * i) for i in range(10))


def to26(v):
    return [(v >> (26 * i)) & M26 for i in range(10)]


def operands():
    rng = random.Random(41)
    ops = []
    # magnitude 1 (canonical digit ranges) and anywhere up to the 2^30 bound
    for _ in range(400):
        ops.append([rng.randrange(1 << 26) for _ in range(9)]
                   + [rng.randrange(1 << 22)])
    for _ in range(400):
        ops.append([rng.randrange(BOUND + 1) for _ in range(10)])
    # limbs close to the bound
    for _ in range(100):
        ops.append([BOUND - rng.randrange(4) for _ in range(10)])
    ops.append([BOUND] * 10)
    ops.append([0] * 10)
    ops += [to26(P), to26(P + 1), to26(P - 1)]
    for i in range(10):
        ops.append([BOUND if j == i else 0 for j in range(10)])
    return ops


def check(r, want, what):
    assert val(r) % P == want, what
    assert all(r[i] <= 1 << 26 for i in range(9)), what
    assert r[9] < 1 << 22, what


def test_fe26_sqr_through_reduce19(shim):
    for a in operands():
        r = (ctypes.c_uint32 * 10)()
        shim.host_fe26_sqr(arr(a), r)
        check(r, val(a) ** 2 % P, a)


def test_fe26_mul_through_reduce19(shim):
    ops = operands()
    special = ops[900:]  # all-bound, zero, p, p+1, p-1, the ten single-limb ones
    assert len(special) == 15 and special[0] == [BOUND] * 10
    rng = random.Random(42)
    pairs = [(a, b) for a in special for b in special]
    pairs += [(a, rng.choice(ops)) for a in ops]
    pairs += [(rng.choice(ops), b) for b in special for _ in range(8)]
    for a, b in pairs:
        r = (ctypes.c_uint32 * 10)()
        shim.host_fe26_mul(arr(a), arr(b), r)
        check(r, val(a) * val(b) % P, (a, b))
