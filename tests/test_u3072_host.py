"""The engine's host U3072 arithmetic (kv_u3072.h: u3072_mul_full, u3072_fold,
u3072_mulmod, u3072_canon), compiled with g++ (tests/host_shim/u3072.cpp) and
run over the crafted operand set of tests/u3072_cases.py. The reference is
Python integer arithmetic mod P = 2^3072 - 1103717; equality is exact after
reducing both sides mod P, because the engine keeps values in [0, 2^3072).

This is also the check that the operand set and the reference are right
before the GPU wave kernel sees them (test_gpu_u3072_wave.py)."""
import ctypes
import os
import subprocess

import pytest

import u3072_cases as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_DIR = os.path.join(REPO, "tests", "host_shim")
CSRC = os.path.join(REPO, "rusty_kaspa_amd", "csrc")
LIB = os.path.join(SHIM_DIR, "libu3072shim.so")

L48 = ctypes.c_uint64 * 48


@pytest.fixture(scope="module")
def shim():
    srcs = [os.path.join(SHIM_DIR, "u3072.cpp"), os.path.join(CSRC, "kv_u3072.h")]
    if (not os.path.exists(LIB)
            or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in srcs)):
        tmp = f"{LIB}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O1", "-fPIC", "-shared", "-I", CSRC, srcs[0],
                        "-o", tmp], check=True)
        os.replace(tmp, LIB)
    return ctypes.CDLL(LIB)


def mulmod(shim, a, b):
    r = L48()
    shim.host_u3072_mulmod(L48(*U.limbs_of(a)), L48(*U.limbs_of(b)), r)
    return sum(v << (64 * i) for i, v in enumerate(r))


def canon(shim, v):
    a = L48(*U.limbs_of(v))
    shim.host_u3072_canon(a)
    return sum(x << (64 * i) for i, x in enumerate(a))


def test_operand_set_reaches_third_carry():
    """The condition on the set itself: some pair takes u3072_fold's final
    `if (c)` wrap, which random operands never do."""
    hits = [(a, b) for a, b in U.PAIRS if U.fold_third_carry(a, b)]
    assert hits, "no operand pair reaches the third carry of u3072_fold"
    # and the set is not degenerate the other way round
    assert len(hits) < len(U.PAIRS)


def test_mulmod_crafted_pairs(shim):
    for idx, (a, b) in enumerate(U.PAIRS):
        got = mulmod(shim, a, b)
        assert 0 <= got < U.R
        assert got % U.P == a * b % U.P, (idx, hex(a)[:20], hex(b)[:20])


def test_mulmod_zero_and_chains(shim):
    for v in U.FIXED:
        assert mulmod(shim, 0, v) % U.P == 0
        assert mulmod(shim, v, 0) % U.P == 0
    for start in (U.P - 1, U.R - 1):
        acc, want = start, start % U.P
        for _ in range(63):
            acc = mulmod(shim, acc, start)
            want = want * start % U.P
            assert acc % U.P == want


def test_canon_exact(shim):
    """u3072_canon returns exactly v mod P: one subtraction for [P, 2^3072),
    none below."""
    vals = [0] + list(U.FIXED) + [t for t in U.TARGETS]
    vals += [U.P - 2, U.P + 2, U.R - 2, U.P + U.C - 1]
    seen_ge = seen_lt = 0
    for v in vals:
        assert canon(shim, v) == v % U.P, hex(v)[:24]
        seen_ge += v >= U.P
        seen_lt += v < U.P
    assert seen_ge >= 5 and seen_lt >= 5


def test_mulmod_then_canon_is_canonical(shim):
    for a, b in U.TARGETED_PAIRS + [(x, x) for x in U.FIXED]:
        assert canon(shim, mulmod(shim, a, b)) == a * b % U.P
