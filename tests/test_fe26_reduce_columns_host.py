"""fe26_reduce19 on RAW column sums, run ON CPU from the device header
(tests/host_shim/reduce19.cpp, g++, KV_HOST_TEST asserts live: the input caps
and every intermediate bound of the header comment) against Python integers.

For columns t[0..18] under the documented caps t[k] <= n_k * 2^60,
n_k = min(k + 1, 19 - k), the output must have the value
sum t[k] * 2^(26k) mod p and the limb bounds l0..l8 <= 2^26, l9 < 2^22.
The same shim source, built as a stand-alone program under
-fsanitize=address,undefined, repeats the edge columns and a random sweep."""
import ctypes
import os
import random
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_DIR = os.path.join(REPO, "tests", "host_shim")
CSRC = os.path.join(REPO, "rusty_kaspa_amd", "csrc")
LIB = os.path.join(SHIM_DIR, "libreduce19shim.so")
PROG = os.path.join(SHIM_DIR, "reduce19_san")

P = 2**256 - 0x1000003D1
CAPS = [min(k + 1, 19 - k) << 60 for k in range(19)]
LOW = 0xFFFFFFFF


def _stale(out, srcs):
    return (not os.path.exists(out)
            or os.path.getmtime(out) < max(os.path.getmtime(p) for p in srcs))


def _sources():
    return [os.path.join(SHIM_DIR, "reduce19.cpp"), os.path.join(SHIM_DIR, "shim.h"),
            os.path.join(CSRC, "kv_secp_device.h")]


@pytest.fixture(scope="module")
def shim():
    srcs = _sources()
    if _stale(LIB, srcs):
        tmp = f"{LIB}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O1", "-fPIC", "-shared", "-I", CSRC, "-I", SHIM_DIR,
                        srcs[0], "-o", tmp], check=True)
        os.replace(tmp, LIB)
    return ctypes.CDLL(LIB)


def check(shim, t):
    assert all(0 <= t[k] <= CAPS[k] for k in range(19)), "test input past the caps"
    r = (ctypes.c_uint32 * 10)()
    shim.host_fe26_reduce19((ctypes.c_uint64 * 19)(*t), r)
    want = sum(t[k] << (26 * k) for k in range(19)) % P
    got = sum(int(r[i]) << (26 * i) for i in range(10))
    assert got % P == want, t
    assert all(r[i] <= 1 << 26 for i in range(9)), (t, list(r))
    assert r[9] < 1 << 22, (t, list(r))


def test_each_column_alone(shim):
    # a wrong destination column or shift shows on a single nonzero column
    for k in range(19):
        for v in (CAPS[k], 1, LOW, 1 << 32, CAPS[k] - 1):
            check(shim, [v if i == k else 0 for i in range(19)])


def test_all_columns_at_their_caps(shim):
    check(shim, list(CAPS))


def test_low_halves_all_ones_high_halves_largest(shim):
    # the largest value under the cap whose low half is 0xFFFFFFFF
    check(shim, [(c - (1 << 32)) | LOW for c in CAPS])
    check(shim, [LOW] * 19)


def test_low_halves_zero(shim):
    check(shim, [c & ~LOW for c in CAPS])
    rng = random.Random(61)
    for _ in range(200):
        check(shim, [rng.randrange((c >> 32) + 1) << 32 for c in CAPS])


def test_random_columns_under_the_caps(shim):
    rng = random.Random(62)
    for _ in range(100_000):
        check(shim, [rng.randrange(c + 1) for c in CAPS])


def test_standalone_program_under_host_sanitizers():
    srcs = _sources()
    if _stale(PROG, srcs):
        tmp = f"{PROG}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-DKV_REDUCE19_MAIN",
                        "-I", CSRC, "-I", SHIM_DIR, srcs[0], "-o", tmp], check=True)
        os.replace(tmp, PROG)
    out = subprocess.run([PROG], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 bad" in out.stdout
