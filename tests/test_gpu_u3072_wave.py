"""GPU: the wave-cooperative U3072 multiply (u3072_wave_mulmod) through its two
kernels, kv_u3072_reduce_wave_kernel and kv_u3072_reduce_wave_acc_kernel, one
launch at a time via the kv_test_u3072_reduce hook, on the crafted operands of
tests/u3072_cases.py. The reference is Python integer arithmetic mod
P = 2^3072 - 1103717 over the same index sets (w, w+stride, ...); equality is
exact after reducing both sides mod P. test_u3072_host.py checks the same
operand set against the host arithmetic without a GPU."""
import ctypes
import hashlib
import random

import pytest

import u3072_cases as U

pytestmark = pytest.mark.gpu

ONE = U.to_bytes(1)
L48 = ctypes.c_uint64 * 48


@pytest.fixture(scope="module")
def engine():
    from rusty_kaspa_amd.engine import Engine
    eng = Engine()
    yield eng
    eng.close()


def pack(vals):
    return b"".join(U.to_bytes(v) for v in vals)


def unpack(buf):
    return [U.from_bytes(buf[i:i + 384]) for i in range(0, len(buf), 384)]


def chain_products(vals, stride, start=None):
    """Python reference: wave w multiplies vals[w], vals[w+stride], ... into
    start[w] (or into one)."""
    out = []
    for w in range(stride):
        acc = 1 if start is None else start[w]
        for v in vals[w::stride]:
            acc = acc * v % U.P
        out.append(acc % U.P)
    return out


def run_plain(engine, vals, stride):
    got, _ = engine.u3072_reduce_hook(pack(vals), len(vals), stride)
    return got


def run_acc(engine, vals, stride, acc):
    got, counted = engine.u3072_reduce_hook(pack(vals), len(vals), stride,
                                            pack(acc))
    assert counted == len(vals)
    return got


def assert_mod_equal(got_buf, want, what):
    got = unpack(got_buf)
    assert len(got) == len(want)
    bad = [w for w, (g, e) in enumerate(zip(got, want)) if g % U.P != e]
    assert not bad, (what, "first wrong waves", bad[:8], "of", len(want))


# every pair of the operand set, plus zero against a few of them
PAIRS = U.PAIRS + [(0, v) for v in U.FIXED[:9]] + [(v, 0) for v in U.FIXED[:9]] \
    + [(0, 0)]


def test_plain_every_pair(engine):
    """n = 2·stride: wave w gets elements w and w+stride, so one launch does
    one multiply per pair."""
    stride = len(PAIRS)
    vals = [a for a, _ in PAIRS] + [b for _, b in PAIRS]
    want = [a * b % U.P for a, b in PAIRS]
    assert want == chain_products(vals, stride)
    assert_mod_equal(run_plain(engine, vals, stride), want, "plain pairs")


def test_acc_every_pair(engine):
    """acc kernel, n = stride: acc[w] (first operand) times elements[w]."""
    stride = len(PAIRS)
    acc = [a for a, _ in PAIRS]
    vals = [b for _, b in PAIRS]
    want = [a * b % U.P for a, b in PAIRS]
    assert_mod_equal(run_acc(engine, vals, stride, acc), want, "acc pairs")


def test_pass_through(engine):
    for v in (U.R - 1, U.P, 0, U.RANDOMS[0]):
        got = run_plain(engine, [v], 1)
        assert got == U.to_bytes(v)  # one element: copied, not multiplied


@pytest.mark.parametrize("n,stride", [(64, 1), (65, 2), (25, 8)])
def test_chain_shapes(engine, n, stride):
    rng = random.Random(n * 1000 + stride)
    pool = [v for v in U.FIXED if v % U.P] + [t for t in U.TARGETS]
    vals = [rng.choice(pool) for _ in range(n)]
    assert_mod_equal(run_plain(engine, vals, stride),
                     chain_products(vals, stride), "plain chain")
    acc = [rng.choice(pool) for _ in range(stride)]
    assert_mod_equal(run_acc(engine, vals, stride, acc),
                     chain_products(vals, stride, acc), "acc chain")
    # one zero element annihilates exactly its own chain
    vals[n // 2] = 0
    want = chain_products(vals, stride)
    assert want.count(0) == 1
    assert_mod_equal(run_plain(engine, vals, stride), want, "plain chain, zero")


def test_idle_waves(engine):
    """stride > n: an idle wave writes the identity in the plain kernel and
    leaves its accumulator bit-for-bit alone in the acc kernel."""
    n, stride = 3, 8
    vals = [U.P - 1, U.R - 1, U.RANDOMS[1]]
    got = run_plain(engine, vals, stride)
    for w in range(n):
        assert got[384 * w:384 * (w + 1)] == U.to_bytes(vals[w])
    for w in range(n, stride):
        assert got[384 * w:384 * (w + 1)] == ONE, w
    # distinctive, mostly non-canonical accumulators
    acc = [U.R - 1 - w for w in range(stride)]
    got = run_acc(engine, vals, stride, acc)
    assert_mod_equal(got[:384 * n], [a * v % U.P for a, v in zip(acc, vals)],
                     "acc, busy waves")
    assert got[384 * n:] == pack(acc[n:])


def test_acc_no_elements(engine):
    acc = [U.R - 1, U.P, 0, U.RANDOMS[2], 2]
    got, counted = engine.u3072_reduce_hook(b"", 0, len(acc), pack(acc))
    assert counted == 0
    assert got == pack(acc)


@pytest.mark.parametrize("v", [U.P - 1, U.R - 1], ids=["P-1", "2^3072-1"])
def test_chain_of_64_copies(engine, v):
    want = pow(v, 64, U.P)
    if v == U.P - 1:
        assert want == 1
    assert_mod_equal(run_plain(engine, [v] * 64, 1), [want], "64 copies")
    assert_mod_equal(run_plain(engine, [v] * 63, 1), [pow(v, 63, U.P)],
                     "63 copies")
    assert_mod_equal(run_acc(engine, [v] * 64, 1, [v]), [pow(v, 65, U.P)],
                     "acc, 64 copies")


def test_combine_and_finalize_crafted(oracle, engine):
    """Crafted partials through Engine.muhash_combine and muhash_finalize: the
    host u3072_mulmod / u3072_canon as linked into the product library, vs the
    oracle's ok_u3072_mul + ok_muhash_finalize and plain Python."""
    nz = [v for v in U.FIXED if v % U.P] + [a for a, _ in U.TARGETED_PAIRS[:6]]
    rng = random.Random(768)
    cases = [(a, b) for a, b in U.TARGETED_PAIRS]
    cases += [(rng.choice(nz), rng.choice(nz)) for _ in range(40)]
    for i, (num_b, den_b) in enumerate(cases):
        num_a, den_a = nz[i % len(nz)], nz[(7 * i + 3) % len(nz)]
        acc = bytearray(U.to_bytes(num_a) + U.to_bytes(den_a))
        engine.muhash_combine(acc, U.to_bytes(num_b) + U.to_bytes(den_b))
        onum, oden = L48(*U.limbs_of(num_a)), L48(*U.limbs_of(den_a))
        oracle.ok_u3072_mul(onum, L48(*U.limbs_of(num_b)))
        oracle.ok_u3072_mul(oden, L48(*U.limbs_of(den_b)))
        got_num, got_den = U.from_bytes(bytes(acc[:384])), U.from_bytes(bytes(acc[384:]))
        ref_num, ref_den = num_a * num_b % U.P, den_a * den_b % U.P
        assert got_num % U.P == ref_num == U.from_bytes(bytes(onum)) % U.P, i
        assert got_den % U.P == ref_den == U.from_bytes(bytes(oden)) % U.P, i
        got = engine.muhash_finalize(bytes(acc))
        out = (ctypes.c_uint8 * 32)()
        oracle.ok_muhash_finalize(onum, oden, out)
        q = ref_num * pow(ref_den, -1, U.P) % U.P
        py = hashlib.blake2b(U.to_bytes(q), digest_size=32,
                             key=b"MuHashFinalize").digest()
        assert bytes(out) == py, i
        assert got == py, i
    # non-canonical numerators straight into finalize: canon must subtract
    for num in (U.P + 1, U.R - 1, U.R - U.C, U.P - 1):
        got = engine.muhash_finalize(U.to_bytes(num) + ONE)
        py = hashlib.blake2b(U.to_bytes(num % U.P), digest_size=32,
                             key=b"MuHashFinalize").digest()
        assert got == py, hex(num)[:24]
