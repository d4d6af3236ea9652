"""Crafted U3072 operands for the MuHash group arithmetic, as plain Python
ints, shared by the host-shim test and the GPU wave-reduce test.

The engine keeps values in [0, 2^3072), not canonical, so the set holds
operands from [P, 2^3072) too. The reference for every product is Python
integer arithmetic mod P; comparison is exact after reducing both sides.

Random (ChaCha20) operands make a carry that ripples over more than a lane or
two a 2^-64 event per limb. The fixed operands below sit on the edges of the
representation, and the targeted pairs multiply to a residue whose limbs are
nearly all ones (or all zeros below a borrow), which is what makes the last
carry pass of a multiply ripple across limbs and wrap through 2^3072 = C.
"""
import random

LIMBS = 48
C = 1103717
R = 2**3072
P = R - C
M64 = 2**64 - 1


def limbs_of(v):
    assert 0 <= v < R
    return [(v >> (64 * i)) & M64 for i in range(LIMBS)]


def to_bytes(v):
    return v.to_bytes(384, "little")


def from_bytes(b):
    assert len(b) == 384
    return int.from_bytes(b, "little")


def _one_limb(k):
    return M64 << (64 * k)


def _ones_but_limb0(l0):
    return (R - 1) - M64 + l0


_rng = random.Random(3072)
RANDOMS = [_rng.getrandbits(3072) for _ in range(3)]

# non-zero fixed operands (zero is for the reduce kernels only: finalize
# would have to invert it)
FIXED = (
    [1, 2, C, P - 1, P, P + 1, R - 1, R - C, R - C - 1]
    + [_one_limb(k) for k in (0, 1, 46, 47)]
    + [_ones_but_limb0(l0) for l0 in (0, 1, 2**64 - C, 2**64 - C - 1)]
    + [2**3071, 2**1536, 2**1536 - 1]
    + RANDOMS
)
assert all(0 < v < R for v in FIXED)

# products that land on these residues: limbs nearly all ones / a long borrow
TARGETS = (
    [P - 1, P - 2, (R - 1) % P]
    + [2**(64 * k) - 1 for k in (1, 2, 24, 47)]
    + [P - 2**(64 * k) for k in (1, 2, 24, 47)]
)


def _targeted_pairs():
    rng = random.Random(30720)
    pairs = []
    for t in TARGETS:
        for _ in range(3):
            a = rng.getrandbits(3072)
            if a % P == 0:
                continue
            b = t * pow(a, -1, P) % P
            assert a * b % P == t % P
            pairs.append((a, b))
    return pairs


TARGETED_PAIRS = _targeted_pairs()
ALL_PAIRS = [(a, b) for a in FIXED for b in FIXED]
PAIRS = ALL_PAIRS + TARGETED_PAIRS


def fold_third_carry(a, b):
    """Whether the host fold's last carry fires for a*b: with the 96-limb
    product N = hi*2^3072 + lo, pass 1 forms s = lo + C*hi (49 limbs) and
    pass 2 adds C*(s >> 3072) to the low 48 limbs; the third wrap is the
    carry out of that addition."""
    n = a * b
    s = (n % R) + C * (n // R)
    return ((s % R) + C * (s // R)) >= R
