"""Python big-int secp256k1, shared by the joint fixed-base table tests
(test_gcomb16_host.py, test_gpu_gcomb16.py). Not a test module."""

P = 2**256 - 0x1000003D1
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
     0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A6855419 << 64
     | 0x9C47D08FFB10D4B8)


def ec_add(a, b):
    """Affine add; None is infinity."""
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


def _jdbl(a):
    x, y, z = a
    if z == 0:
        return a
    yy = y * y % P
    s = 4 * x * yy % P
    m = 3 * x * x % P
    nx = (m * m - 2 * s) % P
    return (nx, (m * (s - nx) - 8 * yy * yy) % P, 2 * y * z % P)


def _jadd_affine(a, b):
    x1, y1, z1 = a
    if z1 == 0:
        return (b[0], b[1], 1)
    zz = z1 * z1 % P
    u2 = b[0] * zz % P
    s2 = b[1] * zz * z1 % P
    h = (u2 - x1) % P
    r = (s2 - y1) % P
    if h == 0:
        return _jdbl(a) if r == 0 else (1, 1, 0)
    hh = h * h % P
    hhh = hh * h % P
    v = x1 * hh % P
    nx = (r * r - hhh - 2 * v) % P
    return (nx, (r * (v - nx) - y1 * hhh) % P, z1 * h % P)


def ec_mul(k, pt):
    """k·pt for an affine pt (double-and-add in Jacobian form, one inversion)."""
    k %= N
    if k == 0 or pt is None:
        return None
    acc = (1, 1, 0)
    for bit in bin(k)[2:]:
        acc = _jdbl(acc)
        if bit == "1":
            acc = _jadd_affine(acc, pt)
    if acc[2] == 0:
        return None
    zi = pow(acc[2], -1, P)
    return (acc[0] * zi * zi % P, acc[1] * zi ** 3 % P)


def multiples(base, count):
    """[1·base, 2·base, …, count·base] as affine points."""
    out, acc = [], None
    for _ in range(count):
        acc = ec_add(acc, base)
        out.append(acc)
    return out


def joint_entry(idx, gmul, hmul):
    """Entry hi<<8|lo of the joint table: lo·G + hi·H (entry 0 is G).
    gmul/hmul are multiples(G, 255) and multiples(H, 255)."""
    lo, hi = idx & 255, idx >> 8
    if hi == 0:
        return gmul[max(lo, 1) - 1]
    if lo == 0:
        return hmul[hi - 1]
    return ec_add(gmul[lo - 1], hmul[hi - 1])


def rep_byte(b, count=32):
    return int.from_bytes(bytes([b]) * count, "big")


def crafted_g_scalars():
    """The G scalars that walk the joint table's edges: empty and full halves,
    the carry across bit 128, the top of the scalar range, every byte equal,
    zero bytes alternating with full ones in both phases, and one half zero
    with every byte of the other non-zero."""
    alt_a = int.from_bytes(bytes([0xFF, 0x00] * 16), "big")
    alt_b = int.from_bytes(bytes([0x00, 0xFF] * 16), "big")
    hi_only = int.from_bytes(bytes(range(1, 17)), "big") << 128
    lo_only = int.from_bytes(bytes(range(0xF0, 0xE0, -1)), "big")
    return [0, 1, 2**128 - 1, 2**128, 2**128 + 1, N - 1, N - 2,
            rep_byte(0x01), rep_byte(0x80), alt_a, alt_b, hi_only, lo_only]
