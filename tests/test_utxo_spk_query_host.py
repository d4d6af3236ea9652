"""The script-public-key query functions of kv_utxo_query_kernels.hip, run ON
CPU from the device source (tests/host_shim/utxo_spk_query.cpp, g++):
spk_query_build makes the open-addressing table the engine uploads, and
spk_query_match routes a packed 64-byte table value to the query its script
equals. The reference is a Python dict keyed by (version, script) ⇔ the
utxoindex's key version ‖ len ‖ script
(indexes/utxoindex/src/stores/indexed_utxos.rs:156-198).

Every case runs against two builds of the shim: the real hash, and
KV_SPK_HASH_CONST, under which every script hash is equal. Results must be
identical: the compare decides, the hash only routes. The same kinds of cases
run once more as a stand-alone program under -fsanitize=address,undefined."""
import ctypes
import os
import random
import struct
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_DIR = os.path.join(REPO, "tests", "host_shim")
CSRC = os.path.join(REPO, "rusty_kaspa_amd", "csrc")
INCLUDE = os.path.join(REPO, "include")

F_COINBASE, F_ARENA, F_COVENANT = 1, 2, 4
NONE, BAD = -1, -2
MAX_SPK, QUERY_MAX = 10000, 65536
SPK_LENS = [0, 1, 35, 36, 37, 64, 200, 10000]
QUERY_COUNTS = [0, 1, 2, 3, 64, 1000]


class SpkQuery(ctypes.Structure):
    _fields_ = [("spk_len", ctypes.c_uint32), ("spk_version", ctypes.c_uint16),
                ("zero", ctypes.c_uint16)]


def _sources():
    srcs = [os.path.join(SHIM_DIR, f) for f in ("utxo_spk_query.cpp", "shim.h")]
    srcs += [os.path.join(CSRC, f) for f in (
        "kv_utxo_query_kernels.hip", "kv_utxo_commit_kernels.hip",
        "kv_hash_device.h", "kv_u3072.h")]
    srcs.append(os.path.join(INCLUDE, "kaspa_engine_abi.h"))
    return srcs


def _stale(out, srcs):
    return (not os.path.exists(out)
            or os.path.getmtime(out) < max(os.path.getmtime(p) for p in srcs))


def _build(out, extra):
    srcs = _sources()
    if _stale(out, srcs):
        tmp = f"{out}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O1", *extra, "-I", CSRC, "-I", SHIM_DIR,
                        "-I", INCLUDE, srcs[0], "-o", tmp], check=True)
        os.replace(tmp, out)
    return out


@pytest.fixture(scope="module", params=["hashed", "const_hash"])
def shim(request):
    extra = ["-fPIC", "-shared"]
    name = "libspkqueryshim.so"
    if request.param == "const_hash":
        extra.append("-DKV_SPK_HASH_CONST")
        name = "libspkqueryshim_consthash.so"
    lib = ctypes.CDLL(_build(os.path.join(SHIM_DIR, name), extra))
    lib.host_spk_hash.restype = ctypes.c_uint64
    lib.host_spk_query_slots.restype = ctypes.c_uint32
    lib.const_hash = request.param == "const_hash"
    return lib


# ---------------- table values and the query table ----------------

class Arena:
    """scripts behind a few unrelated bytes each, so offsets are odd; the
    buffer handed to the shim is exactly len(self.data) bytes long"""

    def __init__(self, rng):
        self.rng, self.data = rng, b""

    def put(self, spk):
        self.data += self.rng.randbytes(3)
        off = len(self.data)
        self.data += spk
        return off

    def buffer(self):
        return (ctypes.c_uint8 * len(self.data)).from_buffer_copy(self.data) \
            if self.data else None


def table_value(rng, arena, version, spk, covenant=False, coinbase=False):
    """the packed 64-byte value as the table holds it"""
    flags = F_COINBASE if coinbase else 0
    if covenant or len(spk) > 36:
        flags |= F_ARENA | (F_COVENANT if covenant else 0)
        field = struct.pack("<I", arena.put(spk)) \
            + (rng.randbytes(32) if covenant else bytes(32))
    else:
        field = spk.ljust(36, b"\0")
    return struct.pack("<QQHHI", rng.randrange(1 << 64), rng.randrange(1 << 64),
                       flags, version, len(spk)) + field + bytes(4)


class QueryTable:
    def __init__(self, shim, queries):
        self.shim, self.n = shim, len(queries)
        self.q = (SpkQuery * max(self.n, 1))()
        for i, (version, spk) in enumerate(queries):
            self.q[i] = SpkQuery(len(spk), version, 0)
        self.blob = b"".join(spk for _, spk in queries)
        self.slots = shim.host_spk_query_slots(ctypes.c_size_t(self.n))
        assert self.slots >= max(64, 2 * self.n)
        assert self.slots & (self.slots - 1) == 0
        self.off = (ctypes.c_uint32 * max(self.n, 1))()
        self.hash = (ctypes.c_uint64 * self.slots)()
        self.qidx = (ctypes.c_uint32 * self.slots)()
        assert shim.host_spk_query_check(self.q, ctypes.c_size_t(self.n),
                                         ctypes.c_size_t(len(self.blob))) == 0
        self.rc = shim.host_spk_query_build(
            self.q, ctypes.c_size_t(self.n), self.blob, self.off, self.hash,
            self.qidx, ctypes.c_uint32(self.slots))

    def match(self, val64, arena_buf, arena_len):
        assert self.rc == 0 and len(val64) == 64
        return self.shim.host_spk_query_match(
            val64, arena_buf, ctypes.c_uint64(arena_len), self.hash, self.qidx,
            self.q, self.off, self.blob, ctypes.c_uint32(self.slots),
            ctypes.c_uint32(self.n))


def script_cases(rng):
    """[(version, script, covenant)]: the entries every test looks up"""
    by_len = {ln: rng.randbytes(ln) for ln in SPK_LENS}
    cases = [(0, spk, False) for spk in by_len.values()]
    cases.append((1, by_len[35], False))              # differs in version only
    cases += [(0, b"abc", False), (0, b"abc\0", False)]  # both inline
    cases.append((0, by_len[36] + b"\7", False))  # arena, shares the inline 36
    cases.append((0, rng.randbytes(20), True))    # covenant: 20 bytes, arena
    return cases


def near_misses(rng, cases):
    out = []
    for version, spk, _ in cases:
        out.append((version + 2, spk))
        if spk:
            out.append((version, spk[:-1] + bytes([spk[-1] ^ 1])))
            out.append((version, spk[:-1]))
        if len(spk) < MAX_SPK:
            out.append((version, spk + b"\0"))
    return out


def queries_for(rng, cases, n_q):
    """n_q distinct queries: about half of them scripts of `cases`, then near
    misses of those, then random ones"""
    present = [(v, s) for v, s, _ in cases]
    rng.shuffle(present)
    pool = present[:(n_q + 1) // 2] + near_misses(rng, cases)
    seen, queries = set(), []
    while len(queries) < n_q:
        q = pool.pop(0) if pool else (rng.randrange(3),
                                      rng.randbytes(rng.randrange(70)))
        if q not in seen:
            seen.add(q)
            queries.append(q)
    rng.shuffle(queries)
    assert len(queries) == n_q
    return queries


@pytest.mark.parametrize("n_q", QUERY_COUNTS)
def test_match_equals_dict(shim, n_q):
    rng = random.Random(4000 + n_q)
    cases = script_cases(rng)
    arena = Arena(rng)
    values = [table_value(rng, arena, v, s, covenant=c, coinbase=i % 4 == 0)
              for i, (v, s, c) in enumerate(cases)]
    queries = queries_for(rng, cases, n_q)
    model = {q: i for i, q in enumerate(queries)}
    table = QueryTable(shim, queries)
    assert table.rc == 0
    buf = arena.buffer()
    hits = 0
    for (version, spk, _), val in zip(cases, values):
        want = model.get((version, spk), NONE)
        assert table.match(val, buf, len(arena.data)) == want, (version, len(spk))
        hits += want != NONE
    if n_q >= 64:
        assert hits == len(cases)  # every case is among the present half
    elif n_q:
        assert 0 < hits < len(cases)
    else:
        assert hits == 0


def test_the_special_pairs_route_apart(shim):
    """each of the look-alike pairs, queried one at a time: only the entry
    with exactly that (version, length, bytes) matches"""
    rng = random.Random(41)
    base = rng.randbytes(36)
    cov_spk = rng.randbytes(20)
    cases = [(0, b"abc", False), (0, b"abc\0", False), (0, base, False),
             (0, base + b"\0", False), (0, base[:35], False), (1, base, False),
             (0, cov_spk, True), (0, cov_spk, False), (0, b"", False),
             (0, b"", True)]
    arena = Arena(rng)
    values = [table_value(rng, arena, v, s, covenant=c) for v, s, c in cases]
    buf = arena.buffer()
    for version, spk in {(v, s) for v, s, _ in cases}:
        table = QueryTable(shim, [(version, spk)])
        got = [table.match(val, buf, len(arena.data)) for val in values]
        # the covenant id plays no part: both holders of cov_spk match
        assert got == [0 if (v, s) == (version, spk) else NONE
                       for v, s, _ in cases]


def test_inline_padding_is_not_compared(shim):
    rng = random.Random(42)
    spk = rng.randbytes(20)
    val = bytearray(table_value(rng, Arena(rng), 0, spk))
    val[24 + 20:24 + 36] = b"\xaa" * 16
    table = QueryTable(shim, [(0, spk + b"\xaa"), (0, spk)])
    assert table.match(bytes(val), None, 0) == 1


def test_hash_is_over_version_length_and_bytes(shim):
    h = lambda v, s: shim.host_spk_hash(ctypes.c_uint16(v), ctypes.c_uint32(len(s)), s)
    if shim.const_hash:
        assert h(0, b"abc") == h(1, b"abcd") == 0
        return
    distinct = [(0, b""), (1, b""), (0, b"\0"), (0, b"abc"), (0, b"abc\0"),
                (1, b"abc"), (0, b"abd"), (0, bytes(8)), (0, bytes(9)),
                (0, bytes(16)), (0, bytes(7) + b"\1"), (0, bytes(8) + b"\1")]
    assert len({h(v, s) for v, s in distinct}) == len(distinct)
    # nothing past spk + len is read: the same bytes in a longer buffer
    assert h(0, b"abc") == shim.host_spk_hash(ctypes.c_uint16(0),
                                              ctypes.c_uint32(3), b"abcdefghij")


def test_duplicate_queries_are_refused(shim):
    rng = random.Random(43)
    a = rng.randbytes(34)
    b = a[:33] + bytes([a[33] ^ 0x80])
    big = rng.randbytes(MAX_SPK)
    # differing in one byte, in version or in a trailing zero is no duplicate
    ok = [(0, a), (0, b), (1, a), (0, b"abc"), (0, b"abc\0"), (0, b""), (1, b""),
          (0, big), (0, big[:-1] + bytes([big[-1] ^ 1]))]
    assert QueryTable(shim, ok).rc == 0
    for i in range(len(ok)):
        for tail in ([], [(0, rng.randbytes(30))]):
            assert QueryTable(shim, ok + [ok[i]] + tail).rc == 1, i
    assert QueryTable(shim, [(0, a), (0, a)]).rc == 1
    many = [(0, rng.randbytes(34)) for _ in range(999)]
    assert QueryTable(shim, many).rc == 0
    assert QueryTable(shim, many + [many[500]]).rc == 1


def test_argument_rules(shim):
    def check(heads, blob_len):
        arr = (SpkQuery * max(len(heads), 1))(*[SpkQuery(*h) for h in heads])
        return shim.host_spk_query_check(arr, ctypes.c_size_t(len(heads)),
                                         ctypes.c_size_t(blob_len))
    assert check([], 0) == 0
    assert check([], 1) == -1
    assert check([(3, 0, 0), (MAX_SPK, 7, 0)], 3 + MAX_SPK) == 0
    assert check([(MAX_SPK + 1, 0, 0)], MAX_SPK + 1) == -1
    assert check([(3, 0, 1)], 3) == -1
    assert check([(3, 0, 0), (4, 0, 0)], 8) == -1
    assert check([(3, 0, 0), (4, 0, 0)], 6) == -1
    assert check([(0, 0, 0)] * QUERY_MAX, 0) == 0  # duplicates are build's business
    assert check([(0, 0, 0)] * (QUERY_MAX + 1), 0) == -1


def test_bad_references_are_reported_not_followed(shim):
    """the arena buffer is exactly arena_len bytes: the sanitizer build of the
    same cases (below) would catch a read through any of these"""
    rng = random.Random(44)
    arena = Arena(rng)
    spk = rng.randbytes(200)
    good = table_value(rng, arena, 0, spk)
    inline = table_value(rng, arena, 0, rng.randbytes(30))
    n = len(arena.data)
    buf = arena.buffer()
    for table in (QueryTable(shim, [(0, spk), (0, b"x")]), QueryTable(shim, [])):
        hit = 0 if table.n else NONE
        assert table.match(good, buf, n) == hit
        assert table.match(good, buf, n - 1) == BAD
        assert table.match(good, None, 0) == BAD
        for off in (n - 199, n, 0xFFFFFFF0):
            moved = good[:24] + struct.pack("<I", off) + good[28:]
            assert table.match(moved, buf, n) == BAD, off
        too_long = good[:20] + struct.pack("<I", MAX_SPK + 1) + good[24:]
        assert table.match(too_long, buf, n) == BAD
        assert table.match(inline[:20] + struct.pack("<I", 37) + inline[24:],
                           buf, n) == BAD
        # a covenant id where an inline script would be
        assert table.match(inline[:16] + struct.pack("<H", F_COVENANT) + inline[18:],
                           buf, n) == BAD
        assert table.match(inline, buf, n) == NONE


@pytest.mark.parametrize("const_hash", [False, True])
def test_standalone_program_under_host_sanitizers(const_hash):
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-DKV_SPK_QUERY_MAIN"]
    name = "utxo_spk_query_san"
    if const_hash:
        extra.append("-DKV_SPK_HASH_CONST")
        name += "_consthash"
    prog = _build(os.path.join(SHIM_DIR, name), extra)
    out = subprocess.run([prog], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 bad" in out.stdout
