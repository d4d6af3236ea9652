"""Probe: UTXO-set commitment and verified import throughput on one GPU.

Builds a 4M-slot table holding 1M random inline entries plus 1,000 arena
entries and prints one JSON line with
  - kv_utxo_commitment kernel_ms (best of 3) and entries/s,
  - kv_utxo_import_chunk entries/s at 64K-entry chunks (wall time, uploads
    included) into a fresh table,
  - the CPU figure measured in the same run: the oracle's ok_muhash_element +
    ok_u3072_mul, single thread, over 20,000 of the same entries.
It also cross-checks the three results against each other mod P. There is no
pass threshold on the rates.
"""
import ctypes
import json
import os
import struct
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

P = 2**3072 - 1103717
N_INLINE = 1 << 20
N_ARENA = 1000
ARENA_SPK = 200
CHUNK = 1 << 16
N_CPU = 20000
CAPACITY = 2 << 20  # kv_utxo_reset doubles it into 4M slots


def make_entries():
    rs = np.random.RandomState(5)
    n = N_INLINE + N_ARENA
    ops = rs.randint(0, 256, size=(n, 36), dtype=np.uint8)
    ops[:, 33:] = 0  # index < 256
    ents = np.zeros((n, 64), dtype=np.uint8)
    ents[:, 0:6] = rs.randint(0, 256, size=(n, 6), dtype=np.uint8)   # amount
    ents[:, 8:13] = rs.randint(0, 256, size=(n, 5), dtype=np.uint8)  # daa
    ents[:N_INLINE, 20] = 34                                          # spk_len
    ents[:N_INLINE, 24:58] = rs.randint(0, 256, size=(N_INLINE, 34),
                                        dtype=np.uint8)
    ents[N_INLINE:, 20:24] = np.frombuffer(struct.pack("<I", ARENA_SPK),
                                           dtype=np.uint8)
    spks = rs.randint(0, 256, size=(N_ARENA, ARENA_SPK), dtype=np.uint8)
    return ops, ents, spks


def serialise(op, ent, spk):
    """write_utxo (consensus/core/src/muhash.rs:55-69) of one packed entry"""
    amount, daa, flags, ver, ln = struct.unpack_from("<QQHHI", ent)
    return (op + struct.pack("<QQ", daa, amount) + bytes([flags & 1])
            + struct.pack("<HQ", ver, ln) + spk)


def num(partial):
    return int.from_bytes(bytes(partial[:384]), "little")


def main():
    from rusty_kaspa_amd.engine import Engine  # needs __graft_entry__.build()

    oracle = ctypes.CDLL(os.path.join(REPO, "oracle", "liboracle.so"))
    ops, ents, spks = make_entries()
    n = N_INLINE + N_ARENA
    eng = Engine()
    ctx = ctypes.c_void_p(eng.ctx)
    one = (1).to_bytes(384, "little")

    # verified import of the whole set, 64K-entry chunks (the last chunk also
    # carries the arena entries' scripts)
    assert eng.lib.kv_utxo_reset(ctx, ctypes.c_uint64(CAPACITY)) == 0
    acc = bytearray(one + one)
    chunks = []
    for lo in range(0, n, CHUNK):
        hi = min(n, lo + CHUNK)
        blob = spks[max(lo, N_INLINE) - N_INLINE:max(hi, N_INLINE) - N_INLINE]
        chunks.append((ops[lo:hi].tobytes(), ents[lo:hi].tobytes(),
                       blob.tobytes(), hi - lo))
    t0 = time.perf_counter()
    for c_ops, c_ents, c_blob, m in chunks:
        eng.utxo_import_chunk(c_ops, c_ents, c_blob, m, acc)
    import_s = time.perf_counter() - t0

    # whole-table commitment of what the import stored
    runs = []
    for _ in range(3):
        partial, n_live, ms = eng.utxo_commitment()
        runs.append(ms)
    assert n_live == n, (n_live, n)
    agree = num(partial) % P == num(acc) % P

    # CPU: the oracle over the first N_CPU entries, single thread
    datas = [serialise(ops[i].tobytes(), ents[i].tobytes(),
                       ents[i, 24:58].tobytes()) for i in range(N_CPU)]
    U = ctypes.c_uint64 * 48
    cpu_acc, elem = U(), U()
    oracle.ok_u3072_one(cpu_acc)
    t0 = time.perf_counter()
    for d in datas:
        oracle.ok_muhash_element(d, ctypes.c_size_t(len(d)), elem)
        oracle.ok_u3072_mul(cpu_acc, elem)
    cpu_s = time.perf_counter() - t0
    # the same N_CPU entries through the engine, as a cross-check of the figure
    assert eng.lib.kv_utxo_reset(ctx, ctypes.c_uint64(N_CPU)) == 0
    acc2 = bytearray(one + one)
    eng.utxo_import_chunk(ops[:N_CPU].tobytes(), ents[:N_CPU].tobytes(), b"",
                          N_CPU, acc2)
    cpu_val = sum(int(cpu_acc[i]) << (64 * i) for i in range(48))
    agree_cpu = cpu_val % P == num(acc2) % P
    window = eng.utxo_commitment_window()
    eng.close()

    best = min(runs)
    print(json.dumps({
        "probe": "utxo_commit",
        "slots": 2 * CAPACITY, "entries": n, "arena_entries": N_ARENA,
        "window_slots": window,
        "commitment_kernel_ms": round(best, 3),
        "commitment_kernel_ms_runs": [round(x, 3) for x in runs],
        "commitment_entries_per_s": round(n / best * 1000),
        "import_chunk_entries": CHUNK,
        "import_wall_s": round(import_s, 4),
        "import_entries_per_s": round(n / import_s),
        "cpu_oracle_entries": N_CPU,
        "cpu_oracle_entries_per_s": round(N_CPU / cpu_s),
        "commitment_equals_import_acc": bool(agree),
        "import_equals_cpu_oracle": bool(agree_cpu),
    }), flush=True)
    return 0 if agree and agree_cpu else 1


if __name__ == "__main__":
    sys.exit(main())
