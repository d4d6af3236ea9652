"""Probe: what tombstone churn costs the GPU UTXO table, and what
kv_utxo_rehash gives back, on one GPU.

Builds utxo_commit_probe's table (4M slots, 1M inline entries plus 1,000 arena
entries), then churns it: each round removes a random share of the live
inline keys and inserts as many fresh uniform keys, and overwrites some arena
entries, until n_empty is under 5% of the slots. Before and after
kv_utxo_rehash(0) it records
  - kv_utxo_stats,
  - kernel_ms (best of 3) of a 262,144-key all-miss kv_utxo_lookup,
  - entries/s of a full kv_utxo_export_chunk walk in 64K-entry chunks (wall
    time, copies back included, best of 3),
and kernel_ms of the rehash itself, plus three more rehashes of the then clean
table and one kv_utxo_commitment for scale. It prints one JSON line. It also checks
that the rehash left kv_utxo_commitment unchanged mod P and the walk's entry
count equal to n_live. There is no pass threshold on the times.
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

from utxo_commit_probe import (ARENA_SPK, CAPACITY, CHUNK, N_ARENA,  # noqa: E402
                               N_INLINE, P, make_entries, num)

N_MISS = 1 << 18
CHURN = N_INLINE // 2   # inline keys replaced per round
ARENA_CHURN = 100       # arena entries overwritten per round
MAX_ROUNDS = 64
EMPTY_TARGET = 0.05
SPK_CAP = 1 << 20


def upsert(eng, ops, ents, blob=b""):
    n = len(ops)
    for lo in range(0, n, CHUNK):
        hi = min(n, lo + CHUNK)
        rc = eng.lib.kv_utxo_upsert_spk(
            ctypes.c_void_p(eng.ctx), ops[lo:hi].tobytes(), ents[lo:hi].tobytes(),
            blob, ctypes.c_size_t(len(blob)), ctypes.c_size_t(hi - lo))
        if rc:
            raise RuntimeError(eng.lib.kv_last_error().decode())


def remove(eng, ops):
    rc = eng.lib.kv_utxo_remove(ctypes.c_void_p(eng.ctx), ops.tobytes(),
                                ctypes.c_size_t(len(ops)))
    if rc:
        raise RuntimeError(eng.lib.kv_last_error().decode())


def miss_lookup_ms(eng, miss_ops):
    n = len(miss_ops)
    bm = (ctypes.c_uint64 * ((n + 63) // 64))()
    ms = ctypes.c_double()
    buf = miss_ops.tobytes()
    runs = []
    for _ in range(3):
        rc = eng.lib.kv_utxo_lookup(ctypes.c_void_p(eng.ctx), buf,
                                    ctypes.c_size_t(n), None, bm, ctypes.byref(ms))
        if rc:
            raise RuntimeError(eng.lib.kv_last_error().decode())
        runs.append(ms.value)
    hits = sum(bin(w).count("1") for w in bm)
    return min(runs), hits


def export_walk(eng, slots):
    """a full walk in CHUNK-entry chunks: (entries, script bytes, calls, s)"""
    ops = (ctypes.c_uint8 * (36 * CHUNK))()
    ents = (ctypes.c_uint8 * (64 * CHUNK))()
    spk = (ctypes.c_uint8 * SPK_CAP)()
    cur, used, n = ctypes.c_uint64(0), ctypes.c_size_t(), ctypes.c_size_t()
    total = spk_total = calls = 0
    t0 = time.perf_counter()
    while True:
        rc = eng.lib.kv_utxo_export_chunk(
            ctypes.c_void_p(eng.ctx), ctypes.byref(cur), ctypes.c_size_t(CHUNK),
            ops, ents, spk, ctypes.c_size_t(SPK_CAP), ctypes.byref(used),
            ctypes.byref(n))
        if rc:
            raise RuntimeError(eng.lib.kv_last_error().decode())
        calls += 1
        total += n.value
        spk_total += used.value
        if n.value == 0 and cur.value == slots:
            break
    return total, spk_total, calls, time.perf_counter() - t0


def measure(eng, miss_ops):
    st = eng.utxo_stats()
    ms, hits = miss_lookup_ms(eng, miss_ops)
    walks = [export_walk(eng, st["slots"]) for _ in range(3)]
    total, spk_total, calls, _ = walks[-1]
    secs = min(w[3] for w in walks)
    return {
        "stats": st,
        "miss_lookup_kernel_ms": round(ms, 3),
        "miss_lookup_hits": hits,
        "export_entries": total,
        "export_spk_bytes": spk_total,
        "export_calls": calls,
        "export_wall_s_runs": [round(w[3], 4) for w in walks],
        "export_entries_per_s": round(total / secs) if secs else 0,
    }


def main():
    from rusty_kaspa_amd.engine import Engine  # needs __graft_entry__.build()

    ops, ents, spks = make_entries()
    eng = Engine()
    ctx = ctypes.c_void_p(eng.ctx)
    assert eng.lib.kv_utxo_reset(ctx, ctypes.c_uint64(CAPACITY)) == 0
    upsert(eng, ops[:N_INLINE], ents[:N_INLINE])
    upsert(eng, ops[N_INLINE:], ents[N_INLINE:], spks.tobytes())
    fresh_stats = eng.utxo_stats()
    slots = fresh_stats["slots"]

    rs = np.random.RandomState(6)
    miss_ops = rs.randint(0, 256, size=(N_MISS, 36), dtype=np.uint8)
    miss_ops[:, 33:] = 0
    fresh_ms, _ = miss_lookup_ms(eng, miss_ops)

    rounds = 0
    st = fresh_stats
    while st["n_empty"] >= EMPTY_TARGET * slots and rounds < MAX_ROUNDS:
        rows = rs.choice(N_INLINE, size=CHURN, replace=False)
        remove(eng, ops[rows])
        new_ops = rs.randint(0, 256, size=(CHURN, 36), dtype=np.uint8)
        new_ops[:, 33:] = 0
        ops[rows] = new_ops
        upsert(eng, ops[rows], ents[rows])
        arows = N_INLINE + rs.choice(N_ARENA, size=ARENA_CHURN, replace=False)
        blob = rs.randint(0, 256, size=(ARENA_CHURN, ARENA_SPK), dtype=np.uint8)
        upsert(eng, ops[arows], ents[arows], blob.tobytes())
        rounds += 1
        st = eng.utxo_stats()

    before = measure(eng, miss_ops)
    c0, n0, _ = eng.utxo_commitment()
    rehash_ms = eng.utxo_rehash(0)
    c1, n1, _ = eng.utxo_commitment()
    after = measure(eng, miss_ops)
    # the same call again, on a table with nothing to reclaim
    clean_ms = [eng.utxo_rehash(0) for _ in range(3)]
    c2, n2, commit_ms = eng.utxo_commitment()
    eng.close()

    n = N_INLINE + N_ARENA
    ok = (num(c0) % P == num(c1) % P == num(c2) % P and n0 == n1 == n2 == n
          and before["export_entries"] == after["export_entries"] == n
          and before["miss_lookup_hits"] == after["miss_lookup_hits"] == 0
          and after["stats"]["n_tomb"] == 0
          and after["stats"]["arena_used"] == after["stats"]["arena_live_bytes"]
          == N_ARENA * ARENA_SPK)
    print(json.dumps({
        "probe": "utxo_rehash",
        "slots": slots, "entries": n, "arena_entries": N_ARENA,
        "churn_rounds": rounds, "churn_keys_per_round": CHURN,
        "reached_empty_target": bool(st["n_empty"] < EMPTY_TARGET * slots),
        "miss_keys": N_MISS,
        "fresh_stats": fresh_stats,
        "fresh_miss_lookup_kernel_ms": round(fresh_ms, 3),
        "before": before,
        "rehash_kernel_ms": round(rehash_ms, 3),
        "after": after,
        "clean_rehash_kernel_ms_runs": [round(x, 3) for x in clean_ms],
        "commitment_kernel_ms": round(commit_ms, 3),
        "export_chunk_entries": CHUNK,
        "consistent": bool(ok),
    }), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
