"""Probe: queries by script public key on the GPU-resident UTXO table.

Runs on the commit probe's table (4M slots, 1M random inline entries plus
1,000 arena entries) and prints one JSON line with
  - kv_utxo_balance_by_spk kernel_ms (best of 3) and wall ms for 0, 1, 1,000
    and 65,536 queries, half of them present (the single one present),
  - the same on a hot-address table in which all 1M entries carry one script,
    the worst case of the per-query atomics, for 1 and 1,000 queries,
  - both of the above with the wave-combining path of the balance kernel on
    (default) and off (KV_UTXO_QUERY_COMBINE=0, a second engine),
  - a full kv_utxo_find_by_spk walk for 1,000 queries (wall time, calls),
  - beside them, in the same run: kv_utxo_stats (the same scan with no script
    read: the floor; wall time, it reports no kernel time) and the wall time
    of a full kv_utxo_export_chunk walk, which is what a host must do today
    before it can filter.
Every balance is cross-checked against numpy sums. There is no pass threshold
on the times.
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

from utxo_commit_probe import CAPACITY, N_ARENA, N_INLINE, make_entries  # noqa: E402

QUERY_COUNTS = [0, 1, 1000, 65536]
RUNS = 3


def load(eng, ops, ents, spks):
    ctx = ctypes.c_void_p(eng.ctx)
    assert eng.lib.kv_utxo_reset(ctx, ctypes.c_uint64(CAPACITY)) == 0
    blob = spks.tobytes()
    rc = eng.lib.kv_utxo_upsert_spk(ctx, ops.tobytes(), ents.tobytes(), blob,
                                    ctypes.c_size_t(len(blob)),
                                    ctypes.c_size_t(len(ops)))
    assert rc == 0, eng.lib.kv_last_error()


def amounts(ents):
    return ents[:, 0:8].copy().view("<u8").reshape(-1)


def make_queries(rs, ents, n_q):
    """n_q distinct 34-byte queries, the first ceil(n_q / 2) of them scripts of
    inline entries; returns (queries, expected balances)"""
    n_present = (n_q + 1) // 2
    rows = rs.choice(N_INLINE, size=n_present, replace=False)
    amt = amounts(ents)
    queries = [(0, ents[r, 24:58].tobytes()) for r in rows]
    want = [int(amt[r]) for r in rows]
    absent = rs.randint(0, 256, size=(n_q - n_present, 34), dtype=np.uint8)
    queries += [(0, a.tobytes()) for a in absent]
    want += [0] * (n_q - n_present)
    return queries, want


def time_balance(eng, queries, want, total, n_live):
    kernel, wall = [], []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        bal, cnt, tot, live, ms = eng.utxo_balance_by_spk(queries)
        wall.append((time.perf_counter() - t0) * 1e3)
        kernel.append(ms)
        assert bal == want and tot == total and live == n_live
    return {"kernel_ms": round(min(kernel), 4),
            "kernel_ms_runs": [round(x, 4) for x in kernel],
            "wall_ms": round(min(wall), 3)}


def time_stats(eng):
    wall = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        st = eng.utxo_stats()
        wall.append((time.perf_counter() - t0) * 1e3)
    return st, round(min(wall), 3)


def find_walk(eng, queries, max_entries, slots):
    t0 = time.perf_counter()
    cursor, calls, n_total = 0, 0, 0
    while True:
        cursor, _, n = eng.utxo_find_by_spk(cursor, queries, max_entries)
        calls += 1
        n_total += n
        if n == 0 and cursor == slots:
            break
    return {"max_entries": max_entries, "matches": n_total, "calls": calls,
            "wall_ms": round((time.perf_counter() - t0) * 1e3, 3)}


def export_walk(eng, slots):
    t0 = time.perf_counter()
    cursor, calls, n_total = 0, 0, 0
    while True:
        cursor, _, _, _, n = eng.utxo_export_chunk(cursor, 1 << 16, 1 << 22)
        calls += 1
        n_total += n
        if n == 0 and cursor == slots:
            break
    return {"entries": n_total, "calls": calls,
            "wall_ms": round((time.perf_counter() - t0) * 1e3, 3)}


def measure(eng, ops, ents, spks, with_walks):
    """everything for one engine: the random table, then the hot one"""
    rs = np.random.RandomState(9)
    n = len(ops)
    out = {}
    load(eng, ops, ents, spks)
    total = int(amounts(ents).sum(dtype=np.uint64))
    st, stats_wall = time_stats(eng)
    assert st["n_live"] == n
    out["stats_wall_ms"] = stats_wall
    out["balance"] = {}
    for n_q in QUERY_COUNTS:
        queries, want = make_queries(rs, ents, n_q)
        out["balance"][str(n_q)] = time_balance(eng, queries, want, total, n)
        if n_q == 1000 and with_walks:
            out["find_walk_1000_queries"] = [
                find_walk(eng, queries, m, st["slots"]) for m in (4096, 64)]
    if with_walks:
        out["export_walk"] = export_walk(eng, st["slots"])
    # the hot table: every entry (the arena ones too, now inline) pays into
    # one script
    hot = ents.copy()
    hot[:, 20:24] = 0
    hot[:, 20] = 34
    hot[:, 24:58] = rs.randint(0, 256, size=34, dtype=np.uint8)
    hot[:, 58:64] = 0
    load(eng, ops, hot, spks[:0])
    hot_q = (0, hot[0, 24:58].tobytes())
    out["hot_balance"] = {}
    for n_q in (1, 1000):
        queries, want = make_queries(rs, ents, n_q - 1)
        queries, want = [hot_q] + queries, [total] + [0] * (n_q - 1)
        out["hot_balance"][str(n_q)] = time_balance(eng, queries, want, total, n)
    _, out["hot_stats_wall_ms"] = time_stats(eng)
    return out


def main():
    from rusty_kaspa_amd.engine import Engine  # needs __graft_entry__.build()

    ops, ents, spks = make_entries()
    result = {"probe": "utxo_query", "slots": 2 * CAPACITY,
              "entries": N_INLINE + N_ARENA, "arena_entries": N_ARENA,
              "runs": RUNS}
    os.environ.pop("KV_UTXO_QUERY_COMBINE", None)
    eng = Engine()
    result["window_slots"] = eng.utxo_commitment_window()
    result["combine_on"] = measure(eng, ops, ents, spks, with_walks=True)
    eng.close()
    os.environ["KV_UTXO_QUERY_COMBINE"] = "0"  # read once, in kv_create
    eng = Engine()
    result["combine_off"] = measure(eng, ops, ents, spks, with_walks=False)
    eng.close()
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
