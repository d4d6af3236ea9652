"""Probe: what it costs to keep a diff revertible on the GPU UTXO table, on one
GPU.

Builds utxo_commit_probe's table (4M slots, 1M inline entries plus 1,000 arena
entries). For diffs of 3,000 and of 30,000 outpoints per side (one block; a
wide mergeset), 1% of each side in the arena, it times, in alternating rounds
on the same table,
  - journal:   kv_utxo_apply_diff, then kv_utxo_revert (wall time of each call,
               and the kernel_ms each reports);
  - plain:     the same diff through kv_utxo_remove + kv_utxo_upsert_spk, which
               cannot be undone;
  - host_undo: the same diff the way a host keeps it revertible without the
               journal: kv_utxo_lookup_spk of the removed side to host memory,
               then kv_utxo_remove + kv_utxo_upsert_spk.
After a plain or host_undo round the table is put back, untimed, by the inverse
remove + upsert. Every call ends in a stream synchronisation, so wall times are
of finished work. It prints one JSON line, with the best and the median of the
rounds, and the journal bytes of one diff. It also checks that kv_utxo_commitment
after all rounds equals the one before, mod P. There is no pass threshold on
the times.
"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

from utxo_commit_probe import (ARENA_SPK, CAPACITY, N_ARENA, N_INLINE, P,  # noqa: E402
                               make_entries, num)
from utxo_rehash_probe import remove, upsert  # noqa: E402

DIFFS = (3000, 30000)
ARENA_SHARE = 100  # one outpoint in 100 of each side has an arena script
ROUNDS = 7         # after one warm-up round


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def make_diff(rs, ops, ents, spks, d):
    """(removed ops, removed entries, removed scripts, added ops, added
    entries, added scripts): d live keys out, d fresh keys in"""
    n_arena = min(d // ARENA_SHARE, N_ARENA)
    rows = np.concatenate([
        rs.choice(N_INLINE, size=d - n_arena, replace=False),
        N_INLINE + rs.choice(N_ARENA, size=n_arena, replace=False)])
    rem_spk = spks[rows[d - n_arena:] - N_INLINE]
    add_ops = rs.randint(0, 256, size=(d, 36), dtype=np.uint8)
    add_ops[:, 33:] = 0
    add_ents = np.zeros((d, 64), dtype=np.uint8)
    add_ents[:, 0:6] = rs.randint(0, 256, size=(d, 6), dtype=np.uint8)
    add_ents[:d - n_arena, 20] = 34
    add_ents[:d - n_arena, 24:58] = rs.randint(0, 256, size=(d - n_arena, 34),
                                               dtype=np.uint8)
    add_ents[d - n_arena:, 20] = ARENA_SPK
    add_spk = rs.randint(0, 256, size=(n_arena, ARENA_SPK), dtype=np.uint8)
    return ops[rows], ents[rows], rem_spk, add_ops, add_ents, add_spk


def summary(ms):
    return {"best_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3)}


def run_diff(eng, diff):
    rem_ops, rem_ents, rem_spk, add_ops, add_ents, add_spk = diff
    d = len(rem_ops)
    ctx = ctypes.c_void_p(eng.ctx)
    rem_b, add_b = rem_ops.tobytes(), add_ops.tobytes()
    add_e, add_s = add_ents.tobytes(), add_spk.tobytes()
    out = (ctypes.c_uint8 * (64 * d))()
    bm = (ctypes.c_uint64 * ((d + 63) // 64))()
    spk = (ctypes.c_uint8 * max(1, rem_spk.size))()
    used = ctypes.c_size_t()

    def plain():  # argument bytes prepared outside, as for the journaled call
        rc = eng.lib.kv_utxo_remove(ctx, rem_b, ctypes.c_size_t(d))
        rc = rc or eng.lib.kv_utxo_upsert_spk(ctx, add_b, add_e, add_s,
                                              ctypes.c_size_t(len(add_s)),
                                              ctypes.c_size_t(d))
        if rc:
            raise RuntimeError(eng.lib.kv_last_error().decode())

    def host_lookup():
        rc = eng.lib.kv_utxo_lookup_spk(ctx, rem_b, ctypes.c_size_t(d), out, bm, spk,
                                        ctypes.c_size_t(len(spk)), ctypes.byref(used))
        if rc:
            raise RuntimeError(eng.lib.kv_last_error().decode())

    def put_back():
        remove(eng, add_ops)
        upsert(eng, rem_ops, rem_ents, rem_spk.tobytes())

    t = {k: [] for k in ("apply_wall", "apply_kernel", "revert_wall", "revert_kernel",
                         "plain_wall", "host_undo_wall", "host_undo_lookup_wall")}
    journal_bytes = missing = overwrote = 0
    for r in range(ROUNDS + 1):
        ms_apply, (token, res) = timed(
            lambda: eng.utxo_apply_diff(rem_b, add_b, add_e, add_s))
        ms_revert, _ = timed(lambda: eng.utxo_revert(token))
        revert_kernel = eng.utxo_journal_stats()["last_revert_kernel_ms"]
        ms_plain, _ = timed(plain)
        put_back()
        ms_look, _ = timed(host_lookup)
        ms_rest, _ = timed(plain)
        put_back()
        journal_bytes = res["journal_bytes"]
        missing += res["n_removed_missing"]
        overwrote += res["n_added_overwrote"]
        if r == 0:
            continue  # warm-up: first launches, buffer growth
        t["apply_wall"].append(ms_apply)
        t["apply_kernel"].append(res["kernel_ms"])
        t["revert_wall"].append(ms_revert)
        t["revert_kernel"].append(revert_kernel)
        t["plain_wall"].append(ms_plain)
        t["host_undo_lookup_wall"].append(ms_look)
        t["host_undo_wall"].append(ms_look + ms_rest)
    hits = sum(bin(w).count("1") for w in bm)
    return {
        "outpoints_per_side": d,
        "arena_per_side": int(rem_spk.shape[0]),
        "journal_bytes": journal_bytes,
        "journal": {k: summary(t[k]) for k in ("apply_wall", "apply_kernel",
                                               "revert_wall", "revert_kernel")},
        "plain": summary(t["plain_wall"]),
        "host_undo": summary(t["host_undo_wall"]),
        "host_undo_lookup": summary(t["host_undo_lookup_wall"]),
    }, (missing == 0 and overwrote == 0 and hits == d)


def main():
    from rusty_kaspa_amd.engine import Engine  # needs __graft_entry__.build()

    ops, ents, spks = make_entries()
    eng = Engine()
    ctx = ctypes.c_void_p(eng.ctx)
    assert eng.lib.kv_utxo_reset(ctx, ctypes.c_uint64(CAPACITY)) == 0
    upsert(eng, ops[:N_INLINE], ents[:N_INLINE])
    upsert(eng, ops[N_INLINE:], ents[N_INLINE:], spks.tobytes())
    c0, n0, _ = eng.utxo_commitment()
    rs = np.random.RandomState(8)
    results, ok = [], True
    for d in DIFFS:
        res, clean = run_diff(eng, make_diff(rs, ops, ents, spks, d))
        results.append(res)
        ok = ok and clean
    c1, n1, _ = eng.utxo_commitment()
    stats = eng.utxo_stats()
    journal = eng.utxo_journal_stats()
    eng.close()
    ok = bool(ok and n0 == n1 == N_INLINE + N_ARENA and num(c0) % P == num(c1) % P
              and journal["n_records"] == 0)
    print(json.dumps({
        "probe": "utxo_reorg",
        "slots": stats["slots"], "entries": n1, "arena_entries": N_ARENA,
        "rounds": ROUNDS,
        "diffs": results,
        "final_stats": stats,
        "consistent": ok,
    }), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
