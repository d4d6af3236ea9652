#!/usr/bin/env python3
"""Benchmark: batched Schnorr sig-verifies/sec (BASELINE.json configs[1], the
headline). A plain run sets up, warms up, times --steps passes of the verify
kernel and prints ONE JSON result line. `--full` adds everything else: the
txs-validated/sec leg on the full block path (configs[2] shape, its line is
printed first, the headline verify line LAST), the OpenMP cpu_baseline legs
and the verdict-bitmap spot-check against the oracle.

`--dump-outputs DIR` writes what the last timed step returned to its caller
as DIR/<name>.npy (float32/float64): the per-tuple verdicts of the verify
leg, and the per-tx codes/fees plus the muhash commitment of the block leg.
Inputs are seeded, so two builds can be compared output for output.

Workloads:
  verify ("schnorr-verify-1M"): 1M synthetic (r,s,pk,msg) tuples, 128B each,
  staged into HBM; one STEP = one pass of the kv_verify_schnorr_batch kernel
  with inputs already resident. Tuples are deterministic (seed recorded),
  signed for real by the oracle's BIP-340 signer, and PRE-GENERATED into
  bench_data/ by __graft_entry__.build() (pregenerate_inputs below) so the
  driver's timed region dominates the run instead of tuple generation.

  block ("block-validate-config3"): 32 blocks x 300 txs of the config-3 mix
  (70% 1-in P2PK schnorr / 20% multi-input / 10% ECDSA) through
  kv_validate_block with FULL flags + the muhash finalize. The blob is handed
  over as host memory — the real call pattern — so this rate is
  PCIe-inclusive (noted in DESIGN.md).

cpu_baseline (--full only): the oracle restatement ("port" kind) with OpenMP
on the host cores over a bounded sample of the same inputs.

Multi-GPU (the driver launches us under torch.distributed.run): weak scaling —
every rank verifies/validates its own batch (identical cached tuple batch per
rank; per-rank block blobs), with the real path's exchanges over RCCL/xGMI:
the verdict-bitmap all-reduce (verify) and the 768B muhash-partial all-gather
+ multiplicative fold (block).
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

SEED = 42
DEFAULT_TUPLES = 1 << 20  # 1M — the BASELINE config-2 batch
INVALID_PERMILLE = 0  # all-valid variant is the headline; 10%-invalid via flag
DATA_DIR = os.path.join(REPO, "bench_data")

# Algorithmic work accounting for the verify-kernel roofline (single committed
# account, mirrored by DESIGN.md §4): the GLV-split ladder — 4-bit windows for
# the per-signature P streams (affine batch-inverted table), 8-bit fixed-base
# comb digits for the shared-G streams — does
#   132 Jacobian doubles  x  7 fe_mul-equiv      =  924
#   100 mixed adds        x 11                   = 1100
#     (66 signed-window P-stream + 34 G-comb)
#    34 phi-multiplies    x  1                   =   34
#     8-entry signed P-table build 7 x 11        =   77
#    table batch-inversion (prefix 6 + inv 269
#      + back-sub 12 + 4x7 per-entry)            =  315
#    x-lift sqrt (addition chain)                =  266
#    final inversion (addition chain)            =  269  (+ ~100 misc: scalar
#    decomposition muls, digit recode, challenge) ≈ 3,085 fe_mul-equivalents
# per verify; each 10x26-limb fe_mul ≈ 170 u32-ALU-op equivalents (100 v_mad
# 32x32 column products + fold/normalize) → ≈ 0.52e6 u32-ops per verify.
ALG_FE_MULS_PER_VERIFY = 3085
ALG_OPS_PER_FE_MUL = 170
ALG_OPS_PER_VERIFY = ALG_FE_MULS_PER_VERIFY * ALG_OPS_PER_FE_MUL  # 524,450
# gfx950 VALU issue peak: 256 CU x 4 SIMD x 32 lanes x 2.4 GHz = 78.6 T u32/s
VALU_PEAK_TOPS = 78.6
# Memory-side traffic per verify, measured by rocprofv3 --pmc FETCH_SIZE /
# WRITE_SIZE (separate passes) on 262144-tuple staged dispatches of the
# SHIPPING kernel (signed P table + G comb + pair-window frames):
# (5.684e6 + 4.668e6) KiB / 262144 = 40,438 B/verify (fetch 22.2KB + write
# 18.2KB — scratch table reads + the per-frame accumulator spill; vs 128B of
# algorithmic input; r1 baseline 119,296). Provenance:
# profiles/r02e_shipping_kernel_pmc.json.
TRAFFIC_BYTES_PER_VERIFY = 40438


def log(msg):
    print(f"[bench] {msg}", file=sys.stderr, flush=True)


def load_oracle():
    so = os.path.join(REPO, "oracle", "liboracle.so")
    if not os.path.exists(so) and int(os.environ.get("LOCAL_RANK", "0")) == 0:
        # only rank 0 builds; the .so normally ships prebuilt in-tree
        subprocess.run(["make", "-s", "-C", os.path.join(REPO, "oracle")], check=True)
    for _ in range(60):
        if os.path.exists(so):
            break
        time.sleep(1)
    return ctypes.CDLL(so)


def tuple_cache_path(n, seed, invalid_permille):
    return os.path.join(DATA_DIR, f"tuples_s{seed}_n{n}_i{invalid_permille}.bin")


def host_threads(world=1):
    """OpenMP width for the oracle legs: OMP_NUM_THREADS when the host sets it
    (a job may own fewer CPUs than the machine has), else the visible cores."""
    env = os.environ.get("OMP_NUM_THREADS", "")
    if env.isdigit() and int(env) > 0:
        return int(env)
    return max(8, (os.cpu_count() or 8) // max(1, world))


def gen_tuples(n, seed, invalid_permille, world=1):
    """Cached when the pre-generated file exists (bench_data/); else generate
    with the oracle signer (outside any timed region either way). The tuples
    are a pure function of (seed, index), so both paths give the same bytes."""
    cache = tuple_cache_path(n, seed, invalid_permille)
    if os.path.exists(cache) and os.path.getsize(cache) == n * 128:
        with open(cache, "rb") as f:
            raw = f.read()
        log(f"loaded {n} cached tuples ({cache})")
        return ctypes.create_string_buffer(raw, n * 128)
    oracle = load_oracle()
    buf = ctypes.create_string_buffer(n * 128)
    t0 = time.time()
    oracle.ok_gen_schnorr_tuples(ctypes.c_uint64(seed), ctypes.c_size_t(n),
                                 ctypes.c_uint32(invalid_permille), buf,
                                 host_threads(world))
    log(f"generated {n} tuples in {time.time()-t0:.1f}s (seed {seed})")
    return buf


def pregenerate_inputs():
    """Called by __graft_entry__.build(): write the default run's 1M-tuple
    batch into bench_data/ once, so a plain run loads it instead of signing
    1M messages on the host before its first step."""
    cache = tuple_cache_path(DEFAULT_TUPLES, SEED, INVALID_PERMILLE)
    if os.path.exists(cache) and os.path.getsize(cache) == DEFAULT_TUPLES * 128:
        return
    buf = gen_tuples(DEFAULT_TUPLES, SEED, INVALID_PERMILLE)
    os.makedirs(DATA_DIR, exist_ok=True)
    tmp = f"{cache}.{os.getpid()}.tmp"
    with open(tmp, "wb") as f:
        f.write(buf.raw)
    os.replace(tmp, cache)  # atomic: a reader never sees a partial file


def dump_outputs(out_dir, arrays):
    """--dump-outputs: one DIR/<name>.npy per array the last timed step handed
    back to its caller (float32, or float64 where values may exceed 2^24)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for name, arr in arrays.items():
        assert arr.dtype in (np.float32, np.float64), name
        total += arr.nbytes
        np.save(os.path.join(out_dir, f"{name}.npy"), arr)
    assert total <= 64 << 20, f"--dump-outputs wrote {total} bytes (> 64 MB)"
    log(f"dumped {', '.join(arrays)} to {out_dir} ({total/1e6:.1f} MB)")


def gen_block_blob(oracle, rank, n_txs, adversarial):
    mix = dict(pct_multi_input=20, pct_ecdsa=10)
    tag = "cfg3"
    if adversarial:
        # BASELINE config 5: invalid sigs + large multisig scripts exercising
        # branch divergence (the 1M-entry UTXO-set leg is the block-utxo mode
        # with a pre-seeded table; table scaling in tests/test_gpu_utxo.py)
        mix = dict(pct_multi_input=20, pct_ecdsa=10, pct_multisig=10,
                   pct_invalid=10)
        tag = "cfg5"
    cache = os.path.join(DATA_DIR, f"blob_s{SEED + rank}_t{n_txs}_{tag}.bin")
    if os.path.exists(cache):
        with open(cache, "rb") as f:
            blob = f.read()
        log(f"loaded cached block blob ({cache}, {len(blob)/1e6:.1f} MB)")
        return blob
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    from workload import gen_block
    t0 = time.time()
    blob, _ = gen_block(oracle, seed=SEED + rank, n_txs=n_txs, **mix)
    log(f"generated {n_txs} mixed txs ({len(blob)/1e6:.1f} MB blob) "
        f"in {time.time()-t0:.1f}s")
    return blob


def cpu_baseline_leg(oracle, tuples, n):
    """Oracle ('port') timed on host cores over a bounded sample (~10-30s)."""
    cores = os.cpu_count() or 8
    sample = min(n, 1 << 18)  # 262144 ≈ 8s at ~34k/s on 8 cores
    words = (sample + 63) // 64
    bm = (ctypes.c_uint64 * words)()
    t0 = time.perf_counter()
    oracle.ok_verify_schnorr_batch(tuples, ctypes.c_size_t(sample), cores, bm)
    dt = time.perf_counter() - t0
    return {
        "value": round(sample / dt, 1),
        "unit": "sig-verifies/sec",
        "cores": cores,
        "kind": "port",
        "sample": f"{sample} tuples of the same batch, {dt:.1f}s wall",
    }


class KvTimings(ctypes.Structure):
    _fields_ = [("subhash_ms", ctypes.c_double), ("s_assemble_ms", ctypes.c_double),
                ("e_assemble_ms", ctypes.c_double), ("schnorr_ms", ctypes.c_double),
                ("ecdsa_ms", ctypes.c_double), ("muhash_ms", ctypes.c_double),
                ("n_schnorr", ctypes.c_uint64), ("n_ecdsa", ctypes.c_uint64)]


def block_mode(args, dist_ctx=None):
    """txs-validated/sec on the full block path (BASELINE config 3 shape:
    300 txs/block). One step = one kv_validate_block call over a
    mergeset-sized batch of blocks + the muhash finalize."""
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    distributed = world > 1
    oracle = load_oracle()
    n_txs = args.block_batch * 300
    # each rank validates its own shard of blocks (blocks are independent;
    # the only cross-rank step in the real path is the muhash combine)
    blob = gen_block_blob(oracle, rank, n_txs, args.adversarial)
    from rusty_kaspa_amd.engine import Engine
    # sig cache OFF for the bench: the batch is reused across timed steps and
    # a cache hit would skip the verify work being measured
    eng = Engine(device=local_rank, sig_cache_size=0)

    utxo = args.mode == "block-utxo"
    if utxo:
        # populate path: entries resolve from the GPU-resident UTXO table
        # (kv_validate_block_utxo). apply_diff stays off so the step is
        # steady-state repeatable; the diff-apply cost is covered by
        # tests/test_gpu_validate_utxo.py.
        from rusty_kaspa_amd.blob import strip_utxo_entries
        stripped, seeds = strip_utxo_entries(blob)
        lib = eng.lib
        ctx = ctypes.c_void_p(eng.ctx)
        assert lib.kv_utxo_reset(ctx, ctypes.c_uint64(2 * len(seeds))) == 0
        ops = b"".join(op for op, _ in seeds)
        ents = b"".join(e for _, e in seeds)
        assert lib.kv_utxo_upsert(ctx, ops, ents, ctypes.c_size_t(len(seeds))) == 0
        log(f"UTXO table seeded: {len(seeds)} entries")
        blob = stripped

    if distributed:
        import torch
        import torch.distributed as dist
        gather_buf = [torch.zeros(768, dtype=torch.uint8,
                                  device=f"cuda:{local_rank}")
                      for _ in range(world)]
        mine = torch.zeros(768, dtype=torch.uint8, device=f"cuda:{local_rank}")

    def one_step():
        if utxo:
            codes, fees, partial = eng.validate_block_utxo(
                blob, n_txs, 10**9, 10**9, 0, apply_diff=False)
        else:
            codes, fees, partial = eng.validate_block(blob, n_txs, 10**9, 10**9, 0,
                                                      raw=True)
        if distributed:
            # the real path's one exchange: allgather the 768B muhash
            # (numerator‖denominator) partials over RCCL, fold the
            # multiplicative combine on rank 0 (not an RCCL builtin)
            import torch
            import torch.distributed as dist
            mine.copy_(torch.frombuffer(bytearray(partial), dtype=torch.uint8))
            dist.all_gather(gather_buf, mine)
            if rank == 0:
                acc = bytearray(gather_buf[0].cpu().numpy().tobytes())
                for r in range(1, world):
                    eng.muhash_combine(acc, gather_buf[r].cpu().numpy().tobytes())
                mh = eng.muhash_finalize(bytes(acc))
            else:
                mh = None
        else:
            mh = eng.muhash_finalize(bytes(partial))
        return codes, fees, mh

    for _ in range(args.warmup):
        codes, _, _ = one_step()
    if args.adversarial:
        bad = sum(1 for c in codes if c != 0)
        assert 0 < bad < len(codes), "adversarial mix must reject some txs"
        log(f"adversarial: {bad}/{len(codes)} txs rejected (expected)")
    else:
        assert all(c == 0 for c in codes), "unexpected invalid txs in bench batch"
    if distributed:
        import torch
        import torch.distributed as dist
        dist.barrier()
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = one_step()
    elapsed = time.perf_counter() - t0
    if distributed:
        import torch
        import torch.distributed as dist
        torch.cuda.synchronize()
        dist.barrier()
        el = torch.tensor([elapsed], device=f"cuda:{local_rank}")
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
        elapsed = float(el.item())
    value = world * n_txs * args.steps / elapsed

    # dominant-kernel roofline from the engine's hipEvent timings of the last
    # step: the schnorr verify kernel (the ALU hot spot of the path)
    tm = KvTimings()
    assert eng.lib.kv_get_validate_timings(ctypes.c_void_p(eng.ctx),
                                           ctypes.byref(tm)) == 0
    roofline = None
    if tm.schnorr_ms > 0 and tm.n_schnorr > 0:
        ach = ALG_OPS_PER_VERIFY * tm.n_schnorr / (tm.schnorr_ms / 1e3) / 1e12
        roofline = {
            "bound": "valu",  # integer-VALU compute roofline (no MFMA path
            # exists for 256-bit carry arithmetic); peak = gfx950 u32 issue peak
            "achieved": round(ach, 2),
            "peak": VALU_PEAK_TOPS,
            "unit": "TFLOP/s",
            "frac": round(ach / VALU_PEAK_TOPS, 4),
            "traffic": (TRAFFIC_BYTES_PER_VERIFY * tm.n_schnorr
                        if TRAFFIC_BYTES_PER_VERIFY else None),
            "kernel": "kv_schnorr_verify_kernel",
            "kernel_ms": {"subhash": round(tm.subhash_ms, 3),
                          "assemble": round(tm.s_assemble_ms + tm.e_assemble_ms, 3),
                          "schnorr": round(tm.schnorr_ms, 3),
                          "ecdsa": round(tm.ecdsa_ms, 3),
                          "muhash": round(tm.muhash_ms, 3)},
        }

    if args.dump_outputs and rank == 0:
        import numpy as np
        codes, fees, mh = last
        dump_outputs(args.dump_outputs, {
            "block_tx_codes": np.array(codes[:], dtype=np.float32),
            "block_tx_fees": np.array(fees[:], dtype=np.float64),
            "block_muhash": np.frombuffer(mh, dtype=np.uint8).astype(np.float32),
        })

    cpu_baseline = None
    if args.full and not args.skip_cpu_baseline and world == 1:
        cores = os.cpu_count() or 8
        codes_a = (ctypes.c_int32 * n_txs)()
        fees_a = (ctypes.c_uint64 * n_txs)()
        mh_a = (ctypes.c_uint8 * 32)()
        t0 = time.perf_counter()
        oracle.ok_validate_block_parallel(blob, len(blob), 10**9, 10**9, 0, cores,
                                          codes_a, fees_a, mh_a)
        dt = time.perf_counter() - t0
        cpu_baseline = {"value": round(n_txs / dt, 1), "unit": "txs-validated/sec",
                        "cores": cores, "kind": "port",
                        "sample": f"{n_txs} txs, one full pass, {dt:.1f}s wall"}

    result = {
        "metric": "txs-validated/sec",
        "value": round(value, 1),
        "unit": "txs/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1000, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u256",
        "data": "synthetic (seeded oracle-signed config-3 mix; batch reused across steps)",
        "config": {"workload": ("block-validate-utxo-config3" if args.mode == "block-utxo"
                                else "block-validate-config3"),
                   "blocks_per_step": args.block_batch, "txs_per_block": 300,
                   "mix": ("60p2pk/20multi-in/10ecdsa/10multisig+10pct-invalid"
                           if args.adversarial else "70p2pk/20multi-in/10ecdsa"),
                   "flags": "FULL", "sig_cache": "off",
                   "parallelism": f"dp{world}" if world > 1 else "single"},
        "roofline": roofline,
        "cpu_baseline": cpu_baseline,
    }
    if rank == 0:
        print(json.dumps(result), flush=True)
    eng.close()


def verify_mode(args):
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    distributed = world > 1

    import torch
    n = args.tuples
    # identical cached batch on every rank (weak scaling: each rank does the
    # full batch of work; the bitmap exchange below keeps the real
    # collective in the step). Per-rank seeds only when generating live.
    tuples = gen_tuples(n, SEED, args.invalid_permille, world)

    from rusty_kaspa_amd.engine import Engine
    eng = Engine(device=local_rank, sig_cache_size=0)
    lib = eng.lib
    ctx = ctypes.c_void_p(eng.ctx)

    rc = lib.kv_stage_tuples(ctx, tuples, ctypes.c_size_t(n), 0)
    assert rc == 0, lib.kv_last_error().decode()

    kernel_ms = ctypes.c_double()
    words = (n + 63) // 64
    bitmap_t = (torch.zeros(words, dtype=torch.int64, device=f"cuda:{local_rank}")
                if distributed else None)

    def one_step():
        rc = lib.kv_verify_staged(ctx, ctypes.c_size_t(n), 0, ctypes.byref(kernel_ms))
        assert rc == 0, lib.kv_last_error().decode()
        if distributed:
            # the real path's exchange: the global verdict bitmap over
            # RCCL/xGMI (identical batches → MAX keeps bits exact)
            import torch.distributed as dist
            dist.all_reduce(bitmap_t, op=dist.ReduceOp.MAX)
        return kernel_ms.value

    # warmup
    for _ in range(args.warmup):
        one_step()
    torch.cuda.synchronize()
    if distributed:
        import torch.distributed as dist
        dist.barrier()
    torch.cuda.synchronize()

    kernel_times = []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        kernel_times.append(one_step())
    torch.cuda.synchronize()
    if distributed:
        import torch.distributed as dist
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0

    if distributed:
        import torch.distributed as dist
        t = torch.tensor([elapsed], device=f"cuda:{local_rank}")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    total_verifies = n * args.steps * world
    value = total_verifies / elapsed
    ms_per_step = elapsed / args.steps * 1000.0

    # what the last timed step left for its caller: the verdict bitmap
    got = (ctypes.c_uint64 * words)()
    if args.full or args.dump_outputs:
        rc = lib.kv_fetch_bitmap(ctx, ctypes.c_size_t(n), got)
        assert rc == 0, lib.kv_last_error().decode()

    if args.dump_outputs and rank == 0:
        import numpy as np
        bits = np.unpackbits(np.frombuffer(got, dtype=np.uint8),
                             bitorder="little")[:n]
        cap = 1 << 23  # 32 MB of float32; larger batches dump a fixed sample
        if n > cap:
            idx = np.sort(np.random.default_rng(SEED).choice(n, cap, replace=False))
            bits = bits[idx]
        dump_outputs(args.dump_outputs,
                     {"verify_verdicts": bits.astype(np.float32)})

    if args.full:
        # correctness cross-check (outside timed region): bitmap vs oracle
        oracle = load_oracle()
        exp_words = (ctypes.c_uint64 * words)()
        sample = min(n, 1 << 14)
        oracle.ok_verify_schnorr_batch(tuples, ctypes.c_size_t(sample),
                                       os.cpu_count() or 8, exp_words)
        for i in range(sample // 64):
            assert got[i] == exp_words[i], f"bitmap mismatch at word {i}"
        log(f"verdict bitmap spot-check vs oracle OK ({sample} tuples)")

    avg_kernel_ms = sum(kernel_times) / len(kernel_times)
    log(f"kernel ms/step min={min(kernel_times):.2f} "
        f"avg={avg_kernel_ms:.2f} max={max(kernel_times):.2f} "
        f"(spread > ~10% = the box is clock-throttling; box-to-box spread "
        f"20-45M verifies/s observed on this pool)")
    achieved_tops = ALG_OPS_PER_VERIFY * n / (avg_kernel_ms / 1e3) / 1e12
    roofline = {
        "bound": "valu",  # integer-VALU compute roofline: no MFMA path exists
        # for 256-bit carry arithmetic; peak is the gfx950
        # u32 VALU issue peak.
        "achieved": round(achieved_tops, 2),
        "peak": VALU_PEAK_TOPS,
        "unit": "TFLOP/s",
        "frac": round(achieved_tops / VALU_PEAK_TOPS, 4),
        "traffic": (TRAFFIC_BYTES_PER_VERIFY * n
                    if TRAFFIC_BYTES_PER_VERIFY else None),
        "kernel": "kv_schnorr_verify_kernel",
        "kernel_ms": round(avg_kernel_ms, 3),
    }

    cpu_baseline = None
    if args.full and rank == 0 and world == 1 and not args.skip_cpu_baseline:
        cpu_baseline = cpu_baseline_leg(load_oracle(), tuples, n)

    if rank == 0:
        result = {
            "metric": "sig-verifies/sec",
            "value": round(value, 1),
            "unit": "verifies/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,  # no published reference numbers
            "dtype": "u256",  # 256-bit modular integer arithmetic
            "data": "synthetic (seeded oracle-signed BIP-340 tuples, cached batch)",
            "config": {
                "workload": "schnorr-verify-1M",
                "tuples_per_gpu": n,
                "invalid_permille": args.invalid_permille,
                "parallelism": f"shard{world}" if world > 1 else "single",
            },
            "roofline": roofline,
            "cpu_baseline": cpu_baseline,
        }
        print(json.dumps(result), flush=True)

    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--tuples", type=int, default=DEFAULT_TUPLES)
    ap.add_argument("--invalid-permille", type=int, default=INVALID_PERMILLE)
    ap.add_argument("--full", action="store_true",
                    help="also run the block-path leg, the cpu_baseline legs "
                         "and the oracle spot-check (a plain run only times "
                         "the headline verify leg)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy")
    ap.add_argument("--skip-cpu-baseline", action="store_true",
                    help="with --full: leave the cpu_baseline legs out")
    ap.add_argument("--mode", choices=["both", "verify", "block", "block-utxo"],
                    default=None,
                    help="default: verify; with --full: both")
    ap.add_argument("--block-batch", type=int, default=32,
                    help="blocks (of 300 txs) per step in the block leg")
    ap.add_argument("--adversarial", action="store_true",
                    help="BASELINE config-5 mix: 10%% invalid + multisig")
    args = ap.parse_args()
    if args.mode is None:
        args.mode = "both" if args.full else "verify"

    world = int(os.environ.get("WORLD_SIZE", "1"))
    # torch must own HIP runtime initialization BEFORE the engine loads it:
    # initializing the runtime through libkaspa_gpu first leaves torch's
    # device enumeration empty ("No HIP GPUs are available")
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group(backend="nccl")
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))

    if args.mode in ("block", "block-utxo"):
        block_mode(args)
    elif args.mode == "verify":
        verify_mode(args)
    else:  # both: block line first, the headline verify line LAST
        block_mode(args)
        verify_mode(args)

    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
