"""Throughput of the bzip2 size path: one JSON line with pair-compressions/s of the GPU
(all ordered pairs of a set, singles included in the wall time), the device time of the pair batches, a parity
spot check against bz2.compress, and the CPU baseline: bz2.compress of a sample of the same pairs on every core of
this host (threads: the call releases the GIL).

    python tools/gpu_bzip2_bench.py --n 64 --len 1000000 [--related 0.02] [--cpu-sample N]
"""
import argparse
import bz2
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_set(n, length, related, seed):
    rng = np.random.default_rng(seed)
    if not related:
        return [ACGT[rng.integers(0, 4, length)].tobytes() for _ in range(n)]
    anc = ACGT[rng.integers(0, 4, length)]
    out = []
    for _ in range(n):
        a = anc.copy()
        k = rng.random(length) < related
        a[k] = ACGT[rng.integers(0, 4, int(k.sum()))]
        out.append(a.tobytes())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--len", type=int, default=1000000)
    ap.add_argument("--related", type=float, default=0.0, help="mutation rate of mutants of one ancestor (0 = unrelated)")
    ap.add_argument("--cpu-sample", type=int, default=0,
                    help="pairs compressed by the CPU baseline (default 8 x the core count: several waves, a steady rate)")
    ap.add_argument("--check", type=int, default=16, help="pairs checked against bz2.compress")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    a.cpu_sample = a.cpu_sample or 8 * os.cpu_count()
    from snacc_amd.hip_backend import HipContext
    seqs = make_set(a.n, a.len, a.related, a.seed)
    rng = np.random.default_rng(a.seed + 1)
    with HipContext(0, defer_singles=1) as ctx:          # as the CLI: a bzip2 run never needs the lz4 phase A
        ctx.upload(seqs)
        t0 = time.perf_counter()
        singles = ctx.bzip2_singles()
        pairs = ctx.bzip2_pairs()
        wall = time.perf_counter() - t0
        kernel_ms = ctx.bzip2_last_ms()
    ij = [tuple(map(int, rng.integers(0, a.n, 2))) for _ in range(a.check)]
    with ThreadPoolExecutor(os.cpu_count()) as ex:
        want = list(ex.map(lambda p: len(bz2.compress(seqs[p[0]] + seqs[p[1]])), ij))
        ok = all(int(pairs[i, j]) == w for (i, j), w in zip(ij, want)) and int(singles[0]) == len(bz2.compress(seqs[0]))
        sample = [tuple(map(int, rng.integers(0, a.n, 2))) for _ in range(a.cpu_sample)]
        t0 = time.perf_counter()
        list(ex.map(lambda p: len(bz2.compress(seqs[p[0]] + seqs[p[1]])), sample))
        cpu_wall = time.perf_counter() - t0
    n_pairs = a.n * a.n
    gpu_rate = n_pairs / wall
    cpu_rate = a.cpu_sample / cpu_wall
    print(json.dumps({"tool": "gpu_bzip2_bench", "n": a.n, "len": a.len, "related": a.related, "pairs": n_pairs,
                      "gpu_wall_s": round(wall, 3), "kernel_ms": round(kernel_ms, 1),
                      "gpu_pair_compr_per_s": round(gpu_rate, 1), "cpu_cores": os.cpu_count(),
                      "cpu_pair_compr_per_s": round(cpu_rate, 1), "speedup": round(gpu_rate / cpu_rate, 2),
                      "parity_ok": bool(ok), "parity_checked": a.check}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
