#!/usr/bin/env python3
"""Cost of Pauli expectation values on one GPU (fp64): prints one JSON line.

  python tools/bench_pauli.py [--qubits 30] [--reps 7] [--warmup 2] [--out FILE]

Times (milliseconds, median of --reps after --warmup calls; every timed call
returns a value, so it ends in a device synchronise):
  total_prob_cold   calcTotalProb after a gate and a sync (the norm cache misses):
                    one plain read of the state
  prod_z / prod_x_top / prod_x0
                    one calcExpecPauliProd: a Z-only string, X on the top qubit,
                    X on qubit 0
  workaround_x_top  the same term without the new call: cloneQureg + pauliX +
                    calcInnerProduct through a second register
  ising / random100 calcExpecPauliSum of the 59-term open-chain transverse-field
                    Ising Hamiltonian (n - 1 ZZ + n X) and of 100 seeded random
                    strings of weight <= 4: time, pauliPasses, value
  *_term_by_term    the same sums through one calcExpecPauliProd per term
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("QUEST_BACKEND", "hip")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=2, help="random layers applied to |+..+> first")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()

    import numpy as np

    import quest_amd as qa
    from quest_amd.models import random_layered
    from quest_amd.ops import capi

    env = qa.Env()
    if capi.getQuESTBackend() != "HIP" and not os.environ.get("QUEST_BENCH_ALLOW_CPU"):
        sys.exit("bench_pauli.py measures the HIP library on a GPU (QUEST_BENCH_ALLOW_CPU=1: dry run on the host)")
    n = a.qubits
    reg, work = qa.Register(env, n), qa.Register(env, n)
    reg.init_plus()
    random_layered(n, a.layers, seed=1).apply(reg)
    reg.sync()

    def timed(fn, before=None):
        ts, val = [], None
        for k in range(a.warmup + a.reps):
            if before:
                before()
            t0 = time.perf_counter()
            val = fn()
            t1 = time.perf_counter()
            if k >= a.warmup:
                ts.append((t1 - t0) * 1e3)
        return statistics.median(ts), min(ts), val

    def touch():   # a gate and a sync: the next read finds no cache
        reg.rz(0, 1e-3)
        reg.sync()

    res = {"qubits": n, "precision": capi.binding().prec, "backend": capi.getQuESTBackend(), "reps": a.reps,
           "layout": capi.getQubitLayout(reg.q)}
    ms, lo, val = timed(reg.total_prob, touch)
    res["total_prob_cold_ms"], res["total_prob_cold_min_ms"] = ms, lo
    cold = ms

    singles = {"prod_z": {0: "Z", n // 2: "Z", n - 1: "Z"}, "prod_x_top": {n - 1: "X"}, "prod_x0": {0: "X"}}
    for name, term in singles.items():
        qs = list(term)
        codes = ["IXYZ".index(term[q]) for q in qs]
        ms, lo, val = timed(lambda: capi.calcExpecPauliProd(reg.q, qs, codes))
        res[name] = {"ms": ms, "min_ms": lo, "value": val, "vs_total_prob_cold": ms / cold}

    def workaround():
        work.clone_from(reg)
        work.x(n - 1)
        return work.inner(reg).real

    ms, lo, val = timed(workaround)
    res["workaround_x_top"] = {"ms": ms, "min_ms": lo, "value": val,
                               "speedup_of_prod": ms / res["prod_x_top"]["ms"]}

    rng = np.random.default_rng(2024)
    ising = [{q: "Z", q + 1: "Z"} for q in range(n - 1)] + [{q: "X"} for q in range(n)]
    ising_c = [-1.0] * (n - 1) + [-0.5] * n
    rand = []
    for _ in range(100):
        w = int(rng.integers(1, 5))
        qs = rng.choice(n, size=min(w, n), replace=False)
        rand.append({int(q): "XYZ"[rng.integers(3)] for q in qs})
    rand_c = list(rng.normal(size=100))

    for name, terms, coeffs in (("ising", ising, ising_c), ("random100", rand, rand_c)):
        def whole():
            return reg.expec_pauli_sum(terms, coeffs)

        def each():
            s = 0.0
            for t, c in zip(terms, coeffs):
                qs = list(t)
                s += c * capi.calcExpecPauliProd(reg.q, qs, ["IXYZ".index(t[q]) for q in qs])
            return s

        capi.resetQuESTStats()
        whole()
        st = capi.getQuESTStats()
        ms, lo, val = timed(whole)
        ms1, lo1, val1 = timed(each)
        passes = int(st["pauliPasses"])
        res[name] = {"terms": len(terms), "ms": ms, "min_ms": lo, "value": val, "pauliPasses": passes,
                     "ms_per_pass": ms / passes, "pass_vs_total_prob_cold": ms / passes / cold,
                     "term_by_term_ms": ms1, "term_by_term_value": val1, "speedup": ms1 / ms,
                     "terms_per_pass": len(terms) / passes}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    reg.close()
    work.close()


if __name__ == "__main__":
    main()
