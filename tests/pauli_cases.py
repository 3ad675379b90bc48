"""Shared by the Pauli expectation tests (test_pauli_expec.py,
test_pauli_expec_gpu.py, pauli_worker.py): the case list and the oracle.

The oracle applies the 2x2 Pauli matrices qubit by qubit to a copy of the NumPy
state (quest_amd.utils.oracle) and takes <psi|P psi> or Tr(P rho) -- nothing of
the index formula the library uses."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np

from quest_amd.utils import oracle as O

PAULI = {"X": O.X, "Y": O.Y, "Z": O.Z}
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# reductions of normalised states (tests/test_perm_kernels.py)
TOL = {2: 1e-11, 1: 2e-5, 4: 1e-11}


def expec_sv(v, n, term) -> float:
    w = O.StateVector(n, v)
    for q, p in enumerate(term):
        if p != "I":
            w.apply(PAULI[p], q)
    return float(np.vdot(v, w.v).real)


def expec_dm(rho, n, term) -> float:
    # P rho: the Paulis act on the row qubits of the column-major flat matrix
    w = O.StateVector(2 * n, np.asarray(rho).reshape(-1, order="F"))
    for q, p in enumerate(term):
        if p != "I":
            w.apply(PAULI[p], q)
    return float(np.trace(w.v.reshape(1 << n, 1 << n, order="F")).real)


def random_strings(rng, n, count, weight=None):
    """Strings over IXYZ; weight: probability of a non-identity letter per
    qubit (None: every letter uniform over IXYZ)."""
    out = []
    for _ in range(count):
        if weight is None:
            out.append("".join("IXYZ"[k] for k in rng.integers(0, 4, size=n)))
        else:
            out.append("".join("XYZ"[rng.integers(3)] if rng.random() < weight else "I" for _ in range(n)))
    return out


def case_list(n, rng):
    """Every case class of the issue for an n-qubit register."""
    def single(q, p):
        return "I" * q + p + "I" * (n - 1 - q)

    cases = ["I" * n]
    for q in sorted({0, n // 2, n - 1}):
        cases += [single(q, p) for p in "XYZ"]
    cases += ["X" * n, "Y" * n, "Z" * n]
    if n > 1:   # the other parity of the number of Y's
        cases.append("Y" * (n - 1) + "I")
    return cases + random_strings(rng, n, 40)


def ising_chain(n):
    """Open-chain transverse-field Ising terms: n - 1 ZZ, then n X."""
    terms = [{q: "Z", q + 1: "Z"} for q in range(n - 1)] + [{q: "X"} for q in range(n)]
    return terms, [-1.0] * (n - 1) + [-0.5] * n


def as_string(term, n):
    if isinstance(term, dict):
        s = ["I"] * n
        for q, p in term.items():
            s[q] = p
        return "".join(s)
    return term + "I" * (n - len(term))


def batches_bound(terms, n, tile_qubits, low_qubits, max_terms):
    """Passes the documented grouping (quest_amd.h) makes for terms on the
    identity layout of one rank: first fit in term order, X / Y terms first."""
    if n < tile_qubits:
        return -(-len(terms) // max_terms)
    cap = tile_qubits - low_qubits
    strs = [as_string(t, n) for t in terms]
    his = [frozenset(q for q, p in enumerate(s) if p in "XY" and q >= low_qubits) for s in strs]
    hasx = [any(p in "XY" for p in s) for s in strs]
    batches = []   # [set of positions, count]
    for phase in (True, False):
        for hi, hx in zip(his, hasx):
            if hx != phase:
                continue
            for b in batches:
                if b[1] < max_terms and len(b[0] | hi) <= cap:
                    b[0] |= hi
                    b[1] += 1
                    break
            else:
                batches.append([set(hi), 1])
    return len(batches)


# A register after eight random layers (the wave engine leaves its qubits on
# other positions), in a process of its own: the backend and planner are chosen
# at start-up.
AFTER_GATES = r'''
import sys
import numpy as np
import quest_amd as qa
from quest_amd.models import random_layered
from quest_amd.ops import capi
sys.path.insert(0, sys.argv[1])
from pauli_cases import expec_sv, random_strings
n, tol = int(sys.argv[2]), float(sys.argv[3])
env = qa.Env()
reg = qa.Register(env, n)
reg.init_plus()
random_layered(n, 8, seed=21).apply(reg)
reg.flush()
lay = capi.getQubitLayout(reg.q)
assert lay != list(range(n)), lay   # a permuted layout, or the test checks nothing
norm = reg.total_prob()
rng = np.random.default_rng(9)
terms = random_strings(rng, n, 18, weight=0.3) + ["X" * n, "Y" * (n - 1) + "Z"]
got = reg.expec_pauli_terms(terms)
assert capi.getQubitLayout(reg.q) == lay          # no relayout, no canonicalisation
capi.resetQuESTStats()
assert reg.total_prob() == norm
assert capi.getQuESTStats()["reductions"] == 0    # the norm cache survived: stateGen untouched
again = reg.expec_pauli_terms(terms)
assert again.tolist() == got.tolist()
copy = qa.Register(env, n)
copy.clone_from(reg)
v = copy.to_numpy()                                # canonicalises the copy only
assert capi.getQubitLayout(reg.q) == lay
want = np.array([expec_sv(v, n, t) for t in terms])
err = float(np.max(np.abs(got - want)))
print("max error", err)
assert err < tol, list(zip(terms, got, want))
print("pauli after gates ok")
'''


def run_after_gates(backend, n, tol, extra=None, timeout=300):
    e = dict(os.environ, QUEST_BACKEND=backend, **(extra or {}))
    if backend == "cpu":
        e["QUEST_CPU_PLANNER"] = "3"
    out = subprocess.run([sys.executable, "-c", AFTER_GATES, HERE, str(n), repr(tol)], cwd=ROOT, env=e,
                         capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "pauli after gates ok" in out.stdout
