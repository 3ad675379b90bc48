"""Pauli expectation values (calcExpecPauliProd / Sum / Terms) on the host
build: every case class against the NumPy oracle (Pauli matrices applied to a
copy of the state, pauli_cases.py), the three API forms against each other,
a permuted layout under the wave planner's host emulation, density matrices,
validation, and 2 / 4 ranks over the socket transport."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import quest_amd as qa  # noqa: E402
from helpers import load_state, oracle_for  # noqa: E402
from pauli_cases import (TOL, as_string, case_list, expec_dm, expec_sv, ising_chain, random_strings,  # noqa: E402
                         run_after_gates)
from quest_amd.ops import capi  # noqa: E402
from quest_amd.utils import oracle as O  # noqa: E402

CODES = {"I": 0, "X": 1, "Y": 2, "Z": 3}


def _tol():
    return TOL[capi.binding().prec]


@pytest.mark.parametrize("n", [1, 3, 8, 16])
def test_case_classes(env, n):
    rng = np.random.default_rng(100 + n)
    reg = qa.Register(env, n)
    v = O.random_state(rng, n)
    load_state(reg, v)
    cases = case_list(n, rng)
    got = reg.expec_pauli_terms(cases)
    want = np.array([expec_sv(v, n, c) for c in cases])
    assert np.max(np.abs(got - want)) < _tol(), list(zip(cases, got, want))
    assert abs(got[0] - reg.total_prob()) < _tol()   # the identity string is the norm
    assert reg.expec_pauli_terms(cases).tolist() == got.tolist()   # bit-identical on repetition
    reg.close()


def test_api_forms_agree(env):
    n = 8
    rng = np.random.default_rng(5)
    reg = qa.Register(env, n)
    v = O.random_state(rng, n)
    load_state(reg, v)
    terms = random_strings(rng, n, 25) + ising_chain(n)[0]
    coeffs = rng.normal(size=len(terms))
    each = reg.expec_pauli_terms(terms)
    total = reg.expec_pauli_sum(terms, coeffs)
    want = np.array([expec_sv(v, n, as_string(t, n)) for t in terms])
    assert np.max(np.abs(each - want)) < _tol()
    assert abs(total - float(coeffs @ each)) < _tol()
    assert abs(total - float(coeffs @ want)) < _tol() * len(terms)
    # term by term through calcExpecPauliProd, targets in shuffled order, identities left out or kept
    for k, t in enumerate(terms):
        s = as_string(t, n)
        qs = [q for q in rng.permutation(n) if s[q] != "I" or rng.random() < 0.5] or [0]
        p = capi.calcExpecPauliProd(reg.q, qs, [CODES[s[q]] for q in qs])
        assert abs(p - each[k]) < _tol(), (s, qs, p, each[k])
    # string and dict forms of the same terms
    dicts = [{q: p for q, p in enumerate(as_string(t, n)) if p != "I"} for t in terms]
    assert np.array_equal(reg.expec_pauli_terms(dicts), each)
    assert reg.expec_pauli("XZ") == reg.expec_pauli({0: "X", 1: "Z"}) == reg.expec_pauli("XZ" + "I" * (n - 2))
    with pytest.raises(ValueError):
        reg.expec_pauli("XQ")
    with pytest.raises(ValueError):
        reg.expec_pauli({n: "X"})
    reg.close()


def test_reads_leave_caches_and_counters(env):
    """A read: no QASM, the norm cache stays valid, counters count."""
    n = 8
    reg = qa.Register(env, n)
    reg.init_plus()
    reg.ry(3, 0.3)
    reg.start_qasm()
    reg.total_prob()
    log = reg.qasm
    capi.resetQuESTStats()
    terms, coeffs = ising_chain(n)
    reg.expec_pauli_sum(terms, coeffs)
    st = capi.getQuESTStats()
    assert st["pauliTerms"] == len(terms) and 1 <= st["pauliPasses"] == st["reductions"], st
    capi.resetQuESTStats()
    reg.total_prob()
    assert capi.getQuESTStats()["reductions"] == 0   # still cached: the state generation did not move
    assert reg.qasm == log
    reg.close()


def test_after_gates_on_permuted_layout():
    run_after_gates("cpu", 20, 1e-11)


@pytest.mark.parametrize("n", [2, 6])
def test_density(env, n):
    rng = np.random.default_rng(40 + n)
    reg = qa.Register(env, n, density=True)
    o = oracle_for(reg, rng)
    for q in range(n):
        U = O.random_unitary(rng)
        reg.unitary(q, U)
        o.apply(U, q)
    reg.cnot(0, n - 1)
    o.apply(O.X, n - 1, [0])
    reg.damping(n - 1, 0.3)
    o.damping(n - 1, 0.3)
    cases = case_list(n, rng)
    got = reg.expec_pauli_terms(cases)
    want = np.array([expec_dm(o.rho, n, c) for c in cases])
    assert np.max(np.abs(got - want)) < _tol(), list(zip(cases, got, want))
    coeffs = rng.normal(size=len(cases))
    assert abs(reg.expec_pauli_sum(cases, coeffs) - float(coeffs @ want)) < _tol() * len(cases)
    # a pure-state density matrix gives the state-vector's values
    psi = qa.Register(env, n)
    v = O.random_state(rng, n)
    load_state(psi, v)
    reg.init_pure(psi)
    assert np.max(np.abs(reg.expec_pauli_terms(cases) - psi.expec_pauli_terms(cases))) < _tol()
    reg.close()
    psi.close()


def test_validation(env):
    n = 4
    reg, small, dens = qa.Register(env, n), qa.Register(env, n - 1), qa.Register(env, n, density=True)
    reg.init_plus()
    reg.ry(1, 0.4)
    before = reg.to_numpy()
    prod, total, terms = capi.calcExpecPauliProd, capi.calcExpecPauliSum, capi.calcExpecPauliTerms
    ident = [0] * n
    bad = [
        (33, lambda: prod(reg.q, [0, 1], [1, 4])),               # bad Pauli code
        (33, lambda: prod(reg.q, [0, 1], [-1, 1])),
        (33, lambda: total(reg.q, [0, 1, 2, 7], [1.0])),
        (33, lambda: terms(reg.q, [0, 1, 2, 3, 5, 0, 0, 0])),
        (9, lambda: prod(reg.q, [1, 2, 1], [1, 1, 1])),          # repeated target
        (2, lambda: prod(reg.q, [0, n], [1, 1])),                # target out of range
        (2, lambda: prod(reg.q, [-1], [1])),
        (34, lambda: prod(reg.q, [], [], 0)),                    # numTargets 0 and n + 1
        (34, lambda: prod(reg.q, list(range(n)) + [0], [1] * (n + 1))),
        (35, lambda: total(reg.q, ident, [1.0], 0)),             # numSumTerms 0
        (35, lambda: terms(reg.q, ident, 0)),
        (19, lambda: prod(reg.q, [0], [1], 1, small.q)),         # workspace of the wrong size
        (19, lambda: total(reg.q, ident, [1.0], 1, small.q)),
        (20, lambda: prod(reg.q, [0], [1], 1, dens.q)),          # workspace of the wrong type
        (20, lambda: total(reg.q, ident, [1.0], 1, dens.q)),
    ]
    for code, call in bad:
        with pytest.raises(capi.QuESTError) as e:
            call()
        assert e.value.code == code, (code, str(e.value))
    assert np.array_equal(reg.to_numpy(), before)
    # the register itself and another register of the same shape are valid workspaces
    other = qa.Register(env, n)
    a = prod(reg.q, [1], [1], 1, other.q)
    assert a == prod(reg.q, [1], [1]) and abs(a - np.vdot(before, _x_on(before, n, 1)).real) < _tol()
    for r in (reg, small, dens, other):
        r.close()


def _x_on(v, n, q):
    w = O.StateVector(n, v)
    w.apply(O.X, q)
    return w.v


@pytest.mark.parametrize("ranks", [2, 4])
def test_distributed(env, tmp_path, ranks):
    from pauli_worker import N_DM, N_SV, compute
    from quest_amd.parallel import spawn_local

    want = compute(env)
    out = str(tmp_path / f"pauli_{ranks}.npz")
    res = spawn_local([os.path.join(HERE, "pauli_worker.py"), out], ranks,
                      env_extra={"QUEST_BACKEND": "cpu", "PYTHONPATH": ROOT}, timeout=300)
    for r, p in enumerate(res):
        assert p.returncode == 0, f"rank {r}:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    with np.load(out) as z:
        got = {k: z[k] for k in z.files}
    assert int(got["_ranks"]) == ranks
    for k in ("z_only", "x_top", "sv", "sv_sum", "sv_norm", "sv_relabel", "state_after", "dm", "dm_state"):
        np.testing.assert_allclose(got[k], want[k], rtol=0, atol=1e-11, err_msg=k)
    assert int(got["z_swaps"]) == 0 and int(got["x_swaps"]) >= 1, (got["z_swaps"], got["x_swaps"])
    assert int(got["wide_code"]) == 36
    for r in range(1, ranks):   # the same values on every rank
        with np.load(f"{out}.rank{r}.npz") as z:
            for k in ("sv", "sv_relabel", "dm"):
                np.testing.assert_allclose(z[k], want[k], rtol=0, atol=1e-11, err_msg=f"rank {r} {k}")
    # and the single-process values are the oracle's
    from pauli_cases import as_string as _s
    from pauli_worker import sv_terms

    rng = np.random.default_rng(77)
    v = O.random_state(rng, N_SV)
    first = sv_terms(N_SV)
    ref = np.array([expec_sv(v, N_SV, _s(t, N_SV)) for t in first])
    assert np.max(np.abs(want["sv"][:len(first)] - ref)) < 1e-11
    assert N_DM == 5
