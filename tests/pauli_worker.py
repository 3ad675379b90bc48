"""Pauli expectation values whose results must not depend on the number of
ranks: ``python tests/pauli_worker.py <out.npz>`` runs compute() as one rank of
a multi-process job (rank 0 writes); the tests call compute() in process for
the single-rank values."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

N_SV, N_DM = 10, 5


def sv_terms(n):
    """The top qubit t is a rank qubit on 2 ranks, t and u = t - 1 on 4: Z on
    them, X / Y on them, mixtures."""
    t, u = n - 1, n - 2
    return [{t: "Z"}, {u: "Z", t: "Z"}, {0: "Z", t: "Z"}, {t: "X"}, {t: "Y"}, {u: "X", t: "X"},
            {u: "Y", t: "X", 0: "Z"}, {t: "X", u: "Z"}, {0: "X", t: "X"}, {3: "Y", t: "Y", u: "Z", 5: "X"},
            {u: "Y"}, "Z" * n, "XYZIIXYZ" + "I" * (n - 10) + "XY"]


DM_TERMS = [{4: "Z"}, {4: "X"}, {4: "Y", 3: "Z"}, {3: "X", 4: "X", 0: "Y"}, "XXXXX", "YZYZY", "IIIII", {0: "X"}]


def compute(env, n_sv=N_SV):
    import quest_amd as qa
    from helpers import apply_random_ops, load_state
    from pauli_cases import random_strings
    from quest_amd.ops import capi
    from quest_amd.utils import oracle as O
    from scenarios import NullOracle

    rng = np.random.default_rng(77)
    out = {}
    v = O.random_state(rng, n_sv)
    terms = sv_terms(n_sv) + [s for s in random_strings(rng, n_sv, 12, weight=0.4) if sum(c in "XY" for c in s) <= 6]
    coeffs = rng.normal(size=len(terms))
    r = qa.Register(env, n_sv)
    load_state(r, v)
    capi.resetQuESTStats()
    out["z_only"] = r.expec_pauli_terms(terms[:3])
    out["z_swaps"] = capi.getQuESTStats()["swaps"]
    out["x_top"] = r.expec_pauli({n_sv - 1: "X"})
    out["x_swaps"] = capi.getQuESTStats()["swaps"]
    out["sv"] = r.expec_pauli_terms(terms)
    out["sv_sum"] = r.expec_pauli_sum(terms, coeffs)
    out["sv_norm"] = r.total_prob()
    # pauliX on the top qubit: on several ranks the chunk placement is relabelled
    r2 = qa.Register(env, n_sv)
    load_state(r2, v)
    r2.x(n_sv - 1)
    out["sv_relabel"] = r2.expec_pauli_terms(terms)
    out["state_after"] = r2.to_numpy()
    if env.num_ranks > 1:   # X / Y on more qubits than a chunk holds
        try:
            r.expec_pauli("X" * n_sv)
            out["wide_code"] = 0
        except capi.QuESTError as e:
            out["wide_code"] = e.code
    d = qa.Register(env, N_DM, density=True)
    d.init_plus()
    apply_random_ops(d, NullOracle(), rng, 40, noise=True)
    dterms = DM_TERMS + random_strings(rng, N_DM, 8)
    out["dm"] = d.expec_pauli_terms(dterms)
    out["dm_state"] = d.to_numpy()
    for reg in (r, r2, d):
        reg.close()
    return out


def main():
    import quest_amd as qa

    env = qa.Env()
    res = compute(env, int(os.environ.get("PAULI_WORKER_QUBITS", N_SV)))
    res["_ranks"] = env.num_ranks
    res["_transport"] = qa.capi.getQuESTTransport()
    if env.rank == 0:
        np.savez(sys.argv[1], **{k: np.asarray(v) for k, v in res.items()})
    else:   # every rank holds the same values
        np.savez(f"{sys.argv[1]}.rank{env.rank}.npz", **{k: np.asarray(res[k]) for k in ("sv", "sv_relabel", "dm")})
    env.close()


if __name__ == "__main__":
    main()
