"""Pauli expectation values on the GPU: the batched tile kernel (several
tiles, several workgroups' partials, X / Y above the tile), the generic kernel
(chunks smaller than a tile, strings too wide for one), the density kernel,
the fp32 library, a permuted layout and two ranks sharing the GPU -- against
the NumPy oracle of pauli_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def genv():
    import quest_amd as qa

    e = qa.Env()
    assert qa.capi.getQuESTBackend() == "HIP", "HIP library not loaded on a GPU test run"
    return e


def _check_cases(genv, n, seed):
    import quest_amd as qa
    from helpers import load_state
    from pauli_cases import TOL, case_list, expec_sv
    from quest_amd.utils import oracle as O

    rng = np.random.default_rng(seed)
    reg = qa.Register(genv, n)
    v = O.random_state(rng, n)
    load_state(reg, v)
    cases = case_list(n, rng)
    got = reg.expec_pauli_terms(cases)
    want = np.array([expec_sv(v, n, c) for c in cases])
    err = float(np.max(np.abs(got - want)))
    print(f"n={n}: max error {err:.3e} over {len(cases)} strings")
    assert err < TOL[2], list(zip(cases, got, want))
    return reg, v, cases, got


def test_sixteen_qubits(genv):
    """16 tiles of 2^12: the case list (single X on qubit 15 sits above the
    tile's padding, all-X / all-Y take the generic kernel), a 48-term sum, and
    bit-identical repetition."""
    from pauli_cases import TOL, expec_sv, random_strings
    from quest_amd.ops import capi

    n = 16
    reg, v, cases, got = _check_cases(genv, n, 316)
    assert reg.expec_pauli_terms(cases).tolist() == got.tolist()
    assert reg.expec_pauli("X" * n) == reg.expec_pauli("X" * n)
    rng = np.random.default_rng(48)
    terms = random_strings(rng, n, 48, weight=0.25)
    coeffs = rng.normal(size=48)
    free0 = _free_bytes()
    total = reg.expec_pauli_sum(terms, coeffs)
    assert total == reg.expec_pauli_sum(terms, coeffs)
    assert _free_bytes() == free0   # no second register, no workspace
    want = float(coeffs @ np.array([expec_sv(v, n, t) for t in terms]))
    print(f"48-term sum: {total!r} vs {want!r}")
    assert abs(total - want) < TOL[2] * 48
    assert capi.calcExpecPauliProd(reg.q, [15, 0], [2, 3]) == reg.expec_pauli({0: "Z", 15: "Y"})
    reg.close()


def _free_bytes():
    import torch

    return torch.cuda.mem_get_info()[0]


@pytest.mark.parametrize("n", [3, 8])
def test_smaller_than_a_tile(genv, n):
    reg = _check_cases(genv, n, 300 + n)[0]
    reg.close()


def test_batching_is_real(genv):
    import quest_amd as qa
    from helpers import load_state
    from pauli_cases import TOL, as_string, batches_bound, expec_sv, ising_chain
    from quest_amd.ops import capi
    from quest_amd.utils import oracle as O

    n = 16
    rng = np.random.default_rng(31)
    reg = qa.Register(genv, n)
    v = O.random_state(rng, n)
    load_state(reg, v)
    terms, coeffs = ising_chain(n)
    assert len(terms) == 31
    capi.resetQuESTStats()
    got = reg.expec_pauli_sum(terms, coeffs)
    st = capi.getQuESTStats()
    bound = batches_bound(terms, n, capi.PAULI_TILE_QUBITS, capi.PAULI_TILE_LOW_QUBITS, capi.PAULI_MAX_TERMS_PER_PASS)
    print(f"ising16: pauliPasses {st['pauliPasses']} (bound {bound}), pauliTerms {st['pauliTerms']}")
    assert bound < 31
    assert st["pauliTerms"] == 31 and 1 <= st["pauliPasses"] <= bound and st["reductions"] == st["pauliPasses"], st
    want = float(np.dot(coeffs, [expec_sv(v, n, as_string(t, n)) for t in terms]))
    assert abs(got - want) < TOL[2] * 31, (got, want)
    reg.close()


def test_permuted_layout():
    """n = 20 after eight layers on the wave engine: the qubits sit on other
    positions, the masks go through the layout, nothing is canonicalised."""
    from pauli_cases import run_after_gates

    run_after_gates("hip", 20, 1e-11, timeout=200)


FP32 = r'''
import sys
import numpy as np
import quest_amd as qa
sys.path.insert(0, sys.argv[1])
from helpers import load_state
from pauli_cases import TOL, case_list, expec_sv
from quest_amd.ops import capi
from quest_amd.utils import oracle as O
assert capi.getQuESTBackend() == "HIP" and capi.binding().prec == 1
env = qa.Env()
n = 16
rng = np.random.default_rng(132)
reg = qa.Register(env, n)
v = O.random_state(rng, n)
load_state(reg, v)
cases = case_list(n, rng)
got = reg.expec_pauli_terms(cases)
v32 = v.astype(np.complex64).astype(complex)
want = np.array([expec_sv(v32, n, c) for c in cases])
err = float(np.max(np.abs(got - want)))
print("fp32 max error", err)
assert err < TOL[1], list(zip(cases, got, want))
assert reg.expec_pauli_terms(cases).tolist() == got.tolist()
print("pauli fp32 ok")
'''


def test_fp32_library():
    e = dict(os.environ, QUEST_BACKEND="hip", QUEST_PREC="1")
    out = subprocess.run([sys.executable, "-c", FP32, HERE], cwd=ROOT, env=e, capture_output=True, text=True,
                         timeout=200)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "pauli fp32 ok" in out.stdout


def test_density(genv):
    import quest_amd as qa
    from helpers import oracle_for
    from pauli_cases import TOL, expec_dm, random_strings
    from quest_amd.utils import oracle as O

    n = 7
    rng = np.random.default_rng(77)
    reg = qa.Register(genv, n, density=True)
    o = oracle_for(reg, rng)
    reg.h(2)
    o.apply(O.H, 2)
    reg.damping(6, 0.2)
    o.damping(6, 0.2)
    terms = random_strings(rng, n, 20)
    got = reg.expec_pauli_terms(terms)
    want = np.array([expec_dm(o.rho, n, t) for t in terms])
    err = float(np.max(np.abs(got - want)))
    print(f"density n=7: max error {err:.3e}")
    assert err < TOL[2], list(zip(terms, got, want))
    reg.close()


def test_two_ranks_on_one_gpu(genv, tmp_path):
    """QUEST_COMM=ipc, n = 16: X on the top (rank) qubit swaps it in once, Z
    there is a per-rank sign; values equal the single-rank ones."""
    from pauli_worker import compute
    from quest_amd.parallel import spawn_local

    want = compute(genv, 16)
    out = str(tmp_path / "pauli_ipc.npz")
    res = spawn_local([os.path.join(HERE, "pauli_worker.py"), out], 2,
                      env_extra={"QUEST_BACKEND": "hip", "PYTHONPATH": ROOT, "QUEST_COMM": "ipc",
                                 "QUEST_COMM_TIMEOUT": "120", "PAULI_WORKER_QUBITS": "16"}, timeout=200)
    for r, p in enumerate(res):
        assert p.returncode == 0, f"rank {r}:\n{p.stdout[-1500:]}\n{p.stderr[-2500:]}"
    with np.load(out) as z:
        got = {k: z[k] for k in z.files}
    assert int(got["_ranks"]) == 2 and "IPC" in str(got["_transport"])
    for k in ("z_only", "x_top", "sv", "sv_sum", "sv_relabel", "dm"):
        np.testing.assert_allclose(got[k], want[k], rtol=0, atol=1e-11, err_msg=k)
    assert int(got["z_swaps"]) == 0 and int(got["x_swaps"]) >= 1, (got["z_swaps"], got["x_swaps"])
