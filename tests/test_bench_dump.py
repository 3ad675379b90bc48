"""bench.py --dump-outputs on the host build: one float64 file of (re, im)
columns per seed, the same from run to run; a state above the budget is
written as the documented sample of 4096-amplitude blocks, whose rows equal
those of the whole state."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bench(outdir, *args):
    env = dict(os.environ, QUEST_BACKEND="cpu", OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "QUEST_BOOTSTRAP_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "1", "--warmup", "0", "--dump-outputs", str(outdir), *args]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["steps"] == 1 and d["ms_per_step"] > 0
    return {f: np.load(os.path.join(outdir, f)) for f in sorted(os.listdir(outdir))}


def test_dump_outputs_whole_state_same_from_run_to_run(tmp_path):
    a = _bench(tmp_path / "a", "--qubits", "14")
    b = _bench(tmp_path / "b", "--qubits", "14")
    assert sorted(a) == [f"state_seed{s}.npy" for s in sorted((7, 11, 12, 13, 17), key=str)]
    for f, x in a.items():
        assert x.dtype == np.float64 and x.shape == (1 << 14, 2), (f, x.dtype, x.shape)
        assert abs(float((x ** 2).sum()) - 1) < 1e-12
        assert np.array_equal(x, b[f]), f
    assert not np.array_equal(a["state_seed7.npy"], a["state_seed11.npy"])


def test_dump_outputs_sample_of_a_large_state(tmp_path):
    import bench

    n, seeds = 18, list(range(7, 20))   # 13 states of 2^18 amplitudes: 52 MiB, above the budget
    got = _bench(tmp_path / "s", "--qubits", str(n), "--seeds", ",".join(map(str, seeds)))
    whole = _bench(tmp_path / "w", "--qubits", str(n), "--seed", "7")["state_seed7.npy"]
    assert whole.shape == (1 << n, 2)
    blocks = bench.DUMP_BUDGET_BYTES // 16 // len(seeds) // bench.DUMP_BLOCK
    assert 0 < blocks < (1 << n) // bench.DUMP_BLOCK
    picks = np.sort(np.random.default_rng(bench.DUMP_RNG_SEED).choice((1 << n) // bench.DUMP_BLOCK, size=blocks,
                                                                     replace=False))
    rows = np.concatenate([np.arange(p * bench.DUMP_BLOCK, (p + 1) * bench.DUMP_BLOCK) for p in picks])
    assert len(got) == len(seeds)
    for f, x in got.items():
        assert x.dtype == np.float64 and x.shape == (blocks * bench.DUMP_BLOCK, 2), (f, x.shape)
    assert sum(x.nbytes for x in got.values()) <= bench.DUMP_BUDGET_BYTES
    assert np.array_equal(got["state_seed7.npy"], whole[rows])
