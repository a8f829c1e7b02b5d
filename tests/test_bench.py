"""bench.py's plain run and --dump-outputs: the helpers that write the outputs (CPU), and one plain run on the device."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_write_outputs_keeps_small_arrays_whole(tmp_path):
    rng = np.random.default_rng(1)
    arrays = {"a": rng.random((7, 3)), "b": rng.random(11).astype(np.float32)}
    bench.write_outputs(str(tmp_path), arrays)
    for name, a in arrays.items():
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float64 and got.shape == a.shape
        assert np.array_equal(got, a.astype(np.float64))


def test_write_outputs_samples_the_same_entries_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 8 * 3000)
    rng = np.random.default_rng(2)
    arrays = {"x": rng.random(10000), "y": rng.random((500, 4))}
    for d in ("one", "two"):
        bench.write_outputs(str(tmp_path / d), arrays, rank=1, world=2)
    total = 0
    for name, a in arrays.items():
        one = np.load(tmp_path / "one" / f"{name}_rank1.npy")
        two = np.load(tmp_path / "two" / f"{name}_rank1.npy")
        assert np.array_equal(one, two) and one.dtype == np.float64
        assert np.isin(one, a.reshape(-1)).all()          # entries of the array, not something computed from them
        total += one.nbytes
    assert total <= bench.DUMP_BYTES / 2                  # this rank's share of the budget


def test_csr_values_are_in_row_column_order_and_leave_the_matrix_alone():
    rp = np.array([0, 2, 3], np.int32)
    ci = np.array([1, 0, 1], np.int32)
    M = sp.csr_matrix((np.array([1.0, 2.0, 3.0]), ci, rp), shape=(2, 2))
    assert np.array_equal(bench.csr_values(M), [2.0, 1.0, 3.0])
    assert np.array_equal(M.indices, [1, 0, 1]) and np.array_equal(M.data, [1.0, 2.0, 3.0])


@pytest.mark.gpu
def test_plain_run_times_the_steps_asked_for_and_dumps_the_last_state(tmp_path):
    """`bench.py --steps N --warmup W`: one window of exactly N steps, the headline keys, none of the --full legs; the
    outputs of the last step as float64 .npy files within 64 MB."""
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 6 and line["warmup"] == 2 and line["value"] > 0 and line["ms_per_step"] > 0
    assert len(line["timing"]["repeats_ms_per_step"]) == 1
    for k in ("roofline", "kernels_us_per_step", "with_solves", "cpu_baseline", "config3_leg", "dg_variant", "spike_window"):
        assert k not in line, k
    files = sorted(os.listdir(out))
    for name in ("A_emi", "P_emi", "A_knp", "b_emi", "b_knp", "phi_0", "phi_1", "phi_M_1", "ode_states_0"):
        assert f"{name}.npy" in files, files
    size = 0
    for f in files:
        a = np.load(out / f)
        assert a.dtype == np.float64 and a.size > 0 and np.isfinite(a).all(), f
        size += os.path.getsize(out / f)
    assert size <= 64e6
