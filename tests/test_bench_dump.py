"""`bench.py --dump-outputs` on the host: file names, dtypes, the seeded sample of long arrays and the size limit."""

import os

import numpy as np

from conftest import ROOT


def _bench():
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_for_tests", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_long_arrays_are_cut_to_the_same_seeded_sample_and_everything_is_float64(tmp_path):
    bench = _bench()
    k = bench.DUMP_MAX_ELEMENTS
    rng = np.random.default_rng(5)
    n, m = k + 1000, 3 * k
    arrays = dict(dt=rng.random(7), pcg_iterations=np.arange(7, dtype=np.int32), probe_mu=None,
                  psi=rng.random(n) + 1j * rng.random(n), mu=rng.random(n), supercurrent=rng.random(m), normal_current=rng.random(m))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    a = {f[:-4]: np.load(os.path.join(tmp_path, "a", f)) for f in os.listdir(tmp_path / "a")}
    b = {f[:-4]: np.load(os.path.join(tmp_path, "b", f)) for f in os.listdir(tmp_path / "b")}
    assert set(a) == {"dt", "pcg_iterations", "psi_real", "psi_imag", "mu", "supercurrent", "normal_current",
                      f"sample_index_{n}", f"sample_index_{m}"}
    assert all(v.dtype == np.float64 for v in a.values()) and sum(v.nbytes for v in a.values()) <= bench.DUMP_MAX_BYTES
    assert all(np.array_equal(a[key], b[key]) for key in a)  # the same sample on every run
    assert np.array_equal(a["dt"], arrays["dt"]) and np.array_equal(a["pcg_iterations"], np.arange(7))
    idx = a[f"sample_index_{n}"].astype(np.int64)
    assert len(idx) == k and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(a["psi_real"], arrays["psi"].real[idx]) and np.array_equal(a["mu"], arrays["mu"][idx])
    idx = a[f"sample_index_{m}"].astype(np.int64)
    assert np.array_equal(a["normal_current"], arrays["normal_current"][idx])
