"""Generate `fields_reference_small.npz` by running the REFERENCE's own Biot-Savart loops (build container only).

    python tests/golden/generate_golden_fields.py [--out DIR]

imports py-tdgl v0.8.3 through `_reference_shim.py` and calls `tdgl.em._biot_savart_2d_vector` and
`tdgl.em._biot_savart_2d_z` (the Numba loops behind `Solution.field_at_position`; pint is mocked by the shim, but
these two functions do not touch it) on 500 random sources in the plane z = z0 and 64 targets above, below and beside
the sheet, some of them very close to it and some very far away.  The fixture is data only: inputs, the reference's
outputs (tesla per the reference's convention: they carry its `mu_0 / 4 pi`) and the reference's own `em.mu_0`, which
differs from this package's `MU_0` in the 10th digit -- tests compare the bare sums, output / (mu_0 / 4 pi).
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from _reference_shim import import_reference  # noqa: E402

tdgl = import_reference()
from tdgl import em  # noqa: E402

OUT_DIR = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE


def main():
    rng = np.random.default_rng(20240607)
    n, z0 = 500, 0.35
    src_xy = rng.uniform([-3.0, -2.0], [3.0, 2.0], size=(n, 2))
    areas = rng.uniform(0.5, 1.5, size=n) * (6.0 * 4.0 / n)
    K = rng.normal(size=(n, 2))
    targets = np.concatenate([
        # above and below the sheet at ordinary heights
        np.column_stack([rng.uniform(-3.5, 3.5, 16), rng.uniform(-2.5, 2.5, 16), z0 + rng.uniform(0.2, 2.0, 16)]),
        np.column_stack([rng.uniform(-3.5, 3.5, 16), rng.uniform(-2.5, 2.5, 16), z0 - rng.uniform(0.2, 2.0, 16)]),
        # beside the sheet: in its plane (dz = 0) and near it, outside the sources' rectangle
        np.column_stack([rng.uniform(3.2, 6.0, 8) * rng.choice([-1.0, 1.0], 8), rng.uniform(-4.0, 4.0, 8), z0 * np.ones(8)]),
        np.column_stack([rng.uniform(-6.0, 6.0, 8), rng.uniform(2.2, 5.0, 8) * rng.choice([-1.0, 1.0], 8),
                         z0 + rng.normal(scale=0.05, size=8)]),
        # very different heights: a hair above the sheet ... far away
        np.column_stack([rng.uniform(-2.5, 2.5, 16), rng.uniform(-1.5, 1.5, 16),
                         z0 + np.logspace(-4, 4, 16) * rng.choice([-1.0, 1.0], 16)]),
    ])
    positions = np.column_stack([src_xy, z0 * np.ones(n)])
    B_vector = em._biot_savart_2d_vector(targets, positions, K, areas)
    B_z = em._biot_savart_2d_z(targets, positions, K, areas)
    assert B_vector.shape == (len(targets), 3) and B_z.shape == (len(targets),)
    assert np.isfinite(B_vector).all() and np.isfinite(B_z).all()
    path = os.path.join(OUT_DIR, "fields_reference_small.npz")
    np.savez(path, src_xy=src_xy, areas=areas, z0=np.float64(z0), K=K, targets=targets, B_vector=B_vector, B_z=B_z,
             mu_0=np.float64(em.mu_0))
    print(path, os.path.getsize(path), "bytes; mu_0 =", repr(float(em.mu_0)))


if __name__ == "__main__":
    main()
