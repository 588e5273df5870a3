"""tools/knn_pair_model.py is the CPU model of the retired pair-lane kNN kernel (two lanes per query, two lists merged at the end).  Pinned here, on
the CPU: the model answers exactly like the oracle, and so does its step-by-step emulation of the per-lane threshold selection -- on the distributions
the GPU tests use for the kNN kernels (ties everywhere, duplicates, far offset, fewer points than a chunk)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _cases():
    rng = np.random.default_rng(5)
    return {
        "lattice": np.stack(np.meshgrid(np.arange(14), np.arange(14), np.arange(10), indexing="ij"), -1).reshape(-1, 3) * 0.25,
        "identical": np.tile([[1.0, 2.0, 3.0]], (700, 1)),
        "offset": rng.uniform(-1, 1, (2500, 3)) + [1e5, -2e5, 3e4],
        "two_scales": np.vstack([rng.normal(size=(1500, 3)) * 0.01, rng.uniform(-50, 50, (1200, 3))]),
        "few": rng.uniform(-1, 1, (70, 3)),
        "duplicates": np.repeat(rng.uniform(-1, 1, (300, 3)), 9, axis=0),
    }


@pytest.mark.parametrize("name", ["lattice", "offset", "few", "duplicates"])
def test_pair_lane_model_and_staged_selection_are_exact(orc, name):
    """Two lists per query over disjoint candidates, each lane selecting over its OWN list, merged at the end."""
    import knn_pair_model as pm

    pts = _cases()[name].astype(np.float32)
    ref = orc.knn(pts.astype(np.float64), pm.K, method="brute")
    rounds0, out0 = pm.run(pts)
    np.testing.assert_array_equal(out0, ref)
    rounds1, out1 = pm.run(pts, select=(8, 0))
    np.testing.assert_array_equal(out1, ref)
    assert rounds1.sum() <= rounds0.sum()
