"""A residual rotation of half a turn, where a caller sees it: terms-only problems through glim_amd_bundle_align (N = 2) and
glim_amd_graph_align (N = 33), tests/se3_range_cases.py's chain_scene and huber_scene.  Pose 0 starts an exact half turn about z from its
prior, or pi - 1e-9 about (1, -2, 3); the expected first cost r^T L r and the s of the Huber between are tests/se3_reference.py's at 200 bits,
kept in tests/golden/se3_range.npz with gates propagated from the terms' (make_golden_se3.py::e2e).  With se3_log as it stood, the half turn's
rotational residual was 0: the first cost lacked 2 x 1e2 x pi^2, the pose never moved, and the Huber between counted as an inlier."""
import numpy as np
import pytest

import se3_range_cases as sc
from align_cases import ctx  # noqa: F401 (a fixture)
from test_gicp import POSE_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tab():
    return sc.load()


@pytest.mark.parametrize("start", [0, 1], ids=["half_turn_z", "near_pi_skew"])
@pytest.mark.parametrize("which,N", [("bundle", 2), ("graph", 33)])
def test_a_pose_half_a_turn_from_its_prior_pays_for_it_and_comes_home(ctx, tab, which, N, start):
    from glim_amd import api

    priors, betweens, X0 = sc.chain_scene(N, tab["e2e_start"][start])
    res, rows, _ = getattr(api, which + "_align_debug_trace")([], priors, betweens, X0, ctx=ctx)
    want, gate = tab["e2e_cost"][start], tab["e2e_cost_gate"][start]
    print(which, N, sc.E2E_STARTS[start], res.status_name, res.iterations, res.trials, "first cost", rows[0]["cost"], "off by", rows[0]["cost"] - want, "gate", gate,
          "pose 0 ends off by", np.abs(res.poses[0] - priors[0][1]).max())
    assert want > 2 * sc.E2E_PRECISION * 9.8  # the prior and the first between each see (nearly) pi
    assert abs(rows[0]["cost"] - want) <= gate
    assert np.abs(res.poses[0] - priors[0][1]).max() <= POSE_TOL
    assert res.cost <= 1e-12 * want


@pytest.mark.parametrize("which", ["bundle", "graph"])
def test_a_huber_between_half_a_turn_off_is_down_weighted_by_k_over_s(ctx, tab, which):
    from glim_amd import api

    priors, betweens, dampings, X0 = sc.huber_scene(tab["e2e_start"][0])
    res, rows, _ = getattr(api, which + "_align_debug_trace")([], priors, betweens, X0, ctx=ctx, dampings=dampings)
    s, s_gate = tab["e2e_huber_s"]
    k = sc.E2E_WIDTH
    print(which, "weight", res.between_weights[0], "k / s", k / s, "first cost", rows[0]["cost"], "k (2 s - k)", k * (2 * s - k))
    assert s > 10 * 3.14 and np.abs(res.poses - np.stack(X0)).max() < 1e-20  # the dampings held the poses: the kept evaluation is the first
    assert abs(rows[0]["cost"] - k * (2 * s - k)) <= 2 * k * s_gate + 8 * sc.EPS * k * 2 * s  # the prior's term is zero
    assert abs(res.between_weights[0] - k / s) <= k / s**2 * s_gate + 8 * sc.EPS * k / s
