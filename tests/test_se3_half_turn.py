"""The prior of the scan-to-keyframes loop (glim_amd/csrc/keyframe_lm_step.hpp) half a turn from its pose, through the host driver of
tests/test_keyframe_align.py: the prior's contribution to round 0 -- r^T L r and J^T L r -- against tests/se3_reference.py at 200 bits
(tests/golden/se3_range.npz, e2e_prior_cost).  With se3_log as it stood, an exact half turn contributed a cost and a gradient of zero.  The
device's loops run the same starts in tests/test_se3_half_turn_gpu.py."""
import numpy as np
import pytest

import lm_restatement as lmr
import se3_range_cases as sc
from align_cases import build_driver
from test_keyframe_align import run_cpp_step


@pytest.fixture(scope="module")
def step_exe(tmp_path_factory):
    return build_driver(tmp_path_factory, "keyframe_lm_step", "-Wno-unknown-pragmas")


@pytest.mark.parametrize("start", [0, 1], ids=["half_turn_z", "near_pi_skew"])
def test_the_keyframe_prior_half_a_turn_away_has_its_cost_and_its_gradient(step_exe, tmp_path, start):
    tab = sc.load()
    X_init = sc.pose44(tab["e2e_start"][start])
    prior = (np.eye(4), sc.E2E_PRECISION * np.eye(6))
    rows = run_cpp_step(step_exe, tmp_path, lmr.params(), [np.eye(4)], X_init, [np.zeros(29)], prior)  # one target, an empty record: round 0's prior
    pc = rows[0]["prior"]
    want, gate = tab["e2e_prior_cost"][start], tab["e2e_prior_gate"][start]
    print(sc.E2E_STARTS[start], "prior cost", pc[27], "off by", pc[27] - want, "gate", gate, "J^T L r", pc[21:27])
    assert want > sc.E2E_PRECISION * 9.8 and abs(pc[27] - want) <= gate
    # J_r(r)^-T r = r for a pure rotation (r is the axis of its own Jacobian), so J^T L r = 1e2 r: of length 1e2 pi, none of it translational
    assert abs(np.linalg.norm(pc[21:24]) - sc.E2E_PRECISION * np.sqrt(want / sc.E2E_PRECISION)) <= 1e-9 and np.abs(pc[24:27]).max() <= 1e-9
