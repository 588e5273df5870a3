"""glim_amd/csrc/ct_se3.hpp on the device (glim_amd_debug_se3_eval: one thread per case, blocks of 64) against the multiprecision table
tests/golden/se3_range.npz, with the gates of tests/test_se3_range.py: the device's sin, cos, atan2 and sqrt and its FMA contraction are not
the host's, so the device gets its own check of the same cases.  The table needs no mpmath here.

The header's worst error / gate per operation, host | device (one MI355X run), is MEASURED below -- a record, not a bound; every run prints
its own.  The gates themselves are quoted in tests/test_se3_range.py."""
import numpy as np
import pytest

import se3_range_cases as sc
from align_cases import ctx  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu
INVALID = -1
# worst error / gate over all cases and blocks: host (g++ -O2 -ffp-contract=off) | device (one MI355X run)
MEASURED = {"exp": (0.63, 0.63), "log": (0.60, 0.64), "jr": (0.62, 0.62), "jr_inv": (0.76, 0.62), "ad": (0.12, 0.12), "prior": (0.65, 0.86),
            "between": (0.74, 0.75), "ct": (0.72, 0.72)}
# with se3_log's axis from R - R^T up to sin(theta) = 0.14 instead of 0.3 the device missed at theta = 3 about (1, 1, 1): log v 1.2, prior r_omega
# 1.4 and J 1.5, between r_omega 1.3 (the host: 0.8 to 0.99); the absolute errors are in the header's comment


@pytest.fixture(scope="module")
def tab():
    return sc.load()


@pytest.mark.parametrize("op", [o[1] for o in sc.OPS])
def test_the_header_meets_the_table_on_the_device(ctx, tab, op):
    from glim_amd import api

    assert api.SE3_DEBUG_OPS[op] == sc.OP[op][:3]
    x = tab[op + "_in"]
    got = api.se3_debug_eval(op, x, ctx=ctx)
    failed, ratio, err = sc.compare(op, tab, got)
    print(f"{op}: worst error / gate per block " + " ".join(f"{n}={r:.2g}" for n, r in zip(sc.OP[op][4], np.nanmax(ratio, axis=0))))
    assert len(failed) == 0, f"{len(failed)} cases\n" + sc.describe(op, tab, failed, ratio, err)
    assert got.tobytes() == api.se3_debug_eval(op, x, ctx=ctx).tobytes()  # a second call: the same bytes
    for count in (1, 63, 64, 65):  # a lone thread, a ragged block, a full one, a second block of one thread: the full table's rows
        assert api.se3_debug_eval(op, x[:count], ctx=ctx).tobytes() == got[:count].tobytes(), count


def test_a_half_turn_has_a_residual_of_pi_on_the_device(ctx, tab):
    from glim_amd import api

    for op in ("log", "prior", "between"):
        rows = [-9, -6, -3] if op == "log" else [-3, -2, -1]  # about x, y, z
        got = api.se3_debug_eval(op, tab[op + "_in"][rows], ctx=ctx)
        assert np.abs(np.linalg.norm(got[:, :3], axis=1) - np.pi).max() <= tab[op + "_gate"][rows, 0].max(), op
        assert np.array_equal(np.abs(got[:, :3]) > 1.0, np.eye(3, dtype=bool)), op


def test_what_the_window_refuses(ctx, tab):
    from glim_amd import _lib

    f = _lib.lib().glim_amd_debug_se3_eval
    x, out = np.ascontiguousarray(tab["between_in"][:2]), np.full((2, 84), 7.0)
    dp = lambda a: _lib.C.cast(a.ctypes.data, _lib.C.POINTER(_lib.C.c_double))  # noqa: E731
    assert f(ctx._h, 0, -1, dp(x), dp(out)) == INVALID
    assert f(ctx._h, -1, 2, dp(x), dp(out)) == INVALID and f(ctx._h, 8, 2, dp(x), dp(out)) == INVALID
    assert f(None, 0, 2, dp(x), dp(out)) == INVALID and f(ctx._h, 0, 2, None, dp(out)) == INVALID and f(ctx._h, 0, 2, dp(x), None) == INVALID
    assert f(ctx._h, 6, 0, dp(x), dp(out)) == 0
    assert (out == 7.0).all()  # none of these wrote
