"""What tests/test_se3_range.py (host), tests/test_se3_range_gpu.py (device) and tests/golden/make_golden_se3.py share: the operations of
glim_amd/csrc/ct_se3.hpp the table tests/golden/se3_range.npz covers, their strides, the output blocks a gate belongs to, and the comparison
of a set of outputs with the table.  numpy only (the table exists so that a machine without mpmath can check).  A plain module: no tests."""
import os

import numpy as np

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "se3_range.npz")
EPS = 2.0**-52
BANDS = ("theta < 0.02", "0.02 <= theta <= 3", "pi - 1e-3 .. pi - 1e-9", "pi - 1e-12 .. pi")
T_CLASSES = ("t = 0", "|t| ~ 0.5", "|t| ~ 3.6e3")


def _m6(off, stride=6, col=0):
    """the four 3 x 3 blocks of a row-major 6 x 6 at `off` inside rows of `stride`: top-left, top-right, lower-left, lower-right"""
    at = lambda r0, c0: [off + stride * (r0 + r) + col + c0 + c for r in range(3) for c in range(3)]  # noqa: E731
    return [at(0, 0), at(0, 3), at(3, 0), at(3, 3)]


_POSE = [[4 * r + c for r in range(3) for c in range(3)], [3, 7, 11]]
_TAN = [[0, 1, 2], [3, 4, 5]]
_M6_NAMES = ["TL", "TR", "LL", "LR"]

# op code (glim_amd_debug_se3_eval), name, doubles in, doubles out, blocks (index lists into one output), block names
OPS = [
    (0, "exp", 6, 12, _POSE, ["R", "t"]),
    (1, "log", 12, 6, _TAN, ["omega", "v"]),
    (2, "jr", 6, 36, _m6(0), _M6_NAMES),
    (3, "jr_inv", 6, 36, _m6(0), _M6_NAMES),
    (4, "ad", 12, 36, _m6(0), _M6_NAMES),
    (5, "prior", 24, 42, _TAN + _m6(6), ["r_omega", "r_v"] + ["J_" + n for n in _M6_NAMES]),
    (6, "between", 36, 78, _TAN + _m6(6, 12, 0) + _m6(6, 12, 6), ["r_omega", "r_v"] + ["JX_" + n for n in _M6_NAMES] + ["JY_" + n for n in _M6_NAMES]),
    (7, "ct", 25, 84, _POSE + _m6(12) + _m6(48), ["T_R", "T_t"] + ["D0_" + n for n in _M6_NAMES] + ["D1_" + n for n in _M6_NAMES]),
]
OP = {name: (code, n_in, n_out, blocks, names) for code, name, n_in, n_out, blocks, names in OPS}


def load():
    return dict(np.load(TABLE))


def block_errors(op, got, want):
    """max |got - want| per case and block -> (cases, blocks); NaN where the output is not finite"""
    d = np.abs(np.asarray(got) - np.asarray(want))
    return np.stack([d[:, idx].max(axis=1) for idx in OP[op][3]], axis=1)


def compare(op, tab, got, rows=None):
    """`got` (cases x out) against the table's rows (all by default).  A case passes when every block is within its gate of the expected
    output; a case whose rotation's sign the data does not determine (<op>_alt_rows: the half turns) may instead meet the other logarithm's
    outputs (<op>_alt_out), all blocks of it.  -> (positions in `rows` that failed, error / gate per case and block, errors)"""
    n = len(tab[op + "_in"])
    rows = np.arange(n) if rows is None else np.asarray(rows)
    got = np.asarray(got, dtype=np.float64).reshape(len(rows), OP[op][2])
    gate = tab[op + "_gate"][rows]
    err = block_errors(op, got, tab[op + "_out"][rows])
    alt = np.full(n, -1)
    alt[tab[op + "_alt_rows"]] = np.arange(len(tab[op + "_alt_rows"]))
    for k, r in enumerate(rows):
        if alt[r] >= 0:
            e2 = block_errors(op, got[k:k + 1], tab[op + "_alt_out"][alt[r]:alt[r] + 1])[0]
            if not np.all(err[k] <= gate[k]) and np.all(e2 <= gate[k]):
                err[k] = e2
    ok = np.all(err <= gate, axis=1)  # NaN compares false
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / gate)
    return np.flatnonzero(~ok), ratio, err


def describe(op, tab, failed, ratio, err, rows=None):
    names = OP[op][4]
    out = []
    for k in failed[:12]:
        r = k if rows is None else rows[k]
        b = int(np.argmax(np.where(np.isnan(ratio[k]), np.inf, ratio[k])))
        out.append(f"{op} case {r} ({BANDS[tab[op + '_band'][r]]}; {T_CLASSES[tab[op + '_tclass'][r]]}): block {names[b]} off by {err[k, b]:.3g}, gate {tab[op + '_gate'][r, b]:.3g}")
    return "\n".join(out)


# ---- the end-to-end scenes (tests/test_se3_half_turn_gpu.py, tests/test_se3_half_turn.py): terms only, every entry of every pose a double whose
# products here are exact, so that what the loop's first evaluation sees is what the reference was given -----------------------------------------
E2E_PRECISION = 1e2
E2E_STEP = (0.5, 0.25, 0.0)
E2E_WIDTH = 1.0  # the Huber width of the scene with one between
E2E_STARTS = ("an exact half turn about z", "pi - 1e-9 about (1, -2, 3)")


def pose44(v12):
    return np.vstack([np.asarray(v12, dtype=np.float64).reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])


def chain_scene(N, start12):
    """a prior of precision 1e2 at the identity on pose 0, a chain of N - 1 betweens of the same precision along pure translations, every pose
    at its place but pose 0, which starts at `start12` (a row of the table's e2e_start) -> priors, betweens, X0"""
    poses = [np.eye(4) for _ in range(N)]
    for k in range(N):
        poses[k][:3, 3] = k * np.array(E2E_STEP)
    D = np.eye(4)
    D[:3, 3] = E2E_STEP
    L = E2E_PRECISION * np.eye(6)
    return [(0, poses[0], L)], [(k, k + 1, D.copy(), L) for k in range(N - 1)], [pose44(start12)] + poses[1:]


def huber_scene(start12):
    """two poses, a prior on pose 0 where it is, one between of width E2E_WIDTH whose residual is `start12`'s rotation, and a damping of 1e30
    on both poses: no step moves a pose by more than 1e-27, so the kept weights are the first evaluation's -> priors, betweens, dampings, X0"""
    priors, betweens, X0 = chain_scene(2, np.eye(4)[:3].reshape(12))
    X0[1] = X0[1] @ pose44(start12)
    return priors, [betweens[0] + (E2E_WIDTH,)], [(0, 1e30), (1, 1e30)], X0
