"""glim_amd/csrc/ct_se3.hpp on the host, and glim_amd/se3.py, against the multiprecision table tests/golden/se3_range.npz (the reference
tests/se3_reference.py at 200 bits, rounded once) over the whole range of rotation angles: 0, 1e-300, 1e-9, 1e-4, both sides of the series
switch 0.02, 0.1, 1, 2, 3, pi - 1e-3 ... pi - 1e-12, the double nearest pi and the exact half turns, about nine axes, with translational
parts 0, 0.5 m and 3.6 km.  The device runs the same table in tests/test_se3_range_gpu.py.

Gates (tests/golden/make_golden_se3.py prints them; none is taken from the header): per output block and case class, 8 x the largest error
of the reference's own formulas in correctly rounded double arithmetic against its 200-bit run, never less than 8 eps max|expected block|.
As generated, over all classes: rotation blocks (R, Jw, Ad's R) 1.8e-15 ... 6.3e-15; omega 3.6e-17 (theta < 0.02) ... 5.6e-15; translation
blocks and the Jacobians' lower-left blocks 3.6e-16 ... 4.8e-15 at 0.5 m and 2e-12 ... 2e-11 at 3.6 km; the between term, whose poses lie
1.4 km out: r_v 1.3e-12 ... 1.5e-11, its Jacobians' lower-left blocks 6.5e-13 ... 2.1e-11; the bucket poses' T_t 2.4e-14 ... 6.4e-12.  The zero
blocks of the 6 x 6 matrices have gate 0: they are zero.  A case's gate is its class's, or 8 eps of its own block where that is larger.

What the header as it stood before this table missed, on the host (the driver of this module built over the old header): in log, prior and
between alike every exact half turn (omega = 0 returned, off by pi) and every case from pi - 1e-3 on that is not about a coordinate axis (up to
3e-7 in the band to pi - 1e-9, 3 to 5 beyond, against 5.6e-15), while theta <= 3 passed; below 0.02 the log factor lacked 31 theta^6 / 15120
(2.6e-15 against 3.6e-17); and in jr, jr_inv, the terms' Jacobians and the bucket poses' D0 / D1 the lower-left block at 0.02 <= theta <= 0.1,
whose closed-form coefficients cancel (4.4e-14 at 0.5 m and 3.3e-10 at 3.6 km just above 0.02, against 6.8e-16 and 4.9e-12)."""
import os
import subprocess

import numpy as np
import pytest

import se3_range_cases as sc
from align_cases import build_driver

SAMPLE = 37  # every SAMPLE-th case of an operation, and its last, are recomputed with mpmath


@pytest.fixture(scope="module")
def tab():
    return sc.load()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory, "se3_range")


def run_driver(driver, tmp_path, op, x):
    fin, fout = str(tmp_path / (op + ".in")), str(tmp_path / (op + ".out"))
    np.ascontiguousarray(x, dtype=np.float64).tofile(fin)
    subprocess.check_call([driver, op, fin, fout], stdout=subprocess.DEVNULL)
    return np.fromfile(fout, dtype=np.float64).reshape(len(x), sc.OP[op][2])


def test_the_table_covers_what_it_says(tab):
    for _, op, n_in, n_out, blocks, names in sc.OPS:
        n = len(tab[op + "_in"])
        assert tab[op + "_in"].shape == (n, n_in) and tab[op + "_out"].shape == (n, n_out) and tab[op + "_gate"].shape == (n, len(blocks)), op
        assert sorted(i for b in blocks for i in b) == list(range(n_out)), op  # the blocks cover every output once
        assert np.isfinite(tab[op + "_out"]).all() and (tab[op + "_gate"] >= 0).all(), op
        assert n >= {"prior": 147, "between": 147, "ct": 324}.get(op, 432), op
    assert os.path.getsize(sc.TABLE) < 700 * 1024
    for op in ("log", "prior", "between"):  # the three hand-made half turns are there, and their sign is open
        assert len(tab[op + "_alt_rows"]) >= 3 and set(range(len(tab[op + "_in"]) - 3, len(tab[op + "_in"]))) <= set(tab[op + "_alt_rows"].tolist()), op
    for op in ("exp", "jr", "jr_inv", "ad", "ct"):
        assert len(tab[op + "_alt_rows"]) == 0, op


@pytest.mark.parametrize("op", [o[1] for o in sc.OPS])
def test_the_table_is_what_its_generator_writes(tab, op):
    """every input, and a fixed sample of the expected outputs recomputed with mpmath at 200 bits: equal bytes"""
    pytest.importorskip("mpmath")
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(sc.TABLE)))
    import make_golden_se3 as gen

    cases = gen.cases(op)
    X = np.array([c[0] for c in cases], dtype=np.float64)
    assert X.tobytes() == tab[op + "_in"].tobytes()
    assert [c[1] for c in cases] == tab[op + "_band"].tolist() and [c[2] for c in cases] == tab[op + "_tclass"].tolist()
    alt = {int(r): k for k, r in enumerate(tab[op + "_alt_rows"])}
    for r in sorted(set(range(0, len(X), SAMPLE)) | {len(X) - 1}):
        out, other = gen.expected(op, list(X[r]))
        assert np.array(out).tobytes() == tab[op + "_out"][r].tobytes(), (op, r)
        assert (other is not None) == (r in alt), (op, r)
        if other is not None:
            assert np.array(other).tobytes() == tab[op + "_alt_out"][alt[r]].tobytes(), (op, r)


@pytest.mark.parametrize("op", [o[1] for o in sc.OPS])
def test_the_header_meets_the_table_on_the_host(tab, driver, tmp_path, op):
    got = run_driver(driver, tmp_path, op, tab[op + "_in"])
    failed, ratio, err = sc.compare(op, tab, got)
    print(f"{op}: worst error / gate per block " + " ".join(f"{n}={r:.2g}" for n, r in zip(sc.OP[op][4], np.nanmax(ratio, axis=0))))
    assert len(failed) == 0, f"{len(failed)} cases\n" + sc.describe(op, tab, failed, ratio, err)


def test_a_half_turn_has_a_residual_of_pi(tab, driver, tmp_path):
    """the three hand-made half turns, as log, prior and between see them: |omega| = pi, whichever sign (the bug this table was made for
    returned omega = 0, a residual and a gradient of zero)"""
    for op in ("log", "prior", "between"):
        rows = [-9, -6, -3] if op == "log" else [-3, -2, -1]  # about x, y, z
        got = run_driver(driver, tmp_path, op, tab[op + "_in"][rows])
        assert np.abs(np.linalg.norm(got[:, :3], axis=1) - np.pi).max() <= tab[op + "_gate"][rows, 0].max(), op
        assert np.array_equal(np.abs(got[:, :3]) > 1.0, np.eye(3, dtype=bool)), op


def test_the_python_maps_meet_the_table(tab):
    """glim_amd.se3.se3_exp / se3_log, the host-side product code the callers build poses and residuals with"""
    from glim_amd import se3

    got = np.array([se3.se3_exp(x)[:3].reshape(12) for x in tab["exp_in"]])
    failed, ratio, err = sc.compare("exp", tab, got)
    assert len(failed) == 0, sc.describe("exp", tab, failed, ratio, err)
    got = np.array([se3.se3_log(np.vstack([x.reshape(3, 4), [0, 0, 0, 1]])) for x in tab["log_in"]])
    failed, ratio, err = sc.compare("log", tab, got)
    assert len(failed) == 0, sc.describe("log", tab, failed, ratio, err)
