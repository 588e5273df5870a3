"""The catalogue of tests/covariance_cases.py on the CPU: the oracle (and, where oracle/_ref is built, the compiled reference) against the
multiprecision reference, the conditions that make each case a valid one, and the record tests/golden/covariance_cases.json of the oracle's
own error per case -- which the device test (tests/test_covariance_cases_gpu.py) builds its bounds from."""
import json
import os

import numpy as np
import pytest

import covariance_cases as cc


def oracle_on_case(orc, case, fmt, ref=False):
    """(normals, covs) of the group's members, each listing the whole group"""
    v = case.values(fmt)
    nb = np.tile(np.arange(len(v), dtype=np.int32), (len(v), 1))
    return orc.covariances(v, nb, k_neighbors=case.k_neighbors, ref=ref)


def measure(orc):
    out = {}
    for case in cc.CASES:
        out[case.name] = {}
        for fmt in cc.FORMATS:
            r = cc.case_reference(case, fmt)
            normals, _ = oracle_on_case(orc, case, fmt)
            m = {"kind": case.kind, "gap": r.gap}
            if case.kind in ("conditioned", "flip"):
                m["oracle_sine"] = max(cc.sine(n, r.vec_mp) for n in normals)
            out[case.name][fmt] = m
    return out


@pytest.fixture(scope="module")
def measured(orc):
    return measure(orc)


@pytest.mark.parametrize("fmt", cc.FORMATS)
@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.name)
def test_oracle_meets_the_multiprecision_reference_on_the_catalogue(orc, measured, case, fmt):
    r = cc.case_reference(case, fmt)
    v = case.values(fmt)
    normals, covs = oracle_on_case(orc, case, fmt)
    if orc.ref_lib() is not None:  # the compiled reference, where it is built: the restatement's values
        rn, rc = oracle_on_case(orc, case, fmt, ref=True)
        np.testing.assert_array_equal(rn, normals)
        np.testing.assert_array_equal(rc, covs)
    np.testing.assert_allclose(np.linalg.norm(normals, axis=1), 1.0, atol=1e-14)
    assert np.all(np.einsum("ni,ni->n", v, normals) <= 0.0)
    np.testing.assert_allclose(covs, np.eye(3)[None] - 0.999 * normals[:, :, None] * normals[:, None, :], atol=1e-12)
    m = measured[case.name][fmt]
    print(f"{case.name} [{fmt}]: eigenvalues {r.ev}, relative gap {r.gap:.3e}, oracle sine {m.get('oracle_sine')}")
    if case.kind in ("conditioned", "flip"):
        assert r.gap >= cc.MIN_GAP
        # the closed-form solver loses ~eps / gap, and the one-pass sums eps |p|^2 / spread^2; 1e-7 separates "meets the reference" from any
        # wrong answer (the nearest designed alternative, the other value format of the 200 m plane, is > 1e-5 away)
        assert m["oracle_sine"] < 1e-7
    elif case.kind == "exact":
        assert np.array_equal(v, case.points)  # dyadic: the FP32 rounding changes nothing
        np.testing.assert_array_equal(normals, case.expected_normals(fmt))
        np.testing.assert_array_equal(covs.astype(np.float32), cc.expected_covariance(case.expected_normals(fmt)))
    else:
        assert r.ev[1] - r.ev[0] <= 1e-30 * r.ev[2] and r.ev[2] > 0  # ev0 == ev1 in the reference
        assert max(cc.rayleigh_excess(n, r) for n in normals) <= 1e-5
        if case.name == "octahedron_prolate":
            assert np.all(np.abs(normals[:, 2]) <= 2.0**-23)


def test_the_catalogue_is_what_it_claims(orc):
    # the exact cases take the arms they were designed for
    assert np.array_equal(cc.BY_NAME["grid_4x3"].expected_normals(), np.tile([0.0, 0, 1], (12, 1)))
    assert np.array_equal(cc.BY_NAME["octahedron_iso"].expected_normals(), np.tile([-1.0, 0, 0], (6, 1)))
    ob = cc.BY_NAME["octahedron_oblate"]
    assert np.sum(ob.points @ ob.e == 0.0) == 4                  # the centre ring: p . n == 0, the solver's sign shows
    assert ob.expected_normals().tolist() == [[0, 0, 1]] * 4 + [[0, 0, -1], [0, 0, 1]]
    assert np.array_equal(cc.BY_NAME["identical_x_pos"].expected_normals(), np.tile([-1.0, 0, 0], (10, 1)))
    assert np.array_equal(cc.BY_NAME["identical_x_neg"].expected_normals(), np.tile([1.0, 0, 0], (10, 1)))
    assert cc.BY_NAME["identical_k1"].k_neighbors == 1 and cc.RUNS == [(12, 12), (10, 10), (10, 6), (10, 1)]
    # the 200 m plane tells the FP64 points from their FP32 image: the two references are further apart than any bound used on either
    pl = cc.BY_NAME["plane_200m"]
    assert np.all(pl.points[:, :2] != pl.values("f32")[:, :2])
    apart = cc.sine(cc.case_reference(pl, "f64").vec, cc.case_reference(pl, "f32").vec_mp)
    print(f"plane_200m: sine between the reference of the FP64 points and that of their FP32 roundings = {apart:.3e}")
    assert apart >= 1e-5
    assert cc.case_reference(pl, "f64").ev[0] < 1e-40  # an exact plane
    # the flip pair: mirrored values, opposite oracle normals, every member on the same side
    a, b = cc.BY_NAME["flip_patch"], cc.BY_NAME["flip_patch_mirrored"]
    assert b.mirror_of == a.name and np.array_equal(a.points, -b.points)
    for fmt in cc.FORMATS:
        na, nb_ = oracle_on_case(orc, a, fmt)[0], oracle_on_case(orc, b, fmt)[0]
        np.testing.assert_array_equal(na, -nb_)
        assert np.all(na == na[0])
    # layout: one cloud of at most 600 points, fillers come from another group
    pts, rows = cc.assemble("f64")
    assert len(pts) <= 600
    for width, k in cc.RUNS:
        nb = cc.neighbor_lists(rows, width)
        assert nb.min() >= 0 and nb.max() < len(pts)
        for c in cc.CASES:
            r = rows[c.name]
            assert np.all(nb[r] == nb[r[0]]) and set(nb[r[0], :min(width, len(r))]) <= set(r)
            assert not set(nb[r[0], len(r):]) & set(r)
        for fmt in cc.FORMATS:  # every run evaluates every group, also those it was not designed for: the solver stays finite on all of them
            normals, covs = orc.covariances(np.asarray(cc.assemble(fmt)[0], dtype=np.float64), nb, k_neighbors=k)
            assert np.isfinite(normals).all() and np.isfinite(covs).all()


def test_oracle_error_record_is_written(measured):
    """Writes tests/golden/covariance_cases.json when GLIM_AMD_WRITE_GOLDEN is set or the file is missing; otherwise checks that the record
    covers the catalogue as it stands."""
    if os.environ.get("GLIM_AMD_WRITE_GOLDEN") or not os.path.exists(cc.GOLDEN):
        with open(cc.GOLDEN, "w") as f:
            json.dump(measured, f, indent=1, sort_keys=True)
            f.write("\n")
    gold = cc.load_golden()
    assert set(gold) == {c.name for c in cc.CASES}
    for c in cc.CASES:
        assert set(gold[c.name]) == set(cc.FORMATS) and all(gold[c.name][f]["kind"] == c.kind for f in cc.FORMATS)


def test_oracle_has_not_drifted_above_its_record(measured):
    gold = cc.load_golden()
    for name, by_fmt in measured.items():
        for fmt, m in by_fmt.items():
            g = gold[name][fmt]
            assert m["gap"] == pytest.approx(g["gap"], rel=1e-12, abs=1e-300), (name, fmt)
            if "oracle_sine" in g:
                # the record was measured with one host math library; another may differ in the last place of the solver's atan2, cos and sin,
                # each of which moves the eigenvector by at most eps / gap: that much, and nothing else, is allowed on top of the record
                slack = 3.0 * 2.220446049250313e-16 / g["gap"]
                assert m["oracle_sine"] <= g["oracle_sine"] + slack, (name, fmt, m["oracle_sine"], g["oracle_sine"])
