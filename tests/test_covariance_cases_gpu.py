"""The covariance kernel (glim_amd/csrc/covariance.hip) on the designed neighbourhoods of tests/covariance_cases.py, in both instances --
covariance_kernel<false> over the FP32 points of PointCloudGPU.clone and covariance_kernel<true> over the FP64 points of api.clone_exact --
against the multiprecision reference, then at the edges of the launch and of the neighbour-list indexing against the oracle.  No case is
excluded and no fraction of points is allowed to miss."""
import numpy as np
import pytest

import covariance_cases as cc
from test_ref import covariance_report, write_report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from glim_amd import api

    return api.Context(0, 1)


def make_cloud(ctx, fmt, points):
    from glim_amd import api

    if fmt == "f64":
        return api.clone_exact(np.asarray(points, dtype=np.float64), ctx=ctx)
    assert points.dtype == np.float32
    return api.PointCloudGPU.clone(points, ctx=ctx)


@pytest.fixture(scope="module")
def runs(ctx):
    """fmt -> (points as FP64 values, rows, {(width, k_neighbors): (covs, normals)}): the whole catalogue in one cloud per point format, one
    estimate_covariances call per neighbour-count case"""
    out = {}
    for fmt in cc.FORMATS:
        pts, rows = cc.assemble(fmt)
        assert len(pts) <= 600
        g = make_cloud(ctx, fmt, pts)
        if fmt == "f64":
            np.testing.assert_array_equal(g.download_points64(), pts)  # the kernel is given the catalogue's FP64 values
        res = {}
        for width, k in cc.RUNS:
            g.set_neighbors(cc.neighbor_lists(rows, width))
            g.estimate_covariances(k)
            _, covs, normals = g.download()
            res[(width, k)] = (covs.copy(), normals.copy())
        out[fmt] = (np.asarray(pts, dtype=np.float64), rows, res)
    return out


def of_case(runs, case, fmt):
    pts, rows, res = runs[fmt]
    covs, normals = res[(case.width, case.k_neighbors)]
    r = rows[case.name]
    return pts[r], covs[r], normals[r]


@pytest.mark.parametrize("fmt", cc.FORMATS)
def test_every_point_of_the_catalogue_keeps_the_invariants(runs, fmt):
    """unit normal, facing the origin, covariance == I - 0.999 n n^T of the downloaded normal to 3e-7 -- in every run, on every point"""
    pts, _, res = runs[fmt]
    for covs, normals in res.values():
        n64 = normals.astype(np.float64)
        np.testing.assert_allclose(np.linalg.norm(n64, axis=1), 1.0, atol=2e-7)
        assert np.all(np.einsum("ni,ni->n", pts, n64) <= 1e-6 * np.linalg.norm(pts, axis=1) + 1e-12)
        np.testing.assert_allclose(covs.astype(np.float64), np.eye(3)[None] - 0.999 * n64[:, :, None] * n64[:, None, :], atol=3e-7)
    # k_neighbors = 1 makes every neighbourhood a single point: the isotropic arm on all of them, (1, 0, 0) flipped by the sign of x
    _, normals = res[(cc.LIST, 1)]
    np.testing.assert_array_equal(normals, np.where(pts[:, :1] > 0.0, [[-1.0, 0.0, 0.0]], [[1.0, 0.0, 0.0]]).astype(np.float32))


def test_conditioned_normals_meet_the_multiprecision_reference(runs):
    """sine of the angle to the reference's eigenvector <= sqrt(3) 2^-24 (FP32 storage of a unit vector) + 10 x the oracle's recorded error
    (tests/golden/covariance_cases.json), on every member of every conditioned and flip case, in both point formats.  The 200 m plane decides
    whether each kernel instance reads its own array: its normal meets the reference of the values it is given and is > 1e-5 from the other."""
    gold = cc.load_golden()
    report = {}
    for case in cc.CASES:
        if case.kind not in ("conditioned", "flip"):
            continue
        for fmt in cc.FORMATS:
            r = cc.case_reference(case, fmt)
            assert r.gap >= cc.MIN_GAP
            _, _, normals = of_case(runs, case, fmt)
            device = max(cc.sine(n, r.vec_mp) for n in normals.astype(np.float64))
            bound = cc.STORAGE + 10.0 * gold[case.name][fmt]["oracle_sine"]
            report[f"{case.name}.{fmt}"] = {"device_sine": device, "bound": bound, "oracle_sine": gold[case.name][fmt]["oracle_sine"], "gap": r.gap}
            print(f"{case.name} [{fmt}]: device sine {device:.3e}, bound {bound:.3e} (oracle {gold[case.name][fmt]['oracle_sine']:.3e}, gap {r.gap:.3f})")
    pl = cc.BY_NAME["plane_200m"]
    for fmt, other in (("f64", "f32"), ("f32", "f64")):
        _, _, normals = of_case(runs, pl, fmt)
        away = min(cc.sine(n, cc.case_reference(pl, other).vec_mp) for n in normals.astype(np.float64))
        report[f"plane_200m.{fmt}"]["sine_to_the_other_formats_reference"] = away
        print(f"plane_200m [{fmt}]: sine to the reference of the {other} values {away:.3e}")
    write_report("covariance_cases_device.json", report)
    for name, m in report.items():
        assert m["device_sine"] <= m["bound"], (name, m)
    for fmt in cc.FORMATS:
        assert report[f"plane_200m.{fmt}"]["sine_to_the_other_formats_reference"] > 1e-5, report[f"plane_200m.{fmt}"]


@pytest.mark.parametrize("fmt", cc.FORMATS)
def test_exact_cases_give_their_stated_values(runs, fmt):
    """dyadic coordinates: the isotropic return (1, 0, 0), the unflipped sign at p . n == 0, k_neighbors < k with foreign entries behind it
    and k_neighbors = 1 -- the stated normal and I - 0.999 n n^T rounded to FP32, value for value (a zero's sign does not count)"""
    for case in cc.CASES:
        if case.kind != "exact":
            continue
        _, covs, normals = of_case(runs, case, fmt)
        want = case.expected_normals(fmt)
        np.testing.assert_array_equal(normals, want.astype(np.float32), err_msg=case.name)
        np.testing.assert_array_equal(covs, cc.expected_covariance(want), err_msg=case.name)
    _, covs, _ = of_case(runs, cc.BY_NAME["octahedron_iso"], fmt)
    np.testing.assert_array_equal(covs[0], np.diag([1e-3, 1.0, 1.0]).astype(np.float32))


@pytest.mark.parametrize("fmt", cc.FORMATS)
def test_degenerate_cases_keep_the_invariants_and_the_oracles_exact_values(runs, orc, fmt):
    for case in cc.CASES:
        if case.kind != "degenerate":
            continue
        r = cc.case_reference(case, fmt)
        pts, covs, normals = of_case(runs, case, fmt)
        n64 = normals.astype(np.float64)
        np.testing.assert_allclose(np.linalg.norm(n64, axis=1), 1.0, atol=2e-7)
        excess = max(cc.rayleigh_excess(n, r) for n in n64)
        print(f"{case.name} [{fmt}]: (n^T Sigma n - ev0) / ev2 = {excess:.3e}")
        assert excess <= 1e-5, case.name
        if case.name == "octahedron_prolate":
            assert np.all(np.abs(n64[:, 2]) <= 2.0**-23)
        if case.exact_oracle:
            nb = np.tile(np.arange(len(pts), dtype=np.int32), (len(pts), 1))
            on, _ = orc.covariances(pts, nb, k_neighbors=case.k_neighbors)
            np.testing.assert_array_equal(normals, on.astype(np.float32), err_msg=case.name)
            np.testing.assert_array_equal(covs, cc.expected_covariance(on), err_msg=case.name)


@pytest.mark.parametrize("fmt", cc.FORMATS)
def test_flip_pair_gives_opposite_normals_facing_the_origin(runs, fmt):
    a, b = cc.BY_NAME["flip_patch"], cc.BY_NAME["flip_patch_mirrored"]
    pa, ca, na = of_case(runs, a, fmt)
    pb, cb, nb = of_case(runs, b, fmt)
    np.testing.assert_array_equal(pa, -pb)
    # negating every point negates the sums and leaves every product: the same matrix, the same eigenvector, the other flip
    np.testing.assert_array_equal(na, -nb)
    np.testing.assert_array_equal(ca, cb)
    assert np.all(np.einsum("ni,ni->n", pa, na.astype(np.float64)) < 0.0) and np.all(np.einsum("ni,ni->n", pb, nb.astype(np.float64)) < 0.0)


def edge_cloud(n, seed):
    """uniform in a 10 m cube 20 m from the origin (so that about half the solver's eigenvectors get flipped); every point has its OWN list:
    itself, then nine random indices; index 0 and index n - 1 both occur"""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-5.0, 5.0, (n, 3)) + [20.0, -3.0, 4.0]
    nb = rng.integers(0, n, (n, cc.LIST)).astype(np.int32)
    nb[:, 0] = np.arange(n)
    nb[0, 1], nb[n - 1, 2] = n - 1, 0
    return pts, nb


@pytest.mark.parametrize("fmt", cc.FORMATS)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_launch_and_indexing_edges_against_the_oracle(ctx, orc, n, fmt):
    """one point, one short of / exactly / one past a 256-thread block, two blocks and one thread; k_neighbors == k and < k"""
    pts, nb = edge_cloud(n, 1000 + n)
    assert nb.min() == 0 and nb.max() == n - 1
    if n > 1:  # the solver's own eigenvector (before the flip) points away from the origin on some points and towards it on others
        d = pts[nb] - pts[nb].mean(1, keepdims=True)
        side = np.array([pts[i] @ orc.eigen3(d[i].T @ d[i] / cc.LIST)[1][:, 0] for i in range(n)])
        assert 0.2 < np.mean(side > 0.0) < 0.8 and np.abs(side).min() > 1e-3
    g = make_cloud(ctx, fmt, pts if fmt == "f64" else pts.astype(np.float32))
    given = g.download_points64() if fmt == "f64" else g.download(covs=False, normals=False)[0].astype(np.float64)
    np.testing.assert_array_equal(given, pts if fmt == "f64" else pts.astype(np.float32).astype(np.float64))
    g.set_neighbors(nb)
    for k in (10, 7):
        g.estimate_covariances(k)
        _, covs, normals = g.download()
        rn, rc = orc.covariances(given, nb, k_neighbors=k)
        frac, worst_gap = covariance_report(given, nb, k, covs, normals, rc, rn)
        print(f"n = {n}, k_neighbors = {k} [{fmt}]: fraction beyond 1e-5 = {frac:.2e}, largest relative gap among them = {worst_gap:.2e}")
        assert frac == 0.0 or worst_gap < 1e-6, (n, k, fmt, frac, worst_gap)


@pytest.mark.parametrize("fmt", cc.FORMATS)
def test_three_points_with_five_neighbours_read_the_zero_tail(ctx, orc, fmt):
    pts = np.array([[4.0, 1.0, 0.5], [4.5, 1.25, 0.25], [3.75, 0.5, 1.0]])
    g = make_cloud(ctx, fmt, pts if fmt == "f64" else pts.astype(np.float32))
    nb = g.find_neighbors(5)
    assert nb.shape == (3, 5) and np.all(nb[:, 3:] == 0) and all(sorted(r[:3]) == [0, 1, 2] for r in nb.tolist())
    g.estimate_covariances(5)
    _, covs, normals = g.download()
    rn, rc = orc.covariances(pts, nb, k_neighbors=5)
    frac, worst_gap = covariance_report(pts, nb, 5, covs, normals, rc, rn)
    assert frac == 0.0 or worst_gap < 1e-6, (frac, worst_gap)


@pytest.mark.parametrize("fmt", cc.FORMATS)
def test_repeated_calls_give_identical_bytes(ctx, fmt):
    pts, nb = edge_cloud(513, 7)
    g = make_cloud(ctx, fmt, pts if fmt == "f64" else pts.astype(np.float32))
    g.set_neighbors(nb)

    def run(k):
        g.estimate_covariances(k)
        _, covs, normals = g.download()
        return covs.tobytes() + normals.tobytes()

    first = run(10)
    assert run(10) == first
    other = run(7)
    assert other != first
    assert run(10) == first
