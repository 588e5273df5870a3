"""The clouds and the reference of tests/test_gicp_search.py: what the GICP search index (nearest() in glim_amd/csrc/gicp.hip) must return on
clouds a LiDAR scan of a room never produces -- exact ties, points at the radius, duplicates, points on cell faces, non-finite points,
every regime of the cell edge h, and radii at the limit of the bounded ring walk.

The reference is brute force in NumPy and shares nothing with the oracle's C: for a query q, d = (dx*dx + dy*dy) + dz*dz in FP64 over all
finite target points (rounded to FP32 first, as the device stores them), the first minimum (the smallest index), -1 when d > max_d^2 or q is
not finite.  Family 1 (exact data) keeps q = R p + t exact in any operation order: coordinates are multiples of 2^-6 below 2^10, rotations are
signed permutations.  Family 2 (general poses) has the oracle as a second reference, which follows the device's FMA order for q."""
import numpy as np

GRID_HALF = 1048576.0  # the index's grid: 2^20 cells either side of the origin on each axis
MAX_RING = 64          # GICP_MAX_RING
EDGE_SHRINK = 0.999999  # GICP_EDGE_SHRINK


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def eye_covs(n):
    return np.tile(np.eye(3), (n, 1, 1))


def transform(T, p):
    """q = R p + t on the FP32-rounded source, entry by entry (no BLAS: the same bits everywhere)"""
    p = f32(p)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore"):  # 0 * inf of a non-finite source point
        return np.stack([(T[r, 0] * x + T[r, 1] * y) + (T[r, 2] * z + T[r, 3]) for r in range(3)], axis=1)


def brute_force(target, q, max_d, usable=None):
    """-> (corr, multiplicity, d2): per query the smallest index among the nearest finite target points or -1, how many target points share
    that smallest distance (0: there is no finite target point, or q is not finite), and the distance squared.  usable: a mask of the target
    points the search may return (default: the finite ones); indices stay those of `target`."""
    t = f32(target).reshape(-1, 3)
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    ok = np.isfinite(t).all(axis=1) if usable is None else (np.asarray(usable, dtype=bool) & np.isfinite(t).all(axis=1))
    idx = np.flatnonzero(ok)
    corr = np.full(len(q), -1, dtype=np.int32)
    mult = np.zeros(len(q), dtype=np.int64)
    d2 = np.full(len(q), np.inf)
    qok = np.flatnonzero(np.isfinite(q).all(axis=1))
    if len(idx) == 0 or len(qok) == 0:
        return corr, mult, d2
    tf = t[idx]
    for s in range(0, len(qok), 256):
        sel = qok[s:s + 256]
        dx, dy, dz = (q[sel, a][:, None] - tf[None, :, a] for a in range(3))
        d = (dx * dx + dy * dy) + dz * dz
        j = np.argmin(d, axis=1)  # the first minimum: the smallest index
        dj = d[np.arange(len(sel)), j]
        mult[sel] = (d == dj[:, None]).sum(axis=1)
        d2[sel] = dj
        corr[sel] = np.where(dj <= max_d * max_d, idx[j], -1)
    return corr, mult, d2


def half_sum_d2(corr, d2):
    """the factor's error with identity covariances on both sides: M = (I + R I R^T)^-1 = I / 2, so error = sum r^T M r = 0.5 sum d^2"""
    return 0.5 * float(d2[corr >= 0].sum())


# ---- the build's choice of the cell edge, restated (glim_amd_nn_index_create) -------------------------------------------------------------
def in_grid(target, h):
    t = f32(target).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        c = t * (1.0 / h)
        return np.isfinite(t).all(axis=1) & ((c >= -GRID_HALF) & (c < GRID_HALF)).all(axis=1)


def cell_edge(target, hint):
    """-> (h, mask of the target points that get a cell): pass 1 at h = hint learns the extent in cells, then the edge that gives about 3 points
    per occupied cell of a surface-like cloud, clamped to [hint / 3, hint]"""
    t = f32(target).reshape(-1, 3)
    R = hint if hint > 0.0 else 1.0
    h = R
    ok = in_grid(t, h)
    if ok.any():
        c = np.floor(t[ok] * (1.0 / h))
        ex, ey, ez = ((c[:, a].max() - c[:, a].min() + 1) * h for a in range(3))
        area = ex * ey + ey * ez + ex * ez
        h_new = min(R, max(R / 3.0, np.sqrt(3.0 * 2.0 * area / len(t))))
        if h_new != h:
            h = h_new
            ok = in_grid(t, h)
    return h, ok


def rings_needed(d, h):
    """GicpTarget::rings: the rings after which the walk's own (shrunk) count of the scanned cube covers d; more than MAX_RING is refused"""
    return int(np.ceil(d / (h * EDGE_SHRINK)))


# ---- family 1: exact data -----------------------------------------------------------------------------------------------------------------
IDENTITY = np.eye(4)
RZ90 = np.array([[0.0, -1.0, 0.0, 0.5], [1.0, 0.0, 0.0, -1.0], [0.0, 0.0, 1.0, 0.25], [0.0, 0.0, 0.0, 1.0]])  # Rz(90 deg), t = (0.5, -1, 0.25)
EXACT_POSES = {"identity": IDENTITY, "rz90": RZ90}


def exact_inverse(T):
    Ti = np.eye(4)
    Ti[:3, :3] = T[:3, :3].T
    Ti[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return Ti + 0.0  # no negative zeros


def is_exact(a):
    a = np.asarray(a, dtype=np.float64)
    a = a[np.isfinite(a)]
    return bool(np.all(a * 64 == np.round(a * 64)) and np.all(np.abs(a) <= 1024))


def lattice_target():
    """the 12^3 lattice with spacing 0.5 on [-3, 2.5]^3 in a seeded random index order"""
    g = -3.0 + 0.5 * np.arange(12)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return p[np.random.default_rng(11).permutation(len(p))]


def lattice_source():
    """64 each: body centres of lattice cells (8-way ties at the identity pose), face centres (4-way), edge midpoints (2-way) and lattice
    points themselves (d = 0); the base points are drawn from the whole lattice, so some lie on its boundary and tie less"""
    rng = np.random.default_rng(12)
    out = []
    for axes in (3, 2, 1, 0):
        base = -3.0 + 0.5 * rng.integers(0, 12, size=(64, 3))
        off = np.zeros((64, 3))
        for i in range(64):
            off[i, rng.permutation(3)[:axes]] = 0.25
        out.append(base + off)
    return np.concatenate(out)


LATTICE_MAX_D = (1.0, 0.5, 0.433, 0.25)  # 0.433: just below the body centres' sqrt(3) / 4; 0.25: the edge midpoints lie AT the radius
LATTICE_HINTS = (0.5, 0.3)  # 0.5: h = 0.5, lattice points on cell faces, margin 0, negative cells; 0.3: tied candidates in different cells and rings


def radius_case():
    """-> (target, source, max_d, expected): two matches at exactly the radius, two misses just beyond it (one by 2^-6, one by an FP32 ulp)"""
    target = np.array([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0]])
    source = np.array([[0.75, 0.0, 0.0], [10.0, -0.75, 0.0], [0.765625, 0.0, 0.0], [10.0, 0.0, 0.7500001]])
    return target, source, 0.75, np.array([0, 1, -1, -1], dtype=np.int32)


PILE = np.array([1.25, -2.5, 0.75])
PILE_FIRST = 137  # the pile's smallest original index


def duplicates_target():
    """300 copies of PILE at every other original index from PILE_FIRST on, among 700 uniform points of [-4, 4)^3"""
    rng = np.random.default_rng(13)
    p = rng.integers(-256, 256, size=(1000, 3)) / 64.0
    p[PILE_FIRST + 2 * np.arange(300)] = PILE
    return p


def duplicates_source():
    """128 queries within 3/64 per axis of the pile (4 of them on it), 128 anywhere in the cube"""
    rng = np.random.default_rng(14)
    near = PILE + rng.integers(-3, 4, size=(128, 3)) / 64.0
    near[:4] = PILE
    return np.concatenate([near, rng.integers(-256, 256, size=(128, 3)) / 64.0])


def identical_target():
    """1000 times one point: one cell, no key bits, a one-bit sort"""
    return np.tile(np.array([[-0.5, 2.0, 1.5]]), (1000, 1))


def identical_source():
    rng = np.random.default_rng(15)
    p = np.array([-0.5, 2.0, 1.5]) + rng.integers(-64, 65, size=(64, 3)) / 64.0
    p[:2] = [-0.5, 2.0, 1.5]
    return p


def tiny_targets():
    return {"n1": np.array([[0.5, -0.25, 1.0]]), "n2": np.array([[0.5, -0.25, 1.0], [-0.5, -0.25, 1.0]])}  # n2: x = 0 ties between the two


def tiny_source():
    rng = np.random.default_rng(16)
    p = rng.integers(-96, 97, size=(64, 3)) / 64.0
    p[:8, 0] = 0.0  # on the bisector of the n2 target
    p[8] = [0.5, -0.25, 1.0]
    return p


def broken_target():
    """every other point of a 4^3 lattice replaced by NaN, +inf, -inf or a point with one such coordinate; the finite ones keep their indices"""
    g = -1.0 + 0.5 * np.arange(4)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[np.random.default_rng(17).permutation(64)]
    bad = [np.nan, np.inf, -np.inf]
    for k, i in enumerate(range(0, 64, 2)):
        if k % 2:
            p[i] = bad[k % 3]
        else:
            p[i, k % 3] = bad[(k // 2) % 3]
    return p


def nonfinite_target():
    p = np.full((48, 3), np.nan)
    p[1::3] = np.inf
    p[2::3] = -np.inf
    return p


def broken_source():
    """queries on and between the points of the 4^3 lattice, with non-finite ones among them"""
    rng = np.random.default_rng(18)
    p = -1.0 + 0.25 * rng.integers(0, 8, size=(96, 3))
    p[5] = np.nan
    p[17, 1] = np.inf
    p[40, 2] = -np.inf
    p[41, 0] = np.nan
    return p


def exact_cases():
    """name -> dict(target, source, max_ds, hints (None: the index is built with max_d), poses).  The lattice's source is one cloud, which the
    second pose moves to other places of the lattice (z + 0.25: lattice points become edge midpoints); every other case gives its queries
    in the target's frame, so that they stay where the case wants them: exact_source() takes them back through the pose."""
    both = ("identity", "rz90")
    rt, rs, rd, _ = radius_case()
    tiny = tiny_targets()
    return {
        "lattice": dict(target=lattice_target(), source=lattice_source(), max_ds=LATTICE_MAX_D, hints=LATTICE_HINTS, poses=both),
        "radius": dict(target=rt, source=rs, max_ds=(rd,), hints=(None,), poses=("identity",)),
        "duplicates": dict(target=duplicates_target(), source=duplicates_source(), max_ds=(1.0, 0.25), hints=(None,), poses=both),
        "identical": dict(target=identical_target(), source=identical_source(), max_ds=(1.0, 0.25), hints=(None,), poses=both),
        "n1": dict(target=tiny["n1"], source=tiny_source(), max_ds=(1.0, 0.25), hints=(None,), poses=both),
        "n2": dict(target=tiny["n2"], source=tiny_source(), max_ds=(1.0, 0.25), hints=(None,), poses=both),
        "broken": dict(target=broken_target(), source=broken_source(), max_ds=(1.0, 0.25), hints=(None,), poses=both),
        "nonfinite": dict(target=nonfinite_target(), source=broken_source(), max_ds=(1.0,), hints=(None,), poses=both),
    }


def exact_source(name, case, pose):
    return case["source"] if name == "lattice" else transform(exact_inverse(EXACT_POSES[pose]), case["source"])


def exact_runs():
    """every (case name, pose name, hint, max_d) of family 1"""
    return [(name, pose, hint, max_d) for name, c in exact_cases().items() for pose in c["poses"] for hint in c["hints"] for max_d in c["max_ds"]]


# ---- family 2: general pose ---------------------------------------------------------------------------------------------------------------
GENERAL_XI = [0.3, -0.2, 0.9, 0.4, -0.3, 0.2]
LINE_DIR = np.array([0.6, 0.64, 0.48])  # a unit vector off every axis: the bounding box of the line is large, the area estimate degenerate


def general_targets():
    rng = np.random.default_rng(21)
    blob = np.array([5.0, -3.0, 1.0]) + 0.3 * rng.standard_normal((4096, 3))
    plane = np.concatenate([rng.uniform(-3.2, 3.2, size=(4096, 2)), np.full((4096, 1), -1.5)], axis=1)
    line = (rng.uniform(-40.0, 40.0, size=2048))[:, None] * LINE_DIR[None, :]
    clusters = np.concatenate([2990.0 + 0.05 * rng.uniform(-0.5, 0.5, size=(512, 3)), -2990.0 + 0.05 * rng.uniform(-0.5, 0.5, size=(512, 3))])
    clusters = clusters[rng.permutation(1024)]
    return {"blob": f32(blob), "plane": f32(plane), "line": f32(line), "clusters": f32(clusters), "duplicates": duplicates_target()}


GENERAL_MAX_D = {"blob": (0.25, 1.0), "plane": (0.25, 1.0), "line": (0.25, 1.0), "clusters": (0.01, 0.05), "duplicates": (0.25, 1.0)}
GENERAL_QUERIES = 512


def general_source(target, T, max_d, seed):
    """GENERAL_QUERIES source points p (FP32) with T p = a target point + N(0, (0.6 max_d)^2) per axis; every eighth is a stray with five times
    that noise, so that a target dense enough to have a point within max_d of anything near it rejects some queries too"""
    rng = np.random.default_rng(seed)
    sigma = 0.6 * max_d * np.where(np.arange(GENERAL_QUERIES) % 8 == 7, 5.0, 1.0)
    q = target[rng.integers(0, len(target), size=GENERAL_QUERIES)] + sigma[:, None] * rng.standard_normal((GENERAL_QUERIES, 3))
    x, y, z = (q[:, a] - T[a, 3] for a in range(3))  # p = R^T (q - t), entry by entry like transform()
    return f32(np.stack([(T[0, c] * x + T[1, c] * y) + T[2, c] * z for c in range(3)], axis=1))


def general_runs():
    return [(name, max_d) for name, ds in GENERAL_MAX_D.items() for max_d in ds]


def general_case(name, max_d, T):
    target = general_targets()[name]
    return target, general_source(target, T, max_d, seed=100 + general_runs().index((name, max_d)))


# ---- the ring limit -----------------------------------------------------------------------------------------------------------------------
RING_HINT = 0.9
RING_D = 21 * RING_HINT  # the documented limit; with h = hint / 3.0 (a dense target) d / h = 63.00000000000001
RING_EPS = 1e-3  # how far inside / outside the radius the queries lie: far above the FP32 spacing of their coordinates (2e-6 at 32 m)


def nearest_distance(target, q):
    _, _, d2 = brute_force(target, q, np.inf)
    return np.sqrt(d2)


def ring_limit_source(target, seed):
    """64 queries: 32 directions from the target's centroid, on each the FP32 point whose nearest target point is RING_EPS inside RING_D and
    the one RING_EPS outside (bisection on the distance along the ray, which grows with it once outside the cloud)"""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((32, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    c = target.mean(axis=0)
    out = []
    for want in (RING_D - RING_EPS, RING_D + RING_EPS):
        lo, hi = np.zeros(32), np.full(32, RING_D + 2.0 * np.abs(target - c).max() + 1.0)
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            far = nearest_distance(target, c + mid[:, None] * u) > want
            hi = np.where(far, mid, hi)
            lo = np.where(far, lo, mid)
        out.append(f32(c + (0.5 * (lo + hi))[:, None] * u))
    return np.concatenate(out)


# ---- out of the grid ----------------------------------------------------------------------------------------------------------------------
OUT_HINT = 0.001  # h = 0.001: the grid ends 1048.576 m from the origin


def out_of_grid_case():
    """-> (target, source, max_d): 512 points in a 5 cm cluster at the origin, 256 at +2990 m and 256 with only x there -- outside the grid of an
    index built with OUT_HINT -- in a random order; queries around points of all three"""
    rng = np.random.default_rng(31)
    near = 0.05 * rng.uniform(-0.5, 0.5, size=(512, 3))
    far = 2990.0 + 0.05 * rng.uniform(-0.5, 0.5, size=(256, 3))
    far_x = 0.05 * rng.uniform(-0.5, 0.5, size=(256, 3))
    far_x[:, 0] += 2990.0
    target = f32(np.concatenate([near, far, far_x])[rng.permutation(1024)])
    max_d = 5 * OUT_HINT
    source = f32(target[rng.integers(0, 1024, size=384)] + 0.6 * max_d * rng.standard_normal((384, 3)))
    return target, source, max_d
