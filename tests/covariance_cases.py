"""Designed neighbourhoods for the covariance kernel (glim_amd/csrc/covariance.hip) and a multiprecision reference of what it computes.

A neighbourhood is a group of k points in which every member lists the whole group, so the answer for all k members is one eigen-problem
(plus each member's own flip).  The catalogue below names the groups; assemble() lays them out in ONE cloud and neighbor_lists() writes the
lists a run needs (tests install them with PointCloudGPU.set_neighbors).  Kinds:

  conditioned  relative gap (ev1 - ev0) / ev2 >= 0.05 in the reference: the normal is compared with the reference's eigenvector
  exact        dyadic coordinates, every sum exact: the normal and I - 0.999 n n^T are stated, and asserted value for value
  degenerate   ev0 == ev1: the eigenvector is not defined; invariants (and the oracle's values where no libm call rounds) are asserted
  flip         a conditioned patch and its point reflection through the origin: opposite normals, both facing the origin

Groups hold ten points and use lists of ten; the octahedra hold six (k_neighbors = 6 on lists of ten), one group of identical points is run
with k_neighbors = 1, and the 4 x 3 grid holds twelve, so it gets a run of its own on lists of twelve (RUNS).

reference() is written from the definition -- two-pass population covariance and mpmath's symmetric eigen-solver at 200 bits -- and shares no
formula with the closed-form trigonometric solver of the kernel and the oracle.  It takes the exact values the code under test is given: the
FP64 points (fmt "f64"; clone_exact on the device) or their FP32 roundings (fmt "f32"; clone).  A plain module: it holds no tests."""
import json
import os

import numpy as np
from mpmath import mp, mpf

PREC = 200
LIST = 10                    # width of the neighbour lists of every group of at most ten points
W = 1.0 - 1e-3               # I - W n n^T, as the kernel states it
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "covariance_cases.json")
FORMATS = ("f64", "f32")
MIN_GAP = 0.05
STORAGE = float(np.sqrt(3.0) * 2.0**-24)  # a unit vector stored in FP32: each component within half an ulp (<= 2^-24) of its value


class Case:
    def __init__(self, name, kind, points, k_neighbors=None, e=None, mirror_of=None, exact_oracle=False):
        self.name, self.kind = name, kind
        self.points = np.ascontiguousarray(points, dtype=np.float64)
        self.k_neighbors = len(self.points) if k_neighbors is None else k_neighbors   # how many list entries the run reads
        self.width = max(LIST, len(self.points))                                       # width of the list this group needs
        self.e = None if e is None else np.array(e, dtype=np.float64)                  # exact: the solver's eigenvector before the flip
        self.mirror_of = mirror_of
        self.exact_oracle = exact_oracle   # degenerate: no libm call of the solver returns a rounded value, so the oracle's values are owed

    def values(self, fmt):
        """the values the code under test is given, as FP64 numbers"""
        return self.points if fmt == "f64" else self.points.astype(np.float32).astype(np.float64)

    def expected_normals(self, fmt="f64"):
        """exact cases: e, flipped where p . e > 0 (cloud_covariance_estimation.cpp:98-101) -- p . e == 0 keeps the solver's sign"""
        p = self.values(fmt)
        flip = p @ self.e > 0.0
        return np.where(flip[:, None], -self.e[None, :], self.e[None, :])


def expected_covariance(n):
    """I - 0.999 n n^T in the kernel's operation order, rounded to FP32 (rows of 3 x 3)"""
    n = np.asarray(n, dtype=np.float64)
    return (np.eye(3)[None] - (W * n[:, :, None]) * n[:, None, :]).astype(np.float32)


def _frame(normal, spin=0.0):
    """orthonormal columns (u, v, normal)"""
    n = np.asarray(normal, dtype=np.float64)
    n = n / np.linalg.norm(n)
    a = np.array([1.0, 0.0, 0.0]) if abs(n[0]) < 0.8 else np.array([0.0, 1.0, 0.0])
    u = np.cross(n, a)
    u /= np.linalg.norm(u)
    v = np.cross(n, u)
    c, s = np.cos(spin), np.sin(spin)
    return np.stack([c * u + s * v, -s * u + c * v, n], axis=1)


def _patch(seed, centre, spread, ratios, normal, spin=0.3):
    rng = np.random.default_rng(seed)
    local = rng.uniform(-1.0, 1.0, (LIST, 3)) * (spread * np.asarray(ratios, dtype=np.float64))
    return local @ _frame(normal, spin).T + np.asarray(centre, dtype=np.float64)


def _octahedron(centre, half_z):
    h = np.array([[0.5, 0, 0], [-0.5, 0, 0], [0, 0.5, 0], [0, -0.5, 0], [0, 0, half_z], [0, 0, -half_z]])
    return h + np.asarray(centre, dtype=np.float64)


def _plane_200m():
    """points EXACTLY on the plane z = 20 + dx / 4 - dy / 2 about (200, -150, 20): offsets are multiples of 2^-20 within +-0.05 m, so every
    coordinate is an FP64 number -- and none of x, y an FP32 one (ulp 2^-16 there): the FP32 roundings lie ~1e-5 m off the plane"""
    rng = np.random.default_rng(77)
    d = rng.integers(-52428, 52429, (LIST, 2)) | 1   # odd multiples of 2^-20
    dx, dy = d[:, 0] * 2.0**-20, d[:, 1] * 2.0**-20
    return np.stack([200.0 + dx, -150.0 + dy, 20.0 + dx / 4 - dy / 2], axis=1)


def _catalogue():
    g = np.mgrid[0:4, 0:3].reshape(2, -1).T * 0.25
    patch = _patch(21, (6.0, 2.0, -1.0), 0.5, (1, 0.6, 0.05), (1.0, 0.3, -0.2))
    line_t = np.array([-1.0, -0.75, -0.5, -0.25, 0.0, 0.125, 0.25, 0.5, 0.75, 1.0])
    return [
        Case("patch_ratio_0.3", "conditioned", _patch(1, (8.0, -3.0, 1.0), 0.5, (1, 0.6, 0.3), (0.2, -0.5, 1.0))),
        Case("patch_ratio_0.01", "conditioned", _patch(2, (-7.0, 4.0, 2.0), 0.5, (1, 0.6, 0.01), (-0.7, 0.4, 0.3))),
        Case("prolate", "conditioned", _patch(3, (3.0, 9.0, -2.0), 0.4, (1, 0.5, 0.15), (0.5, 0.5, -0.6))),
        Case("spread_1e3_at_5e3", "conditioned", _patch(4, (3000.0, -4000.0, 500.0), 1e3, (1, 0.6, 0.05), (0.3, 0.2, 1.0))),
        Case("spread_1e-3_near_origin", "conditioned", _patch(5, (0.01, -0.012, 0.008), 1e-3, (1, 0.6, 0.05), (1.0, -0.4, 0.5))),
        Case("spread_1e-4_at_3e-4", "conditioned", _patch(6, (2e-4, -2e-4, 1e-4), 1e-4, (1, 0.6, 0.05), (-0.3, 1.0, 0.4))),
        Case("plane_200m", "conditioned", _plane_200m()),
        Case("grid_4x3", "exact", np.c_[g + [1.0, 2.0], np.full(12, -1.5)], e=(0, 0, 1)),
        Case("octahedron_iso", "exact", _octahedron((4, 0, 0), 0.5), e=(1, 0, 0)),
        Case("octahedron_oblate", "exact", _octahedron((4, 0, 0), 0.25), e=(0, 0, 1)),
        Case("identical_x_pos", "exact", np.tile([2.5, -1.25, 0.75], (LIST, 1)), e=(1, 0, 0)),
        Case("identical_x_neg", "exact", np.tile([-2.5, 1.25, 0.75], (LIST, 1)), e=(1, 0, 0)),
        Case("identical_k1", "exact", np.tile([3.25, 0.5, -0.75], (LIST, 1)), k_neighbors=1, e=(1, 0, 0)),
        # ev0 == ev1 < ev2.  The solver's q rounds to 2e-18, not 0: theta ~ 3.5e-9, the roots differ by ~6e-9 and the ordinary arm runs on
        # diag(d, d, 1.5) - whose cross products hold exact zeros, so the result is a coordinate axis whatever the last place of sin / cos
        Case("octahedron_prolate", "degenerate", _octahedron((4, 0, 0), 0.75), exact_oracle=True),
        # rank one.  q clamps to 0 exactly, atan2(0, +) = 0, cos = 1, sin = 0: ev0 == ev1 bit for bit, which is the lambda0 == lambda1 arm with
        # its self-referencing orthonormalisation, and no libm call on it returns a rounded value
        Case("collinear", "degenerate", np.array([3.0, -1.0, 2.0]) + line_t[:, None] * np.array([1.0, 2.0, -2.0]), exact_oracle=True),
        Case("flip_patch", "flip", patch),
        Case("flip_patch_mirrored", "flip", -patch, mirror_of="flip_patch"),
    ]


CASES = _catalogue()
BY_NAME = {c.name: c for c in CASES}
RUNS = sorted({(c.width, c.k_neighbors) for c in CASES}, reverse=True)   # (list width, k_neighbors) of the runs the catalogue needs


def assemble(fmt):
    """(points of the whole catalogue in one cloud -- FP64 values for "f64", float32 for "f32" -- and name -> index array of the group)"""
    rows, parts, at = {}, [], 0
    for c in CASES:
        rows[c.name] = np.arange(at, at + len(c.points))
        parts.append(c.points)
        at += len(c.points)
    pts = np.concatenate(parts)
    return (pts if fmt == "f64" else pts.astype(np.float32)), rows


def neighbor_lists(rows, width):
    """every member of a group lists the whole group; entries a run does not read (beyond the group) hold a member of the NEXT group, so
    that reading past k_neighbors -- or with the wrong row stride -- changes the sums.  A group larger than `width` is cut (not checked there)."""
    n = sum(len(r) for r in rows.values())
    nb = np.zeros((n, width), dtype=np.int32)
    for gi, c in enumerate(CASES):
        r = rows[c.name]
        other = rows[CASES[(gi + 1) % len(CASES)].name]
        row = list(r[:width]) + [other[j % len(other)] for j in range(width - min(width, len(r)))]
        nb[r] = np.array(row, dtype=np.int32)[None, :]
    return nb


class Reference:
    def __init__(self, ev, vec, sigma):
        self.ev_mp, self.vec_mp, self.sigma_mp = ev, vec, sigma
        self.ev = [float(x) for x in ev]
        self.vec = np.array([float(x) for x in vec])
        self.gap = float((ev[1] - ev[0]) / ev[2]) if ev[2] > 0 else 0.0


def reference(values, prec=PREC):
    """population covariance of the rows of `values` (exact FP64 numbers), two-pass, and its symmetric eigen-decomposition at `prec` bits:
    ascending eigenvalues and the unit eigenvector of the smallest"""
    with mp.workprec(prec):
        P = [[mpf(float(x)) for x in p] for p in values]
        k = len(P)
        mean = [sum((p[a] for p in P), mpf(0)) / k for a in range(3)]
        D = [[p[a] - mean[a] for a in range(3)] for p in P]
        sigma = [[sum((d[a] * d[b] for d in D), mpf(0)) / k for b in range(3)] for a in range(3)]
        E, Q = mp.eigsy(mp.matrix(sigma))
        order = sorted(range(3), key=lambda i: E[i])
        v = [Q[r, order[0]] for r in range(3)]
        nv = mp.sqrt(sum((x * x for x in v), mpf(0)))
        return Reference([E[i] for i in order], [x / nv for x in v], sigma)


_refs = {}


def case_reference(case, fmt):
    key = (case.name, fmt)
    if key not in _refs:
        _refs[key] = reference(case.values(fmt)[:case.k_neighbors])
    return _refs[key]


def sine(n, ref_vec, prec=PREC):
    """sine of the angle between the direction of n (FP64 numbers, any length > 0) and a unit reference vector, evaluated at `prec` bits"""
    with mp.workprec(prec):
        n = [mpf(float(x)) for x in n]
        v = list(ref_vec)
        c = [n[1] * v[2] - n[2] * v[1], n[2] * v[0] - n[0] * v[2], n[0] * v[1] - n[1] * v[0]]
        return float(mp.sqrt(sum((x * x for x in c), mpf(0))) / mp.sqrt(sum((x * x for x in n), mpf(0))))


def rayleigh_excess(n, ref, prec=PREC):
    """(n^T Sigma n / n^T n - ev0) / ev2 with the reference's covariance"""
    with mp.workprec(prec):
        n = [mpf(float(x)) for x in n]
        q = sum((n[a] * ref.sigma_mp[a][b] * n[b] for a in range(3) for b in range(3)), mpf(0)) / sum((x * x for x in n), mpf(0))
        return float((q - ref.ev_mp[0]) / ref.ev_mp[2])


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
