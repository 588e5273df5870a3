"""NumPy (FP64) restatement of the plane bundle-adjustment tool's device side (include/glim_amd.h "Plane / edge bundle-adjustment factors and
ball selection"): the ball selection in the device's documented operation order, the sums and covariance of
bundle_adjustment_modal.cpp:177-178, the radius search of :186-227, and the plane / edge eigenvalue factor in the POINT-PAIR form -- never
through per-frame moments, which is what the device uses and what this file is there to check.

The factor.  With q_i = R_f p_i + t_f, m the mean, C the covariance, (lambda_k, u_k) its eigenpairs, e the eigenvalue index,
a_i = u_e . (q_i - m), b_ik = u_k . (q_i - m) and J_i = dq_i / dxi = [-R hat(p_i), R] (tangent [rotation, translation], T Exp(xi)):

    gradient   sum_i J_i^T (2 / N) a_i u_e
    H_ij       (2 / N)(delta_ij - 1 / N) u_e u_e^T + sum_{k != e} (2 / N^2) / (lambda_e - lambda_k) (a_i u_k + b_ik u_e)(b_jk u_e + a_j u_k)^T
    H          sum_ij J_i^T H_ij J_j

`factor_pairs` evaluates that double sum literally (O(N^2), small N only); `factor` sums the same per-point vectors first
(x_i = J_i^T u_e, w_ik = J_i^T (a_i u_k + b_ik u_e)), which is the same double sum with the two indices separated; the CPU test holds
the two against each other.  The edge kind adds the results for e = 0 and e = 1.

Gates of tests/test_plane_ba_gpu.py, derived here and computed by the test from its data -- none comes from what the device returns:

  sums       the device and NumPy add the same terms in two orders, so an entry of a sum of n terms x_i may differ by at most
             2 (n - 1) u sum |x_i|, u = 2^-53 (each order is within (n - 1) u sum |x_i| of the exact sum).
  eigenpairs the closed-form solver is not backward stable to the last place, so its own error on this scene's covariances is measured on
             the CPU (oracle.eigen3): the residual |C u - lambda u| / |C| and the orthonormality defect |U^T U - I|; the gate is 8 x the
             worst, the margin covering last-place differences of the device's atan2 / cos / sin.
  factor     two parts.  (a) the solver: the restatement is run with numpy's eigh and with oracle.eigen3's eigenpairs, and 8 x the worst
             relative difference of g and of H is the solver's share.  (b) the sums: the device's covariance differs from the
             restatement's by at most dC = (b_qq + 2 |m| b_q) / N per entry, b the sum bound above over the points taken about the
             first one; an eigenvalue moves by at most |dC| and an eigenvector by |dC| / gap (gap: the smallest |lambda_e - lambda_k|
             that enters), and every term of g and H is a product of at most four such quantities and 1 / gap, so to first order the
             relative change is at most 16 |dC|_F / gap.  gate = 8 x (a) + (b).  The input condition lambda_2 / gap <= 10, asserted on
             the restatement, keeps (b) small.  "Relative" is, for g, to the largest entry of sum_i |J_i^T (2 / N) a_i u_e| (`g_scale`)
             and, for H, to the largest entry of the sum of the magnitudes of its three parts (`H_scale`: the per-frame blocks, the mean
             term, the eigenvector terms).  g and H themselves are no yardsticks, because they vanish -- identically for a factor of one
             frame, whose cost no pose changes, and g nearly at poses the points were generated with -- while every one of their terms
             keeps its size and its rounding error.
"""
import numpy as np

from glim_amd.se3 import hat, se3_exp

U = 2.0 ** -53


# ---- selection, in the device's operation order: elementwise, every product and sum rounded --------------------------------------------
def transform(points, T, center):
    """q = R p + (t - c): d = t - c first, then ((R0 p_x + R1 p_y) + R2 p_z) + d per row"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    T = np.asarray(T, dtype=np.float64)
    d = T[:3, 3] - np.asarray(center, dtype=np.float64)
    q = np.empty_like(p)
    for r in range(3):
        q[:, r] = ((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + d[r]
    return q


def sqnorm(q):
    return (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]


def select(clouds, poses, center, radius):
    """-> (pairs n x 2 int32 ascending in (sub-map, point), q n x 3)"""
    pairs, qs = [], []
    r2 = radius * radius
    for s, (p, T) in enumerate(zip(clouds, poses)):
        q = transform(p, T, center)
        idx = np.nonzero(sqnorm(q) < r2)[0]
        pairs.append(np.stack([np.full(len(idx), s), idx], axis=1))
        qs.append(q[idx])
    return np.concatenate(pairs).astype(np.int32).reshape(-1, 2), np.concatenate(qs).reshape(-1, 3)


# ---- statistics ----------------------------------------------------------------------------------------------------------------------------
def sums(q):
    return len(q), q.sum(axis=0), np.einsum("ia,ib->ab", q, q)


def covariance(n, s, S):
    """bundle_adjustment_modal.cpp:177-178"""
    mean = s / n
    return (S - np.outer(mean, s)) / n


def sum_bounds(q):
    """2 (n - 1) u sum |x_i| for the entries of sum q and sum q q^T"""
    n = len(q)
    return 2 * (n - 1) * U * np.abs(q).sum(axis=0), 2 * (n - 1) * U * np.einsum("ia,ib->ab", np.abs(q), np.abs(q))


# ---- the radius search ---------------------------------------------------------------------------------------------------------------------
def auto_radius(evaluate, r0, min_radius, max_radius, plane_eps):
    """bundle_adjustment_modal.cpp:186-227.  evaluate(r) -> (count, eigenvalues).  -> (radius, trace): one (radius, count, eigenvalues,
    decision) per evaluation, a trial that left the range included (count -1)."""
    cur = r0
    n, lam = evaluate(r0)
    trace = [(r0, n, lam, "initial")]
    stop = "trials"
    for _ in range(10):
        with np.errstate(all="ignore"):
            trial = cur * 0.8 if lam[0] / lam[2] > plane_eps else cur * 1.1
        if trial < min_radius or trial > max_radius:
            trace.append((trial, -1, np.full(3, np.nan), "range"))
            stop = "range"
            break
        tn, tl = evaluate(trial)
        if tn < 10:
            trace.append((trial, tn, tl, "few_points"))
            stop = "few_points"
            break
        if trial > r0 and tl[0] / tl[2] > plane_eps:
            trace.append((trial, tn, tl, "plane_eps"))
            stop = "plane_eps"
            break
        trace.append((trial, tn, tl, "taken"))
        cur, n, lam = trial, tn, tl
    return cur, stop, trace


# ---- the factor, point by point ------------------------------------------------------------------------------------------------------------
def _world(frames, poses):
    q, J, owner = [], [], []
    for f, (p, T) in enumerate(zip(frames, poses)):
        p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
        R, t = np.asarray(T)[:3, :3], np.asarray(T)[:3, 3]
        q.append(p @ R.T + t)
        for pi in p:
            J.append(np.hstack([-R @ hat(pi), R]))
        owner += [f] * len(p)
    return np.concatenate(q), np.array(J), np.array(owner)


def eigh_pairs(C):
    lam, V = np.linalg.eigh(C)
    return lam, V


def _single(frames, poses, e, eig):
    q, J, owner = _world(frames, poses)
    N, K = len(q), len(frames)
    m = q.mean(axis=0)
    d = q - m
    C = d.T @ d / N
    lam, V = eig(C)
    ue = V[:, e]
    a = d @ ue
    x = np.einsum("iab,a->ib", J, ue)  # J_i^T u_e
    g = np.zeros(6 * K)
    H = np.zeros((6 * K, 6 * K))
    X = np.zeros((K, 6))
    scale = 0.0  # the largest entry of sum_i |J_i^T (2 / N) a_i u_e|: the size of what is added up, whatever cancels in the sum
    for f in range(K):
        sel = owner == f
        g[6 * f : 6 * f + 6] = (2.0 / N) * (a[sel, None] * x[sel]).sum(axis=0)
        scale = max(scale, ((2.0 / N) * np.abs(a[sel, None] * x[sel]).sum(axis=0)).max())
        H[6 * f : 6 * f + 6, 6 * f : 6 * f + 6] += (2.0 / N) * np.einsum("ia,ib->ab", x[sel], x[sel])
        X[f] = x[sel].sum(axis=0)
    Hs = np.abs(H) + (2.0 / N**2) * np.outer(np.abs(X).reshape(-1), np.abs(X).reshape(-1))  # the sizes of H's parts, as `scale` for g
    H -= (2.0 / N**2) * np.outer(X.reshape(-1), X.reshape(-1))
    for k in range(3):
        if k == e:
            continue
        uk = V[:, k]
        b = d @ uk
        w = a[:, None] * np.einsum("iab,a->ib", J, uk) + b[:, None] * x
        W = np.array([w[owner == f].sum(axis=0) for f in range(K)]).reshape(-1)
        H += (2.0 / N**2) / (lam[e] - lam[k]) * np.outer(W, W)
        Hs += np.abs((2.0 / N**2) / (lam[e] - lam[k])) * np.outer(np.abs(W), np.abs(W))
    return lam[e], g, H, lam, (scale, Hs.max())


def factor(frames, poses, kind=0, eig=eigh_pairs):
    """-> {cost, g, H, eigenvalues}; frames: K arrays of frame-local points, poses: K 4 x 4"""
    cost, g, H, lam, scale = _single(frames, poses, 0, eig)
    if kind == 1:
        c1, g1, H1, _, s1 = _single(frames, poses, 1, eig)
        cost, g, H, scale = cost + c1, g + g1, H + H1, (scale[0] + s1[0], scale[1] + s1[1])
    tiny = np.finfo(np.float64).tiny  # (an exactly planar selection has a_i = 0: every term of g is zero)
    return {"cost": cost, "g": g, "H": H, "eigenvalues": lam, "g_scale": max(scale[0], tiny), "H_scale": max(scale[1], tiny)}


def factor_pairs(frames, poses, e=0, eig=eigh_pairs):
    """the double sum over point pairs, literally (small N)"""
    q, J, owner = _world(frames, poses)
    N, K = len(q), len(frames)
    m = q.mean(axis=0)
    d = q - m
    lam, V = eig(d.T @ d / N)
    ue = V[:, e]
    a = d @ ue
    g = np.zeros(6 * K)
    H = np.zeros((6 * K, 6 * K))
    for i in range(N):
        fi = owner[i]
        g[6 * fi : 6 * fi + 6] += J[i].T @ ((2.0 / N) * a[i] * ue)
        for j in range(N):
            fj = owner[j]
            Hij = (2.0 / N) * ((1.0 if i == j else 0.0) - 1.0 / N) * np.outer(ue, ue)
            for k in range(3):
                if k == e:
                    continue
                uk = V[:, k]
                bik, bjk = d[i] @ uk, d[j] @ uk
                Hij += (2.0 / N**2) / (lam[e] - lam[k]) * np.outer(a[i] * uk + bik * ue, bjk * ue + a[j] * uk)
            H[6 * fi : 6 * fi + 6, 6 * fj : 6 * fj + 6] += J[i].T @ Hij @ J[j]
    return {"cost": lam[e], "g": g, "H": H, "eigenvalues": lam}


def numeric_gradient(frames, poses, kind=0, h=1e-6):
    """central differences of the cost under T Exp(xi)"""
    K = len(frames)
    g = np.zeros(6 * K)

    def cost(ps):
        q, _, _ = _world(frames, ps)
        d = q - q.mean(axis=0)
        lam = np.linalg.eigvalsh(d.T @ d / len(q))
        return lam[0] if kind == 0 else lam[0] + lam[1]

    for f in range(K):
        for a in range(6):
            xi = np.zeros(6)
            xi[a] = h
            plus = [T @ se3_exp(xi) if i == f else T for i, T in enumerate(poses)]
            minus = [T @ se3_exp(-xi) if i == f else T for i, T in enumerate(poses)]
            g[6 * f + a] = (cost(plus) - cost(minus)) / (2 * h)
    return g


def factor_gates(frames, poses, kind, oracle_eig):
    """the gates of the docstring for one (frames, poses): {g, H, cost, condition}"""
    ref = factor(frames, poses, kind)
    alt = factor(frames, poses, kind, eig=oracle_eig)
    lam = ref["eigenvalues"]
    gap = (lam[1] - lam[0]) if kind == 0 else (lam[2] - lam[1])
    dg = np.abs(ref["g"] - alt["g"]).max() / ref["g_scale"]
    dH = np.abs(ref["H"] - alt["H"]).max() / ref["H_scale"]
    q, _, _ = _world(frames, poses)
    qq = q - q[0]
    bq, bqq = sum_bounds(qq)
    N = len(q)
    dC = np.linalg.norm((bqq + 2 * np.outer(np.abs(qq.mean(axis=0)), bq)) / N)
    share = 16 * dC / gap
    return {"g": 8 * dg + share, "H": 8 * dH + share, "cost": 8 * np.abs(alt["eigenvalues"] - lam).max() + dC, "condition": lam[2] / gap,
            "solver_g": dg, "solver_H": dH, "sum_share": share}


# ---- the scene of the GPU test -------------------------------------------------------------------------------------------------------------
CENTER = np.array([20.5, -13.25, 3.0])


def make_scene(seed=7, line=False):
    """S = 4 clouds of 1, 257, 1000 and 0 points from a 2 cm slab through CENTER plus clutter (line=True: a 2 cm rod instead, for the edge
    kind); poses with translations of order 20 m, cloud 1 under the identity so that its point 0, CENTER + (1, 0, 0), has q.q == 1 exactly.
    Clouds 0, 1 and 3 are FP64 clouds; cloud 2 is an FP32 cloud (its points are rounded here, as clone() rounds them)."""
    rng = np.random.default_rng(seed)
    n = np.array([0.3, -0.2, 0.93])
    n /= np.linalg.norm(n)
    e1 = np.cross(n, [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(n, e1)
    sizes = [1, 257, 1000, 0]
    poses = [se3_exp([0.3, -0.2, 0.5, 18.0, -22.0, 4.0]), np.eye(4), se3_exp([-0.4, 0.1, 1.2, -21.0, 15.0, -3.0]), se3_exp([0.1, 0.2, 0.3, 19.0, 20.0, 1.0])]
    clouds = []
    for s, (k, T) in enumerate(zip(sizes, poses)):
        ab = rng.uniform(-1.3, 1.3, size=(k, 2))
        if line:
            ab[:, 1] = rng.uniform(-0.01, 0.01, size=k)
        z = rng.uniform(-0.01, 0.01, size=k)
        w = CENTER + ab[:, :1] * e1 + ab[:, 1:] * e2 + z[:, None] * n
        clutter = rng.random(k) < 0.1
        if not line:
            w[clutter] = CENTER + rng.uniform(-1.3, 1.3, size=(int(clutter.sum()), 3))
        if s == 0:
            w = CENTER + np.array([[0.25, 0.125, 0.0]])  # the one-point cloud's point lies inside the ball
        p = (w - T[:3, 3]) @ T[:3, :3]
        if s == 1:
            p[0] = CENTER + np.array([1.0, 0.0, 0.0])
        if s == 2:
            p = p.astype(np.float32).astype(np.float64)
        clouds.append(p.reshape(-1, 3))
    return clouds, poses


# ---- helpers of the C++ programs under tests/cpp ---------------------------------------------------------------------------------------------
def write_problem(path, frames, poses, kind):
    """kind K n | n lines "frame x y z" | K lines of 12 pose entries: the input of test_plane_ba_host.cpp and test_plane_ba_drop_in.cpp"""
    with open(path, "w") as f:
        f.write(f"{kind} {len(frames)} {sum(len(p) for p in frames)}\n")
        for s, p in enumerate(frames):
            for x in p:
                f.write(f"{s} {float(x[0])!r} {float(x[1])!r} {float(x[2])!r}\n")
        for T in poses:
            f.write(" ".join(repr(float(v)) for v in np.asarray(T)[:3, :4].reshape(12)) + "\n")


def build_drop_in(tmp_path):
    """tests/cpp/test_plane_ba_drop_in.cpp over the drop-in include tree; tests/cpp/plane_ba_standin (the N-key HessianFactor) goes in front of
    the stand-in third-party headers (which are not warning-clean: -w)"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_plane_ba_drop_in")
    inc = [os.path.join(root, "tests", "cpp", "plane_ba_standin"), os.path.join(root, "adapters", "gtsam_points_hip"), os.path.join(root, "adapters", "gtsam"),
           os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "glim_standin")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-w"] + ["-I" + d for d in inc] + [os.path.join(root, "tests", "cpp", "test_plane_ba_drop_in.cpp"), "-o", exe,
                           "-L" + os.path.join(root, "glim_amd"), "-lglim_amd", "-Wl,-rpath," + os.path.join(root, "glim_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-L/opt/rocm/lib", "-lamdhip64"])
    return exe
