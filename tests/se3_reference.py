"""SE(3) in multiprecision (mpmath) with gtsam::Pose3's right-perturbation conventions: the reference of tests/golden/make_golden_se3.py and
tests/test_se3_range.py for what glim_amd/csrc/ct_se3.hpp computes in FP64.  Tangents are (omega, v), poses 3 x 4 (rows of [R | t]), 6 x 6
matrices [[A, 0], [B, A]].  Everything is a nested list of mpf; every public function takes the working precision in bits (200 by default;
53 is double arithmetic, correctly rounded operation by operation, on these same formulas).

Written from the definitions, not from the header: the scalar coefficients are their power series below 1 rad and closed forms above, the
lower-left block Q of the Jacobian is the double power series sum_{n,m} (-1)^(n+m+1) W^n V W^m / (n+m+2)! (entire in omega, no cancelling
closed form anywhere), inverses are linear solves.  Log takes the angle from atan2(|vee|, (tr - 1) / 2) and the axis from R - R^T while
cos(theta) >= -1/2, beyond that from the symmetric part (R + R^T) / 2 - cos(theta) I = (1 - cos(theta)) n n^T, whose largest column is
well conditioned up to the half turn; its sign is that of vee, and at an exact half turn (vee = 0) the first non-zero component is positive.
A plain module: it holds no tests."""
from mpmath import mp, mpf

PREC = 200


# ---- small dense helpers on nested lists -------------------------------------------------------------------------------------------------
def _eye(n=3):
    return [[mpf(1) if r == c else mpf(0) for c in range(n)] for r in range(n)]


def _mm(A, B):
    return [[sum((A[r][k] * B[k][c] for k in range(len(B))), mpf(0)) for c in range(len(B[0]))] for r in range(len(A))]


def _mv(A, x):
    return [sum((A[r][k] * x[k] for k in range(len(x))), mpf(0)) for r in range(len(A))]


def _tr(A):
    return [[A[c][r] for c in range(len(A))] for r in range(len(A[0]))]


def _lin(*terms):
    """sum of s * M over (s, M)"""
    M0 = terms[0][1]
    return [[sum((s * M[r][c] for s, M in terms), mpf(0)) for c in range(len(M0[0]))] for r in range(len(M0))]


def _neg(A):
    return [[-x for x in row] for row in A]


def _inv(A):
    return (mp.matrix(A) ** -1).tolist()


def hat(w):
    return [[mpf(0), -w[2], w[1]], [w[2], mpf(0), -w[0]], [-w[1], w[0], mpf(0)]]


def _norm(w):
    return mp.sqrt(sum((x * x for x in w), mpf(0)))


def _alt_series(t2, k0):
    """sum_{k >= 0} (-1)^k t2^k / (2 k + k0)!"""
    term, total, k = mpf(1) / mp.factorial(k0), mpf(0), 0
    tiny = mpf(2) ** (-mp.prec - 16)
    while True:
        total += term
        k += 1
        term = -term * t2 / ((2 * k + k0 - 1) * (2 * k + k0))
        if abs(term) < tiny * abs(total):
            return total


def _abc(th):
    """sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3"""
    if th < 1:
        t2 = th * th
        return _alt_series(t2, 1), _alt_series(t2, 2), _alt_series(t2, 3)
    return mp.sin(th) / th, (1 - mp.cos(th)) / th**2, (th - mp.sin(th)) / th**3


def _pose(R, t):
    return [list(R[r]) + [t[r]] for r in range(3)]


def _rot(T):
    return [list(T[r][:3]) for r in range(3)]


def _trans(T):
    return [T[r][3] for r in range(3)]


def _block6(A, B):
    Z = [[mpf(0)] * 3 for _ in range(3)]
    return [A[r] + Z[r] for r in range(3)] + [B[r] + A[r] for r in range(3)]


def _mpf_all(x):
    return [_mpf_all(y) for y in x] if hasattr(x, "__len__") else mpf(float(x)) if not isinstance(x, mpf) else x


def _as_pose(T):
    T = _mpf_all(T)
    return [T[4 * r:4 * r + 4] for r in range(3)] if len(T) == 12 else [list(T[r][:4]) for r in range(3)]


# ---- the maps, at the precision in force -------------------------------------------------------------------------------------------------
def _exp(xi):
    w, v = xi[:3], xi[3:]
    a, b, c = _abc(_norm(w))
    W = hat(w)
    W2 = _mm(W, W)
    return _pose(_lin((1, _eye()), (a, W), (b, W2)), _mv(_lin((1, _eye()), (b, W), (c, W2)), v))


def _log_rot(R, flip=False):
    vee = [(R[2][1] - R[1][2]) / 2, (R[0][2] - R[2][0]) / 2, (R[1][0] - R[0][1]) / 2]
    s, cth = _norm(vee), (R[0][0] + R[1][1] + R[2][2] - 1) / 2
    th = mp.atan2(s, cth)
    if cth >= mpf(-1) / 2:
        w = vee if th == 0 else [x * th / mp.sin(th) for x in vee] if th >= 1 else [x / _alt_series(th * th, 1) for x in vee]
    else:
        S = [[(R[r][c] + R[c][r]) / 2 - (cth if r == c else 0) for c in range(3)] for r in range(3)]
        j = max(range(3), key=lambda i: S[i][i])
        n = [S[r][j] for r in range(3)]
        n = [x / _norm(n) for x in n]
        d = sum((x * y for x, y in zip(vee, n)), mpf(0))
        if d < 0 or (d == 0 and [x for x in n if x != 0][0] < 0):
            n = [-x for x in n]
        w = [th * x for x in n]
    return [-x for x in w] if flip else w


def _log(T, flip=False):
    w = _log_rot(_rot(T), flip)
    _, b, c = _abc(_norm(w))
    W = hat(w)
    V = _lin((1, _eye()), (b, W), (c, _mm(W, W)))
    v = mp.lu_solve(mp.matrix(V), mp.matrix(_trans(T)))
    return w + [v[i] for i in range(3)]


def _jr_blocks(xi):
    w, v = xi[:3], xi[3:]
    th = _norm(w)
    _, b, c = _abc(th)
    W, V = hat(w), hat(v)
    Jw = _lin((1, _eye()), (-b, W), (c, _mm(W, W)))
    # Q = sum_k (-1)^(k+1) / (k+2)! S_k, S_k = sum_{n+m=k} W^n V W^m = W S_(k-1) + V W^k
    tiny = mpf(2) ** (-mp.prec - 16)
    S, Wk, Q, k, bound = V, _eye(), _lin((mpf(-1) / 2, V)), 0, mpf(1) / 2
    while bound > tiny:
        k += 1
        Wk = _mm(Wk, W)
        S = _lin((1, _mm(W, S)), (1, _mm(V, Wk)))
        Q = _lin((1, Q), (mpf(-1) ** (k + 1) / mp.factorial(k + 2), S))
        bound = (k + 1) * th**k / mp.factorial(k + 2)
    return Jw, Q


def _jr(xi):
    return _block6(*_jr_blocks(xi))


def _jr_inv(xi):
    Jw, Q = _jr_blocks(xi)
    Ji = _inv(Jw)
    return _block6(Ji, _neg(_mm(Ji, _mm(Q, Ji))))


def _ad(T):
    R = _rot(T)
    return _block6(R, _mm(hat(_trans(T)), R))


def _inverse(T):
    Rt = _tr(_rot(T))
    return _pose(Rt, [-x for x in _mv(Rt, _trans(T))])


def _compose(A, B):
    RA = _rot(A)
    return _pose(_mm(RA, _rot(B)), [x + y for x, y in zip(_mv(RA, _trans(B)), _trans(A))])


# ---- public: precision is a parameter ----------------------------------------------------------------------------------------------------
def to_double(x):
    """rounded once to double, flattened row-major"""
    return [y for row in x for y in to_double(row)] if hasattr(x, "__len__") else [float(x)]


def Exp(xi, prec=PREC):
    with mp.workprec(prec):
        return _exp(_mpf_all(list(xi)))


def Log(T, prec=PREC, flip=False):
    """flip: the other of the two logarithms of a half turn (omega -> -omega)"""
    with mp.workprec(prec):
        return _log(_as_pose(T), flip)


def J_r(xi, prec=PREC):
    with mp.workprec(prec):
        return _jr(_mpf_all(list(xi)))


def J_r_inv(xi, prec=PREC):
    with mp.workprec(prec):
        return _jr_inv(_mpf_all(list(xi)))


def Ad(T, prec=PREC):
    with mp.workprec(prec):
        return _ad(_as_pose(T))


def compose(A, B, prec=PREC):
    with mp.workprec(prec):
        return _compose(_as_pose(A), _as_pose(B))


def inverse(T, prec=PREC):
    with mp.workprec(prec):
        return _inverse(_as_pose(T))


def prior(P, X, prec=PREC, flip=False):
    """r = Log(P^-1 X) and d r / d X = J_r(r)^-1"""
    with mp.workprec(prec):
        r = _log(_compose(_inverse(_as_pose(P)), _as_pose(X)), flip)
        return r, _jr_inv(r)


def between(D, X, Y, prec=PREC, flip=False):
    """r = Log(D^-1 X^-1 Y) and the 6 x 12 [d r / d X | d r / d Y] = [-J_r(r)^-1 Ad((X^-1 Y)^-1) | J_r(r)^-1]"""
    with mp.workprec(prec):
        XY = _compose(_inverse(_as_pose(X)), _as_pose(Y))
        r = _log(_compose(_inverse(_as_pose(D)), XY), flip)
        Ji = _jr_inv(r)
        JX = _neg(_mm(Ji, _ad(_inverse(XY))))
        return r, [JX[m] + Ji[m] for m in range(6)]


def ct_bucket(X, Y, tk, prec=PREC):
    """T_k = X Exp(t_k Log(X^-1 Y)), D0_k = d T_k / d X, D1_k = d T_k / d Y"""
    with mp.workprec(prec):
        X, tk = _as_pose(X), mpf(float(tk))
        delta = _compose(_inverse(X), _as_pose(Y))
        vel = _log(delta)
        xi = [tk * x for x in vel]
        E = _exp(xi)
        G = _lin((tk, _mm(_jr(xi), _jr_inv(vel))))
        D0 = _lin((1, _ad(_inverse(E))), (-1, _mm(G, _ad(_inverse(delta)))))
        return _compose(X, E), D0, G
