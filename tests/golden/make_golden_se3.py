#!/usr/bin/env python3
"""Generates tests/golden/se3_range.npz: inputs, expected outputs and gates for every routine of glim_amd/csrc/ct_se3.hpp over the whole
range of rotation angles, from tests/se3_reference.py (mpmath).  Needs no GPU.  Run:  python tests/golden/make_golden_se3.py

Per operation <op> of tests/se3_range_cases.py::OPS the table holds <op>_in (doubles), <op>_out (the reference at 200 bits, rounded once to
double), <op>_gate (per case and output block), <op>_band / <op>_tclass (the class of a case: angle band x translation size),
<op>_class_gate (band x translation size x block), <op>_alt_rows / <op>_alt_out (the cases whose rotation is a half turn to within the
rounding of their inputs -- cos(theta) < 0, sin(theta) <= 4 eps -- so that omega is defined up to sign: the outputs of the other logarithm).

Gate: the reference is evaluated a second time at 53 bits (double arithmetic, correctly rounded, on the reference's own formulas); the gate
of a block for a class is 8 x the largest elementwise error of that run against the 200-bit run over the class, and for a case never less
than 8 eps max|expected block|.  A class gate above 1e-9 of the class's largest expected entry refuses the table."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import se3_reference as ref  # noqa: E402
from se3_range_cases import BANDS, EPS, OP, OPS, T_CLASSES, TABLE  # noqa: E402
from mpmath import mp, mpf  # noqa: E402

PI = float(np.pi)
ANGLES = [0.0, 1e-300, 1e-9, 1e-4, np.nextafter(0.02, 0.0), np.nextafter(0.02, 1.0), 0.02, 0.1, 1.0, 2.0, 3.0, PI - 1e-3, PI - 1e-6, PI - 1e-9, PI - 1e-12, PI]
ANGLE_BAND = [0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 2, 2, 2, 3, 3]
AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 1), (1, -2, 3), (-0.61, 0.13, 0.78)]  # normalised at 200 bits
TRANSLATIONS = [(0.0, 0.0, 0.0), (0.4, -0.2, 0.1), (3e3, -2e3, 50.0)]
HALF_TURNS = [np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0])]
CT_TIMES = [0.0, 0.5, 1.0, 1e-3]
PRIOR_P = (0.3, -0.2, 0.5, 1.5, -2.0, 0.7)
BETWEEN_X = (0.1, 0.2, -0.3, 1200.0, -800.0, 30.0)
BETWEEN_D = (0.2, -0.1, 0.4, 1.0, 0.5, -0.3)
CT_X = (0.3, -0.2, 0.5, 12.0, -7.0, 1.5)
EXACT_T = (0.5, -0.25, 0.125)  # of the hand-made half-turn terms: sums with the poses' translations are exact in double


def tangent(axis, angle, v):
    """(angle * axis / |axis|, v): the product at 200 bits, rounded once"""
    with mp.workprec(ref.PREC):
        a = [mpf(x) for x in axis]
        n = mp.sqrt(sum(x * x for x in a))
        return [float(mpf(angle) * x / n) for x in a] + list(v)


def pose_of(xi):
    return ref.to_double(ref.Exp(xi))


def hand_pose(R, t):
    return list(np.hstack([R, np.reshape(t, (3, 1))]).reshape(12))


def tangents():
    return [(tangent(ax, th, v), ANGLE_BAND[i], c) for ax in AXES for i, th in enumerate(ANGLES) for c, v in enumerate(TRANSLATIONS)]


def cases(op):
    """-> [(input doubles, band, translation class)] of an operation, in the table's order"""
    if op in ("exp", "jr", "jr_inv"):
        return tangents()
    if op in ("log", "ad"):
        return [(pose_of(xi), b, c) for xi, b, c in tangents()] + [(hand_pose(H, t), 3, c) for H in HALF_TURNS for c, t in enumerate(TRANSLATIONS)]
    # the terms and the bucket poses: residual translations of the two non-zero sizes in turn (a residual that is zero next to poses a
    # kilometre out has no scale of its own to hold a gate against)
    cycled = [(tangent(ax, th, TRANSLATIONS[1 + (i + j) % 2]), ANGLE_BAND[i], 1 + (i + j) % 2) for j, ax in enumerate(AXES) for i, th in enumerate(ANGLES)]
    eye = hand_pose(np.eye(3), (0, 0, 0))
    if op == "prior":
        P = pose_of(PRIOR_P)
        out = [(P + ref.to_double(ref.compose(P, ref.Exp(xi))), b, c) for xi, b, c in cycled]
        return out + [(eye + hand_pose(H, EXACT_T), 3, 1) for H in HALF_TURNS]
    if op == "between":
        X, D = pose_of(BETWEEN_X), pose_of(BETWEEN_D)
        XD = ref.compose(X, D)
        out = [(D + X + ref.to_double(ref.compose(XD, ref.Exp(xi))), b, c) for xi, b, c in cycled]
        X0 = hand_pose(np.eye(3), (1e3, -2e3, 50.0))
        return out + [(eye + X0 + hand_pose(H, np.add((1e3, -2e3, 50.0), EXACT_T)), 3, 1) for H in HALF_TURNS]
    assert op == "ct"
    X = pose_of(CT_X)
    out = []
    for j, ax in enumerate(AXES):
        for i, th in enumerate(ANGLES):
            if th <= 1.0:
                Y = ref.to_double(ref.compose(X, ref.Exp(tangent(ax, th, TRANSLATIONS[1 + (i + j) % 2]))))
                out += [(X + Y + [tk], ANGLE_BAND[i], 1 + (i + j) % 2) for tk in CT_TIMES]
    return out


def evaluate(op, x, prec=ref.PREC, flip=False):
    """the reference's outputs of one case as a flat list of mpf, in the layout of the header's outputs"""
    flat = lambda M: [y for row in M for y in row]  # noqa: E731
    if op == "exp":
        return flat(ref.Exp(x, prec))
    if op == "log":
        return ref.Log(x, prec, flip)
    if op == "jr":
        return flat(ref.J_r(x, prec))
    if op == "jr_inv":
        return flat(ref.J_r_inv(x, prec))
    if op == "ad":
        return flat(ref.Ad(x, prec))
    if op == "prior":
        r, J = ref.prior(x[:12], x[12:], prec, flip)
        return r + flat(J)
    if op == "between":
        r, J = ref.between(x[:12], x[12:24], x[24:], prec, flip)
        return r + flat(J)
    T, D0, D1 = ref.ct_bucket(x[:12], x[12:24], x[24], prec)
    return flat(T) + flat(D0) + flat(D1)


def residual_pose(op, x):
    """the pose whose logarithm the operation takes (None: it takes none whose sign can be open)"""
    if op == "log":
        return x
    if op == "prior":
        return ref.compose(ref.inverse(x[:12]), x[12:])
    if op == "between":
        return ref.compose(ref.inverse(x[:12]), ref.compose(ref.inverse(x[12:24]), x[24:]))
    return None


def sign_open(op, x):
    """cos(theta) < 0 and sin(theta) <= 4 eps: R - R^T is within the rounding of the double inputs, which therefore do not determine the sign of omega"""
    E = residual_pose(op, x)
    if E is None:
        return False
    with mp.workprec(ref.PREC):
        E = ref._as_pose(E)
        vee = [(E[2][1] - E[1][2]) / 2, (E[0][2] - E[2][0]) / 2, (E[1][0] - E[0][1]) / 2]
        return E[0][0] + E[1][1] + E[2][2] < 1 and mp.sqrt(sum(v * v for v in vee)) <= 4 * EPS


def expected(op, x):
    """-> (outputs rounded once to double, those of the other logarithm or None)"""
    out = [float(v) for v in evaluate(op, x)]
    return out, ([float(v) for v in evaluate(op, x, flip=True)] if sign_open(op, x) else None)


def build(op, log=print):
    _, n_in, n_out, blocks, names = OP[op]
    cs = cases(op)
    X = np.array([c[0] for c in cs], dtype=np.float64).reshape(len(cs), n_in)
    band, tcls = np.array([c[1] for c in cs], dtype=np.int8), np.array([c[2] for c in cs], dtype=np.int8)
    out, err53, alt_rows, alt_out = np.zeros((len(cs), n_out)), np.zeros((len(cs), len(blocks))), [], []
    for k, x in enumerate(X):
        hi = evaluate(op, list(x))
        lo = evaluate(op, list(x), 53)
        out[k] = [float(v) for v in hi]
        cand = [hi]
        if sign_open(op, list(x)):
            other = evaluate(op, list(x), flip=True)
            alt_rows.append(k)
            alt_out.append([float(v) for v in other])
            cand.append(other)
        with mp.workprec(ref.PREC):
            per = [[max(float(abs(lo[i] - c[i])) for i in idx) for idx in blocks] for c in cand]
        err53[k] = min(per, key=max)
    scale = np.stack([np.abs(out[:, idx]).max(axis=1) for idx in blocks], axis=1)
    class_gate = np.zeros((len(BANDS), len(T_CLASSES), len(blocks)))
    gate = np.zeros((len(cs), len(blocks)))
    for b in range(len(BANDS)):
        for c in range(len(T_CLASSES)):
            sel = (band == b) & (tcls == c)
            if not sel.any():
                continue
            class_gate[b, c] = np.maximum(8.0 * err53[sel].max(axis=0), 8.0 * EPS * scale[sel].max(axis=0))
            over = class_gate[b, c] > 1e-9 * scale[sel].max(axis=0)
            if over.any():
                raise SystemExit(f"{op}: gate {class_gate[b, c][over]} of block {np.array(names)[over]} in class ({BANDS[b]}; {T_CLASSES[c]}) is above 1e-9 of its scale")
            gate[sel] = np.maximum(8.0 * err53[sel].max(axis=0), 8.0 * EPS * scale[sel])
            log(f"{op:8s} {BANDS[b]:24s} {T_CLASSES[c]:12s} " + " ".join(f"{n}={g:.2g}" for n, g in zip(names, class_gate[b, c])))
    return {op + "_in": X, op + "_out": out, op + "_gate": gate, op + "_band": band, op + "_tclass": tcls, op + "_class_gate": class_gate,
            op + "_alt_rows": np.array(alt_rows, dtype=np.int32), op + "_alt_out": np.array(alt_out, dtype=np.float64).reshape(len(alt_rows), n_out)}


def e2e_starts():
    return np.array([hand_pose(HALF_TURNS[2], (0, 0, 0)), pose_of(tangent(AXES[7], PI - 1e-9, (0.0, 0.0, 0.0)))])


def e2e(tab):
    """the end-to-end scenes of se3_range_cases.chain_scene / huber_scene: the cost r^T L r of the first evaluation at 200 bits (all terms, and
    the prior alone), and the s =
    sqrt(r^T L r) of the lone Huber between; their gates are the terms' gates (last angle band, |t| ~ 0.5) through d(r^T L r) = 2 L r . dr with
    |dr| <= sqrt(3) gate per block, plus 8 eps of the value for the sums"""
    import se3_range_cases as sc

    starts = e2e_starts()
    cost, gate, pcost, pgate = np.zeros(2), np.zeros(2), np.zeros(2), np.zeros(2)
    with mp.workprec(ref.PREC):
        for i, start in enumerate(starts):
            priors, betweens, X0 = sc.chain_scene(3, start)
            terms = [("prior", ref.prior(priors[0][1], X0[0])[0])] + [("between", ref.between(D, X0[a], X0[b])[0]) for a, b, D, _ in betweens]
            total, g = mpf(0), mpf(0)
            for op, r in terms:
                g_w, g_v = tab[op + "_class_gate"][3, 1, :2]
                total += sc.E2E_PRECISION * sum(x * x for x in r)
                g += 2 * sc.E2E_PRECISION * mp.sqrt(3) * (mp.sqrt(sum(x * x for x in r[:3])) * g_w + mp.sqrt(sum(x * x for x in r[3:])) * g_v)
                if op == "prior":
                    pcost[i], pgate[i] = float(total), float(g + 8 * EPS * total)
            cost[i], gate[i] = float(total), float(g + 8 * EPS * total)
        _, betweens, _, X0 = sc.huber_scene(starts[0])
        r = ref.between(betweens[0][2], X0[0], X0[1])[0]
        s = mp.sqrt(sc.E2E_PRECISION * sum(x * x for x in r))
        g_w, g_v = tab["between_class_gate"][3, 1, :2]
        s_gate = mp.sqrt(sc.E2E_PRECISION) * mp.sqrt(3) * (g_w + g_v) + 8 * EPS * s
        out = {"e2e_start": starts, "e2e_cost": cost, "e2e_cost_gate": gate, "e2e_prior_cost": pcost, "e2e_prior_gate": pgate, "e2e_huber_s": np.array([float(s), float(s_gate)])}
    print("e2e: cost", cost, "gate", gate, "of which the prior", pcost, "gate", pgate, "huber s, gate", out["e2e_huber_s"])
    return out


def main():
    tab = {}
    for _, op, *_ in OPS:
        tab.update(build(op))
        print(f"{op}: {len(tab[op + '_in'])} cases, {len(tab[op + '_alt_rows'])} with an open sign", flush=True)
    tab.update(e2e(tab))
    np.savez_compressed(TABLE, **tab)
    print(f"wrote {TABLE}: {os.path.getsize(TABLE)} bytes")


if __name__ == "__main__":
    main()
