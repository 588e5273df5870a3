"""The continuous-time part of tests/record_slots.py proven on the CPU: ct_record in FP64 against the oracle path (ct_restatement.np_ct_linearize),
the FP32 restatement added in the shape of the device's reduction against the gate, and the gate against the errors a CT kernel can make around
the per-point algebra.  The cases are those of tests/test_gpu_ct_record_slots.py (tests/ct_record_cases.py), with covariances from the oracle
(orc.knn, orc.covariances) and the matched set from the oracle's search.

Figures of one run (the tests print them; -s shows them) are in the docstrings of the tests.
"""
import numpy as np
import pytest

import ct_record_cases as cc
import ct_restatement as ctg
import record_slots as rs

S = rs.additions(1)


@pytest.fixture(scope="module")
def world(orc):
    """the target and the 4096-point scan with oracle covariances, every array holding FP32 values"""
    f32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)  # noqa: E731
    tp = ctg.static_map(16, 512)
    p, _ = ctg.moving_source(16, 256)
    p = f32(p)
    return dict(tp=tp, tc=f32(orc.covariances(tp, orc.knn(tp, 10))[1]), p=p, covs=f32(orc.covariances(p, orc.knn(p, 10))[1]))


@pytest.fixture(scope="module")
def built(orc, world):
    """name -> everything a test needs of a case, computed once: the scene, the pose tables, the oracle path's record and matched set, the
    terms in both precisions"""
    cache = {}

    def get(name):
        if name not in cache:
            case = cc.cases()[name]
            sc = cc.scene(case, world["tp"], world["tc"], world["p"], world["covs"])
            table, idx = ctg.time_table(case["times"])
            T, D0, D1 = ctg.ct_poses(table, case["X"], case["Y"])
            ref = ctg.np_ct_linearize(orc, sc["tp"], sc["tc"], sc["sp"], sc["sc"], case["times"], case["X"], case["Y"], 1.0, poses=(T, D0, D1))
            m = rs.ct_matched(sc, ref["corr"], idx)
            cache[name] = dict(case=case, sc=sc, idx=idx, T=T, D0=D0, D1=D1, ref=ref, m=m, c64=rs.ct_terms(sc, m, np.float64, T), c32=rs.ct_draws(sc, m, T))
        return cache[name]

    return get


NAMES = list(cc.cases())


def test_the_cases_are_what_they_claim(built):
    for name in NAMES:
        b = built(name)
        n = b["case"]["n"]
        assert rs.points_per_thread(n) == 1 and n < 262144  # one point per thread: s = 9
        assert b["ref"]["num_inliers"] > 0, name
    sizes = np.bincount(built("tails")["idx"])
    np.testing.assert_array_equal(sizes, cc.TAILS)
    for k in cc.NBK:
        np.testing.assert_array_equal(np.bincount(built(f"nbk{k}")["idx"]), [3] * k)
    sw = built("sweep")
    assert 80 <= len(sw["T"]) <= 120 and sw["ref"]["num_inliers"] > 1000 and len(set(np.bincount(sw["idx"]).tolist())) > 1
    # the empty bucket matches nothing, the others match what they match in "tails"
    e, t = built("empty-bucket"), built("tails")
    far = np.arange(*e["case"]["far"])
    assert np.all(e["idx"][far] == cc.FAR_BUCKET) and np.all(e["ref"]["corr"][far] == -1) and np.any(t["ref"]["corr"][far] >= 0)
    keep = np.setdiff1d(np.arange(e["case"]["n"]), far)
    np.testing.assert_array_equal(e["ref"]["corr"][keep], t["ref"]["corr"][keep])
    na = built("non-ascending")
    assert np.any(np.diff(na["case"]["times"]) < 0) and len(na["T"]) > 1


@pytest.mark.parametrize("name", NAMES)
def test_fp64_ct_record_agrees_with_the_oracle_path(built, name):
    """ct_record over the FP64 terms equals np_ct_linearize (the oracle's per-bucket GICP records through the chain rule) to 1e-12 of the
    absolute-value sums sum_k |J_k|^T |H_k| |J_k| (as ct_gate forms them)"""
    b = built(name)
    got = rs.ct_record(b["c64"], b["m"]["bucket"], b["D0"], b["D1"])
    want = rs.ct_record_of(b["ref"])
    g = rs.ct_gate(b["c32"], b["c64"], b["m"]["bucket"], b["D0"], b["D1"], S)
    absum = g["fp64"] / (2.0 * (12 + len(b["D0"])) * 2.0 ** -53)
    assert got[0] == want[0] == len(b["m"]["idx"])
    err = np.abs(got - want)[1:]
    assert np.all(err <= 1e-12 * absum[1:]), name  # (entries through D1 = 0 -- one bucket, at t = 0 -- are exactly zero on both sides)
    print(f"{name}: ct_record against the oracle path: at most {np.max(err[absum[1:] > 0] / absum[1:][absum[1:] > 0]):.2e} of the absolute sums")
    # ... and the two layouts are each other's inverse
    np.testing.assert_array_equal(rs.ct_record_of(rs.ct_dict(got)), got)


def _device_record(c32, b, D0=None, D1=None, sums=None):
    """the FP32 terms added as the device adds them (ct_device_sums), then the chain rule and the bucket sum in FP64"""
    sums = rs.ct_device_sums(c32, b["m"]) if sums is None else sums
    return rs.ct_record_of_bucket_sums(sums, len(c32), b["D0"] if D0 is None else D0, b["D1"] if D1 is None else D1)


def test_fp32_restatement_stays_within_the_gate(built):
    """The condition that the inputs were chosen well: on every GPU case the FP32 restatement, added in the shape of the device's reduction per
    bucket block, stays within the m = 2 gate on all 92 entries.  Measured: at most 0.43 of the gate (H9_11 of nbk8: 22 pairs in 8 buckets),
    0.33 on the non-ascending times, 0.13 on the bucket tails, 0.05 on the sweep."""
    for name in NAMES:
        b = built(name)
        g = rs.ct_gate(b["c32"], b["c64"], b["m"]["bucket"], b["D0"], b["D1"], S)
        rec = _device_record(b["c32"][0], b)
        rs.ct_check(rec, g, name)
        frac = np.abs(rec - g["S"])[1:] / np.where(g["gate"][1:] > 0, g["gate"][1:], 1.0)
        j = int(frac.argmax()) + 1
        print(f"{name:14s} FP32 restatement / gate(m = 2): at most {frac.max():.3f} on {rs.CT_NAMES[j]}")


def _old_rule_catches(rec, ref):
    try:
        ctg._check_record(rs.ct_dict(rec), rs.ct_dict(ref))
    except AssertionError:
        return True
    return False


def _mutations(built):
    """(name, case, the mutated device record) -- the FP32 restatement with one error of the code AROUND the per-point algebra"""
    out = []
    # (a) the last point of a bucket evaluated at the next bucket's pose
    b = built("sweep")
    k = 84
    row = int(np.flatnonzero(b["m"]["bucket"] == k)[-1])
    Tm = b["T"][b["m"]["bucket"]].copy()
    Tm[row] = b["T"][k + 1]
    c = b["c32"][0].copy()
    c[row] = rs.gicp(b["m"]["p"][row:row + 1], b["m"]["CA"][row:row + 1], b["m"]["b"][row:row + 1], b["m"]["CB"][row:row + 1], Tm[row], np.float32)[0]
    out.append(("(a) last point of a bucket at the next bucket's pose", "sweep", _device_record(c, b)))
    # (b) the first point of the second block of the three-block bucket (513 points) dropped
    b = built("tails")
    k = cc.TAILS.index(513)
    first = int(np.sum(cc.TAILS[:k])) + 256
    row = int(np.flatnonzero(b["m"]["idx"] == first)[0])  # (the point is matched: asserted by the lookup)
    c = b["c32"][0].copy()
    c[row] = 0.0
    rec = _device_record(c, b)
    out.append(("(b) first point of a block in a three-block bucket dropped (the count kept)", "tails", rec))
    # (c) .. (f): the bucket pass and the sum
    b = built("sweep")
    k = len(b["D0"]) // 2
    D0, D1 = b["D0"].copy(), b["D1"].copy()
    D0[k], D1[k] = b["D1"][k], b["D0"][k]
    out.append(("(c) D0 and D1 swapped in one bucket", "sweep", _device_record(b["c32"][0], b, D0, D1)))
    D1 = b["D1"].copy()
    D1[82][1, 1] *= 1.0 + 1e-3
    out.append(("(d) one entry of one D1 scaled by 1 + 1e-3", "sweep", _device_record(b["c32"][0], b, D1=D1)))
    c = b["c32"][0].copy()
    sel = b["m"]["bucket"] == k
    mm = {key: (v[sel] if isinstance(v, np.ndarray) and len(v) == len(sel) else v) for key, v in b["m"].items()}
    c[sel] = rs.gicp(mm["p"], mm["CA"], mm["b"], mm["CB"], b["T"][k + 1], np.float32)
    D0, D1 = b["D0"].copy(), b["D1"].copy()
    D0[k], D1[k] = b["D0"][k + 1], b["D1"][k + 1]
    out.append(("(e) one bucket at t_{k+1} in place of t_k", "sweep", _device_record(c, b, D0, D1)))
    sums = rs.ct_device_sums(b["c32"][0], b["m"])
    last = sums[-1].copy()
    sums[-1] = 0.0
    rec = _device_record(b["c32"][0], b, sums=sums)
    rec[0] = len(b["c32"][0])  # (the count is compared with ==: left right, so that the entries are what is tested)
    assert np.any(last)
    out.append(("(f) the last bucket row left out of the sum", "sweep", rec))
    return out


def test_gate_catches_errors_around_the_point_algebra(built):
    """Each mutation pushes at least one of the 92 entries beyond the widest gate the GPU tests may use (m = 8) while the unmutated terms pass
    at m = 2; printed: the worst entry and whether ct_restatement._check_record (2e-4 of the largest entry, the error at rtol 2e-4, the
    Gauss-Newton step) would have caught it.  One run (sweep: 86 buckets; tails: 9):
      (a) last point of bucket 84 at the next bucket's pose (sweep)     40 gates on b7        NOT caught by _check_record
      (b) first point of a block in the 513-point bucket dropped        915 gates on H11_11   caught
      (c) D0 and D1 swapped in bucket 43 (sweep)                        624 gates on H0_7     caught
      (d) entry (1, 1) of D1 of bucket 82 scaled by 1 + 1e-3 (sweep)    40 gates on H7_7      NOT caught
      (e) bucket 43 at t_44 (sweep)                                     695 gates on b3       caught
      (f) the last bucket row left out (sweep)                          3863 gates on H7_7    caught
    Where (a) and (d) are put matters: what they change is one point's share of a centimetre and a thousandth of what one D1 entry carries.
    Bucket 84 and entry (1, 1) of bucket 82 are where the sweep shows them best (40 gates); at the sweep's middle (a) stands at 1.8 gates and
    (d), on entry (2, 2), at 0.6: below the gate."""
    unseen = []
    for name, case, rec in _mutations(built):
        b = built(case)
        args = (b["c32"], b["c64"], b["m"]["bucket"], b["D0"], b["D1"], S)
        rs.ct_check(_device_record(b["c32"][0], b), rs.ct_gate(*args), case)
        wide = rs.ct_gate(*args, m=rs.M_MAX)
        over = np.abs(rec - wide["S"])[1:] / wide["gate"][1:]
        j = int(over.argmax()) + 1
        old = _old_rule_catches(rec, wide["S"])
        print(f"{name:76s} trips {rs.CT_NAMES[j]:7s} at {over.max():10.1f} gates (m = 8); _check_record: {'caught' if old else 'NOT caught'}")
        assert over.max() > 1.0, name
        if not old:
            unseen.append(name[:3])
    assert {"(a)", "(d)"} <= set(unseen), unseen


def test_frozen_gate_catches_a_wrong_kept_metric(built):
    """ct_error_kernel's term per kept pair, at the evaluation poses of the GPU tests: (g) the kept M left in the source frame, (h) M made
    with the evaluation pose's rotation.  Against the m = 8 gate of slot 27; the old rule is rtol = 2e-4 on the error.  One run:
      sweep (R_k: a yaw of 10 to 15 degrees)         (g) 4935 gates, caught by the old rule     (h) 59 gates, caught
      registered (R_k a milliradian from I)          (g) 53 gates, NOT caught (1.3e-4 of e)     (h) 421 gates, caught"""
    unseen = []
    for case in ("sweep", "registered"):
        b = built(case)
        Xe, Ye = cc.moved(b["case"]["X"], b["case"]["Y"])
        Te = ctg.ct_poses(ctg.time_table(b["case"]["times"])[0], Xe, Ye)[0]
        e64 = rs.ct_frozen_terms(b["m"], b["T"], Te, np.float64)
        e32 = rs.ct_frozen_draws(b["m"], b["T"], Te)
        g2, g8 = rs.error_gate(e32, e64, S), rs.error_gate(e32, e64, S, m=rs.M_MAX)
        dev = lambda e: float(rs.ct_device_sums(np.pad(e[:, None], ((0, 0), (27, 0))), b["m"])[:, 27].sum())  # noqa: E731
        assert abs(dev(e32[0]) - g2["S"]) <= g2["gate"]
        for name, kw in (("(g) kept M left in the source frame", dict(rotate=False)), ("(h) M with the evaluation pose's rotation", dict(R_from_eval=True))):
            bad = dev(rs.ct_frozen_terms(b["m"], b["T"], Te, np.float32, **kw))
            over = abs(bad - g8["S"]) / g8["gate"]
            old = abs(bad - g8["S"]) > 2e-4 * abs(g8["S"])
            print(f"{case}: {name:44s} {over:10.1f} gates (m = 8); rtol 2e-4 on the error: {'caught' if old else 'NOT caught'}")
            assert over > 1.0, name
            if not old:
                unseen.append(name[:3])
    assert unseen == ["(g)"], unseen  # on the scan that barely rotates
