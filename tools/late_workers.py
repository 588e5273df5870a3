#!/usr/bin/env python3
"""Who is late in a single-factor resident session: the workers that share a compute unit with a finalising block against all workers.

  python tools/late_workers.py <tail_probe.json> [<tail_probe.json> ...] > profiles/r12/probe/late_workers.json

Input: files of tools/resident_tail_probe.py.  Per run: which worker blocks sit on a compute unit that also holds a finalising block (equal `cu`),
their "loop left", "row computed" and "row published" stamps beside the quartiles of all workers, and whether the run's last worker -- the one the
record waits for -- is one of them."""
import json
import sys

import numpy as np

STAMPS = ("loop_left", "row_computed", "row_published")


def run_report(run):
    b = {k: np.asarray(v) for k, v in run["blocks"].items()}
    w = b["worker"].astype(bool)
    cu = b["cu"]
    co = w & np.isin(cu, np.unique(cu[~w]))
    last = int(np.argmax(np.where(w, b["row_published"], -1.0)))
    out = {"blocks": int(len(w)), "workers": int(w.sum()), "compute_units_used": int(len(np.unique(cu))), "co_resident_workers": np.nonzero(co)[0].tolist(),
           "last_worker": last, "last_worker_is_co_resident": bool(co[last])}
    for s in STAMPS:
        v = b[s]
        q = np.percentile(v[w], [0, 25, 50, 75, 100])
        out[s] = {"all_workers_min_q1_median_q3_max": [round(float(x), 2) for x in q], "co_resident": [round(float(x), 2) for x in v[co]],
                  "co_resident_median": round(float(np.median(v[co])), 2) if co.any() else None,
                  "others_max": round(float(v[w & ~co].max()), 2) if (w & ~co).any() else None}
    out["co_resident_median_published_beyond_upper_quartile"] = bool(co.any() and np.median(b["row_published"][co]) > np.percentile(b["row_published"][w], 75))
    return out


def main():
    reports = []
    for path in sys.argv[1:]:
        d = json.load(open(path))
        for i, run in enumerate(d["runs"]):
            r = run_report(run)
            r.update(file=path.split("/")[-1], run=i, lib=d.get("lib"))
            reports.append(r)
    n_last = sum(r["last_worker_is_co_resident"] for r in reports)
    n_q = sum(r["co_resident_median_published_beyond_upper_quartile"] for r in reports)
    json.dump({"what": "microseconds after the leader block saw the pose; a worker is co-resident when its compute unit (XCC_ID and the CU / SA / SE bits of "
                       "HW_ID) also holds a finalising block of the session",
               "runs": reports, "runs_whose_last_worker_is_co_resident": n_last, "runs_with_co_resident_median_published_beyond_q3": n_q, "of": len(reports)},
              sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
