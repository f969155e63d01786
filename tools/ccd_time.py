"""Times cd_find_ccd after cd_build_tree on the 1 M cloth (mi355_synth.cloth_pair(500); quad edge ~0.0058) for x1 = x0 and a few
motion magnitudes (mi355_synth.cloth_motion: the sheets approach by --approach quad edges each, plus a wave of the same amplitude),
next to cd_find_proximity at the same distance: host clock around the synchronising call, one warm-up, median of --reps calls;
pair, candidate, gate and evaluation counts.  The per-kernel split comes from a separate run under rocprofv3 --kernel-trace --stats."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpu-computing-course_amd", "pyhost"))

import mi355_synth as synth  # noqa: E402
import mi355cd  # noqa: E402


def _median(fn, reps):
    fn()                                                                    # warm-up (buffers sized)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--quads", type=int, default=500)
    ap.add_argument("--dist", type=float, default=0.001)
    ap.add_argument("--motions", type=str, default="0,0.25,1,4", help="approach = wave amplitude, in quad edges")
    ap.add_argument("--throw", action="store_true", help="also throw one vertex across the mesh")
    a = ap.parse_args()
    verts, vidx = synth.cloth_pair(a.quads)
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        cd.build_tree()
        med, mn, out = _median(lambda: cd.find_proximity(a.dist, cap=1 << 24), a.reps)
        print(json.dumps({"call": "find_proximity", "triangles": int(vidx.shape[0]), "dist": a.dist, "median_ms": round(med, 4),
                          "min_ms": round(mn, 4), "reps": a.reps, "pairs": int(out[2]), "tested": int(cd.proximity_tested)}), flush=True)
        for mo in (float(x) for x in a.motions.split(",")):
            x1 = synth.cloth_motion(verts, approach=mo, wave=mo, throw=a.throw, quads=a.quads)
            med, mn, out = _median(lambda: cd.find_ccd(x1, a.dist, cap=1 << 24), a.reps)
            info = cd.ccd_info
            p, toi, dd, n, rc = out
            print(json.dumps({"call": "find_ccd", "motion_edges": mo, "throw": a.throw, "dist": a.dist, "median_ms": round(med, 4),
                              "min_ms": round(mn, 4), "reps": a.reps, "pairs": int(n), "at_t0": int(np.sum(toi == 0.0)),
                              "candidates": int(info.n_candidates), "tested": int(info.n_tested), "evals": int(info.n_evals),
                              "unresolved": int(info.n_unresolved), "rc": int(rc)}), flush=True)


if __name__ == "__main__":
    main()
