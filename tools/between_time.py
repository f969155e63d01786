"""Times the queries between two meshes (cd_find_collisions_between, cd_find_proximity_between, cd_find_ccd_between) on the two sheets of
mi355_synth.cloth_pair(500) (2 x 500 k triangles; quad edge ~0.0058) as two contexts, both trees built beforehand: host clock around the
synchronising call, one warm-up, median of --reps calls.  Contact; proximity per distance; CCD at each distance with cloth_motion's x1
for both sheets (both moving) and for sheet A only (B static).  For comparison, cd_find_proximity(0) and cd_self_collide on the merged 1 M
mesh in the same process.  The per-kernel split comes from a separate run under rocprofv3 --kernel-trace --stats."""
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
    return round(float(np.median(ts)), 4), round(float(np.min(ts)), 4), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--quads", type=int, default=500)
    ap.add_argument("--dists", type=str, default="0,0.0005,0.001")
    ap.add_argument("--motion", type=float, default=0.25, help="cloth_motion approach = wave amplitude, in quad edges")
    ap.add_argument("--no-merged", action="store_true")
    a = ap.parse_args()
    verts, vidx = synth.cloth_pair(a.quads)
    nt, half = vidx.shape[0], verts.shape[0] // 2
    na = nt // 2
    x1 = synth.cloth_motion(verts, approach=a.motion, wave=a.motion, quads=a.quads)
    cap = 1 << 24
    if not a.no_merged:
        with mi355cd.CollisionDetector(verts, vidx) as m:
            m.build_tree()
            med, mn, out = _median(lambda: m.find_proximity(0.0, cap=cap), a.reps)
            print(json.dumps({"call": "merged find_proximity", "triangles": nt, "dist": 0.0, "median_ms": med, "min_ms": mn,
                              "pairs": int(out[2]), "tested": int(m.proximity_tested)}), flush=True)
    with mi355cd.CollisionDetector(verts[:half], vidx[:na]) as A, \
            mi355cd.CollisionDetector(verts[half:], (vidx[na:] - half).astype(np.uint32)) as B:
        A.build_tree(); B.build_tree()
        for first, second, tag in ((A, B, "a=A"), (B, A, "a=B")):
            med, mn, out = _median(lambda: first.find_collisions_between(second, cap=cap), a.reps)
            print(json.dumps({"call": "find_collisions_between", "roles": tag, "triangles": [first.nt, second.nt], "median_ms": med,
                              "min_ms": mn, "pairs": int(out[1]), "tested": int(first.between_tested), "reps": a.reps}), flush=True)
        for d in (float(x) for x in a.dists.split(",")):
            med, mn, out = _median(lambda: A.find_proximity_between(B, d, cap=cap), a.reps)
            print(json.dumps({"call": "find_proximity_between", "dist": d, "median_ms": med, "min_ms": mn, "pairs": int(out[2]),
                              "tested": int(A.between_tested), "reps": a.reps}), flush=True)
        for d in (float(x) for x in a.dists.split(",") if float(x) > 0):
            for mode, ea, eb in (("both", x1[:half], x1[half:]), ("b static", x1[:half], None)):
                med, mn, out = _median(lambda: A.find_ccd_between(B, d, ea, eb, cap=cap), a.reps)
                info = A.ccd_info
                print(json.dumps({"call": "find_ccd_between", "moving": mode, "motion_edges": a.motion, "dist": d, "median_ms": med,
                                  "min_ms": mn, "pairs": int(out[3]), "at_t0": int(np.sum(out[1] == 0.0)), "candidates": int(info.n_candidates),
                                  "tested": int(info.n_tested), "evals": int(info.n_evals), "unresolved": int(info.n_unresolved),
                                  "reps": a.reps}), flush=True)


if __name__ == "__main__":
    main()
