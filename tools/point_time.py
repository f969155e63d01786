"""Times cd_closest_points on the 1 M cloth (mi355_synth.cloth_pair(500)), the tree built beforehand: host clock around the synchronising
call (upload of the points, the walk, the read-back of every output), one warm-up, median of --reps calls.  Query sets, 2^20 points each:
  coherent  the vertices of the cloth's second sheet moved by a third of the sheets' gap towards the first, in mesh order, repeated to 2^20
            (neighbouring points share a wave and walk neighbouring paths)
  shuffled  the same points in a random order (what incoherent waves cost)
  box       random points in the root box
  radius    the box points with rmax = 2 quad edges (most find nothing: the walk is bounded from the start)
  any       the same with CD_POINT_ANY
For each set the seed's share is recorded too: CD_POINT_ANY with rmax = +inf returns exactly the triangle phase 1 ends at, and pt_tri
of that triangle (cd_pt_tri_points) says whether it already is at the nearest distance ("seed_is_nearest": phase 2 only confirms it) or,
for the sets with a radius, within rmax ("seed_within": phase 1 alone ends a CD_POINT_ANY lane).
The kernel's own time comes from a separate run under rocprofv3 --kernel-trace --stats."""
from __future__ import annotations

import argparse
import ctypes as C
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
    ap.add_argument("--points", type=int, default=1 << 20)
    a = ap.parse_args()
    verts, vidx = synth.cloth_pair(a.quads)
    verts = np.asarray(verts, dtype=np.float64)
    edge = 2.88 / a.quads
    n = a.points
    g = np.random.default_rng(1)
    half = vidx.shape[0] // 2
    first, second = verts[np.unique(vidx[:half])], verts[np.unique(vidx[half:])]
    gap = second.mean(axis=0) - first.mean(axis=0)
    coherent = np.resize(second - gap / 3.0, (n, 3))
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    box = lo + (hi - lo) * g.random((n, 3))
    tris = verts[vidx.astype(np.int64)]
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        cd.build_tree()
        for name, pts, rmax, any_within in (("coherent", coherent, np.inf, False), ("shuffled", coherent[g.permutation(n)], np.inf, False),
                                            ("box", box, np.inf, False), ("radius", box, 2.0 * edge, False), ("any", box, 2.0 * edge, True)):
            p4 = mi355cd.pack_points(pts, rmax)                            # packed once: the timed call is cd_closest_points itself
            face, ids, dist = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n)
            q, uv, feat, side, info = np.empty((n, 3)), np.empty((n, 2)), np.empty(n, np.uint8), np.empty(n, np.uint8), mi355cd.CdPointInfo()
            outs = (vp(face),) + (None,) * 6 if any_within else (vp(face), vp(ids), vp(dist), vp(q), vp(uv), vp(feat), vp(side))
            call = lambda: cd.lib.cd_closest_points(cd._ctx, vp(p4), n, mi355cd.CD_POINT_ANY if any_within else 0, *outs, C.byref(info))
            med, mn, rc = _median(call, a.reps)
            assert rc == mi355cd.CD_OK, rc
            row = {"set": name, "points": n, "triangles": int(vidx.shape[0]), "median_ms": med, "min_ms": mn, "found": int(info.n_found),
                   "boxes_per_point": round(info.node_visits / n, 2), "pt_tri_per_point": round(info.tri_tests / n, 3),
                   "Mpoints_per_s_host": round(n / med / 1e3, 1), "reps": a.reps}
            seed, _ = cd.closest_points(pts, any_within=True)              # rmax = +inf: the triangle phase 1 ends at
            dseed = mi355cd.pt_tri_points(pts, tris[seed])[0]
            if any_within or np.isfinite(rmax):
                row["seed_within"] = round(float((dseed <= rmax).mean()), 4)
            if not any_within:
                row["seed_is_nearest"] = round(float((dseed[face != mi355cd.POINT_NONE] == dist[face != mi355cd.POINT_NONE]).mean()), 4)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
