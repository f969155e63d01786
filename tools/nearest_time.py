"""Times cd_nearest_between on the two sheets of mi355_synth.cloth_pair(500) as two contexts (500 000 triangles each), trees built
beforehand: host clock around the synchronising C call into preallocated arrays (the walk, the witness, the read-back of every
output), one warm-up, median of --reps calls.  Cases:
  rows_inf      flags = 0, rmax = +inf
  rows_2_edges  flags = 0, rmax = 2 quad edges
  min_inf       CD_NEAREST_MIN, rmax = +inf
and the same three with sheet b lifted by --apart quad edges (the loose-seed case: the first candidate is far, the bound starts wide).
In the same process, the calls a user had before cd_nearest_between existed:
  prox_witness_at_sep      cd_find_proximity_between_witness with dist = the separation distance MIN returned -- a lower bound for any
                           retry loop, since it is handed the answer
  prox_witness_2_edges     the same with dist = 2 quad edges: every pair the rows_2_edges call reduces (--heavy-reps calls: millions of rows)
  closest_points_of_verts  b.closest_points(a's vertices): misses every edge-edge minimum
Each case is one JSON line.  The kernels' own times come from a separate run under rocprofv3 --kernel-trace --stats."""
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


def _timed(fn, reps):
    fn()                                                                    # warm-up (buffers sized)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(np.min(ts)), 4), "max_ms": round(float(np.max(ts)), 4), "reps": reps}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--heavy-reps", type=int, default=5)
    ap.add_argument("--quads", type=int, default=500)
    ap.add_argument("--apart", type=float, default=10.0)
    a = ap.parse_args()
    verts, vidx = synth.cloth_pair(a.quads)
    na, half = vidx.shape[0] // 2, verts.shape[0] // 2
    va, ia, vb0, ib = verts[:half], vidx[:na], verts[half:], (vidx[na:] - half).astype(np.uint32)
    edge = 2.88 / a.quads
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    for lift in (0.0, a.apart):
        vb = vb0.copy()
        vb[:, 1] += lift * edge
        with mi355cd.CollisionDetector(va, ia) as ca, mi355cd.CollisionDetector(vb, ib) as cb:
            ca.build_tree(); cb.build_tree()
            lib = ca.lib
            faces, ids, dist = np.empty((na, 2), np.uint32), np.empty((na, 2), np.uint32), np.empty(na)
            wa = mi355cd._WitnessArrays(na)
            info = mi355cd.CdNearestInfo()
            sep = None
            for name, rmax, flags in (("rows_inf", np.inf, 0), ("rows_2_edges", 2 * edge, 0), ("min_inf", np.inf, mi355cd.CD_NEAREST_MIN)):
                call = lambda: lib.cd_nearest_between(ca._ctx, cb._ctx, float(rmax), flags, vp(faces), vp(ids), vp(dist), C.byref(wa.out), C.byref(info))
                t, rc = _timed(call, a.reps)
                assert rc == mi355cd.CD_OK, rc
                rows = 1 if flags else na
                row = {"case": name, "lift_edges": lift, "na": na, "nb": int(ib.shape[0]), **t, "found": int(info.n_found),
                       "boxes_per_row": round(info.node_visits / na, 2), "tri_distance_per_row": round(info.tri_tests / na, 3),
                       "dist_min": float(dist[:rows].min()), "dist_max": float(dist[:rows].max())}
                if flags:
                    sep = float(dist[0])
                print(json.dumps(row), flush=True)
            for name, d, reps in (("prox_witness_at_sep", sep, a.reps), ("prox_witness_2_edges", 2 * edge, a.heavy_reps)):
                n_pairs = ca.find_proximity_between(cb, d, cap=1)[2]
                cap = max(int(n_pairs), 1)
                pairs, dd, wb = np.empty((cap, 2), np.uint32), np.empty(cap), mi355cd._WitnessArrays(cap)
                n, tested = C.c_uint64(0), C.c_uint64(0)
                call = lambda: lib.cd_find_proximity_between_witness(ca._ctx, cb._ctx, float(d), vp(pairs), vp(dd), cap, C.byref(n), C.byref(tested), C.byref(wb.out))
                t, rc = _timed(call, reps)
                assert rc == mi355cd.CD_OK and n.value == n_pairs, (rc, n.value, n_pairs)
                print(json.dumps({"case": name, "lift_edges": lift, "dist": d, **t, "pairs": int(n.value), "tri_distance": int(tested.value)}), flush=True)
                del pairs, dd, wb
            p4 = mi355cd.pack_points(va, np.inf)
            nv = p4.shape[0]
            f1, i1, d1, q1, uv1 = np.empty(nv, np.uint32), np.empty(nv, np.uint32), np.empty(nv), np.empty((nv, 3)), np.empty((nv, 2))
            fe1, s1, pinfo = np.empty(nv, np.uint8), np.empty(nv, np.uint8), mi355cd.CdPointInfo()
            call = lambda: lib.cd_closest_points(cb._ctx, vp(p4), nv, 0, vp(f1), vp(i1), vp(d1), vp(q1), vp(uv1), vp(fe1), vp(s1), C.byref(pinfo))
            t, rc = _timed(call, a.reps)
            assert rc == mi355cd.CD_OK, rc
            print(json.dumps({"case": "closest_points_of_verts", "lift_edges": lift, "points": nv, **t, "dist_min": float(d1.min()),
                              "boxes_per_point": round(pinfo.node_visits / nv, 2), "pt_tri_per_point": round(pinfo.tri_tests / nv, 3)}), flush=True)


if __name__ == "__main__":
    main()
