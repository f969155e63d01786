"""Times cd_nearest_self on mi355_synth.cloth_pair(500) as ONE context (1 000 000 triangles), tree built beforehand: host clock around
the synchronising C call into preallocated arrays (the walk, the witness, the read-back of every output), one warm-up, median of --reps
calls.  Cases:
  rows_inf      flags = 0, rmax = +inf
  rows_2_edges  flags = 0, rmax = 2 quad edges
  min_inf       CD_NEAREST_MIN, rmax = +inf
In the same process, the call a user had before cd_nearest_self existed:
  prox_witness_at_clearance  cd_find_proximity_witness with dist = the clearance MIN returned -- a lower bound for any guess-and-retry
                             loop, since it is handed the answer
  prox_witness_2_edges       the same with dist = 2 quad edges: every pair the rows_2_edges call reduces (--heavy-reps calls)
--counts: instead, the counters of the seed decision -- boxes and tri_distance a row at rmax = +inf on cloth_pair(300) and
soup(100 000, 0.02, 4), one call each (MI355CD_LIB picks the build: the shipped one, or tools/ab_build.sh's -DCD_NEAREST_SELF_SEED=0).
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


def counts():
    for name, (v, i) in (("cloth300", synth.cloth_pair(300)), ("soup100k", synth.soup(100_000, e=0.02, seed=4))):
        with mi355cd.CollisionDetector(v, i) as cd:
            cd.build_tree()
            for minimum in (False, True):
                g = cd.nearest_self(np.inf, minimum=minimum)
                print(json.dumps({"case": "counts", "mesh": name, "lib": os.environ.get("MI355CD_LIB", "default"), "min": minimum, "nt": cd.nt,
                                  "found": int(g.info.n_found), "boxes_per_row": round(g.info.node_visits / cd.nt, 2),
                                  "tri_distance_per_row": round(g.info.tri_tests / cd.nt, 3), "dist_sum": float(g.dist.sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--heavy-reps", type=int, default=5)
    ap.add_argument("--quads", type=int, default=500)
    ap.add_argument("--counts", action="store_true")
    ap.add_argument("--no-proximity", action="store_true", help="the three cases only (the kernel-trace run)")
    a = ap.parse_args()
    if a.counts:
        return counts()
    verts, vidx = synth.cloth_pair(a.quads)
    nt = vidx.shape[0]
    edge = 2.88 / a.quads
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        cd.build_tree()
        lib = cd.lib
        faces, ids, dist = np.empty((nt, 2), np.uint32), np.empty((nt, 2), np.uint32), np.empty(nt)
        wa = mi355cd._WitnessArrays(nt)
        info = mi355cd.CdNearestInfo()
        clearance = None
        for name, rmax, flags in (("rows_inf", np.inf, 0), ("rows_2_edges", 2 * edge, 0), ("min_inf", np.inf, mi355cd.CD_NEAREST_MIN)):
            call = lambda: lib.cd_nearest_self(cd._ctx, float(rmax), flags, vp(faces), vp(ids), vp(dist), C.byref(wa.out), C.byref(info))
            t, rc = _timed(call, a.reps)
            assert rc == mi355cd.CD_OK, rc
            rows = 1 if flags else nt
            print(json.dumps({"case": name, "lib": os.environ.get("MI355CD_LIB", "default"), "nt": nt, **t, "found": int(info.n_found),
                              "boxes_per_row": round(info.node_visits / nt, 2), "tri_distance_per_row": round(info.tri_tests / nt, 3),
                              "dist_min": float(dist[:rows].min()), "dist_max": float(dist[:rows].max())}), flush=True)
            if flags:
                clearance = float(dist[0])
        if a.no_proximity:
            return
        for name, d, reps in (("prox_witness_at_clearance", clearance, a.reps), ("prox_witness_2_edges", 2 * edge, a.heavy_reps)):
            n_pairs = cd.find_proximity(d, cap=1)[2]
            cap = max(int(n_pairs), 1)
            pairs, dd, wb = np.empty((cap, 2), np.uint32), np.empty(cap), mi355cd._WitnessArrays(cap)
            n, tested = C.c_uint64(0), C.c_uint64(0)
            call = lambda: lib.cd_find_proximity_witness(cd._ctx, float(d), vp(pairs), vp(dd), cap, C.byref(n), C.byref(tested), C.byref(wb.out))
            t, rc = _timed(call, reps)
            assert rc == mi355cd.CD_OK and n.value == n_pairs, (rc, n.value, n_pairs)
            print(json.dumps({"case": name, "dist": d, **t, "pairs": int(n.value), "tri_distance": int(tested.value)}), flush=True)
            del pairs, dd, wb


if __name__ == "__main__":
    main()
