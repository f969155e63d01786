"""Times the swept-segment queries against what a caller had before them, in the method of tools/segments_time.py:
host clock around the synchronising C call into preallocated arrays, --warm warm-ups (the candidate buffer has grown), median / min /
max of --reps calls, everything in one process.  The items are the edges of one sheet of mi355_synth.cloth_pair(--quads), in mesh
order, against the other sheet; both sheets move to mi355_synth.cloth_motion(x0, approach = wave = --motion quad edges); dist =
--thickness edges.  One JSON line a workload:
  rows     cd_sweep_segments_all (count only / rows and every value), beside cd_sweep_points_all on three sample points an edge (at
           1/4, 1/2, 3/4, moving with the edge) at dist + L/4, L the edge's larger length over the step: the substitute's covering radius
  first    cd_sweep_segments (every value)
  between  cd_find_ccd_between with a second context built from the edges as degenerate triangles (a, b, b): the query alone on a
           context that is there, and with cd_create, the upload and cd_build_tree a call, which is what a step pays
The lines are printed and written to --log (default profiles/r23_experiments/sweep_segments.log, from its start; '' for none)."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "gpu-computing-course_amd", "pyhost"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, _p)

import mi355_synth as synth  # noqa: E402
import mi355cd  # noqa: E402

vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


def _times(fn, reps, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3)}


def _info(i):
    return {"candidates": int(i.n_candidates), "gate": int(i.n_tested), "evals": int(i.n_evals), "unresolved": int(i.n_unresolved)}


def _rows_calls(cd, fn, items, x1, arrays_of, reps, warm):
    """count only, then rows and every value of a swept all-results call `fn`"""
    n, info = C.c_uint64(0), mi355cd.CdCcdInfo()
    res = {"count_only": _times(lambda: fn(cd._ctx, vp(x1), vp(items), items.shape[0], None, None, 0, C.byref(n), None, C.byref(info)), reps, warm)}
    total = int(n.value)
    res["count_only"].update(rows=total, **_info(info))
    rows = np.empty((max(total, 1), 2), np.uint32)
    a = arrays_of(max(total, 1))
    res["rows_values"] = _times(lambda: fn(cd._ctx, vp(x1), vp(items), items.shape[0], None, vp(rows), total, C.byref(n), C.byref(a.out), C.byref(info)), reps, warm)
    assert n.value == total
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--quads", type=int, default=500)
    ap.add_argument("--thickness", type=float, default=0.5, help="dist in edges of the cloth")
    ap.add_argument("--motion", type=float, default=1.0, help="approach = wave amplitude, in quad edges")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r23_experiments", "sweep_segments.log"))
    a = ap.parse_args()
    log = None
    if a.log:
        os.makedirs(os.path.dirname(a.log), exist_ok=True)
        log = open(a.log, "w")
        log.write("# tools/sweep_segments_time.py: one sheet's edges, moving, against the other sheet of cloth_pair(%d) (DESIGN.md section 26)\n" % a.quads)

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    v, i = synth.cloth_pair(a.quads)
    x0 = np.asarray(v, dtype=np.float64)
    x1 = np.ascontiguousarray(synth.cloth_motion(x0, approach=a.motion, wave=a.motion, quads=a.quads))
    half = i.shape[0] // 2
    fa, fb = i[:half], i[half:]
    e = np.unique(np.sort(np.concatenate([fa[:, [0, 1]], fa[:, [1, 2]], fa[:, [2, 0]]], axis=0), axis=1), axis=0)
    a0, b0, a1, b1 = x0[e[:, 0]], x0[e[:, 1]], x1[e[:, 0]], x1[e[:, 1]]
    L = np.maximum(np.linalg.norm(b0 - a0, axis=1), np.linalg.norm(b1 - a1, axis=1))
    dist = a.thickness * 2.88 / a.quads
    used = np.unique(fb)
    vb, vb1, fb = np.ascontiguousarray(x0[used]), np.ascontiguousarray(x1[used]), np.searchsorted(used, fb).astype(np.uint32)
    base = {"triangles": int(fb.shape[0]), "edges": int(e.shape[0]), "dist": dist, "mean_L": float(L.mean()), "motion_edges": a.motion}
    with mi355cd.CollisionDetector(vb, fb) as cd:
        cd.build_tree()
        items = mi355cd.pack_swept_segments(a0, b0, a1, b1, dist)
        w = np.array([0.25, 0.5, 0.75])[None, :, None]
        s0, s1 = (a0[:, None, :] + w * (b0 - a0)[:, None, :]).reshape(-1, 3), (a1[:, None, :] + w * (b1 - a1)[:, None, :]).reshape(-1, 3)
        pts = mi355cd.pack_sweeps(s0, s1, np.repeat(dist + 0.25 * L, 3))
        res = dict(base, workload="rows")
        res["sweep_segments_all"] = _rows_calls(cd, cd.lib.cd_sweep_segments_all, items, vb1, mi355cd._SweepSegmentRowArrays, a.reps, a.warm)
        res["sweep_points_all_3_samples"] = _rows_calls(cd, cd.lib.cd_sweep_points_all, pts, vb1, mi355cd._SweepRowArrays, a.reps, a.warm)
        emit(res)

        n = items.shape[0]
        face = np.empty(n, np.uint32)
        so = mi355cd._SweepSegmentRowArrays(n)
        pinfo = mi355cd.CdPointInfo()
        res = dict(base, workload="first")
        t = _times(lambda: cd.lib.cd_sweep_segments(cd._ctx, vp(vb1), vp(items), n, None, 0, vp(face), C.byref(so.out), C.byref(pinfo)), a.reps, a.warm)
        t.update(found=int(pinfo.n_found), node_visits=int(pinfo.node_visits), evals=int(pinfo.tri_tests))
        res["sweep_segments"] = t
        emit(res)

        # the edges as degenerate triangles (a, b, b) of a second context over sheet A's vertices
        used_a = np.unique(e)
        va, va1 = np.ascontiguousarray(x0[used_a]), np.ascontiguousarray(x1[used_a])
        ea = np.searchsorted(used_a, e).astype(np.uint32)
        fe = np.ascontiguousarray(np.stack([ea[:, 0], ea[:, 1], ea[:, 1]], axis=1))
        nn, info = C.c_uint64(0), mi355cd.CdCcdInfo()
        res = dict(base, workload="between")
        with mi355cd.CollisionDetector(va, fe) as ce:
            ce.build_tree()
            call = lambda c, pairs, toi, d, cap: c.lib.cd_find_ccd_between(c._ctx, vp(va1), cd._ctx, vp(vb1), dist, vp(pairs), vp(toi), vp(d), cap, C.byref(nn), C.byref(info))
            call(ce, None, None, None, 0)
            total = int(nn.value)
            pairs, toi, d = np.empty((max(total, 1), 2), np.uint32), np.empty(max(total, 1)), np.empty(max(total, 1))
            t = _times(lambda: call(ce, pairs, toi, d, total), a.reps, a.warm)
            t.update(pairs=total, **_info(info))
            res["find_ccd_between_query_only"] = t

        def whole():
            with mi355cd.CollisionDetector(va, fe) as c2:
                c2.build_tree()
                call(c2, pairs, toi, d, total)

        res["find_ccd_between_with_context_and_build"] = _times(whole, a.reps, a.warm)
        emit(res)


if __name__ == "__main__":
    main()
