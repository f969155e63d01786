"""Times the segment queries against what a caller had before them, in the method of tools/planes_time.py: host
clock around the synchronising C call into preallocated arrays, --warm warm-ups (the candidate buffer has grown), median / min / max
of --reps calls, everything in one process.  The items are the edges of one sheet of mi355_synth.cloth_pair(--quads), in mesh order,
against the other sheet, at thickness h = --thickness edges.  One JSON line a workload:
  within   cd_segments_within (count only / rows and every value) at radius h, beside cd_points_within on three sample points an edge
           (at 1/4, 1/2, 3/4) at radius h + L/4, L the edge's length: the substitute's covering radius
  closest  cd_segments_closest at radius h beside cd_closest_points on the midpoints at h + L/2, and both with no radius"""
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


def _rows_calls(cd, fn, items, out_of, reps, warm):
    """count only, then rows and values of an all-results call `fn`; out_of(total) -> the out structure and what it points at"""
    n, tested = C.c_uint64(0), C.c_uint64(0)
    res = {"count_only": _times(lambda: fn(cd._ctx, vp(items), items.shape[0], None, 0, C.byref(n), C.byref(tested), None), reps, warm)}
    total = int(n.value)
    res["count_only"].update(rows=total, tested=int(tested.value))
    rows = np.empty((max(total, 1), 2), np.uint32)
    out, keep = out_of(max(total, 1))
    res["rows_values"] = _times(lambda: fn(cd._ctx, vp(items), items.shape[0], vp(rows), total, C.byref(n), None, C.byref(out)), reps, warm)
    assert n.value == total and keep is not None
    return res


def _segment_out(r):
    a = mi355cd._SegmentRowArrays(r)
    return a.out, a


def _point_out(r):
    a = mi355cd._PointRowArrays(r)
    return a.out, a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--quads", type=int, default=500)
    ap.add_argument("--thickness", type=float, default=0.5, help="h in edges of the cloth")
    a = ap.parse_args()

    v, i = synth.cloth_pair(a.quads)
    v = np.asarray(v, dtype=np.float64)
    half = i.shape[0] // 2
    fa, fb = i[:half], i[half:]
    e = np.unique(np.sort(np.concatenate([fa[:, [0, 1]], fa[:, [1, 2]], fa[:, [2, 0]]], axis=0), axis=1), axis=0)
    pa, pb = v[e[:, 0]], v[e[:, 1]]
    L = np.linalg.norm(pb - pa, axis=1)
    h = a.thickness * 2.88 / a.quads
    used = np.unique(fb)
    vb, fb = np.ascontiguousarray(v[used]), np.searchsorted(used, fb).astype(np.uint32)
    base = {"triangles": int(fb.shape[0]), "edges": int(e.shape[0]), "h": h, "mean_L": float(L.mean())}
    with mi355cd.CollisionDetector(vb, fb) as cd:
        cd.build_tree()
        segs = mi355cd.pack_segments(pa, pb, h)
        samples = (pa[:, None, :] + np.array([0.25, 0.5, 0.75])[None, :, None] * (pb - pa)[:, None, :]).reshape(-1, 3)
        pts = mi355cd.pack_points(samples, np.repeat(h + 0.25 * L, 3))
        res = dict(base, workload="within")
        res["segments_within"] = _rows_calls(cd, cd.lib.cd_segments_within, segs, _segment_out, a.reps, a.warm)
        res["points_within_3_samples"] = _rows_calls(cd, cd.lib.cd_points_within, pts, _point_out, a.reps, a.warm)
        print(json.dumps(res), flush=True)

        n = segs.shape[0]
        mid = 0.5 * (pa + pb)
        face = np.empty(n, np.uint32)
        so, po = mi355cd._SegmentRowArrays(n), mi355cd._PointRowArrays(n)
        sinfo, pinfo = mi355cd.CdSegmentInfo(), mi355cd.CdPointInfo()
        res = dict(base, workload="closest")
        for tag, rs, rp in (("radius", h, h + 0.5 * L), ("no_radius", np.inf, np.inf)):
            s7, p4 = mi355cd.pack_segments(pa, pb, rs), mi355cd.pack_points(mid, rp)
            t = _times(lambda: cd.lib.cd_segments_closest(cd._ctx, vp(s7), n, 0, vp(face), C.byref(so.out), C.byref(sinfo)), a.reps, a.warm)
            t.update(found=int(sinfo.n_found), node_visits=int(sinfo.node_visits), tri_tests=int(sinfo.tri_tests))
            res["segments_closest_" + tag] = t
            t = _times(lambda: cd.lib.cd_closest_points(cd._ctx, vp(p4), n, 0, vp(face), vp(po.ids), vp(po.dist), vp(po.closest), vp(po.uv), vp(po.feature),
                                                        vp(po.side), C.byref(pinfo)), a.reps, a.warm)
            t.update(found=int(pinfo.n_found), node_visits=int(pinfo.node_visits), tri_tests=int(pinfo.tri_tests))
            res["closest_points_midpoints_" + tag] = t
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
