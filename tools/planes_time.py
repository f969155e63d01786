"""Times the plane queries in the method of tools/boxes_time.py: host clock around the synchronising C call
into preallocated arrays, --warm warm-ups (the candidate buffer has grown), median / min / max of --reps calls.  One JSON line a
workload, all over mi355_synth.cloth_pair(--quads):
  axis    ONE axis-parallel plane x = the middle of the cloth: cd_planes_cut_all count only (cap_rows = 0) / the rows alone / rows
          and every value, cd_planes_count; beside it, in the same process, the FLAT BOX in the same place (lo == hi in x, the root
          box's extent in y and z): cd_boxes_overlap_all count only / rows / rows and values, cd_boxes_count -- the one-lane-an-item
          walk over nearly the same faces
  skew    1, 64 and 1024 planes with random normals through random points of the root box: the same four plane calls
--label names the build in the output (a library with another CD_PLANE_SLAB is chosen by MI355CD_LIB)."""
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
    """count only, the rows alone, rows and values of an all-results call `fn`; out_of(total) -> the out structure and what it points at"""
    n, tested = C.c_uint64(0), C.c_uint64(0)
    res = {"count_only": _times(lambda: fn(cd._ctx, vp(items), items.shape[0], None, 0, C.byref(n), C.byref(tested), None), reps, warm)}
    total = int(n.value)
    res["count_only"].update(rows=total, tested=int(tested.value))
    rows = np.empty((max(total, 1), 2), np.uint32)
    out, keep = out_of(max(total, 1))
    call = lambda o: fn(cd._ctx, vp(items), items.shape[0], vp(rows), total, C.byref(n), None, o)
    res["rows"] = _times(lambda: call(None), reps, warm)
    res["rows_values"] = _times(lambda: call(C.byref(out)), reps, warm)
    assert n.value == total and keep is not None
    return res


def _plane_out(r):
    a = [np.empty(r, np.uint32), np.empty((r, 6)), np.empty((r, 2), np.uint8), np.empty((r, 2)), np.empty(r, np.uint8)]
    return mi355cd.CdPlaneRows(*(x.ctypes.data for x in a)), a


def _box_out(r):
    a = [np.empty(r, np.uint32), np.empty(r, np.uint8)]
    return mi355cd.CdBoxRows(*(x.ctypes.data for x in a)), a


def _planes(cd, planes, reps, warm):
    res = _rows_calls(cd, cd.lib.cd_planes_cut_all, planes, _plane_out, reps, warm)
    n = planes.shape[0]
    counts = [np.empty(n, np.uint32) for _ in range(3)]
    info = mi355cd.CdPlaneInfo()
    res["count"] = _times(lambda: cd.lib.cd_planes_count(cd._ctx, vp(planes), n, *map(vp, counts), C.byref(info)), reps, warm)
    res["count"].update(found=int(info.n_found), node_visits=int(info.node_visits), tri_tests=int(info.tri_tests),
                        cut=int(counts[0].astype(np.uint64).sum()), below=int(counts[1].astype(np.uint64).sum()), above=int(counts[2].astype(np.uint64).sum()))
    assert res["count"]["cut"] == res["count_only"]["rows"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--quads", type=int, default=500)
    ap.add_argument("--label", default=f"L={mi355cd.CD_PLANE_SLAB}")
    ap.add_argument("--no-boxes", action="store_true", help="skip the flat-box counterpart")
    a = ap.parse_args()

    v, i = synth.cloth_pair(a.quads)
    with mi355cd.CollisionDetector(v, i) as cd:
        cd.build_tree()
        root = cd.root_box()
        lo, hi = root[0::2], root[1::2]
        mid = 0.5 * (lo[0] + hi[0])
        res = {"workload": "axis", "build": a.label, "triangles": int(i.shape[0]), "n_planes": 1}
        res["planes"] = _planes(cd, mi355cd.pack_planes([[1.0, 0.0, 0.0]], [mid]), a.reps, a.warm)
        if not a.no_boxes:
            flat = mi355cd.pack_boxes([[mid, lo[1], lo[2]]], [[mid, hi[1], hi[2]]])
            res["flat_box"] = _rows_calls(cd, cd.lib.cd_boxes_overlap_all, flat, _box_out, a.reps, a.warm)
            count, n_inside = np.empty(1, np.uint32), np.empty(1, np.uint32)
            info = mi355cd.CdBoxInfo()
            res["flat_box"]["count"] = _times(lambda: cd.lib.cd_boxes_count(cd._ctx, vp(flat), 1, 0, vp(count), vp(n_inside), C.byref(info)), a.reps, a.warm)
            res["flat_box"]["count"].update(sum=int(count[0]), node_visits=int(info.node_visits), tri_tests=int(info.tri_tests))
        print(json.dumps(res), flush=True)

        g = np.random.default_rng(31)
        for m in (1, 64, 1024):
            nrm = g.normal(size=(m, 3))
            nrm /= np.linalg.norm(nrm, axis=1)[:, None]
            through = lo + g.random((m, 3)) * (hi - lo)
            res = {"workload": "skew", "build": a.label, "triangles": int(i.shape[0]), "n_planes": m}
            res.update(_planes(cd, mi355cd.pack_planes(nrm, (nrm * through).sum(axis=1)), a.reps, a.warm))
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
