"""Times the box queries: host clock around the synchronising C call into preallocated arrays, --warm warm-ups
(the candidate buffer has grown), median / min / max of --reps calls.  One JSON line a workload.
  cloth   the vertices of mi355_synth.cloth_pair(--quads) as boxes of half-width one quad edge, in mesh order, against that cloth:
          cd_boxes_overlap_all count only (cap_rows = 0) / the rows alone / rows + IDs + inside, cd_boxes_count plain / CD_BOX_ANY;
          beside it, in the same process, cd_points_within on the same vertices with rmax = the same edge
  grid    a --grid^3 occupancy grid, one box a voxel, over a closed torus of about --faces triangles, cd_boxes_count with CD_BOX_ANY
  root    ONE item, the mesh's root box, over the cloth: cd_boxes_count against cd_boxes_overlap_all count only"""
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

import closed_meshes as cm  # noqa: E402
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


def _count(cd, boxes, flags, reps, warm):
    n = boxes.shape[0]
    count = np.empty(n, np.uint32)
    n_inside = None if flags else np.empty(n, np.uint32)
    info = mi355cd.CdBoxInfo()
    t = _times(lambda: cd.lib.cd_boxes_count(cd._ctx, vp(boxes), n, flags, vp(count), vp(n_inside), C.byref(info)), reps, warm)
    t.update(found=int(info.n_found), node_visits=int(info.node_visits), tri_tests=int(info.tri_tests), sum=int(count.astype(np.uint64).sum()))
    return t


def _count_only(cd, fn, items, reps, warm):
    n, tested = C.c_uint64(0), C.c_uint64(0)
    t = _times(lambda: fn(cd._ctx, vp(items), items.shape[0], None, 0, C.byref(n), C.byref(tested), None), reps, warm)
    t.update(rows=int(n.value), tested=int(tested.value))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--quads", type=int, default=500)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--faces", type=int, default=100_000)
    a = ap.parse_args()

    v, i = synth.cloth_pair(a.quads)
    edge = 2.88 / a.quads
    with mi355cd.CollisionDetector(v, i) as cd:
        cd.build_tree()
        boxes = mi355cd.pack_boxes(cd.verts - edge, cd.verts + edge)
        res = {"workload": "cloth", "triangles": int(i.shape[0]), "items": int(boxes.shape[0])}
        res["overlap_all_count_only"] = _count_only(cd, cd.lib.cd_boxes_overlap_all, boxes, a.reps, a.warm)
        total = res["overlap_all_count_only"]["rows"]
        rows, ids, inside = np.empty((max(total, 1), 2), np.uint32), np.empty(max(total, 1), np.uint32), np.empty(max(total, 1), np.uint8)
        out = mi355cd.CdBoxRows(ids.ctypes.data, inside.ctypes.data)
        n = C.c_uint64(0)
        call = lambda o: cd.lib.cd_boxes_overlap_all(cd._ctx, vp(boxes), boxes.shape[0], vp(rows), total, C.byref(n), None, o)
        res["overlap_all_rows"] = _times(lambda: call(None), a.reps, a.warm)
        res["overlap_all_rows_values"] = _times(lambda: call(C.byref(out)), a.reps, a.warm)
        assert n.value == total
        res["count"] = _count(cd, boxes, 0, a.reps, a.warm)
        res["count_any"] = _count(cd, boxes, mi355cd.CD_BOX_ANY, a.reps, a.warm)
        assert res["count"]["sum"] == total
        p4 = mi355cd.pack_points(cd.verts, edge)
        res["points_within_count_only"] = _count_only(cd, cd.lib.cd_points_within, p4, a.reps, a.warm)
        print(json.dumps(res), flush=True)

        root = np.ascontiguousarray(cd.root_box().reshape(1, 6))
        res = {"workload": "root", "triangles": int(i.shape[0]), "items": 1}
        res["count"] = _count(cd, root, 0, a.reps, a.warm)
        res["overlap_all_count_only"] = _count_only(cd, cd.lib.cd_boxes_overlap_all, root, a.reps, a.warm)
        print(json.dumps(res), flush=True)

    nv = 200
    nu = max(3, a.faces // (2 * nv))
    v, f = cm.torus(nu, nv)
    m = a.grid
    lo, hi = v.min(axis=0) - 0.01, v.max(axis=0) + 0.01
    g = np.stack(np.meshgrid(*(np.arange(m),) * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    boxes = mi355cd.pack_boxes(lo + (hi - lo) * (g / m), lo + (hi - lo) * ((g + 1) / m))
    with mi355cd.CollisionDetector(v, f) as cd:
        cd.set_morton_frame(mi355cd.CD_FRAME_AUTO)                             # (the torus is centred on the origin: not the reference's fixed frame)
        cd.build_tree()
        res = {"workload": "grid", "triangles": int(f.shape[0]), "items": int(boxes.shape[0])}
        res["count_any"] = _count(cd, boxes, mi355cd.CD_BOX_ANY, a.reps, a.warm)
        res["count"] = _count(cd, boxes, 0, a.reps, a.warm)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
