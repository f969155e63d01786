"""Times the swept-point queries on the 1 M cloth (mi355_synth.cloth_pair(--quads); quad edge ~0.0058) with the cloth's own vertices as
items, skip_vertex set to each vertex's own index, and x1 = mi355_synth.cloth_motion(x0, approach=m, wave=m) with m = --motion quad
edges: cd_sweep_points_all (count only, and with every value of every row) and cd_sweep_points, next to
cd_find_ccd at the same dist on the same mesh.  Host clock around the synchronising call, --warm warm-ups, median / min / max of --reps
calls; row, candidate, gate and evaluation counts.  One JSON line a call.  The per-kernel device times come from a separate run of this
script under rocprofv3 --kernel-trace --stats."""
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

vp = lambda a: a.ctypes.data_as(C.c_void_p)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--quads", type=int, default=500)
    ap.add_argument("--dist", type=float, default=0.001)
    ap.add_argument("--motion", type=float, default=1.0, help="approach = wave amplitude, in quad edges")
    a = ap.parse_args()

    v, i = synth.cloth_pair(a.quads)
    with mi355cd.CollisionDetector(v, i) as cd:
        cd.build_tree()
        x0 = cd.verts
        x1 = np.ascontiguousarray(synth.cloth_motion(x0, approach=a.motion, wave=a.motion, quads=a.quads))
        nv = x0.shape[0]
        items = mi355cd.pack_sweeps(x0, x1, a.dist)
        skip = np.arange(nv, dtype=np.uint32)
        base = {"triangles": int(i.shape[0]), "items": nv, "dist": a.dist, "motion_edges": a.motion}

        n, info = C.c_uint64(0), mi355cd.CdCcdInfo()
        rc = cd.lib.cd_sweep_points_all(cd._ctx, vp(x1), vp(items), nv, vp(skip), None, 0, C.byref(n), None, C.byref(info))
        assert rc in (mi355cd.CD_OK, mi355cd.CD_OVERFLOW), rc
        total = n.value
        rows = np.empty((max(total, 1), 2), np.uint32)
        arrays = mi355cd._SweepRowArrays(total)
        count = _times(lambda: cd.lib.cd_sweep_points_all(cd._ctx, vp(x1), vp(items), nv, vp(skip), None, 0, C.byref(n), None, C.byref(info)), a.reps, a.warm)
        full = _times(lambda: cd.lib.cd_sweep_points_all(cd._ctx, vp(x1), vp(items), nv, vp(skip), vp(rows), total, C.byref(n), C.byref(arrays.out), C.byref(info)),
                      a.reps, a.warm)
        assert n.value == total
        print(json.dumps(dict(base, call="sweep_points_all", rows=int(total), at_t0=int((arrays.toi[:total] == 0.0).sum()), candidates=int(info.n_candidates),
                              tested=int(info.n_tested), evals=int(info.n_evals), unresolved=int(info.n_unresolved), count_only=count, rows_all_values=full)), flush=True)

        face, ids, toi = np.empty(nv, np.uint32), np.empty(nv, np.uint32), np.empty(nv)
        d, q, uv, feat, side = np.empty(nv), np.empty((nv, 3)), np.empty((nv, 2)), np.empty(nv, np.uint8), np.empty(nv, np.uint8)
        pinfo = mi355cd.CdPointInfo()
        first = _times(lambda: cd.lib.cd_sweep_points(cd._ctx, vp(x1), vp(items), nv, vp(skip), 0, vp(face), vp(ids), vp(toi), vp(d), vp(q), vp(uv), vp(feat), vp(side),
                                                      C.byref(pinfo)), a.reps, a.warm)
        print(json.dumps(dict(base, call="sweep_points", found=int(pinfo.n_found), node_visits=int(pinfo.node_visits), evals=int(pinfo.tri_tests),
                              all_outputs=first)), flush=True)

        ccd = _times(lambda: cd.find_ccd(x1, a.dist, cap=1 << 22), a.reps, a.warm)
        pairs, _, _, np_, rc = cd.find_ccd(x1, a.dist, cap=1 << 22)
        ci = cd.ccd_info
        print(json.dumps(dict(base, call="find_ccd", pairs=int(np_), candidates=int(ci.n_candidates), tested=int(ci.n_tested), evals=int(ci.n_evals),
                              unresolved=int(ci.n_unresolved), all_outputs=ccd)), flush=True)


if __name__ == "__main__":
    main()
