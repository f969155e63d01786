"""Times cd_points_inside and cd_signed_distance on a torus of --nu x --nv quads (1024 x 512: 1 048 576 triangles) as one context, tree
built beforehand in the --frame Morton frame (auto: results never depend on it, the walk's length does), against a --grid^3 lattice of
points over the torus's box in x-fastest order (100^3 = 1 000 000 points): host clock around the synchronising C call into
preallocated arrays (upload, the walk, the read-back of every output), one warm-up, median of --reps calls.  Cases:
  inside_axis0 / 1 / 2   cd_points_inside along x, y, z.  x is the lattice's fastest axis: the lanes of a wave share one column.
  signed_distance_axis2  cd_signed_distance along z
In the same process, the nearest existing means on the same points:
  rays_all_count_axis0 / 1 / 2   cd_cast_rays_all count-only (cap = 0), direction +e_c, tmax = +inf: the crossings above each point
                                 summed over all points (it cannot say which point they belong to, and counts a shared edge twice)
  closest_points                 cd_closest_points, rmax = +inf: the unsigned half of the signed distance
Each case is one JSON line with the counters a point.  The kernels' own times come from a separate run under rocprofv3
--kernel-trace --stats."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import closed_meshes as cm  # noqa: E402
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--heavy-reps", type=int, default=3)
    ap.add_argument("--nu", type=int, default=1024)
    ap.add_argument("--nv", type=int, default=512)
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--frame", choices=("auto", "reference"), default="auto",
                    help="the Morton frame of the tree: CD_FRAME_AUTO (the mesh's own box) or the reference's constants, which do not fit a torus")
    ap.add_argument("--no-existing", action="store_true", help="the new calls only (the kernel-trace run)")
    a = ap.parse_args()
    R, r = 1.0, 0.375
    verts, faces = cm.torus(a.nu, a.nv, R, r)
    gx = np.linspace(-(R + r), R + r, a.grid)
    gz = np.linspace(-r, r, a.grid)
    z, y, x = np.meshgrid(gz, gx, gx, indexing="ij")                         # x fastest in the flattened order
    pts = np.ascontiguousarray(np.stack([x, y, z], axis=-1).reshape(-1, 3))
    n, nt = pts.shape[0], faces.shape[0]
    analytic = cm.torus_distance(pts, R, r) < 0
    vp = lambda arr: arr.ctypes.data_as(C.c_void_p)
    with mi355cd.CollisionDetector(verts, faces) as cd:
        cd.set_morton_frame(mi355cd.CD_FRAME_AUTO if a.frame == "auto" else mi355cd.CD_FRAME_REFERENCE)
        cd.build_tree()
        lib = cd.lib
        print(json.dumps({"case": "setup", "frame": a.frame, "nt": nt, "points": n, "lib": os.environ.get("MI355CD_LIB", "default")}), flush=True)
        inside, na, nb = np.empty(n, np.uint8), np.empty(n, np.uint32), np.empty(n, np.uint32)
        wa, wb = np.empty(n, np.int32), np.empty(n, np.int32)
        info = mi355cd.CdInsideInfo()
        for axis in (0, 1, 2):
            call = lambda: lib.cd_points_inside(cd._ctx, vp(pts), n, axis, 0, vp(inside), vp(na), vp(nb), vp(wa), vp(wb), C.byref(info))
            t, rc = _timed(call, a.reps)
            assert rc == mi355cd.CD_OK, rc
            print(json.dumps({"case": f"inside_axis{axis}", "nt": nt, "points": n, **t, "inside": int(info.n_inside),
                              "differs_from_smooth_torus": int((inside.astype(bool) != analytic).sum()), "open_columns": int(((wa + wb) != 0).sum()),
                              "crossings_above": int(na.sum()), "boxes_per_point": round(info.node_visits / n, 2),
                              "column_tri_per_point": round(info.tri_tests / n, 3)}), flush=True)
        sd, face, ids = np.empty(n), np.empty(n, np.uint32), np.empty(n, np.uint32)
        closest, uv, feature = np.empty((n, 3)), np.empty((n, 2)), np.empty(n, np.uint8)
        pinfo = mi355cd.CdPointInfo()
        call = lambda: lib.cd_signed_distance(cd._ctx, vp(pts), n, 2, 0, vp(sd), vp(face), vp(ids), vp(closest), vp(uv), vp(feature), vp(inside), C.byref(pinfo))
        t, rc = _timed(call, a.heavy_reps)
        assert rc == mi355cd.CD_OK, rc
        print(json.dumps({"case": "signed_distance_axis2", "nt": nt, "points": n, **t, "negative": int((sd < 0).sum()),
                          "max_abs_error_to_smooth_torus": float(np.abs(sd - cm.torus_distance(pts, R, r)).max()),
                          "boxes_per_point": round(pinfo.node_visits / n, 2), "evaluations_per_point": round(pinfo.tri_tests / n, 3)}), flush=True)
        if a.no_existing:
            return
        for axis in (0, 1, 2):
            d = np.zeros((n, 3))
            d[:, axis] = 1.0
            rays = mi355cd.pack_rays(pts, d, np.inf)
            n_rows, n_tested = C.c_uint64(0), C.c_uint64(0)
            call = lambda: lib.cd_cast_rays_all(cd._ctx, vp(rays), n, None, 0, C.byref(n_rows), C.byref(n_tested), None)
            t, rc = _timed(call, a.reps)
            assert rc in (mi355cd.CD_OK, mi355cd.CD_OVERFLOW), rc
            print(json.dumps({"case": f"rays_all_count_axis{axis}", "nt": nt, "points": n, **t, "hits": int(n_rows.value),
                              "ray_tri_per_point": round(n_tested.value / n, 3)}), flush=True)
            del rays
        p4 = mi355cd.pack_points(pts, np.inf)
        dist, side = np.empty(n), np.empty(n, np.uint8)
        call = lambda: lib.cd_closest_points(cd._ctx, vp(p4), n, 0, vp(face), vp(ids), vp(dist), vp(closest), vp(uv), vp(feature), vp(side), C.byref(pinfo))
        t, rc = _timed(call, a.heavy_reps)
        assert rc == mi355cd.CD_OK, rc
        print(json.dumps({"case": "closest_points", "nt": nt, "points": n, **t, "same_as_signed_distance": bool(np.array_equal(dist, np.abs(sd))),
                          "boxes_per_point": round(pinfo.node_visits / n, 2), "pt_tri_per_point": round(pinfo.tri_tests / n, 3)}), flush=True)


if __name__ == "__main__":
    main()
