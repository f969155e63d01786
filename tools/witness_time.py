"""Times the witness calls against the plain ones on the 1 M cloth (mi355_synth.cloth_pair(500); quad edge ~0.0058) after
cd_build_tree: cd_find_proximity / cd_find_proximity_witness at --dist and cd_find_ccd / cd_find_ccd_witness for a motion of --motion
quad edges, interleaved call by call.  Host clock around the synchronising C call into preallocated, touched host arrays sized to the
pair count (no numpy copies inside the timed region); one warm-up each, median and spread (min, max) of --reps calls.  --plain-only
times the two plain calls alone: run it with MI355CD_LIB pointing at another build of the library, alternating processes, to compare
the plain calls of two commits (a library without the witness symbols can be loaded that way: --plain-only touches none of them)."""
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


def _lib(plain_only):
    if not plain_only:
        import mi355cd
        return mi355cd.load_library()
    try:                                        # torch's HIP runtime first, as mi355cd.load_library does
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(os.environ.get("MI355CD_LIB", os.path.join(ROOT, "gpu-computing-course_amd", "libmi355cd.so")))
    vp, u64p = C.c_void_p, C.POINTER(C.c_uint64)
    lib.cd_create.argtypes = [C.POINTER(vp), vp, C.c_uint32, vp, vp, C.c_uint32]
    lib.cd_destroy.argtypes = [vp]; lib.cd_destroy.restype = None
    lib.cd_build_tree.argtypes = [vp]
    lib.cd_find_proximity.argtypes = [vp, C.c_double, vp, vp, C.c_uint64, u64p, u64p]
    lib.cd_find_ccd.argtypes = [vp, vp, C.c_double, vp, vp, vp, C.c_uint64, u64p, vp]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--quads", type=int, default=500)
    ap.add_argument("--dist", type=float, default=0.001)
    ap.add_argument("--motion", type=float, default=0.25)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--tag", type=str, default="this")
    a = ap.parse_args()
    lib = _lib(a.plain_only)
    verts, vidx = synth.cloth_pair(a.quads)
    verts = np.ascontiguousarray(verts, dtype=np.float64); vidx = np.ascontiguousarray(vidx, dtype=np.uint32)
    x1 = np.ascontiguousarray(synth.cloth_motion(verts, approach=a.motion, wave=a.motion, quads=a.quads))
    ctx = C.c_void_p()
    assert lib.cd_create(C.byref(ctx), verts.ctypes.data, verts.shape[0], vidx.ctypes.data, None, vidx.shape[0]) == 0
    assert lib.cd_build_tree(ctx) == 0
    n = C.c_uint64(0)
    lib.cd_find_proximity(ctx, a.dist, None, None, 0, C.byref(n), None); n_prox = n.value
    lib.cd_find_ccd(ctx, x1.ctypes.data, a.dist, None, None, None, 0, C.byref(n), None); n_ccd = n.value
    cap = max(n_prox, n_ccd) + 1024
    pairs, toi, dists = np.zeros((cap, 2), np.uint32), np.zeros(cap), np.zeros(cap)
    calls = {"find_proximity": lambda: lib.cd_find_proximity(ctx, a.dist, pairs.ctypes.data, dists.ctypes.data, cap, C.byref(n), None),
             "find_ccd": lambda: lib.cd_find_ccd(ctx, x1.ctypes.data, a.dist, pairs.ctypes.data, toi.ctypes.data, dists.ctypes.data, cap, C.byref(n), None)}
    if not a.plain_only:
        import mi355cd
        faces, points, bary, feat = np.zeros((cap, 2), np.uint32), np.zeros((cap, 6)), np.zeros((cap, 4)), np.zeros((cap, 2), np.uint8)
        w = mi355cd.CdWitnessOut(faces.ctypes.data, points.ctypes.data, bary.ctypes.data, feat.ctypes.data)
        wf = mi355cd.CdWitnessOut(faces.ctypes.data, None, None, None)
        calls["find_proximity_witness"] = lambda: lib.cd_find_proximity_witness(ctx, a.dist, pairs.ctypes.data, dists.ctypes.data, cap, C.byref(n), None, C.byref(w))
        calls["find_proximity_witness(faces only)"] = lambda: lib.cd_find_proximity_witness(ctx, a.dist, pairs.ctypes.data, dists.ctypes.data, cap, C.byref(n), None, C.byref(wf))
        calls["find_ccd_witness"] = lambda: lib.cd_find_ccd_witness(ctx, x1.ctypes.data, a.dist, pairs.ctypes.data, toi.ctypes.data, dists.ctypes.data, cap, C.byref(n), None, C.byref(w))
    for fn in calls.values():
        assert fn() == 0                                                        # warm-up (device buffers sized)
    ts = {k: [] for k in calls}
    for _ in range(a.reps):                                                     # interleaved, call by call
        for k, fn in calls.items():
            t0 = time.perf_counter()
            rc = fn()
            ts[k].append((time.perf_counter() - t0) * 1e3)
            assert rc == 0
    for k, v in ts.items():
        print(json.dumps({"lib": a.tag, "call": k, "triangles": int(vidx.shape[0]), "dist": a.dist, "motion_edges": a.motion,
                          "pairs": n_ccd if "ccd" in k else n_prox, "reps": a.reps, "median_ms": round(float(np.median(v)), 4),
                          "min_ms": round(float(np.min(v)), 4), "max_ms": round(float(np.max(v)), 4)}), flush=True)
    lib.cd_destroy(ctx)


if __name__ == "__main__":
    main()
