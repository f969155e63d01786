"""Times the contour calls against the plain contact calls on the 1 M cloth (mi355_synth.cloth_pair(500)), trees built beforehand, all
in one process and interleaved call by call: cd_find_collisions; cd_find_collisions_contour with all outputs, with faces only and with
a NULL record; and, on the two sheets as two contexts, cd_find_collisions_between and cd_find_collisions_between_contour.  Host clock
around the synchronising C call into preallocated, touched host arrays sized to the pair count (no numpy copies inside the timed
region); one warm-up each, median and spread (min, max) of --reps calls.  --plain-only times the two plain calls alone: run it with
MI355CD_LIB pointing at another build of the library, alternating processes, to compare the plain calls of two commits (a library
without the contour symbols can be loaded that way: --plain-only touches none of them)."""
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
    lib.cd_find_collisions.argtypes = [vp, vp, C.c_uint64, u64p]
    lib.cd_find_collisions_between.argtypes = [vp, vp, vp, C.c_uint64, u64p, u64p]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--quads", type=int, default=500)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--tag", type=str, default="this")
    a = ap.parse_args()
    lib = _lib(a.plain_only)
    verts, vidx = synth.cloth_pair(a.quads)
    verts = np.ascontiguousarray(verts, dtype=np.float64); vidx = np.ascontiguousarray(vidx, dtype=np.uint32)
    half, na = verts.shape[0] // 2, vidx.shape[0] // 2
    va, vb = np.ascontiguousarray(verts[:half]), np.ascontiguousarray(verts[half:])
    ia, ib = np.ascontiguousarray(vidx[:na]), np.ascontiguousarray((vidx[na:] - half).astype(np.uint32))
    ctx, ca, cb = C.c_void_p(), C.c_void_p(), C.c_void_p()
    for c, v, i in ((ctx, verts, vidx), (ca, va, ia), (cb, vb, ib)):
        assert lib.cd_create(C.byref(c), v.ctypes.data, v.shape[0], i.ctypes.data, None, i.shape[0]) == 0
        assert lib.cd_build_tree(c) == 0
    n, tested = C.c_uint64(0), C.c_uint64(0)
    lib.cd_find_collisions(ctx, None, 0, C.byref(n)); n_self = n.value
    lib.cd_find_collisions_between(ca, cb, None, 0, C.byref(n), None); n_bw = n.value
    cap = max(n_self, n_bw) + 1024
    pairs = np.zeros((cap, 2), np.uint32)
    calls = {"find_collisions": lambda: lib.cd_find_collisions(ctx, pairs.ctypes.data, cap, C.byref(n)),
             "find_collisions_between": lambda: lib.cd_find_collisions_between(ca, cb, pairs.ctypes.data, cap, C.byref(n), C.byref(tested))}
    if not a.plain_only:
        import mi355cd
        faces, code, param, points = np.zeros((cap, 2), np.uint32), np.zeros((cap, 3), np.uint8), np.zeros((cap, 6)), np.zeros((cap, 6))
        w = mi355cd.CdContourOut(faces.ctypes.data, code.ctypes.data, param.ctypes.data, points.ctypes.data)
        wf = mi355cd.CdContourOut(faces.ctypes.data, None, None, None)
        calls["find_collisions_contour"] = lambda: lib.cd_find_collisions_contour(ctx, pairs.ctypes.data, cap, C.byref(n), C.byref(tested), C.byref(w))
        calls["find_collisions_contour(faces only)"] = lambda: lib.cd_find_collisions_contour(ctx, pairs.ctypes.data, cap, C.byref(n), C.byref(tested), C.byref(wf))
        calls["find_collisions_contour(NULL)"] = lambda: lib.cd_find_collisions_contour(ctx, pairs.ctypes.data, cap, C.byref(n), C.byref(tested), None)
        calls["find_collisions_between_contour"] = lambda: lib.cd_find_collisions_between_contour(ca, cb, pairs.ctypes.data, cap, C.byref(n), C.byref(tested), C.byref(w))
    for fn in calls.values():
        assert fn() == 0                                                        # warm-up (device buffers sized)
    ts = {k: [] for k in calls}
    counts = {}
    for _ in range(a.reps):                                                     # interleaved, call by call
        for k, fn in calls.items():
            t0 = time.perf_counter()
            rc = fn()
            ts[k].append((time.perf_counter() - t0) * 1e3)
            assert rc == 0
            counts[k] = (n.value, tested.value if k != "find_collisions" else None)
    for k, v in ts.items():
        print(json.dumps({"lib": a.tag, "call": k, "triangles": int(vidx.shape[0]), "pairs": counts[k][0], "tested": counts[k][1], "reps": a.reps,
                          "median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4), "max_ms": round(float(np.max(v)), 4)}), flush=True)
    for c in (ctx, ca, cb):
        lib.cd_destroy(c)


if __name__ == "__main__":
    main()
