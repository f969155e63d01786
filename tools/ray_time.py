"""Times cd_cast_rays on the 1 M cloth (mi355_synth.cloth_pair(500)), the tree built beforehand: host clock around the synchronising
call (upload of the rays, the walk, the read-back of every output), one warm-up, median of --reps calls.  Ray sets:
  frame     a 1024 x 1024 pinhole camera above the cloth that sees all of it, row by row (coherent: neighbouring pixels share a wave)
  shuffled  the same rays in a random order (what incoherent waves cost)
  segments  2^20 random segments of about ten quad edges, starting in the cloth's box, closest hit
  any       the same segments with CD_RAY_ANY
The kernel's own time comes from a separate run under rocprofv3 --kernel-trace --stats."""
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


def pinhole(eye, target, up, fov_deg, res):
    eye, target, up = (np.asarray(x, dtype=np.float64) for x in (eye, target, up))
    w = target - eye; w /= np.linalg.norm(w)
    uu = np.cross(w, up); uu /= np.linalg.norm(uu)
    vv = np.cross(uu, w)
    c = ((np.arange(res) + 0.5) / res * 2.0 - 1.0) * np.tan(np.radians(fov_deg) / 2.0)
    d = w[None, None, :] + c[None, :, None] * uu[None, None, :] - c[:, None, None] * vv[None, None, :]
    return np.broadcast_to(eye, (res * res, 3)).copy(), d.reshape(-1, 3).copy()


def _median(fn, reps):
    fn()                                                                    # warm-up (buffers sized)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts)), 4), round(float(np.min(ts)), 4), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--quads", type=int, default=500)
    ap.add_argument("--res", type=int, default=1024)
    a = ap.parse_args()
    verts, vidx = synth.cloth_pair(a.quads)
    edge = 2.88 / a.quads
    g = np.random.default_rng(1)
    o, d = pinhole([1.5, 2.5, 0.75], [1.5, -0.1, 0.75], [0.0, 0.0, 1.0], 70.0, a.res)
    p = g.permutation(o.shape[0])
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    so = lo + (hi - lo) * g.random((1 << 20, 3))
    sd = g.normal(size=(1 << 20, 3)); sd *= 10.0 * edge / np.linalg.norm(sd, axis=1, keepdims=True)
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        cd.build_tree()
        for name, oo, dd, tmax, any_hit in (("frame", o, d, np.inf, False), ("shuffled", o[p], d[p], np.inf, False),
                                            ("segments", so, sd, 1.0, False), ("any", so, sd, 1.0, True)):
            rays = mi355cd.pack_rays(oo, dd, tmax)                         # packed once: the timed call is cd_cast_rays itself
            n = rays.shape[0]
            face, ids, t = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n)
            uv, side, info = np.empty((n, 2)), np.empty(n, np.uint8), mi355cd.CdRayInfo()
            vp = lambda x: x.ctypes.data_as(C.c_void_p)
            outs = (vp(face), None, None, None, None) if any_hit else (vp(face), vp(ids), vp(t), vp(uv), vp(side))
            call = lambda: cd.lib.cd_cast_rays(cd._ctx, vp(rays), n, mi355cd.CD_RAY_ANY if any_hit else 0, *outs, C.byref(info))
            med, mn, rc = _median(call, a.reps)
            assert rc == mi355cd.CD_OK, rc
            print(json.dumps({"set": name, "rays": n, "triangles": int(vidx.shape[0]), "median_ms": med, "min_ms": mn, "hits": int(info.n_hits),
                              "boxes_per_ray": round(info.node_visits / n, 2), "ray_tri_per_ray": round(info.tri_tests / n, 3),
                              "Mrays_per_s_host": round(n / med / 1e3, 1), "reps": a.reps}), flush=True)


if __name__ == "__main__":
    main()
