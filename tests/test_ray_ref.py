"""The ray predicate's numpy restatement (tests/ray_ref.py) against exact rational arithmetic, its scale equivariance, the tie rule of
the closest hit, and the C ABI of the two new entry points without a device.  No GPU.

Margins and scales.  With kappa = |e1| |e2| |d| / |det| (>= 1: one over the sine of the triangle's corner times the cosine of the
ray's incidence) and rho = 1 + |o - p0| / min(|e1|, |e2|), the computed u and v are off by a few 2^-53 kappa rho, and t by a few
2^-53 kappa (|o - p0| + |e1| + |e2|) / |d|: those are the scales the quantities below are "away from 0" relative to.
    S_uv = kappa rho                      for u, v and 1 - u - v
    S_t  = kappa (|o - p0| + |e1| + |e2|) / |d|   for t and tmax - t
A pair is DECIDED when each of the exact u, v, 1 - u - v is at least 2^-30 S_uv away from 0 and t, tmax - t at least 2^-30 S_t.

Measured here (the sets below, 8 x 400 pairs, well-conditioned pairs |det| >= 2^-10 |e1| |e2| |d| that both sides hit):
    max |u - u_exact| / rho, |v - v_exact| / rho : 2.44e-14       max |t - t_exact| |d| / (|o - p0| + |e1| + |e2|) : 2.20e-14
The sets are samples, not a worst case: 4 x the larger figure is asserted (ERR_BOUND)."""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import mi355cd
import ray_ref
from conftest import has_gpu

N_EXACT = 400
ERR_MEASURED = 2.44e-14
ERR_BOUND = 4.0 * ERR_MEASURED
BAND = (-300, -200, -150, -127, -64, 64, 127, 128, 200, 256, 300)             # 2^k within the band include/mi355cd.h states


def _norm(v):
    return math.sqrt(float(v[0]) ** 2 + float(v[1]) ** 2 + float(v[2]) ** 2)


def _exact_table():
    rows = []
    for name, (rays, tris) in ray_ref.pair_classes(N_EXACT, seed=5).items():
        hit, t, u, v, side = ray_ref.ray_tri_np(rays, tris)
        for i in range(rays.shape[0]):
            eh, et, eu, ev, det = ray_ref.exact_ray_tri(rays[i], tris[i])
            rows.append((name, i, rays[i], tris[i], bool(hit[i]), t[i], u[i], v[i], int(side[i]), eh, et, eu, ev, det))
    return rows


@pytest.fixture(scope="module")
def table():
    return _exact_table()


def _scales(ray, tri, det):
    e1, e2, tv, d = tri[1] - tri[0], tri[2] - tri[0], ray[0:3] - tri[0], ray[3:6]
    n1, n2, nd, ntv = _norm(e1), _norm(e2), _norm(d), _norm(tv)
    kappa = n1 * n2 * nd / abs(float(det))
    rho = 1.0 + ntv / min(n1, n2)
    return kappa, rho, kappa * rho, kappa * (ntv + n1 + n2) / nd


def test_decision_agrees_with_exact_where_decided_and_gate_rejects_no_such_hit(table):
    decided = {}
    for name, i, ray, tri, hit, t, u, v, side, eh, et, eu, ev, det in table:
        if det == 0:
            assert not hit or name in ("in_plane", "degenerate", "grazing"), (name, i)   # (rounding may give det != 0: then the range checks and the gate decide)
            continue
        with np.errstate(all="ignore"):
            kappa, rho, s_uv, s_t = _scales(ray, tri, det)
        if not (np.isfinite(s_uv) and np.isfinite(s_t)):
            continue
        m_uv, m_t = 2.0 ** -30 * s_uv, 2.0 ** -30 * s_t
        q = [float(eu), float(ev), float(1 - eu - ev)]
        tq = [float(et)] + ([] if ray[6] == np.inf else [float(Fraction(float(ray[6])) - et)])
        if min(abs(x) for x in q) < m_uv or min(abs(x) for x in tq) < m_t:
            continue
        decided[name] = decided.get(name, 0) + 1
        assert hit == eh, (name, i, hit, eh, float(eu), float(ev), float(et), kappa)     # (a decided exact hit the gate rejected would fail here)
        if hit:
            assert side == (1 if det > 0 else 0)
    print("decided pairs per class:", decided)
    assert decided.get("random", 0) > N_EXACT // 2 and decided.get("scaled", 0) > N_EXACT // 2 and decided.get("axis", 0) > N_EXACT // 4
    assert sum(decided.values()) > 2 * N_EXACT


def test_values_agree_with_exact_on_well_conditioned_pairs(table):
    worst_uv, worst_t, n = 0.0, 0.0, 0
    for name, i, ray, tri, hit, t, u, v, side, eh, et, eu, ev, det in table:
        if det == 0 or not (hit and eh):
            continue
        kappa, rho, s_uv, s_t = _scales(ray, tri, det)
        if not kappa <= 2.0 ** 10:
            continue
        n += 1
        e_uv = max(abs(float(Fraction(float(u)) - eu)), abs(float(Fraction(float(v)) - ev))) / rho
        e_t = abs(float(Fraction(float(t)) - et)) * kappa / s_t                           # = |t - t_exact| |d| / (|tv| + |e1| + |e2|)
        worst_uv, worst_t = max(worst_uv, e_uv), max(worst_t, e_t)
    print(f"well-conditioned hits: {n}; max u/v error / rho = {worst_uv:.3e}; max t error |d| / (|tv| + |e1| + |e2|) = {worst_t:.3e}; asserted {ERR_BOUND:.3e}")
    assert n > N_EXACT
    assert worst_uv <= ERR_BOUND and worst_t <= ERR_BOUND


def test_restatement_is_equivariant_under_power_of_two_scaling():
    for name, (rays, tris) in ray_ref.pair_classes(4096, seed=9).items():
        if name == "scaled":
            continue                                                            # (already at 2^+-100: another 2^300 leaves the band)
        base = ray_ref.ray_tri_np(rays, tris)
        for k in BAND:
            rs = rays.copy()
            rs[:, 0:6] = np.ldexp(rays[:, 0:6], k)
            got = ray_ref.ray_tri_np(rs, np.ldexp(tris, k))
            for a, b, what in zip(base, got, ("hit", "t", "u", "v", "side")):
                assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)), (name, k, what)


def test_zero_components_tmax_ends_and_nan_are_handled():
    tri = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])
    down = lambda x, y, z, tm: np.array([[x, y, z, 0.0, 0.0, -1.0, tm]])
    hit, t, u, v, side = ray_ref.ray_tri_np(down(0.25, 0.25, 2.0, np.inf), tri)
    assert hit[0] and t[0] == 2.0 and u[0] == 0.25 and v[0] == 0.25 and side[0] == 1      # counter-clockwise seen from above
    assert ray_ref.ray_tri_np(down(0.25, 0.25, -2.0, np.inf), tri)[0][0] == False         # behind the origin
    up = np.array([[0.25, 0.25, -2.0, 0.0, 0.0, 1.0, np.inf]])
    assert ray_ref.ray_tri_np(up, tri)[0][0] and ray_ref.ray_tri_np(up, tri)[4][0] == 0   # no culling: the clockwise face is hit too
    assert ray_ref.ray_tri_np(down(0.25, 0.25, 2.0, 2.0), tri)[0][0]                      # t == tmax: closed
    assert not ray_ref.ray_tri_np(down(0.25, 0.25, 2.0, np.nextafter(2.0, 0.0)), tri)[0][0]
    assert ray_ref.ray_tri_np(down(0.25, 0.25, 0.0, 0.0), tri)[0][0]                      # tmax = 0, the origin on the triangle
    assert ray_ref.ray_tri_np(down(0.0, 0.0, 1.0, np.inf), tri)[0][0]                     # through a vertex, along an edge's end: closed
    assert ray_ref.ray_tri_np(down(0.5, 0.5, 1.0, np.inf), tri)[0][0]                     # through the hypotenuse: u + v == 1
    flat = np.array([[0.25, 0.25, 0.0, 1.0, 0.0, 0.0, np.inf]])
    assert not ray_ref.ray_tri_np(flat, tri)[0][0]                                        # in the plane: det == 0
    seg = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0]]])
    assert not ray_ref.ray_tri_np(down(0.5, 0.0, 1.0, np.inf), seg)[0][0]                 # a segment is never hit
    bad = down(0.25, 0.25, 2.0, np.inf); bad[0, 1] = np.nan
    assert not ray_ref.ray_tri_np(bad, tri)[0][0]


def test_tie_rule_on_a_shared_edge_and_a_shared_vertex():
    # a fan of four triangles around the origin in the plane z = 0; the ray comes straight down
    verts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    vidx = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]], dtype=np.uint32)
    edge = np.array([[0.0, 0.5, 3.0, 0.0, 0.0, -1.0, np.inf]])                            # through the edge (0, 2) that faces 0 and 1 share
    vert = np.array([[0.0, 0.0, 3.0, 0.0, 0.0, -1.0, np.inf]])                            # through the vertex all four share
    for rays, among in ((edge, [0, 1]), (vert, [0, 1, 2, 3])):
        each = [ray_ref.ray_tri_np(rays, verts[vidx[f]][None])[0][0] for f in range(4)]
        assert [f for f in range(4) if each[f]] == among
        face, ids, t, uv, side = ray_ref.cast_rays_ref(verts, vidx, None, rays)
        assert face[0] == among[0] and ids[0] == among[0] and t[0] == 3.0                 # IDs = face indices: the smallest
        custom = np.array([7, 5, 5, 9], dtype=np.uint32)
        face, ids, t, uv, side = ray_ref.cast_rays_ref(verts, vidx, custom, rays)
        assert (face[0], ids[0]) == (1, 5)                                                # the smallest ID first, then the smaller face index
    # a nearer triangle wins whatever its ID
    verts2 = np.concatenate([verts, verts[:3] + [0.0, 0.0, 1.0]])
    vidx2 = np.concatenate([vidx, np.array([[5, 6, 7]], dtype=np.uint32)])
    face, ids, t, uv, side = ray_ref.cast_rays_ref(verts2, vidx2, np.array([0, 1, 2, 3, 99], dtype=np.uint32), np.array([[0.25, 0.25, 3.0, 0.0, 0.0, -1.0, np.inf]]))
    assert (face[0], ids[0], t[0]) == (4, 99, 2.0)


def test_cast_rays_ref_is_the_all_pairs_minimum():
    import mi355_synth as synth
    verts, vidx = synth.soup(300, e=0.3, seed=2)
    rays = ray_ref.mesh_rays(verts, vidx, 512, seed=1)
    ids = np.random.default_rng(3).integers(0, 40, vidx.shape[0]).astype(np.uint32)      # many equal IDs
    face, oid, t, uv, side = ray_ref.cast_rays_ref(verts, vidx, ids, rays, pairs_per_chunk=7 * 300)
    tris = verts[vidx.astype(np.int64)]
    nh = 0
    for k in range(rays.shape[0]):
        h, tt, uu, vv, ss = ray_ref.ray_tri_np(np.repeat(rays[k:k + 1], tris.shape[0], axis=0), tris)
        if not h.any():
            assert face[k] == ray_ref.MISS and t[k] == np.inf and oid[k] == 0 and not uv[k].any() and side[k] == 0
            continue
        nh += 1
        best = min((tt[f], ids[f], f) for f in np.nonzero(h)[0])
        assert (t[k], oid[k], face[k]) == best and uv[k, 0] == uu[best[2]] and uv[k, 1] == vv[best[2]] and side[k] == ss[best[2]]
    assert nh > 100


def test_argument_errors_of_the_ray_calls_do_not_need_a_device():
    lib = mi355cd.load_library()
    assert lib.cd_cast_rays(None, None, 0, 0, None, None, None, None, None, None) == mi355cd.CD_ERR_ARG
    rays = np.zeros((1, 7)); face = np.zeros(1, dtype=np.uint32)
    assert lib.cd_cast_rays(None, rays.ctypes.data_as(C.c_void_p), 1, 0, face.ctypes.data_as(C.c_void_p), None, None, None, None, None) == mi355cd.CD_ERR_ARG
    assert lib.cd_ray_tri_points(None, None, 4, None, None, None, None) == mi355cd.CD_ERR_ARG
    assert lib.cd_ray_tri_points(rays.ctypes.data_as(C.c_void_p), None, 1, None, None, None, None) == mi355cd.CD_ERR_ARG
    assert C.sizeof(mi355cd.CdRayInfo) == 24 and mi355cd.CD_RAY_ANY == 1


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a box without a GPU")
def test_ray_tri_points_without_a_device_is_an_error_not_a_fallback():
    with pytest.raises(mi355cd.CdError) as e:
        mi355cd.ray_tri_points(np.zeros((2, 7)), np.zeros((2, 3, 3)))
    assert e.value.rc == mi355cd.CD_ERR_NO_DEVICE
