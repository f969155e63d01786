"""The all-pairs restatement of the all-results item queries (tests/within_ref.py) against the single-answer references, and the
conditions the GPU tests' inputs must meet.  No GPU."""
from __future__ import annotations

import numpy as np
import pytest

import point_ref as ptr
import ray_ref as rr
import within_ref as wr

NAMES = wr.SMALL + ["cloth100"]


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def _same(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        if b.dtype == np.float64:
            a, b = _bits(a), _bits(b)
        assert np.array_equal(a, b), (what, k)


def test_the_meshes_are_the_ones_the_gpu_tests_name():
    assert {"soup10k", "duplicates", "custom_ids", "comb", "n1", "n2", "n3", "n63", "n64", "n65"} == set(wr.SMALL)
    assert wr.MESHES["cloth100"][1].shape[0] == 40_000
    assert all(wr.n_items(name) % 64 for name in wr.SMALL)


@pytest.mark.parametrize("factor", [1.0, 3.0])
@pytest.mark.parametrize("name", NAMES)
def test_per_point_minimum_is_the_closest_point_reference(name, factor):
    v, i, ids, edge = wr.MESHES[name]
    pts, w = wr.points(name), wr.want_points(name, factor)
    n = pts.shape[0]
    want = ptr.closest_points_ref(v, i, ids, pts, factor * edge)
    _same(wr.closest_of(w, n), want, (name, factor))
    assert np.array_equal(wr.rows_per_item(w, n) == 0, want[0] == ptr.NONE)
    assert np.unique(w.rows, axis=0).shape[0] == w.rows.shape[0] and (w.dist <= factor * edge).all()


@pytest.mark.parametrize("name", NAMES)
def test_per_ray_minimum_is_the_closest_hit_reference(name):
    v, i, ids, edge = wr.MESHES[name]
    rays, w = wr.rays(name), wr.want_rays(name)
    n = rays.shape[0]
    want = rr.cast_rays_ref(v, i, ids, rays)
    _same(wr.first_hit_of(w, n), want, name)
    assert np.array_equal(wr.rows_per_item(w, n) == 0, want[0] == rr.MISS)
    assert np.unique(w.rows, axis=0).shape[0] == w.rows.shape[0] and (w.t <= rays[w.rows[:, 0], 6]).all()


def test_the_row_sets_do_not_depend_on_the_chunks():
    v, i, ids, edge = wr.MESHES["n65"]
    a = wr.points_within_ref(v, i, ids, wr.points("n65"), 3 * edge, pairs_per_chunk=1 << 9, threads=1)
    _same(a, wr.want_points("n65", 3.0), "points")
    b = wr.cast_rays_all_ref(v, i, ids, wr.rays("n65"), pairs_per_chunk=1 << 9, threads=1)
    _same(b, wr.want_rays("n65"), "rays")


@pytest.mark.parametrize("name", NAMES)
def test_input_conditions(name):
    """The items of the GPU test of the row sets have rowless items and items with several rows on every mesh (the conditions and
    their figures: within_ref.input_conditions)."""
    wr.input_conditions(name)
