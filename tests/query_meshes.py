"""The meshes the proximity, continuous collision and swept-tree tests share (no test in here: importing it generates nothing)."""
from __future__ import annotations

import numpy as np

import mi355_synth as synth


def _comb(codes):
    """The 60-level comb of test_cd_gpu.py's deep-tree test: two tiny triangles per Morton code + one spanning triangle."""
    tris = []
    for code in codes:
        c = np.zeros(3)
        for p in range(60):
            if (code >> p) & 1:
                c[{2: 0, 1: 1, 0: 2}[p % 3]] += float(1 << (p // 3))
        c += 0.5
        for s in (0.0, 0.02):
            tris.append([c + [s, 0, 0], c + [s + 0.2, 0.1, 0], c + [s, 0.1, 0.2]])
    tris.append([[-1.0] * 3, [4.0e6, -1.0, -1.0], [-1.0, 4.0e6, 4.0e6]])
    verts = np.asarray(tris, dtype=np.float64).reshape(-1, 3)
    return verts, np.arange(verts.shape[0], dtype=np.uint32).reshape(-1, 3)


def _meshes():
    v, i = synth.soup(10_000, e=0.05, seed=3); yield "soup10k", v, i, None, 0.05
    v, i = synth.soup(100_000, e=0.02, seed=4); yield "soup100k", v, i, None, 0.02
    v, i = synth.cloth_pair(100); yield "cloth100", v, i, None, 2.88 / 100
    v, i = synth.cloth_pair(100, round_f32=False); yield "cloth100d", v, i, None, 2.88 / 100
    v, i = synth.cloth_pair(300); yield "cloth300", v, i, None, 2.88 / 300
    v, i = synth.cloth_pair(300, round_f32=False); yield "cloth300d", v, i, None, 2.88 / 300
    verts, vidx = synth.soup(500, 0.2, 21)
    v2 = np.concatenate([verts, verts[:300]], axis=0)
    dup = (np.arange(300, dtype=np.uint32) + verts.shape[0]).reshape(100, 3)
    vi = np.concatenate([vidx, dup, np.array([[0, 0, 1], [5, 5, 5]], dtype=np.uint32), vidx[:50]], axis=0)
    yield "duplicates", v2, vi, None, 0.2
    v, i = synth.soup(5000, e=0.05, seed=9)
    ids = np.random.default_rng(1).permutation(10 * i.shape[0])[: i.shape[0]].astype(np.uint32)
    yield "custom_ids", v, i, ids, 0.05
    v, i = _comb([1 << (59 - k) for k in range(60)]); yield "comb", v, i, None, 0.2
    for n in (1, 2, 3, 63, 64, 65):
        v, i = synth.soup(n, e=0.3, seed=n); yield f"n{n}", v, i, None, 0.3
