"""scan_pair's plane pairs (dscan.h scan_pair_k, render_plan.cpp mtsg_scan_layout): the
two records of a fan-triangulated quad share plane and vertex A, so a bounce's
pass forms their t, hu and hv once.  Every lane must end with what the
record-by-record scan gives it: per-sample records and films bit-identical to
the oracle (which traverses its BVH) and to a render with MTSGPU_NO_SCAN_PAIRS
set, with equal ray, shadow-ray and triangle-test counters.  64x48 frames."""
import numpy as np
import pytest

from mitsuba_amd import scenes
from mitsuba_amd.integrator import scan_host
from mitsuba_amd.scene import BSDF, Mesh

pytestmark = pytest.mark.gpu

W, H = 64, 48


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _tri_mesh(pts, idx, bsdf=0):
    return Mesh(np.asarray(pts, np.float32), np.asarray(idx, np.uint32), bsdf=bsdf, faceNormals=True)


def _render_both(ctx, sc, it, monkeypatch, **kw):
    """(with pairs, without pairs): the layout is fixed at upload"""
    out = []
    for off in (False, True):
        if off:
            monkeypatch.setenv('MTSGPU_NO_SCAN_PAIRS', '1')
        else:
            monkeypatch.delenv('MTSGPU_NO_SCAN_PAIRS', raising=False)
        ctx.upload(sc)
        out.append(ctx.render(it, **kw) + (ctx.kernel_variant(),))
    monkeypatch.delenv('MTSGPU_NO_SCAN_PAIRS', raising=False)
    return out


def _records_equal(smp_g, smp_o):
    same = np.all(_bits(smp_g) == _bits(smp_o), axis=1)
    assert same.all(), (np.nonzero(~same)[0][:5], smp_g[~same][:2], smp_o[~same][:2])


def _check_records(ctx, oracle, sc, it, monkeypatch):
    assert sum(scan_host(sc)[2]) > 0
    (film_p, smp_p, st_p, v_p), (film_s, smp_s, st_s, v_s) = _render_both(ctx, sc, it, monkeypatch, samples=True,
                                                                          traversal_stats=True)
    assert v_p['instr'] and v_p['scene_lds'] and v_p == v_s
    film_o, smp_o, st_o = oracle.render(sc, it, samples=True, libm_mode=0)
    _records_equal(smp_p, smp_o)
    _records_equal(smp_s, smp_o)
    for k in ('rays', 'shadow_rays'):
        assert st_p[k] == st_s[k] == st_o[k], k
    assert st_p['tri_tests'] == st_s['tri_tests'] > 0
    assert np.array_equal(_bits(film_p), _bits(film_s))
    return film_p


def test_cornell_records_bitexact(gpu_ctx, oracle, monkeypatch):
    sc, it = scenes.build('C1', width=W, height=H, spp=16)
    assert sum(scan_host(sc)[2]) >= 13
    _check_records(gpu_ctx, oracle, sc, it, monkeypatch)


def test_cornell_bench_kernel_bitexact(gpu_ctx, oracle, monkeypatch):
    """without records: the instantiation bench.py times"""
    sc, it = scenes.build('C1', width=W, height=H, spp=16)
    (film_p, smp, st_p, v_p), (film_s, _, st_s, v_s) = _render_both(gpu_ctx, sc, it, monkeypatch)
    assert smp is None and v_p == v_s and v_p['name'] == 'path_kernel<false, true, 8, 4>', v_p
    film_o, _, st_o = oracle.render(sc, it, libm_mode=0)
    assert np.array_equal(_bits(film_p), _bits(film_o))
    assert np.array_equal(_bits(film_p), _bits(film_s))
    for k in ('samples', 'rays', 'shadow_rays', 'path_length_sum'):
        assert st_p[k] == st_s[k] == st_o[k], k


# a pentagon fan in the plane x + z = 4 (one pair, one single), a lone triangle,
# and a quad split (0,1,2),(2,3,0): coplanar, but its triangles' A differ
PENTAGON = [[1.0, 1.0, 3.0], [2.0, 1.0, 2.0], [2.5, 2.0, 1.5], [1.5, 3.0, 2.5], [0.5, 2.0, 3.5]]
LONE = [[3.0, 0.5, 1.0], [4.0, 0.75, 1.5], [3.5, 2.0, 2.25]]
QUAD = [[3.0, 3.0, 2.0], [4.5, 3.0, 2.0], [4.5, 4.0, 3.0], [3.0, 4.0, 3.0]]


def test_pairs_and_singles_records_bitexact(gpu_ctx, oracle, monkeypatch):
    sc, it = scenes.build('C1', width=W, height=H, spp=8)
    sc.bsdfs = list(sc.bsdfs) + [BSDF('diffuse', reflectance=(0.1, 0.3, 0.9))]
    extra = [_tri_mesh(PENTAGON, [[0, 1, 2], [0, 2, 3], [0, 3, 4]], 3), _tri_mesh(LONE, [[0, 1, 2]], 3),
             _tri_mesh(QUAD, [[0, 1, 2], [2, 3, 0]], 3)]
    sc.meshes = sc.meshes[:-1] + extra + [sc.meshes[-1]]
    rec, n, npairs = scan_host(sc)
    first = sc.num_triangles - 2 - 6       # the pentagon's first primitive
    slot = {int(r[10]): i for i, r in enumerate(rec)}
    off = np.concatenate([[0], np.cumsum(n)])
    group = lambda p: int(np.searchsorted(off, slot[p], side='right') - 1)
    paired = lambda p: slot[p] - off[group(p)] < 2 * npairs[group(p)]
    assert sorted(paired(first + i) for i in range(3)) == [False, True, True]
    assert not paired(first + 3) and not paired(first + 4) and not paired(first + 5)
    assert group(first + 4) == group(first + 5)
    # groups with pairs and singles, only pairs and only singles all occur
    kinds = {(npairs[g] > 0, n[g] > 2 * npairs[g]) for g in range(6) if n[g]}
    assert kinds == {(True, True), (True, False), (False, True)}, (n, npairs)
    _check_records(gpu_ctx, oracle, sc, it, monkeypatch)


def _tie_scene(spp, dup_bsdf):
    sc, it = scenes.build('C1', width=W, height=H, spp=spp)
    short = sc.meshes[5]
    sc.bsdfs = list(sc.bsdfs) + [BSDF('diffuse', reflectance=(0.1, 0.3, 0.9))]
    dup = Mesh(short.positions.copy(), short.indices.copy(), bsdf=len(sc.bsdfs) - 1 if dup_bsdf else short.bsdf,
               faceNormals=True)
    degen = _tri_mesh([[0.5, 0.5, 0.5], [1.0, 1.0, 1.0], [1.5, 1.5, 1.5]], [[0, 1, 2]])
    sc.meshes = list(sc.meshes) + [dup, degen]
    return sc, it


def test_ties_across_and_within_pairs_bitexact(gpu_ctx, oracle, monkeypatch):
    """every hit on the short block is an exact-t tie among four coplanar
    records, two pairs: the larger primitive index (the copy) must win"""
    sc, it = _tie_scene(8, True)
    assert sc.num_triangles <= 64
    film = _check_records(gpu_ctx, oracle, sc, it, monkeypatch)
    sc2, it2 = _tie_scene(8, False)
    gpu_ctx.upload(sc2)
    film_2, _, _ = gpu_ctx.render(it2, samples=True)
    assert not np.array_equal(film, film_2)
