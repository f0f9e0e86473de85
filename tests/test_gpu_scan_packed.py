"""The tiny-scene scan over the canonical-zero copy of the records (render_plan.cpp
mtsg_scan_layout, dscan.h scan_pair_k / scan_k): the scan's copy of a general record has
+0 for a -0 n_u / n_v (n_d != 0), which pairs two more of the Cornell box's faces.  No
scan can tell the copy from the source, so every render must still equal the oracle's
(which keeps the source records) bit for bit: per-sample records, film and counters,
with the instrumented kernels and with those the benchmark times.  (The cases are those
set for round 12's packed barycentrics and packed clip too, which were measured slower
and are not in the tree, DESIGN.md 4: they cover every loop and exit those forms touched.)

Scenes: C1 (the benchmark's 32 triangles: 15 pairs, the red wall's two singles) in 40x16
and 40x24 frames; the synthetic +-0 quads of test_scan_zero_sign_host.py in the room,
also from the axis camera at sample 0 (direction components that are exactly zero); the
tie scene of test_gpu_scan.py (exact-t ties across and within pairs, a degenerate
record); the tilted panel of test_gpu_clip_rcp.py (the slow aligned pass: pairs tested
as singles); a 120-degree camera (the clip's early exits).
Each also without pairs, through the wavefront engine (scan_k) and without the scan;
`direct` and one trace_rays call with mint = 0 read the same copy."""
import os

import numpy as np
import pytest

from mitsuba_amd import scenes
from mitsuba_amd.integrator import plan_host, scan_host
from mitsuba_amd.scene import DirectIntegrator

from test_gpu_clip_rcp import _grazing_light, _wide_fov
from test_gpu_hoisted import COUNTERS, _bits, _check
from test_gpu_scan import _tie_scene
from test_gpu_scan_pairs import _check_records
from test_scan_zero_sign_host import ORDER, first_prim, zero_sign_scene

pytestmark = pytest.mark.gpu

BENCH_KERNEL = 'path_kernel<false, true, 8, 4>'


def _c1(w, h, spp):
    return lambda: scenes.build('C1', width=w, height=h, spp=spp, rfilter='box')


def _zero_axis():
    sc, it = zero_sign_scene(32, 32, 1, room=True)
    assert it.scramble == 0
    assert np.asarray(sc.sensor.toWorld, np.float32)[:3, 2].tolist() == [0.0, 0.0, 1.0]
    return sc, it


SCENES = {'c1_40x16_1': _c1(40, 16, 1), 'c1_40x16_3': _c1(40, 16, 3), 'c1_40x16_5': _c1(40, 16, 5),
          'c1_40x24_1': _c1(40, 24, 1), 'c1_40x24_3': _c1(40, 24, 3), 'c1_40x24_5': _c1(40, 24, 5),
          'zero_sign': lambda: zero_sign_scene(40, 24, 3, room=True), 'zero_sign_axis': _zero_axis,
          'ties': lambda: _tie_scene(32, 24, 4, True), 'tilted_panel': _grazing_light, 'wide_fov': _wide_fov}
# the environment of a render: the default, and the other readers of the scan's copy
MODES = {'default': {}, 'no_pairs': {'MTSGPU_NO_SCAN_PAIRS': '1'}, 'wavefront': {'MTSGPU_ENGINE': 'wavefront'},
         'no_scan': {'MTSGPU_NO_SCAN': '1'}}


@pytest.fixture(scope='module')
def built():
    return {name: make() for name, make in SCENES.items()}


@pytest.mark.parametrize('instr', [True, False], ids=['instr', 'plain'])
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('name', list(SCENES))
def test_scan_bitexact(gpu_ctx, oracle, monkeypatch, built, name, mode, instr):
    for k in ('MTSGPU_NO_SCAN_PAIRS', 'MTSGPU_ENGINE', 'MTSGPU_NO_SCAN'):
        monkeypatch.delenv(k, raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    sc, it = built[name]
    assert 0 < sc.num_triangles <= 64
    rec, n, npairs = scan_host(sc)
    if mode == 'no_pairs':
        assert sum(npairs) == 0
    else:
        assert sum(npairs) >= 15     # C1's, which every scene here holds
    plan = plan_host(sc, it, samples=instr)
    _check(gpu_ctx, oracle, sc, it, instr)
    # which kernel ran: debug counter 15
    v = gpu_ctx.kernel_variant()
    if mode == 'wavefront':
        assert v is None and plan['engine'] == 'wavefront'
        return
    assert v['scene_lds'] and v['instr'] == instr and plan['scan'] == (mode != 'no_scan'), (v, plan['scan'])
    if name.startswith('c1') and not instr:
        assert v['name'] == BENCH_KERNEL


def test_zero_sign_quads_are_seen_and_pair(gpu_ctx, oracle, monkeypatch, built):
    """the synthetic scene through the pair tests' helper (with and without pairs against the
    oracle, triangle-test counters equal), and its quads are hit: each quad's primitives are
    the closest hit of some rays of a grid through it"""
    sc, it = built['zero_sign']
    _check_records(gpu_ctx, oracle, sc, it, monkeypatch)
    gpu_ctx.upload(sc)
    p0 = first_prim(sc)
    from test_scan_zero_sign_host import QUADS
    for i, q in enumerate(ORDER):
        P = np.asarray(QUADS[q], np.float32)
        s, t = np.meshgrid(np.linspace(0.1, 0.9, 8, dtype=np.float32), np.linspace(0.1, 0.9, 8, dtype=np.float32))
        tgt = P[0] + s.reshape(-1, 1) * (P[1] - P[0]) + t.reshape(-1, 1) * (P[3] - P[0])
        o = np.tile(np.array([[2.75, 2.75, -6.0]], np.float32), (tgt.shape[0], 1))
        d = tgt - o
        hg, _ = gpu_ctx.trace_rays(o, d, mint=0.0)
        ho = oracle.trace_rays(sc, o, d, mint=0.0)
        assert np.array_equal(_bits(hg), _bits(ho)), q
        prims = set(hg[:, 3].view(np.uint32).tolist())
        assert {p0 + 2 * i, p0 + 2 * i + 1} <= prims, (q, prims)


def test_ties_records(gpu_ctx, oracle, monkeypatch, built):
    sc, it = built['ties']
    _check_records(gpu_ctx, oracle, sc, it, monkeypatch)


@pytest.mark.parametrize('mode', ['default', 'no_pairs'])
def test_direct_integrator(gpu_ctx, oracle, monkeypatch, mode):
    """direct_kernel's scan_k reads the same copy"""
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    sc, _ = scenes.build('C1', width=40, height=24, spp=2, rfilter='box')
    it = DirectIntegrator(sampleCount=2, rfilter='box', rfilterParam=0.5, shadingSamples=2)
    _check(gpu_ctx, oracle, sc, it, True)


@pytest.mark.parametrize('shadow', [False, True], ids=['closest', 'shadow'])
def test_trace_rays_mint_zero(gpu_ctx, oracle, shadow):
    """trace_rays takes any mint: 0 here, with origins on the room's surfaces (t = +-0 is
    inside the interval), axis-parallel directions and an infinite maxt"""
    sc, _ = scenes.build('C1', width=8, height=8, spp=1)
    gpu_ctx.upload(sc)
    rng = np.random.default_rng(12)
    lo = np.min([m.positions.min(0) for m in sc.meshes], 0)
    hi = np.max([m.positions.max(0) for m in sc.meshes], 0)
    o = rng.uniform(lo, hi, (4096, 3)).astype(np.float32)
    d = rng.normal(size=(4096, 3)).astype(np.float32)
    face = rng.integers(0, 3, 1024)
    o[np.arange(1024), face] = np.where(rng.random(1024) < 0.5, lo[face], hi[face])   # on the bounds' faces
    d[1024:1536, 0] = 0.0
    d[1536:2048, 1] = -0.0
    d[2048:2304, :2] = 0.0
    hg, _ = gpu_ctx.trace_rays(o, d, mint=0.0, maxt=np.inf, shadow=shadow)
    ho = oracle.trace_rays(sc, o, d, mint=0.0, maxt=np.inf, shadow=shadow)
    assert np.array_equal(_bits(hg), _bits(ho)), np.argwhere(_bits(hg) != _bits(ho))[:5]
    assert 0.05 < np.mean(hg[:, 0] > 0 if shadow else hg[:, 3].view(np.uint32) != 0xffffffff) <= 1.0


@pytest.mark.parametrize('instr', [True, False], ids=['instr', 'plain'])
@pytest.mark.parametrize('name', ['c1_40x24_3', 'zero_sign', 'tilted_panel', 'wide_fov'])
def test_variant_without_canonical_zero(gpu_ctx, built, name, instr):
    """The A/B library built with -DMTSG_SCAN_ZERO_SIGN=0 (make variant V=no_zero), where
    present: the same film, records and counters from the same kernel."""
    from mitsuba_amd import LIB_PATH
    from mitsuba_amd.integrator import Context
    sc, it = built[name]
    gpu_ctx.upload(sc)
    film_p, smp_p, st_p = gpu_ctx.render(it, samples=instr)
    v_p = gpu_ctx.kernel_variant()
    assert v_p['scene_lds'] and v_p['instr'] == instr
    lib = os.path.join(os.path.dirname(LIB_PATH), 'variants', 'libmtsgpu_no_zero.so')
    if os.path.exists(lib):
        ctx = Context(lib_path=lib)
        ctx.upload(sc)
        film_v, smp_v, st_v = ctx.render(it, samples=instr)
        v_v = ctx.kernel_variant()
        ctx.close()
        assert v_v == v_p
        assert np.array_equal(_bits(film_p), _bits(film_v))
        if instr:
            assert np.array_equal(_bits(smp_p), _bits(smp_v))
        for k in COUNTERS:
            assert st_p[k] == st_v[k], (k, st_p[k], st_v[k])
