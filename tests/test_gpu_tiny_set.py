"""The tiny-set megakernel on the GPU: path_kernel<*, true, 8, 4> holds the Sobol sampler with
8-nibble indices as compile-time constants (csrc/dmega.h TINY), and render_plan.cpp plan_tiny_set
sends every other megakernel launch of an all-diffuse LDS scene to the generic LDS kernel.

Each case is one small Cornell box render, 48 x 48 to 64 x 64 pixels at 4 to 16 samples (20 where
the smallest record budget the library takes must split a 64 x 64 gaussian render in three).  The
instrumented kernel's per-sample records are compared with the oracle's bit for bit, the
uninstrumented kernel's film and four counters with the oracle's; then the same scene and
settings are rendered with MTSGPU_NO_TINY_SET=1 -- the generic kernel -- and film, records and
counters are equal while debug counter 15 names the other kernel.  The oracle renders each case
once (_ORACLE), shared by its four renders.

The launches routed away from the kernel -- the independent sampler, a Sobol index beyond 32
bits -- and MTSGPU_NO_SCAN, which keeps the kernel and its BVH traversal, are compared with the
oracle the same way.
"""
import numpy as np
import pytest

from mitsuba_amd import scenes
from mitsuba_amd.scene import PathIntegrator, VolpathIntegrator
from test_gpu_hoisted import COUNTERS, _bits

pytestmark = pytest.mark.gpu

PASSES, RETIRED = 11, 12          # debug counters: production passes, samples retired in them
TINY_WORD, GENERIC_WORD, INSTR_BIT = 0x1408, 0x1300, 1 << 13
BUDGET = 1 << 20                  # the smallest MTSGPU_CONTRIB_BYTES the library takes
INSTR = pytest.mark.parametrize('instr', [True, False], ids=['instr', 'plain'])
_ORACLE = {}


def _c1(w, h, spp, rfilter='box', **kw):
    return scenes.build('C1', width=w, height=h, spp=spp, rfilter=rfilter, **kw)


def _straddle():
    """40 x 45 pixels off the tile grid whose left columns look past the box: a wave's 64 items
    hold retired samples, queued ones and the padding of the window's last tiles"""
    sc, it = _c1(64, 48, 5)
    sc.sensor.fov = 75.0
    it.crop = (0, 2, 40, 45)
    return sc, it


def _max_depth(d):
    return lambda: _c1(48, 48, 4, max_depth=d)


def _rr_depth_one():
    """(maxDepth 8: with roulette from the first vertex a path's throughput stays near 1, and
    without a depth limit a few paths of 18432 outlive the sampler's 1024 dimensions)"""
    sc, it = _c1(48, 48, 8, max_depth=8)
    it.rrDepth = 1
    return sc, it


def _volpath():
    sc, _ = _c1(48, 48, 4)
    return sc, VolpathIntegrator(sampleCount=6, rfilter='box', maxDepth=6, rrDepth=2)


def _strict_normals():
    sc, it = _c1(48, 48, 4)
    it.strictNormals = True
    return sc, it


def _alpha():
    sc, it = _c1(56, 48, 4)
    sc.sensor.fov = 75.0
    it.hasAlpha = True
    return sc, it


def _sees_nothing():
    sc, it = _c1(64, 64, 4)
    sc.sensor.fov = 120.0
    it.crop = (0, 0, 13, 11)
    return sc, it


# name: (scene and integrator, row shard, tile shard, environment)
CASES = {
    'straddle': (_straddle, (1, 1, 0), False, {}),
    'max_depth_1': (_max_depth(1), (1, 1, 0), False, {}),
    'max_depth_2': (_max_depth(2), (1, 1, 0), False, {}),
    'rr_depth_1': (_rr_depth_one, (1, 1, 0), False, {}),
    'volpath': (_volpath, (1, 1, 0), False, {}),
    'strict_normals': (_strict_normals, (1, 1, 0), False, {}),
    'alpha': (_alpha, (1, 1, 0), False, {}),
    'gaussian_gather': (lambda: _c1(48, 48, 5, 'gaussian'), (1, 1, 0), False, {}),
    'three_launches': (lambda: _c1(64, 64, 20, 'gaussian'), (1, 1, 0), False, {'MTSGPU_CONTRIB_BYTES': str(BUDGET)}),
    'tile_shard': (lambda: _c1(56, 48, 5), (8, 3, 2), True, {'MTSGPU_ROUND_SHIFT': '1'}),
    'sees_nothing': (_sees_nothing, (1, 1, 0), False, {}),
}


def _oracle(oracle, key, sc, it, row=(1, 1, 0), tile_shard=False, **okw):
    if key not in _ORACLE:
        _ORACLE[key] = oracle.render(sc, it, samples=True, libm_mode=0, row=row, tile_shard=tile_shard, **okw)
    return _ORACLE[key]


def _render(gpu_ctx, sc, it, instr, row=(1, 1, 0), tile_shard=False):
    gpu_ctx.upload(sc)
    film, smp, st = gpu_ctx.render(it, samples=instr, row=row, tile_shard=tile_shard)
    return film, smp, st, gpu_ctx.debug_counters()


def _equal(got, ref, instr):
    film_g, smp_g, st_g = got[:3]
    film_r, smp_r, st_r = ref[:3]
    if instr:
        same = np.all(_bits(smp_g) == _bits(smp_r), axis=1)
        bad = np.nonzero(~same)[0]
        assert same.all(), (bad.size, same.size, bad[:3], smp_g[bad[:2]], smp_r[bad[:2]])
    diff = np.argwhere(_bits(film_g) != _bits(film_r))
    assert diff.size == 0, (len(diff), diff[:4])
    for k in COUNTERS:
        assert st_g[k] == st_r[k], (k, st_g[k], st_r[k])


@INSTR
@pytest.mark.parametrize('name', list(CASES))
def test_tiny_set_kernel_and_its_fallback(gpu_ctx, oracle, monkeypatch, name, instr):
    make, row, tile_shard, env = CASES[name]
    for k in ('MTSGPU_NO_TINY_SET', 'MTSGPU_NO_SCAN', 'MTSGPU_CONTRIB_BYTES', 'MTSGPU_ROUND_SHIFT'):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc, it = make()
    ref = _oracle(oracle, name, sc, it, row, tile_shard)
    tiny = _render(gpu_ctx, sc, it, instr, row, tile_shard)
    c = tiny[3]
    assert c[15] == TINY_WORD | (INSTR_BIT if instr else 0), hex(c[15])
    _equal(tiny, ref, instr)
    st = tiny[2]
    assert c[PASSES] > 0                                   # the start queue
    if name == 'straddle':
        assert 0 < c[RETIRED] < st['samples'] and st['samples'] == 40 * 45 * 5
    if name == 'sees_nothing':
        assert c[RETIRED] == st['samples'] == st['rays'] == 13 * 11 * 4 and st['shadow_rays'] == 0
    if name == 'max_depth_1':
        assert st['path_length_sum'] == st['samples']
    if name == 'three_launches':
        assert gpu_ctx.launch_chunks() == 3
    if name == 'alpha':
        assert c[RETIRED] > 0                              # samples of alpha 0
    monkeypatch.setenv('MTSGPU_NO_TINY_SET', '1')
    gen = _render(gpu_ctx, sc, it, instr, row, tile_shard)
    g = gen[3]
    assert g[15] == GENERIC_WORD | (INSTR_BIT if instr else 0), hex(g[15])
    _equal(gen, tiny, instr)
    assert (g[PASSES], g[RETIRED]) == (c[PASSES], c[RETIRED])


# ---- launches outside the set ---------------------------------------------------------------
@INSTR
def test_independent_sampler_takes_the_generic_kernel(gpu_ctx, oracle, monkeypatch, instr):
    monkeypatch.delenv('MTSGPU_NO_TINY_SET', raising=False)
    sc, _ = _c1(48, 48, 4)
    it = PathIntegrator(sampleCount=5, rfilter='box', sampler='independent')
    got = _render(gpu_ctx, sc, it, instr)
    assert got[3][15] == GENERIC_WORD | (INSTR_BIT if instr else 0) and got[3][PASSES] > 0
    _equal(got, _oracle(oracle, 'independent', sc, it), instr)


@INSTR
def test_index_beyond_32_bits_takes_the_generic_kernel(gpu_ctx, oracle, monkeypatch, instr):
    """a 32768 x 2 film is m = 15: 5 samples per pixel index the sequence with 30 + 3 bits (the
    whole film: a crop window would set the sampler's resolution).  The columns at its centre
    see the box."""
    monkeypatch.delenv('MTSGPU_NO_TINY_SET', raising=False)
    sc, it = _c1(32768, 2, 5)
    got = _render(gpu_ctx, sc, it, instr)
    assert got[3][15] == GENERIC_WORD | (INSTR_BIT if instr else 0)
    _equal(got, _oracle(oracle, 'wide', sc, it), instr)
    assert got[2]['samples'] == 32768 * 2 * 5 and got[2]['rays'] > got[2]['samples']
    # one sample fewer per pixel is 32 bits: the tiny-set kernel
    it4 = PathIntegrator(sampleCount=4, rfilter='box')
    assert _render(gpu_ctx, sc, it4, instr)[3][15] == TINY_WORD | (INSTR_BIT if instr else 0)


@INSTR
def test_no_scan_keeps_the_kernel(gpu_ctx, oracle, monkeypatch, instr):
    """MTSGPU_NO_SCAN=1: the kernel's run-time BVH traversal and its loop without the queue"""
    monkeypatch.delenv('MTSGPU_NO_TINY_SET', raising=False)
    sc, it = _straddle()
    monkeypatch.setenv('MTSGPU_NO_SCAN', '1')
    got = _render(gpu_ctx, sc, it, instr)
    assert got[3][15] == TINY_WORD | (INSTR_BIT if instr else 0) and got[3][PASSES] == 0
    _equal(got, _oracle(oracle, 'straddle', sc, it), instr)
