"""next2d's paired Sobol draws (dsampler.h sobol_sample2): two successive dimensions of one
index share their row addresses when both tables are staged in LDS; a pair that straddles
the staged dimensions, tables in global memory, the independent sampler and the SFMT
replay draw as before.  The pairs of a path are (0,1), (2,3), (5,6), ... (dimension 4 is
the first Russian-roulette draw), so MTSGPU_SOBOL_LDS_DIMS = 1, 3 and 6 split a pair, 0
leaves every table in global memory and 32 is the default.

Each case is one small render compared with the oracle, bit for bit: per-sample records
(where the kernel writes them), film and counters."""
import numpy as np
import pytest

from mitsuba_amd import scenes
from mitsuba_amd.scene import DirectIntegrator, PathIntegrator

pytestmark = pytest.mark.gpu

COUNTERS = ('samples', 'rays', 'shadow_rays', 'path_length_sum')
_oracle_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(gpu_ctx, oracle, key, sc, it, instr, engine=None, **okw):
    """key: the oracle's render of (sc, it) is computed once and shared between the cases"""
    gpu_ctx.upload(sc)
    film_g, smp_g, st_g = gpu_ctx.render(it, samples=instr, engine=engine)
    if key not in _oracle_cache:
        _oracle_cache[key] = oracle.render(sc, it, samples=True, libm_mode=0, **okw)
    film_o, smp_o, st_o = _oracle_cache[key]
    if instr:
        same = np.all(_bits(smp_g) == _bits(smp_o), axis=1)
        bad = np.nonzero(~same)[0]
        assert same.all(), (bad.size, same.size, bad[:3], smp_g[bad[:2]], smp_o[bad[:2]])
    diff = np.argwhere(_bits(film_g) != _bits(film_o))
    assert diff.size == 0, (len(diff), diff[:4])
    for k in COUNTERS:
        assert st_g[k] == st_o[k], (k, st_g[k], st_o[k])
    return st_g


def _c1():
    return scenes.build('C1', width=32, height=32, spp=8, rfilter='box', max_depth=-1)


@pytest.mark.parametrize('instr', [True, False], ids=['instr', 'plain'])
@pytest.mark.parametrize('lds_dims', [0, 1, 3, 4, 6, 7, 32])
def test_megakernel_at_every_split_of_the_staged_dimensions(gpu_ctx, oracle, monkeypatch, lds_dims, instr):
    monkeypatch.setenv('MTSGPU_SOBOL_LDS_DIMS', str(lds_dims))
    sc, it = _c1()
    st = _check(gpu_ctx, oracle, 'c1', sc, it, instr)
    assert st['path_length_sum'] > 3 * st['samples']   # deep paths: pairs well past dimension 7
    v = gpu_ctx.kernel_variant()
    assert v['scene_lds'] and v['instr'] == instr


@pytest.mark.parametrize('lds_dims', [None, 3], ids=['default', 'split3'])
def test_wavefront_engine(gpu_ctx, oracle, monkeypatch, lds_dims):
    if lds_dims is not None:
        monkeypatch.setenv('MTSGPU_SOBOL_LDS_DIMS', str(lds_dims))
    sc, it = _c1()
    _check(gpu_ctx, oracle, 'c1', sc, it, True, engine='wavefront')
    assert gpu_ctx.kernel_variant() is None


@pytest.mark.parametrize('lds_dims', [None, 3], ids=['default', 'split3'])
def test_direct_integrator(gpu_ctx, oracle, monkeypatch, lds_dims):
    if lds_dims is not None:
        monkeypatch.setenv('MTSGPU_SOBOL_LDS_DIMS', str(lds_dims))
    sc, _ = _c1()
    it = DirectIntegrator(sampleCount=8, rfilter='box', rfilterParam=0.5, shadingSamples=2)
    _check(gpu_ctx, oracle, 'c1-direct', sc, it, True)


@pytest.mark.parametrize('instr', [True, False], ids=['instr', 'plain'])
def test_index_of_33_bits_takes_the_13_nibble_tables(gpu_ctx, oracle, instr):
    """a 32768 x 8 film: m = 15, so 8 samples per pixel index the sequence with 2 * 15 + 3
    bits.  (The whole film: a crop window would set the sampler's resolution.)  The eight
    columns at its centre see the box; every other primary ray leaves at once."""
    sc, it = scenes.build('C1', width=32768, height=8, spp=8, rfilter='box', max_depth=-1)
    st = _check(gpu_ctx, oracle, 'c1-wide', sc, it, instr)
    assert st['samples'] == 32768 * 8 * 8 and st['rays'] > st['samples']


@pytest.mark.parametrize('sampler', ['independent', 'independent-sfmt'])
def test_other_samplers_draw_as_before(gpu_ctx, oracle, sampler):
    sc, _ = scenes.build('C1', width=24, height=16, spp=4, rfilter='box')
    it = PathIntegrator(sampleCount=4, rfilter='box', rfilterParam=0.5, sampler=sampler)
    okw = dict(threads=8) if sampler == 'independent-sfmt' else {}
    _check(gpu_ctx, oracle, 'c1-' + sampler, sc, it, True, **okw)
