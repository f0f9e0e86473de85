"""The tiny set on the host (mtsgpu_plan_host): path_kernel<*, true, 8, 4>, the megakernel of the
all-diffuse LDS scenes, is built for the Sobol sampler with sample indices below 2^32 alone
(csrc/dmega.h TINY, csrc/layout.h mtsg_tiny_set).  render_plan.cpp plan_tiny_set sends every other
megakernel launch of such a scene, and every one under MTSGPU_NO_TINY_SET, to the generic LDS
kernel path_kernel<*, true, 0, 3>, which holds every choice at run time.

* The benchmark's C1, C2 and C2g plan the tiny-set kernel, 4 waves per SIMD, 32 Sobol dimensions
  in LDS, as before.
* Each disqualifier on its own plans a kernel that holds the code the launch needs, and `scan`
  and `start_queue` read as they did.  Two of them keep path_kernel<*, true, 8, 4>, which keeps
  that code at run time: MTSGPU_NO_SCAN (tests/test_gpu_scan_packed.py pins the name for it), so
  the BVH traversal and the loop without the queue are still in the kernel; and the direct
  integrator, whose launches run direct_kernel -- the word debug counter 15 reports for them is
  the parent's (tests/test_combo_host.py PARENT_WORDS).
"""
import pytest

import bench
from mitsuba_amd import scenes
from mitsuba_amd.integrator import plan_host
from mitsuba_amd.scene import BSDF, DirectIntegrator, PathIntegrator, Sensor, VolpathIntegrator

TINY = 'path_kernel<false, true, 8, 4>'
GENERIC = 'path_kernel<false, true, 0, 3>'
SWITCHES = ('MTSGPU_NO_TINY_SET', 'MTSGPU_NO_SCAN', 'MTSGPU_NO_SCENE_LDS', 'MTSGPU_NO_DIFF_VARIANT', 'MTSGPU_WAVES',
            'MTSGPU_ENGINE', 'MTSGPU_SOBOL_LDS_DIMS', 'MTSGPU_CONTRIB_BYTES')


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _c1(**kw):
    return scenes.build('C1', width=48, height=48, spp=4, rfilter='box', **kw)


def _names(sc, it, **kw):
    p, q = plan_host(sc, it, **kw), plan_host(sc, it, samples=True, **kw)
    assert q['variant']['name'] == p['variant']['name'].replace('<false', '<true', 1)
    assert (q['scan'], q['start_queue'], q['waves']) == (p['scan'], p['start_queue'], p['waves'])
    return p


@pytest.mark.parametrize('cfg', ['C1', 'C2', 'C2g'])
def test_bench_configurations_plan_the_tiny_set_kernel(cfg):
    sc, it = bench.build_scene(cfg)
    p = _names(sc, it, row=(8, 1, 0), tile_shard=True, cus=256, free_bytes=200 << 30)
    assert p['engine'] == 'megakernel' and p['variant']['name'] == TINY
    assert p['waves'] == 4 and p['lds_dims'] == 32 and p['nibbles'] == 8
    assert p['scene_lds'] and p['scan'] and p['start_queue'] and not p['replay']


def test_qualifying_cornell_launches():
    sc, it = _c1()
    for integ in (it, VolpathIntegrator(sampleCount=4, rfilter='box', strictNormals=True),
                  PathIntegrator(sampleCount=4, rfilter='gaussian', maxDepth=2, rrDepth=1)):
        p = _names(sc, integ)
        assert p['variant']['name'] == TINY and p['variant_word'] == 0x1408 and p['waves'] == 4
        assert p['scan'] and p['start_queue']


# ---- the launches routed to the generic kernel ----------------------------------------------
def test_independent_sampler():
    sc, _ = _c1()
    p = _names(sc, PathIntegrator(sampleCount=4, rfilter='box', sampler='independent'))
    assert p['variant']['name'] == GENERIC and p['waves'] == 3 and p['lds_dims'] == 32
    assert p['scene_lds'] and p['scan'] and p['start_queue'] and not p['replay']


@pytest.mark.parametrize('sampler', ['independent-sfmt', 'independent-sfmt-blocks'])
def test_replay(sampler):
    sc, _ = _c1()
    p = _names(sc, PathIntegrator(sampleCount=4, rfilter='box', sampler=sampler))
    assert p['variant']['name'] == GENERIC and p['waves'] == 3
    assert p['replay'] and p['scan'] and not p['start_queue']


def test_index_of_2_to_32():
    """m = 6 for a 48 x 48 window: 2^20 samples per pixel are 32 index bits, 2^20 + 1 are 33"""
    sc, _ = _c1()
    p = _names(sc, PathIntegrator(sampleCount=1 << 20, rfilter='box'))
    assert p['nibbles'] == 8 and p['variant']['name'] == TINY and p['waves'] == 4
    q = _names(sc, PathIntegrator(sampleCount=(1 << 20) + 1, rfilter='box'))
    assert q['nibbles'] == 13 and q['variant']['name'] == GENERIC and q['waves'] == 3
    assert q['scan'] and q['start_queue'] and q['lds_dims'] == 32
    # the benchmark's 1280 x 720 frame is m = 11: 1024 samples per pixel are 22 + 10 bits, 1025 are 33
    sc, it = bench.build_scene('C2')
    it.sampleCount = 1 << 10
    assert plan_host(sc, it)['variant']['name'] == TINY
    it.sampleCount = (1 << 10) + 1
    assert plan_host(sc, it)['variant']['name'] == GENERIC


def test_no_tiny_set_switch(monkeypatch):
    sc, it = _c1()
    monkeypatch.setenv('MTSGPU_NO_TINY_SET', '1')
    p = _names(sc, it)
    assert p['variant']['name'] == GENERIC and p['variant_word'] == 0x1300 and p['waves'] == 3
    assert p['scan'] and p['start_queue'] and p['lds_dims'] == 32
    monkeypatch.setenv('MTSGPU_WAVES', '4')
    assert plan_host(sc, it)['variant']['name'] == 'path_kernel<false, true, 0, 4>'


# ---- the launches the routing leaves alone --------------------------------------------------
def test_no_scan_keeps_the_kernel_and_its_traversal(monkeypatch):
    sc, it = _c1()
    monkeypatch.setenv('MTSGPU_NO_SCAN', '1')
    p = _names(sc, it)
    assert p['variant']['name'] == TINY and p['waves'] == 4
    assert p['scene_lds'] and not p['scan'] and not p['start_queue']
    monkeypatch.setenv('MTSGPU_NO_TINY_SET', '1')
    q = _names(sc, it)
    assert q['variant']['name'] == GENERIC and not q['scan'] and not q['start_queue']


def test_direct_integrator_plans_what_it_did(monkeypatch):
    sc, _ = _c1()
    it = DirectIntegrator(sampleCount=4)
    p = plan_host(sc, it)
    assert p['variant_word'] == 0x1408 and p['scan'] and not p['start_queue']
    monkeypatch.setenv('MTSGPU_NO_TINY_SET', '1')   # not a megakernel launch: the switch does not reach it
    assert plan_host(sc, it)['variant_word'] == 0x1408
    monkeypatch.delenv('MTSGPU_NO_TINY_SET')
    its = DirectIntegrator(sampleCount=4, sampler='independent')
    assert plan_host(sc, its)['variant_word'] == 0x1408


def test_non_diffuse_bsdf():
    sc, it = _c1()
    sc.bsdfs = [BSDF('roughconductor', distribution='ggx', alpha=0.2, material='Au')] + list(sc.bsdfs[1:])
    p = _names(sc, it)
    assert p['variant']['feat'] & 8 == 0 and p['variant']['waves'] == 3 and p['variant']['scene_lds']
    assert p['scan'] and p['start_queue']


def test_lens_sensor():
    sc, it = _c1()
    s = sc.sensor
    sc.sensor = Sensor(type='thinlens', apertureRadius=0.3, nearClip=s.nearClip, farClip=s.farClip, toWorld=s.toWorld,
                       width=s.width, height=s.height, fov=s.fov, fovAxis=s.fovAxis)
    p = _names(sc, it)
    assert p['variant']['name'] == 'path_kernel<false, true, 3079, 3>' and p['scan'] and not p['start_queue']


def test_other_engines_and_scenes_in_hbm(monkeypatch):
    sc, _ = _c1()
    its = PathIntegrator(sampleCount=4, rfilter='box', sampler='independent')
    assert plan_host(sc, its, engine='wavefront')['variant_word'] == 1 << 16
    assert plan_host(sc, its, fields=['position'])['variant_word'] == (1 << 17) | (1 << 12)
    # an all-diffuse scene left in HBM takes the kernel it took, whatever the sampler
    monkeypatch.setenv('MTSGPU_NO_SCENE_LDS', '1')
    v = plan_host(sc, its)['variant']
    assert not v['scene_lds'] and v == plan_host(sc, PathIntegrator(sampleCount=4, rfilter='box'))['variant']
    monkeypatch.setenv('MTSGPU_NO_TINY_SET', '1')
    assert plan_host(sc, its)['variant'] == v
