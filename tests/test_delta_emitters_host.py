"""Point, spot and directional emitters, host side: the Python constructors' errors (the
reference's texts), the XML loader and save_scene round trip, `position` / `direction` turned
into the plugins' transforms, mtsgpu_check_scene, and the render plan: a delta scene takes
a DELTA variant word, every other scene keeps the word it had before delta emitters existed.
"""
import os

import numpy as np
import pytest

import delta_ref as dr
from mitsuba_amd import scenes
from mitsuba_amd.integrator import VARIANT_DELTA, MtsgpuError, check_scene, kernel_variant_of, plan_host
from mitsuba_amd.scene import DirectIntegrator, Emitter
from mitsuba_amd.transform import Transform
from mitsuba_amd.xmlscene import SceneError, load_scene, save_scene

f32 = np.float32


def _scene(emitters, **kw):
    return dr.delta_scene(emitters, width=32, height=32, spp=4, **kw)


# ---- constructors ---------------------------------------------------------------------------
def test_constructor_errors_carry_the_reference_texts():
    t = Transform().translate(1, 2, 3)
    with pytest.raises(ValueError, match="Only one of the parameters 'position' and 'toWorld' can be used!'"):
        Emitter('point', position=(0, 1, 0), toWorld=t)                 # point.cpp:62-63
    with pytest.raises(ValueError, match="Only one of the parameters 'direction' and 'toWorld'can be used at a time!"):
        Emitter('directional', direction=(0, -1, 0), toWorld=t)         # directional.cpp:61-62
    with pytest.raises(ValueError, match='Scale factors in the emitter-to-world transformation are not allowed!'):
        Emitter('directional', toWorld=Transform().scale(2.0))          # directional.cpp:69-71
    with pytest.raises(ValueError, match="m_cutoffAngle >= m_beamWidth"):
        Emitter('spot', cutoffAngle=20.0, beamWidth=25.0)               # spot.cpp:74
    with pytest.raises(ValueError):
        Emitter('collimated')


def test_defaults():
    sp = Emitter('spot')
    assert sp.cutoffAngle == 20.0 and sp.beamWidth == 15.0 and sp.intensity == (1.0, 1.0, 1.0)   # spot.cpp:69-71
    assert Emitter('point').radiance == (1.0, 1.0, 1.0) and Emitter('point').toWorld is None
    d = Emitter('directional', irradiance=(3, 2, 1))
    assert d.radiance == (3.0, 2.0, 1.0) and d.samplingWeight == 1.0
    desc = Emitter('spot', intensity=(5, 6, 7), cutoffAngle=30.0).to_desc()
    assert desc.type == 4 and list(desc.radiance) == [5.0, 6.0, 7.0]
    assert desc.cutoff_angle == 30.0 and desc.beam_width == 22.5


def test_position_becomes_translate():
    p = (0.1, -2.7, 3.3)
    e = Emitter('point', position=p)
    m = np.eye(4, dtype=f32)
    m[:3, 3] = np.asarray(p, f32)
    inv = np.eye(4, dtype=f32)
    inv[:3, 3] = -np.asarray(p, f32)
    assert np.array_equal(e.toWorld.m, m) and np.array_equal(e.toWorld.inv, inv)     # transform.cpp:33-47


@pytest.mark.parametrize('direction', [(0.3, -1.0, 0.4), (-2.0, 0.5, 0.1), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0)])
def test_direction_becomes_lookat(direction):
    """directional.cpp:64-67: d = normalize(direction); coordinateSystem(d, u, .);
    lookAt(Point(0), Point(d), u) -- restated here with numpy float32 scalars."""
    e = Emitter('directional', direction=direction)
    a = np.asarray(direction, f32)
    ln = f32(np.sqrt(f32(f32(f32(a[0] * a[0]) + f32(a[1] * a[1])) + f32(a[2] * a[2]))))
    d = (a * f32(f32(1) / ln)).astype(f32)
    if abs(d[0]) > abs(d[1]):                                            # util.cpp:592-601
        il = f32(f32(1) / f32(np.sqrt(f32(f32(d[0] * d[0]) + f32(d[2] * d[2])))))
        c = np.array([f32(d[2] * il), 0, f32(-d[0] * il)], f32)
    else:
        il = f32(f32(1) / f32(np.sqrt(f32(f32(d[1] * d[1]) + f32(d[2] * d[2])))))
        c = np.array([0, f32(d[2] * il), f32(-d[1] * il)], f32)
    u = dr.cross(c, d)
    # lookAt (transform.cpp:191-214): dir = normalize(d - 0), left = normalize(cross(up, dir)), newUp = cross(dir, left)
    t = (d - f32(0)).astype(f32)
    dirv = (t * f32(f32(1) / dr.length(t))).astype(f32)
    left = dr.cross(u, dirv)
    left = (left * f32(f32(1) / dr.length(left))).astype(f32)
    new_up = dr.cross(dirv, left)
    m = np.zeros((4, 4), f32)
    m[:3, 0], m[:3, 1], m[:3, 2], m[3, 3] = left, new_up, dirv, 1
    assert np.array_equal(e.toWorld.m.view(np.uint32), m.view(np.uint32))
    # the emitter's direction trafo(Vector(0, 0, 1)) is the normalised `direction` again, to rounding
    assert np.allclose(e.toWorld.m[:3, 2], d, atol=2e-7)
    assert np.array_equal(e.toWorld.inv[:3, :3], e.toWorld.m[:3, :3].T)


# ---- XML ------------------------------------------------------------------------------------
XML = '''<scene version="0.6.0">
  <integrator type="path"><integer name="maxDepth" value="3"/></integrator>
  <sensor type="perspective">
    <transform name="toWorld"><lookat origin="0, 1, -4" target="0, 1, 0" up="0, 1, 0"/></transform>
    <sampler type="sobol"><integer name="sampleCount" value="4"/></sampler>
    <film type="hdrfilm"><integer name="width" value="16"/><integer name="height" value="16"/>
      <rfilter type="box"/></film>
  </sensor>
  <shape type="cube"><bsdf type="diffuse"/></shape>
  %s
</scene>
'''
DELTAS = '''<emitter type="point"><rgb name="intensity" value="3, 2, 1"/><point name="position" x="0.5" y="3" z="-1"/>
    <float name="samplingWeight" value="2"/></emitter>
  <emitter type="spot"><rgb name="intensity" value="9, 8, 7"/><float name="cutoffAngle" value="30"/>
    <transform name="toWorld"><lookat origin="1, 4, -2" target="0, 0, 0" up="0, 1, 0"/></transform></emitter>
  <emitter type="directional"><rgb name="irradiance" value="1, 2, 4"/><vector name="direction" x="0.2" y="-1" z="0.1"/></emitter>'''


def _write(tmp_path, body):
    p = tmp_path / 'scene.xml'
    p.write_text(XML % body)
    return str(p)


def test_xml_load_and_round_trip(tmp_path):
    sc, it = load_scene(_write(tmp_path, DELTAS))
    pt, sp, di = sc.emitters
    assert (pt.type, sp.type, di.type) == ('point', 'spot', 'directional')
    assert pt.radiance == (3.0, 2.0, 1.0) and pt.samplingWeight == 2.0
    assert np.array_equal(pt.toWorld.m[:3, 3], np.asarray((0.5, 3, -1), f32))
    assert sp.cutoffAngle == 30.0 and sp.beamWidth == 22.5 and sp.radiance == (9.0, 8.0, 7.0)
    assert di.radiance == (1.0, 2.0, 4.0)
    assert np.array_equal(di.toWorld.m, Emitter('directional', direction=(0.2, -1, 0.1)).toWorld.m)
    assert check_scene(sc) is None
    out = tmp_path / 'saved'
    os.makedirs(out)
    sc2, _ = load_scene(save_scene(sc, it, str(out)))
    assert [e.type for e in sc2.emitters] == ['point', 'spot', 'directional']
    for a, b in zip(sc.emitters, sc2.emitters):
        assert a.radiance == b.radiance and a.samplingWeight == b.samplingWeight
        assert np.array_equal(a.toWorld.m, b.toWorld.m)
        assert (a.cutoffAngle, a.beamWidth) == (b.cutoffAngle, b.beamWidth)
    # the spot's transform was built from steps: its carried inverse survives as well
    assert np.array_equal(sc.emitters[1].toWorld.inv, sc2.emitters[1].toWorld.inv)


@pytest.mark.parametrize('body,exc,text', [
    ('<emitter type="point"><point name="position" x="1" y="1" z="1"/><transform name="toWorld">'
     '<translate x="1"/></transform></emitter>', SceneError, "Only one of the parameters 'position'"),
    ('<emitter type="directional"><transform name="toWorld"><scale value="2"/></transform></emitter>', SceneError,
     'Scale factors in the emitter-to-world'),
    ('<emitter type="spot"><texture type="checkerboard" name="texture"/></emitter>', NotImplementedError, 'spot'),
    ('<emitter type="collimated"/>', NotImplementedError, 'collimated'),
    ('<shape type="cube"><emitter type="point"/></shape>', NotImplementedError, 'shape-attached emitter "point"'),
])
def test_xml_errors(tmp_path, body, exc, text):
    with pytest.raises(exc, match=text):
        load_scene(_write(tmp_path, body))


# ---- the C ABI ------------------------------------------------------------------------------
def test_check_scene_accepts_and_refuses():
    E = {'point': Emitter('point', position=(2, 4, 2)), 'spot': Emitter('spot', toWorld=Transform().translate(2, 4, 2)),
         'directional': Emitter('directional', direction=(0, -1, 0.2))}
    for e in E.values():
        assert check_scene(_scene([e])[0]) is None
    assert check_scene(_scene(list(E.values()), keep_area=True)[0]) is None
    # the library's own checks (a caller that bypasses the Python constructors)
    bad = Emitter('spot')
    bad.beamWidth = 30.0
    with pytest.raises(MtsgpuError, match='m_cutoffAngle >= m_beamWidth'):
        check_scene(_scene([bad])[0])
    sc = Emitter('directional')
    sc.toWorld = Transform().scale(2.0)
    with pytest.raises(MtsgpuError, match='Scale factors in the emitter-to-world transformation are not allowed!'):
        check_scene(_scene([sc])[0])


# ---- the plan -------------------------------------------------------------------------------
def test_delta_scene_takes_a_delta_variant(monkeypatch):
    for k in ('MTSGPU_NO_SCENE_LDS', 'MTSGPU_ENGINE', 'MTSGPU_WAVES', 'MTSGPU_NO_DIFF_VARIANT'):
        monkeypatch.delenv(k, raising=False)
    sc, it, _ = _scene([Emitter('point', position=(2, 4, 2))])
    p = plan_host(sc, it)
    assert p['variant_word'] & VARIANT_DELTA and p['variant']['delta'] and p['variant']['feat'] == 1031
    assert p['variant']['name'] == 'path_kernel<false, true, 1031, 3>' and p['scene_lds'] and p['scan']
    assert plan_host(sc, it, samples=True)['variant']['name'] == 'path_kernel<true, true, 1031, 3>'
    assert plan_host(sc, it, engine='wavefront')['variant_word'] == (1 << 16) | VARIANT_DELTA
    assert plan_host(sc, DirectIntegrator(sampleCount=4))['variant_word'] & VARIANT_DELTA
    monkeypatch.setenv('MTSGPU_NO_SCENE_LDS', '1')
    v = plan_host(sc, it)['variant']
    assert v['delta'] and not v['scene_lds'] and v['name'] == 'path_kernel<false, false, 1031, %d>' % v['waves']
    # a mixed scene (area light + environment + delta) runs the same set
    monkeypatch.delenv('MTSGPU_NO_SCENE_LDS')
    mixed = _scene([Emitter('directional', direction=(0, -1, 0.2)), Emitter('constant', radiance=(1, 1, 1))],
                   keep_area=True)[0]
    assert plan_host(mixed, it)['variant']['feat'] == 1031


# variant words of the parent commit (no delta emitters in the library) for the benchmark
# configurations at 64 x 48, 4 spp, read from a run of mtsgpu_plan_host on that commit:
# (plain, plain wavefront, instrumented, instrumented wavefront, direct)
PARENT_WORDS = {
    'C1': (0x1408, 0x10000, 0x3408, 0x10000, 0x1408),
    'C2': (0x1408, 0x10000, 0x3408, 0x10000, 0x1408),
    'C3': (0xc431, 0x10000, 0xe431, 0x10000, 0x401),
    'C4': (0x4450, 0x10000, 0x6450, 0x10000, 0x400),
    'C5': (0xc473, 0x10000, 0xe473, 0x10000, 0x403),
}


@pytest.mark.parametrize('cfg', list(PARENT_WORDS))
def test_other_scenes_keep_their_variant(monkeypatch, cfg):
    for k in ('MTSGPU_NO_SCENE_LDS', 'MTSGPU_ENGINE', 'MTSGPU_WAVES', 'MTSGPU_NO_DIFF_VARIANT', 'MTSGPU_NO_BSDF_SETS',
              'MTSGPU_NO_REFN_SPEC'):
        monkeypatch.delenv(k, raising=False)
    sc, it = scenes.build(cfg, width=64, height=48, spp=4)
    got = tuple(plan_host(sc, it, samples=s, engine=e)['variant_word'] for s in (False, True) for e in (None, 'wavefront'))
    got += (plan_host(sc, DirectIntegrator(sampleCount=4))['variant_word'],)
    assert got == PARENT_WORDS[cfg], [hex(w) for w in got]
    assert not any(w & VARIANT_DELTA for w in got)
    v = kernel_variant_of(got[0])
    assert v is not None and not v['delta']


# ---- the energy test's sample count (tests/test_gpu_delta_emitters.py::test_energy_against_proxy) ----
def test_proxy_calibration(oracle):
    """With the oracle alone at delta_ref.PROXY_SPP: the proxy sphere of radius r against the one
    of radius r / 2 under another scramble passes the 4-standard-error statistic, and a 5%
    intensity error fails it by at least twice the bound."""
    spp, r = dr.PROXY_SPP, dr.PROXY_R
    sc1, it1 = dr.proxy_scene(r, spp, scramble=0)
    sc2, it2 = dr.proxy_scene(r / 2, spp, scramble=0x1234567)
    keep = dr.proxy_mask(sc1, oracle, r)
    assert 0 < (~keep).sum() <= keep.size // 100          # at most 1% of the pixels left out
    a = dr.image_mean(oracle.render(sc1, it1, samples=True, libm_mode=0)[1], keep, spp)
    b = dr.image_mean(oracle.render(sc2, it2, samples=True, libm_mode=0)[1], keep, spp)
    z, z5 = dr.z_score(a, b), dr.z_score(a, b, 1.05)
    print('z', z, 'z at a 5% error', z5)
    assert (z <= 4).all() and (z5 >= 8).all(), (z, z5)
