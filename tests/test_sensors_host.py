"""The thinlens, orthographic and telecentric sensors on the host: descriptor, XML, configure
errors, the launch plan of the MTSG_FEAT_SET_LENS kernels, and the numpy restatement
(sensor_ref.py) the GPU tests compare with, checked here as optics without a GPU."""
import ctypes as C

import numpy as np
import pytest

import delta_ref as dr
import sensor_ref as sr
from mitsuba_amd import abi, scenes
from mitsuba_amd.integrator import VARIANT_DELTA, VARIANT_LENS, MtsgpuError, plan_host
from mitsuba_amd.scene import Emitter, FieldIntegrator, Sensor
from mitsuba_amd.xmlscene import SceneError, load_scene, save_scene

f32 = np.float32
SENSORS = ('thinlens', 'orthographic', 'telecentric')


def c1(kind, **kw):
    sc, it = scenes.build('C1', width=32, height=32, spp=4)
    s = sc.sensor
    args = dict(nearClip=s.nearClip, farClip=s.farClip, toWorld=s.toWorld, width=s.width, height=s.height)
    if kind in ('perspective', 'thinlens'):
        args.update(fov=s.fov, fovAxis=s.fovAxis)
    if kind == 'thinlens':
        args.setdefault('apertureRadius', 0.3)
    args.update(kw)
    sc.sensor = Sensor(type=kind, **args)
    return sc, it


# ---- the descriptor -------------------------------------------------------------------------
def test_descriptor_layout_and_round_trip():
    S = abi.SensorDesc
    assert (S.film_height.offset, S.type.offset, S.aperture_radius.offset, S.focus_distance.offset) == (84, 88, 92, 96)
    assert C.sizeof(S) == 100 and abi.SceneDesc.sensor.offset + C.sizeof(S) <= C.sizeof(abi.SceneDesc)
    assert abi.ABI_VERSION == 8
    assert (abi.SENSOR_PERSPECTIVE, abi.SENSOR_THINLENS, abi.SENSOR_ORTHOGRAPHIC, abi.SENSOR_TELECENTRIC) == (0, 1, 2, 3)
    sc, _ = c1('telecentric', apertureRadius=0.25, focusDistance=7.5)
    d = sc.desc().sensor
    assert (d.type, d.aperture_radius, d.focus_distance) == (abi.SENSOR_TELECENTRIC, 0.25, 7.5)
    d = scenes.build('C1', width=32, height=32, spp=4)[0].desc().sensor
    assert (d.type, d.aperture_radius, d.focus_distance) == (0, 0.0, 0.0)


# ---- defaults and errors of the constructors ------------------------------------------------
def test_defaults_and_errors():
    assert Sensor().type == 'perspective'
    s = Sensor(type='thinlens', apertureRadius=0.0, farClip=50.0)
    assert s.apertureRadius == 1e-4 and s.focusDistance == 50.0        # Epsilon; sensor.cpp:162
    t = Sensor(type='telecentric', farClip=20.0)
    assert t.apertureRadius == 0.0 and t.focusDistance == 20.0
    with pytest.raises(ValueError, match='apertureRadius'):
        Sensor(type='thinlens')
    with pytest.raises(ValueError, match='spherical'):
        Sensor(type='spherical')
    with pytest.raises(ValueError, match='apertureRadius'):
        Sensor(type='orthographic', apertureRadius=0.1)
    scaled = np.diag([2.0, 2.0, 1.0, 1.0]).astype(f32)
    with pytest.raises(ValueError, match='Scale factors in the camera-to-world transformation are not allowed!'):
        Sensor(type='thinlens', apertureRadius=0.1, toWorld=scaled)
    Sensor(type='orthographic', toWorld=scaled)
    Sensor(type='telecentric', toWorld=scaled)


def test_configure_errors_of_the_library():
    sc, it = c1('thinlens')
    sc.sensor.toWorld = (np.asarray(sc.sensor.toWorld, f32) @ np.diag([2.0, 2.0, 1.0, 1.0]).astype(f32)).astype(f32)
    with pytest.raises(MtsgpuError, match='Scale factors in the camera-to-world transformation are not allowed!'):
        plan_host(sc, it)
    sc, it = c1('orthographic', nearClip=5.0, farClip=1.0)
    with pytest.raises(MtsgpuError, match="'nearClip' parameter must be smaller than 'farClip'"):
        plan_host(sc, it)
    sc, it = c1('orthographic')
    d = sc.desc()
    d.sensor.type = 4
    p = it.params(32, 32, 0, 0, 32, 32, 0, 1, 0)
    out, dev, buf = (C.c_uint64 * 64)(), (C.c_uint64 * 3)(256, 0, 0), C.create_string_buffer(1024)
    from mitsuba_amd.integrator import load_library
    assert load_library().mtsgpu_plan_host(C.byref(d), C.byref(p), 0, 0, dev, out, 64, buf, 1024) == abi.EINVAL
    assert b'unknown sensor type' in buf.value


# ---- the launch plan ------------------------------------------------------------------------
@pytest.mark.parametrize('kind', SENSORS)
def test_plan_runs_the_lens_set(kind, monkeypatch):
    sc, it = c1(kind)
    p = plan_host(sc, it)
    assert p['variant_word'] & VARIANT_LENS and not p['variant_word'] & VARIANT_DELTA
    assert p['variant']['feat'] == 3079 and p['variant']['lens'] and p['variant']['scene_lds']
    # the scan runs; the start queue does not
    assert p['scan'] and not p['start_queue']
    assert plan_host(c1('perspective')[0], it)['start_queue']
    monkeypatch.setenv('MTSGPU_NO_SCENE_LDS', '1')
    p = plan_host(sc, it)
    assert p['variant']['feat'] == 3079 and not p['variant']['scene_lds']
    monkeypatch.delenv('MTSGPU_NO_SCENE_LDS')
    assert plan_host(sc, it, engine='wavefront')['variant_word'] == (1 << 16) | VARIANT_LENS
    assert plan_host(sc, it, fields=[FieldIntegrator('distance')])['variant_word'] == (1 << 17) | (1 << 12) | VARIANT_LENS
    sc.emitters = list(sc.emitters) + [Emitter('point', intensity=(1.0, 1.0, 1.0), position=(2.0, 2.0, 2.0))]
    w = plan_host(sc, it)['variant_word']
    assert w & VARIANT_LENS and w & VARIANT_DELTA
    # the perspective sensor's plan is what it was
    assert not plan_host(c1('perspective')[0], it)['variant_word'] & VARIANT_LENS


@pytest.mark.parametrize('sampler', ['independent-sfmt', 'independent-sfmt-blocks'])
def test_plan_refuses_the_sfmt_replay(sampler):
    sc, it = c1('thinlens')
    it.sampler = sampler
    with pytest.raises(MtsgpuError) as e:
        plan_host(sc, it)
    assert e.value.code == abi.EINVAL and 'perspective sensor only' in str(e.value)
    plan_host(c1('perspective')[0], it)


# ---- XML ------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', SENSORS)
def test_xml_round_trip(kind, tmp_path):
    kw = dict(apertureRadius=0.125, focusDistance=9.5) if kind != 'orthographic' else {}
    sc, it = c1(kind, **kw)
    if kind != 'thinlens':
        sc.sensor.toWorld = (np.asarray(sc.sensor.toWorld, f32) @ np.diag([3.0, 3.0, 1.0, 1.0]).astype(f32)).astype(f32)
    a, _ = load_scene(save_scene(sc, it, str(tmp_path / 'a')))
    b, _ = load_scene(save_scene(a, it, str(tmp_path / 'b')))
    for s in (a.sensor, b.sensor):
        assert s.type == kind
        assert (s.apertureRadius, s.focusDistance) == (sc.sensor.apertureRadius, sc.sensor.focusDistance)
        assert np.array_equal(np.asarray(s.toWorld, f32), np.asarray(sc.sensor.toWorld, f32))
        assert (f32(s.nearClip), f32(s.farClip), s.width, s.height) == (f32(sc.sensor.nearClip), f32(sc.sensor.farClip), 32, 32)
    if kind == 'thinlens':
        assert (f32(a.sensor.fov), a.sensor.fovAxis) == (f32(sc.sensor.fov), sc.sensor.fovAxis)
    assert bytes(a.desc().sensor) == bytes(sc.desc().sensor)


def _xml(tmp_path, sensor):
    path = tmp_path / 's.xml'
    path.write_text('<scene version="0.6.0"><integrator type="path"/>%s'
                    '<shape type="sphere"><bsdf type="diffuse"/></shape></scene>' % sensor)
    return str(path)


def test_xml_refusals_and_defaults(tmp_path):
    with pytest.raises(NotImplementedError, match='sensor "spherical" .perspective, thinlens, orthographic, telecentric.'):
        load_scene(_xml(tmp_path, '<sensor type="spherical"/>'))
    with pytest.raises(NotImplementedError, match='shutterOpen != shutterClose'):
        load_scene(_xml(tmp_path, '<sensor type="thinlens"><float name="apertureRadius" value="0.1"/>'
                                  '<float name="shutterClose" value="1"/></sensor>'))
    with pytest.raises(SceneError, match='apertureRadius'):
        load_scene(_xml(tmp_path, '<sensor type="thinlens"/>'))
    with pytest.raises(NotImplementedError, match='animation'):
        load_scene(_xml(tmp_path, '<sensor type="orthographic"><animation name="toWorld"/></sensor>'))
    sc, _ = load_scene(_xml(tmp_path, '<sensor type="thinlens"><float name="apertureRadius" value="0"/>'
                                      '<string name="focalLength" value="35mm"/></sensor>'))
    ref, _ = load_scene(_xml(tmp_path, '<sensor type="perspective"><string name="focalLength" value="35mm"/></sensor>'))
    assert (sc.sensor.fov, sc.sensor.fovAxis) == (ref.sensor.fov, ref.sensor.fovAxis) and sc.sensor.fovAxis == 'diagonal'
    assert sc.sensor.apertureRadius == 1e-4 and sc.sensor.focusDistance == sc.sensor.farClip == 1e4
    sc, _ = load_scene(_xml(tmp_path, '<sensor type="telecentric"/>'))
    assert sc.sensor.apertureRadius == 0.0 and sc.sensor.focusDistance == 1e4


# ---- the restatement as optics --------------------------------------------------------------
def _wall_scene(kind, oracle, focus=10.0, radius=1.0):
    """A sensor at the origin looking down +z (toWorld scaled 3 x 3 for the orthographic ones)."""
    W = np.eye(4, dtype=f32)
    kw = dict(nearClip=0.1, farClip=100.0, width=32, height=32)
    if kind == 'thinlens':
        sensor = Sensor(type=kind, fov=40.0, apertureRadius=radius, focusDistance=focus, toWorld=W, **kw)
    else:
        lens = dict(apertureRadius=radius, focusDistance=focus) if kind == 'telecentric' else {}
        sensor = Sensor(type=kind, toWorld=np.diag([3.0, 3.0, 1.0, 1.0]).astype(f32), **lens, **kw)
    sc, _ = scenes.build('C1', width=32, height=32, spp=4)
    sc.sensor = sensor
    return sc


def _film_samples():
    py, px = np.meshgrid(np.arange(32), np.arange(32), indexing='ij')
    sx = (px.reshape(-1) + 0.5).astype(f32)
    sy = (py.reshape(-1) + 0.5).astype(f32)
    rng = np.random.RandomState(7)
    return sx, sy, rng.rand(sx.size).astype(f32), rng.rand(sx.size).astype(f32)


def _at_z(o, d, z):
    t = (z - o[:, 2].astype(np.float64)) / d[:, 2].astype(np.float64)
    return o.astype(np.float64) + d.astype(np.float64) * t[:, None], t


def test_orthographic_restatement(oracle):
    sx, sy, _, _ = _film_samples()
    sc = _wall_scene('orthographic', oracle)
    o, d, mint, maxt = sr.sensor_rays(sc, oracle, sx, sy)
    assert (d == np.array([0, 0, 1], f32)).all() and (mint == f32(0.1)).all() and (maxt == f32(100.0)).all()
    a, t = _at_z(o, d, 10.0)
    assert np.array_equal(t, np.full(t.shape, 10.0)) and np.array_equal(a[:, :2], o[:, :2].astype(np.float64))
    # the film spans [-1, 1]^2 of camera space, 3 units of world per camera unit, x and y mirrored
    # (Transform::scale(-0.5, -0.5 * aspect, 1)); adjacent pixel centres are one dx apart
    m, dx, dy = sr.ortho_matrices(sc.sensor)
    grid = o.reshape(32, 32, 3)
    assert np.allclose(grid[0, 0, :2], [3 * (1 - 1 / 32), 3 * (1 - 1 / 32)], atol=1e-5)
    assert np.allclose(grid[:, 1:, 0] - grid[:, :-1, 0], 3 * dx[0], atol=2e-6) and dx[0] < 0 and dx[1] == 0 == dx[2]
    assert np.allclose(grid[1:, :, 1] - grid[:-1, :, 1], 3 * dy[1], atol=2e-6) and dy[1] < 0


# ---- the restatement is a lens --------------------------------------------------------------
# A diffuse checkerboard wall perpendicular to the optical axis at exactly focusDistance, one
# point light, maxDepth 2, 32 x 32, 4 spp.  In exact arithmetic a lens ray meets the wall where
# the pinhole ray of the same film position does, and a diffuse wall's radiance does not depend
# on the view: Li of the restated lens rays equals Li of the twin's rays sample by sample.  The
# twin's Li is delta_ref.first_hits + first_bounce: the oracle cannot configure a point light,
# and that restatement from its entry points is what the GPU's delta-emitter tests pin.
WALL_Z, WALL_HALF, CHECKER = 10.0, 6.0, 2.0           # 4 x 4 checker cells of 3 units
# the largest relative difference measured over the samples whose two hit points share a
# checker cell (deterministic inputs); the assertion allows twice that (another numpy / libm)
MEASURED = {'thinlens': 9.994e-07, 'telecentric': 4.581e-07}


def _lens_wall(kind, focus):
    from mitsuba_amd.scene import BSDF, Checkerboard, Mesh, PathIntegrator, Scene
    h, z = WALL_HALF, WALL_Z
    pos = np.array([[-h, -h, z], [-h, h, z], [h, h, z], [h, -h, z]], f32)      # normal -z: towards the sensor
    uv = np.array([[0, 0], [0, 1], [1, 1], [1, 0]], f32)
    wall = Mesh(pos, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), texcoords=uv, bsdf=0, faceNormals=True)
    tex = Checkerboard(color0=(0.7, 0.6, 0.5), color1=(0.2, 0.3, 0.4), uscale=CHECKER, vscale=CHECKER)
    em = Emitter('point', intensity=(40.0, 30.0, 20.0), position=(1.0, 2.0, 5.0))
    kw = dict(nearClip=0.1, farClip=100.0, width=32, height=32)
    if kind in ('perspective', 'thinlens'):
        lens = dict(apertureRadius=WALL_Z / 10, focusDistance=focus) if kind == 'thinlens' else {}
        sensor = Sensor(type=kind, fov=40.0, toWorld=np.eye(4, dtype=f32), **lens, **kw)
    else:
        lens = dict(apertureRadius=WALL_Z / 10, focusDistance=focus) if kind == 'telecentric' else {}
        sensor = Sensor(type=kind, toWorld=np.diag([3.0, 3.0, 1.0, 1.0]).astype(f32), **lens, **kw)
    sc = Scene(sensor, [wall], [BSDF('diffuse', reflectance=tex)], [em])
    # the twin the oracle intersects and traces: the same wall, emitting (the oracle needs an emitter
    # it can configure; hits and occlusion do not depend on emission)
    import copy
    twin = sr.pinhole_twin(sc)
    twin.meshes = [copy.copy(wall)]
    twin.meshes[0].emitter = 0
    twin.emitters = [Emitter('area', radiance=(1.0, 1.0, 1.0))]
    return sc, twin, em, PathIntegrator(maxDepth=2, sampleCount=4, rfilter='box')


@pytest.fixture(scope='module')
def film_samples(oracle):
    """The oracle's sample positions of a 32 x 32, 4 spp render (dimensions 0, 1: any scene) and
    its Sobol dimensions 2, 3, the aperture sample."""
    sc, it = scenes.build('C1', width=32, height=32, spp=4)
    it.rfilter = 'box'
    _, smp, _ = oracle.render(sc, it, samples=True, libm_mode=0)
    return (smp[:, 4].copy(), smp[:, 5].copy()) + sr.aperture_samples(oracle, 32, 4)


def _cells(uv):
    return np.floor(uv.astype(np.float64) * 2 * CHECKER).astype(np.int64)


def _compare(oracle, kind, focus, samples):
    """Li of `kind`'s restated rays against Li of its in-focus reference (the pinhole twin for
    thinlens, the orthographic restatement for telecentric): the relative differences of the
    hit samples that share a checker cell, and how many hit samples do not."""
    sx, sy, ax, ay = samples
    sc, twin, em, _ = _lens_wall(kind, focus)
    H = sr.sensor_first_hits(sc, twin, oracle, sx, sy, ax, ay)
    if kind == 'thinlens':
        rsc, rtwin, _, _ = _lens_wall('perspective', focus)
        R = dr.first_hits(rsc, rtwin, oracle, sx, sy)
    else:
        rsc, rtwin, _, _ = _lens_wall('orthographic', focus)
        R = sr.sensor_first_hits(rsc, rtwin, oracle, sx, sy)
    a, _ = dr.first_bounce(sc, twin, oracle, H, 'path', em=em)
    b, _ = dr.first_bounce(rsc, rtwin, oracle, R, 'path', em=em)
    hit = H['valid'] & R['valid']
    same = hit & np.all(_cells(H['uv']) == _cells(R['uv']), 1)
    assert hit.sum() == hit.size and b[hit].min() > 0          # every ray meets the lit wall
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.abs(a.astype(np.float64) - b) / b
    return rel.max(1), hit, same, H, R


@pytest.mark.parametrize('kind', ['thinlens', 'telecentric'])
def test_restatement_is_a_lens(oracle, film_samples, kind):
    rel, hit, same, H, R = _compare(oracle, kind, WALL_Z, film_samples)
    worst = rel[same].max()
    print('%s: largest relative difference %.3e over %d samples, %d left out' % (kind, worst, same.sum(), (hit & ~same).sum()))
    assert (hit & ~same).sum() <= hit.sum() // 100
    tol = 2 * MEASURED[kind]
    assert worst <= tol, (worst, tol)
    # the aperture is used: most origins differ from the reference ray's
    assert (np.abs(H['o'] - (R['o'] if 'o' in R else 0)).max(1) > 0.05).mean() > 0.9
    # negative control: focused 25% off, more than 10% of the hit samples are outside the tolerance
    rel, hit, same, _, _ = _compare(oracle, kind, WALL_Z * 1.25, film_samples)
    out = hit & ~(rel <= tol)
    print('%s defocused: %d of %d outside' % (kind, out.sum(), hit.sum()))
    assert out.sum() * 10 > hit.sum()


def test_orthographic_rays_hit_the_wall(oracle, film_samples):
    sx, sy, _, _ = film_samples
    sc, twin, _, _ = _lens_wall('orthographic', WALL_Z)
    H = sr.sensor_first_hits(sc, twin, oracle, sx, sy)
    assert H['valid'].all() and (H['its'][:, 1] == f32(WALL_Z)).all()          # at the wall's distance
    # the hit's camera-space x, y are the origin's (toWorld: x, y scaled by 3, exactly)
    assert np.array_equal(H['p'][:, 0:2], H['o'][:, 0:2])
