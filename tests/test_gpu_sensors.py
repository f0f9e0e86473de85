"""The thinlens, orthographic and telecentric sensors on the GPU (dsensor.h, the MTSG_FEAT_LENS
kernels).

The oracle cannot configure these sensors; it renders such a scene as the pinhole of the same
fov (the twin).  So, as in test_gpu_delta_emitters.py, the checks are restatements
(sensor_ref.py) from the oracle's entry points, compared bit for bit on uint32 views:

1. rays: a field pass's position, distance, normals, shape and primitive index per sample equal
   oracle_intersect of the restated ray; sample positions equal the twin's;
2. the first bounce under one point light (no random number at the first vertex) equals
   delta_ref.first_bounce of the restated first vertices, for path, volpath and direct, with the
   scene in LDS, in HBM and in the wavefront engine;
3. the emitter pick between a point and a spot light (weights 1 and 3) is read from the Sobol
   dimension the aperture draw leaves it at: 5 under a thinlens (next2D skips 4), 2 orthographic;
4. the engines agree at full depth, records and films, on C1 with its area light and under an
   environment map that is in view (the camera-miss lookup with the sensor's differentials):
   LDS, HBM, plain, wavefront, kd-tree, tile and row shards, render_device, three chunked
   launches, the independent sampler, a gaussian film;
5. the SFMT replay samplers are refused.

C1 (and the analytic-shape box) at 32 x 32, 4 spp.  Debug counter 15 must show a LENS
instantiation every time.  On the parent commit Sensor(type=...) does not exist.
"""
import ctypes as C

import numpy as np
import pytest

import delta_ref as dr
import fields_ref as fr
import sensor_ref as sr
from mitsuba_amd import abi, scenes
from mitsuba_amd.integrator import VARIANT_DELTA, VARIANT_LENS, MtsgpuError
from mitsuba_amd.scene import (DirectIntegrator, Emitter, FieldIntegrator, PathIntegrator, Sensor,
                               VolpathIntegrator)

pytestmark = pytest.mark.gpu

f32 = np.float32
SPP, SIZE = 4, 32
UNDEF = (-1.0, -2.0, -3.0)
NO_TRIANGLE = float(0xffffffff)
SENSORS = ('thinlens', 'orthographic', 'telecentric')
NAMES = ['position', 'distance', 'geoNormal', 'shNormal', 'shapeIndex', 'primIndex']


def with_sensor(sc, kind):
    """sc with its perspective sensor replaced: the thinlens focused on the box's middle, the
    two orthographic views through a toWorld that carries scale (3 x 3 units of film)."""
    s = sc.sensor
    W = np.asarray(s.toWorld, f32).reshape(4, 4)
    if kind == 'thinlens':
        sc.sensor = Sensor(type='thinlens', fov=s.fov, fovAxis=s.fovAxis, nearClip=s.nearClip, farClip=s.farClip,
                           toWorld=W, width=s.width, height=s.height, apertureRadius=0.3, focusDistance=10.8)
    else:
        Ws = (W @ np.diag([3.0, 3.0, 1.0, 1.0]).astype(f32)).astype(f32)
        lens = dict(apertureRadius=0.3, focusDistance=10.8) if kind == 'telecentric' else {}
        sc.sensor = Sensor(type=kind, nearClip=s.nearClip, farClip=s.farClip, toWorld=Ws, width=s.width,
                           height=s.height, **lens)
    return sc


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def assert_bits(a, b, what=''):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.argwhere(bits(a) != bits(b))
    assert bad.size == 0, (what, len(bad), bad[:3].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


def set_engine(monkeypatch, engine):
    if engine == 'hbm':
        monkeypatch.setenv('MTSGPU_NO_SCENE_LDS', '1')
    else:
        monkeypatch.delenv('MTSGPU_NO_SCENE_LDS', raising=False)


def check_word(gpu_ctx, engine):
    word = gpu_ctx.debug_counters()[15]
    assert word & VARIANT_LENS, hex(word)
    if engine in ('wavefront', 'kdtree'):
        assert word & (1 << 16), hex(word)
    else:
        assert bool(word & (1 << 12)) == (engine == 'lds'), hex(word)


def render(gpu_ctx, monkeypatch, sc, it, engine, samples=True, **kw):
    set_engine(monkeypatch, engine)
    gpu_ctx.upload(sc)
    eng = engine if engine in ('wavefront', 'kdtree') else None
    out = gpu_ctx.render(it, samples=samples, engine=eng, **kw)
    check_word(gpu_ctx, engine)
    return out


@pytest.fixture(scope='module')
def twin_samples(oracle):
    """The oracle's render of the pinhole twin of C1: sample positions (the same for every
    sensor: dimensions 0, 1), and the aperture samples (dimensions 2, 3)."""
    sc, it = scenes.build('C1', width=SIZE, height=SIZE, spp=SPP)
    it.rfilter = 'box'
    _, smp, _ = oracle.render(sc, it, samples=True, libm_mode=0)
    ax, ay = sr.aperture_samples(oracle, SIZE, SPP)
    return dict(smp=smp, ax=ax, ay=ay, cache={})


# ---- 1. rays --------------------------------------------------------------------------------
RAYS = [(k, m, e) for k in SENSORS for m, e in (('diffuse', 'lds'), ('diffuse', 'hbm'), ('shapes', 'lds'))]


@pytest.mark.parametrize('kind,materials,engine', RAYS, ids=['-'.join(r) for r in RAYS])
def test_rays(gpu_ctx, oracle, monkeypatch, twin_samples, kind, materials, engine):
    sc, it = scenes.build('C1', width=SIZE, height=SIZE, spp=SPP, materials=materials)
    it.rfilter, it.hasAlpha = 'box', True
    sc = with_sensor(sc, kind)
    set_engine(monkeypatch, engine)
    gpu_ctx.upload(sc)
    _, rec, st = gpu_ctx.render_fields(it, [FieldIntegrator(n, undefined=UNDEF) for n in NAMES], samples=True)
    word = gpu_ctx.debug_counters()[15]
    assert word & VARIANT_LENS and word & (1 << 17) and bool(word & (1 << 12)) == (engine == 'lds'), hex(word)
    T = twin_samples
    assert_bits(rec[:, 0:2], T['smp'][:, 4:6], 'samplePos')
    o, d, _, _ = sr.sensor_rays(sc, oracle, rec[:, 0], rec[:, 1], T['ax'], T['ay'])
    its = fr.oracle_intersect(sr.pinhole_twin(sc), oracle, o, d)
    hit = its[:, 0] == 1.0
    assert hit.sum() > hit.size // 2
    assert_bits(rec[:, 2], hit.astype(f32), 'alpha')
    assert_bits(rec[:, 3], hit.astype(f32), 'hit')
    analytic = np.array([m.analytic for m in sc.meshes])[its[:, 14].astype(np.int64)]
    prim = np.where(analytic, NO_TRIANGLE, its[:, 15]).astype(f32)
    want = {'position': its[:, 2:5], 'distance': np.repeat(its[:, 1:2], 3, 1), 'geoNormal': its[:, 5:8],
            'shNormal': its[:, 8:11], 'shapeIndex': np.repeat(its[:, 14:15], 3, 1),
            'primIndex': np.repeat(prim[:, None], 3, 1)}
    for k, n in enumerate(NAMES):
        exp = np.where(hit[:, None], want[n], np.asarray(UNDEF, f32)[None, :])
        assert_bits(rec[:, 4 + 3 * k:7 + 3 * k], exp, (kind, n))
    if kind == 'thinlens':
        # not a pinhole render: most hit positions differ from the twin's
        po, pd, _, _ = fr.primary_rays(sr.pinhole_twin(sc), oracle, rec[:, 0], rec[:, 1])
        pin = fr.oracle_intersect(sr.pinhole_twin(sc), oracle, po, pd)
        both = hit & (pin[:, 0] == 1.0)
        differ = np.any(bits(its[both, 2:5]) != bits(pin[both, 2:5]), 1)
        assert differ.sum() * 2 >= hit.sum(), (differ.sum(), hit.sum())


# ---- 2. the first bounce under one point light ----------------------------------------------
POINT = dict(intensity=(30.0, 24.0, 12.0), position=(2.1, 4.4, 2.4))
KINDS = {
    'path': lambda strict: PathIntegrator(maxDepth=2, sampleCount=SPP, rfilter='box', strictNormals=strict),
    'volpath': lambda strict: VolpathIntegrator(maxDepth=2, sampleCount=SPP, rfilter='box', strictNormals=strict),
    'direct11': lambda strict: DirectIntegrator(sampleCount=SPP, rfilter='box', strictNormals=strict),
    'direct42': lambda strict: DirectIntegrator(sampleCount=SPP, rfilter='box', strictNormals=strict,
                                                emitterSamples=4, bsdfSamples=2),
}
FIRST = [(s, k, e) for s in SENSORS for k in KINDS for e in ('lds', 'hbm', 'wavefront')
         if not (e == 'wavefront' and k.startswith('direct'))]


@pytest.mark.parametrize('kind,integ,engine', FIRST, ids=['-'.join(f) for f in FIRST])
def test_first_bounce(gpu_ctx, oracle, monkeypatch, twin_samples, kind, integ, engine):
    strict = integ in ('volpath', 'direct42')      # strictNormals on for half of them
    em = Emitter('point', **POINT)
    sc, _, twin = dr.delta_scene([em], width=SIZE, height=SIZE, spp=SPP)
    sc, twin = with_sensor(sc, kind), sr.pinhole_twin(with_sensor(twin, kind))
    T = twin_samples
    cache = T['cache']
    if kind not in cache:
        cache[kind] = sr.sensor_first_hits(sc, twin, oracle, T['smp'][:, 4], T['smp'][:, 5], T['ax'], T['ay'])
    key = (kind, integ)
    if key not in cache:
        cache[key] = dr.first_bounce(sc, twin, oracle, cache[kind], 'direct' if integ.startswith('direct') else integ,
                                     em=em, strict=strict, lum_samples=4 if integ == 'direct42' else 1)
    want, info = cache[key]
    assert info['lit'].sum() > 200 and (info['use'] & ~info['lit']).sum() > 20, (info['lit'].sum(), info['use'].sum())
    _, smp, _ = render(gpu_ctx, monkeypatch, sc, KINDS[integ](strict), engine)
    bad = np.nonzero(np.any(bits(smp[:, 0:3]) != bits(want), 1))[0]
    assert bad.size == 0, (kind, integ, engine, bad.size, bad[:4], smp[bad[:4], 0:3], want[bad[:4]])
    assert_bits(smp[:, 4:6], T['smp'][:, 4:6], 'samplePos')
    assert_bits(smp[:, 3], cache[kind]['valid'].astype(f32) * 0 + 1, 'alpha')      # hasAlpha off: 1


@pytest.mark.parametrize('kind', SENSORS)
def test_path_depth2_is_direct(gpu_ctx, monkeypatch, kind):
    sc, _, _ = dr.delta_scene([Emitter('point', **POINT)], width=SIZE, height=SIZE, spp=SPP)
    sc = with_sensor(sc, kind)
    fp, sp, _ = render(gpu_ctx, monkeypatch, sc, KINDS['path'](False), 'lds')
    fd, sd, _ = render(gpu_ctx, monkeypatch, sc, KINDS['direct11'](False), 'lds')
    assert np.array_equal(bits(sp[:, 0:6]), bits(sd[:, 0:6])) and np.array_equal(bits(fp), bits(fd))
    assert sp[:, 0:3].max() > 0


# ---- 3. the engines agree at full depth -----------------------------------------------------
def env_scene():
    """C1's blocks and floor under an environment map, the walls and ceiling gone: the
    background is in view of every sensor."""
    sc, it = scenes.build('C1', width=SIZE, height=SIZE, spp=SPP, max_depth=-1)
    sc.meshes = [sc.meshes[0]] + list(sc.meshes[5:7])
    yy, xx = np.meshgrid(np.arange(16), np.arange(32), indexing='ij')
    img = np.stack([0.2 + 0.05 * xx, 0.3 + 0.04 * yy, 0.5 + 0.01 * (xx + yy)], -1).astype(f32)
    img[3:5, 8:10] = 20.0
    sc.emitters = [Emitter('envmap', bitmap=img)]
    return sc, it


@pytest.mark.parametrize('which', ['area', 'envmap'])
@pytest.mark.parametrize('kind', SENSORS)
def test_engines_agree(gpu_ctx, monkeypatch, kind, which):
    if which == 'area':
        sc, it = scenes.build('C1', width=SIZE, height=SIZE, spp=SPP, max_depth=-1)
    else:
        sc, it = env_scene()
    it.rfilter = 'box'
    sc = with_sensor(sc, kind)
    ref_film, ref_smp, _ = render(gpu_ctx, monkeypatch, sc, it, 'lds')
    assert np.isfinite(ref_smp).all() and ref_smp[:, 0:3].max() > 0 and ref_smp[:, 6].max() > 3
    if which == 'envmap':
        assert (ref_smp[:, 6] == 1).sum() > 100      # camera rays that miss: the filtered lookup
    runs = {'hbm': dict(engine='hbm'), 'wavefront': dict(engine='wavefront'), 'plain': dict(engine='lds', samples=False),
            'plain-hbm': dict(engine='hbm', samples=False)}
    if which == 'area':
        runs['kdtree'] = dict(engine='kdtree')
    for name, kw in runs.items():
        film, smp, _ = render(gpu_ctx, monkeypatch, sc, it, **kw)
        assert np.array_equal(bits(film), bits(ref_film)), (kind, which, name)
        if smp is not None:
            assert np.array_equal(bits(smp), bits(ref_smp)), (kind, which, name)
    # a tile shard and its complement: the records of each equal the whole render's there
    tile = (np.arange(SIZE * SIZE) // SIZE // 8) * (SIZE // 8) + (np.arange(SIZE * SIZE) % SIZE) // 8
    for phase in (0, 1):
        _, smp, _ = render(gpu_ctx, monkeypatch, sc, it, 'lds', row=(0, 2, phase), tile_shard=True)
        mine = np.repeat(tile % 2 == phase, SPP)
        assert np.array_equal(bits(smp[mine]), bits(ref_smp[mine])), (kind, which, phase)
    # a row shard and its complement (blocks of 8 rows), the same way; the two films sum to the whole
    rows = np.arange(SIZE * SIZE) // SIZE // 8
    parts = []
    for phase in (0, 1):
        film, smp, _ = render(gpu_ctx, monkeypatch, sc, it, 'lds', row=(8, 2, phase))
        mine = np.repeat(rows % 2 == phase, SPP)
        assert np.array_equal(bits(smp[mine]), bits(ref_smp[mine])), (kind, which, 'row', phase)
        parts.append(film)
    assert np.array_equal(bits(parts[0] + parts[1]), bits(ref_film)), (kind, which, 'row shards summed')
    # render_device: a torch film on torch's stream
    import torch
    set_engine(monkeypatch, 'lds')
    gpu_ctx.upload(sc)
    dev = torch.zeros(ref_film.shape, dtype=torch.float32, device='cuda')
    gpu_ctx.render_device(it, dev.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    check_word(gpu_ctx, 'lds')
    assert np.array_equal(bits(dev.cpu().numpy()), bits(ref_film)), (kind, which, 'render_device')
    # the independent sampler: the engines among themselves
    it.sampler = 'independent'
    ifilm, ismp, _ = render(gpu_ctx, monkeypatch, sc, it, 'lds')
    assert not np.array_equal(bits(ismp[:, 0:3]), bits(ref_smp[:, 0:3]))
    for eng in ('hbm', 'wavefront'):
        film, smp, _ = render(gpu_ctx, monkeypatch, sc, it, eng)
        assert np.array_equal(bits(film), bits(ifilm)) and np.array_equal(bits(smp), bits(ismp)), (kind, which, eng)
    # a gaussian film
    it.sampler, it.rfilter = 'sobol', 'gaussian'
    gfilm, _, _ = render(gpu_ctx, monkeypatch, sc, it, 'lds')
    for eng in ('hbm', 'wavefront'):
        film, _, _ = render(gpu_ctx, monkeypatch, sc, it, eng)
        assert np.array_equal(bits(film), bits(gfilm)), (kind, which, eng, 'gaussian')


@pytest.mark.parametrize('which', ['area', 'envmap'])
@pytest.mark.parametrize('kind', SENSORS)
def test_chunked_render(gpu_ctx, monkeypatch, kind, which):
    """Three launches (1 MiB of records holds 2 of the 6 samples of 192 x 128 pixels): the later
    launches start at j0 = 2 and 4, which feeds the sample index of the aperture draw and of the
    camera-miss lookup's re-draw."""
    sc, it = (scenes.build('C1', width=192, height=128, spp=6, max_depth=-1) if which == 'area' else env_scene())
    if which == 'envmap':
        sc.sensor = scenes.build('C1', width=192, height=128, spp=6)[0].sensor
        it.sampleCount = 6
    it.rfilter = 'box'
    sc = with_sensor(sc, kind)
    one_film, one_smp, _ = render(gpu_ctx, monkeypatch, sc, it, 'lds')
    assert gpu_ctx.launch_chunks() == 1
    monkeypatch.setenv('MTSGPU_CONTRIB_BYTES', str(1 << 20))
    film, smp, _ = render(gpu_ctx, monkeypatch, sc, it, 'lds')
    assert gpu_ctx.launch_chunks() == 3, gpu_ctx.launch_chunks()
    wfilm, wsmp, _ = render(gpu_ctx, monkeypatch, sc, it, 'wavefront')
    monkeypatch.delenv('MTSGPU_CONTRIB_BYTES')
    assert np.array_equal(bits(film), bits(one_film)) and np.array_equal(bits(smp), bits(one_smp)), (kind, which)
    assert np.array_equal(bits(wfilm), bits(one_film)) and np.array_equal(bits(wsmp), bits(one_smp)), (kind, which)
    if which == 'envmap':
        assert (one_smp[:, 6] == 1).sum() > 1000 and one_smp[one_smp[:, 6] == 1, 0:3].max() > 0


# ---- the dimension shift --------------------------------------------------------------------
@pytest.mark.parametrize('engine', ['lds', 'hbm', 'wavefront'])
@pytest.mark.parametrize('kind', ['thinlens', 'orthographic'])
def test_emitter_pick_dimension(gpu_ctx, oracle, monkeypatch, twin_samples, kind, engine):
    """A point and a spot light with sampling weights 1 and 3: Scene::sampleEmitterDirect picks
    by sample.x of the first nextSample2D() of Li (path.cpp:176).  orthographic draws nothing
    before Li: Sobol dimensions 2, 3.  thinlens has drawn 2, 3 for the aperture, and
    SobolSampler::next2D at dimension 4 skips to the end of the (empty) array range first
    (sobol.cpp:234-235: m_dimension + 1 >= m_arrayStartDim = 5): dimensions 5, 6, so the pick
    is dimension 5 -- neither 2 nor 4.  Restated as test_gpu_delta_emitters.py does."""
    from mitsuba_amd.transform import Transform
    down = Transform().look_at((2.78, 5.2, 2.8), (2.78, 0.0, 2.8), (0.0, 0.0, 1.0))
    pt = Emitter('point', samplingWeight=1.0, **POINT)
    sp = Emitter('spot', intensity=(60.0, 50.0, 30.0), toWorld=down, cutoffAngle=35.0, beamWidth=20.0, samplingWeight=3.0)
    sc, _, twin = dr.delta_scene([pt, sp], width=SIZE, height=SIZE, spp=SPP)
    sc, twin = with_sensor(sc, kind), sr.pinhole_twin(with_sensor(twin, kind))
    T = twin_samples
    cache = T['cache']
    if kind not in cache:
        cache[kind] = sr.sensor_first_hits(sc, twin, oracle, T['smp'][:, 4], T['smp'][:, 5], T['ax'], T['ay'])
    if (kind, 'pick') not in cache:
        L = oracle.lib()
        pix = np.repeat(np.arange(SIZE * SIZE), SPP)
        px, py = pix % SIZE, pix // SIZE
        j = np.tile(np.arange(SPP), SIZE * SIZE)
        m = int(np.log2(SIZE))
        idx = [L.oracle_sobol_lookup(m, int(jj), int(x), int(y), 0) for x, y, jj in zip(px, py, j)]

        def picks(dim):
            u = np.array([L.oracle_sobol_sample(i, dim, 0) for i in idx], f32)
            norm = f32(f32(1) / f32(f32(1) + f32(3)))        # DiscretePDF over the weights {1, 3} (pmf.h)
            cdf = np.array([0, f32(f32(1) * norm), 1], f32)
            pick = np.where(u <= cdf[1], 0, 1)
            pick = np.where(u == 0, 0, pick)
            return pick, (cdf[pick + 1] - cdf[pick]).astype(f32)
        dim = 5 if kind == 'thinlens' else 2
        pick, em_pdf = picks(dim)
        for other in (2, 4, 5):
            if other != dim:      # the test tells the dimensions apart
                assert (picks(other)[0] != pick).sum() > 500, other
        cache[(kind, 'pick')] = dr.first_bounce(sc, twin, oracle, cache[kind], 'path', em=[pt, sp], em_pdf=em_pdf,
                                                pick=pick) + (pick,)
    want, info, pick = cache[(kind, 'pick')]
    assert (pick == 0).sum() > 500 and (pick == 1).sum() > 2000 and info['lit'].sum() > 200
    _, smp, _ = render(gpu_ctx, monkeypatch, sc, KINDS['path'](False), engine)
    assert gpu_ctx.debug_counters()[15] & VARIANT_DELTA
    bad = np.nonzero(np.any(bits(smp[:, 0:3]) != bits(want), 1))[0]
    assert bad.size == 0, (kind, engine, bad.size, bad[:4], smp[bad[:4], 0:3], want[bad[:4]])
    assert_bits(smp[:, 4:6], T['smp'][:, 4:6], 'samplePos')


def test_orthographic_envmap_lookup_ignores_spp(gpu_ctx, monkeypatch):
    """orthographic's differential directions equal the ray's: d + (d - d) * scale is d whatever
    diffScaleFactor = 1 / sqrt(spp) is, so sample 0..3 of a 4 spp and of a 16 spp render agree."""
    sc, it = env_scene()
    it.rfilter, it.maxDepth = 'box', 1
    sc = with_sensor(sc, 'orthographic')
    _, a, _ = render(gpu_ctx, monkeypatch, sc, it, 'lds')
    it.sampleCount = 16
    _, b, _ = render(gpu_ctx, monkeypatch, sc, it, 'lds')
    b = b.reshape(SIZE * SIZE, 16, -1)[:, :SPP].reshape(-1, b.shape[1])
    miss = a[:, 6] == 1
    assert miss.sum() > 100 and a[miss, 0:3].max() > 0
    assert_bits(a[:, 0:6], b[:, 0:6], 'spp')


# ---- 4. refusals ----------------------------------------------------------------------------
@pytest.mark.parametrize('sampler', ['independent-sfmt', 'independent-sfmt-blocks'])
def test_sfmt_replay_is_refused(gpu_ctx, monkeypatch, sampler):
    sc, it = scenes.build('C1', width=SIZE, height=SIZE, spp=SPP)
    it.rfilter = 'box'
    sc = with_sensor(sc, 'thinlens')
    before, _, _ = render(gpu_ctx, monkeypatch, sc, it, 'lds', samples=False)
    it.sampler = sampler
    with pytest.raises(MtsgpuError) as e:
        gpu_ctx.render(it)
    assert e.value.code == abi.EINVAL and 'perspective sensor only' in str(e.value)
    it.sampler = 'sobol'
    after, _, _ = render(gpu_ctx, monkeypatch, sc, it, 'lds', samples=False)
    assert np.array_equal(bits(before), bits(after))
