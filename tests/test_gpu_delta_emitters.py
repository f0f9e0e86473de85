"""Point, spot and directional emitters on the GPU (ddelta.h, the MTSG_FEAT_DELTA kernels).

The oracle cannot configure a delta emitter, so nothing here compares against an oracle
render of the same scene.  Instead (delta_ref.py):

* the first bounce is restated in numpy float32 from the oracle's entry points -- the camera
  ray, oracle_intersect for the first vertex, the emitter's sampleDirect in the reference's
  operation order, oracle_trace_rays for the shadow ray (or volpath's segment),
  oracle_bsdf_eval -- and compared with the per-sample records bit for bit;
* the engines (megakernel with the scene in LDS and in HBM, instrumented and plain, the
  wavefront engine, chunked launches, a tile shard) must agree bit for bit at full depth;
* the energy of a point light is compared with the oracle's render of a small radiant sphere.

The scene is C1 at 32 x 32, 4 spp: the ceiling light quad is plain white geometry and the
delta emitters are the scene's emitters; the oracle gets the geometry twin (the quad emits).
Debug counter 15 must show that a DELTA instantiation ran.  On the parent commit every
upload here fails with 'unsupported emitter type'.

Not covered: the restatement of the single MIS term of a BSDF-sampled
area-light hit in a mixed scene: at maxDepth 2 that sample's Li also holds the first vertex's emitter sample, which in the
mixed scene may be the area light's (triangle sampling, no oracle entry point), so it is
not restated here; the engines-agree test (which runs that scene at full depth) and the
energy test are its cover.
"""
import numpy as np
import pytest

import delta_ref as dr
from mitsuba_amd.integrator import VARIANT_DELTA
from mitsuba_amd.scene import DirectIntegrator, Emitter, PathIntegrator, VolpathIntegrator
from mitsuba_amd.transform import Transform

pytestmark = pytest.mark.gpu

SPP, SIZE = 4, 32
BUDGET = 1 << 20      # the smallest MTSGPU_CONTRIB_BYTES the library takes


def _emitters():
    down = Transform().look_at((2.78, 5.2, 2.8), (2.78, 0.0, 2.8), (0.0, 0.0, 1.0))
    return {
        'point': Emitter('point', intensity=(30.0, 24.0, 12.0), position=(2.1, 4.4, 2.4)),
        # the beam edge (20 deg) lies on the floor, the cutoff edge (35 deg) on the walls
        'spot': Emitter('spot', intensity=(60.0, 50.0, 30.0), toWorld=down, cutoffAngle=35.0, beamWidth=20.0),
        'dir_direction': Emitter('directional', irradiance=(3.0, 2.5, 1.5), direction=(0.3, -1.0, 0.4)),
        'dir_toworld': Emitter('directional', irradiance=(3.0, 2.5, 1.5),
                               toWorld=Transform().rotate((1.0, 0.0, 0.0), 70.0)),
    }


KINDS = {
    'path': lambda strict: PathIntegrator(maxDepth=2, sampleCount=SPP, rfilter='box', strictNormals=strict),
    'volpath': lambda strict: VolpathIntegrator(maxDepth=2, sampleCount=SPP, rfilter='box', strictNormals=strict),
    'direct11': lambda strict: DirectIntegrator(sampleCount=SPP, rfilter='box', strictNormals=strict),
    'direct42': lambda strict: DirectIntegrator(sampleCount=SPP, rfilter='box', strictNormals=strict,
                                                emitterSamples=4, bsdfSamples=2),
}
ENGINES = ('lds', 'hbm', 'wavefront')


@pytest.fixture(scope='module')
def base(oracle):
    """The oracle's view of the shared geometry: sample positions, alpha and first vertices."""
    sc, it, twin = dr.delta_scene([_emitters()['point']], width=SIZE, height=SIZE, spp=SPP)
    _, smp, _ = oracle.render(twin, it, samples=True, libm_mode=0)
    H = dr.first_hits(sc, twin, oracle, smp[:, 4], smp[:, 5])
    return dict(smp=smp, H=H, twin=twin, cache={})


def _render(gpu_ctx, monkeypatch, sc, it, engine, samples=True, **kw):
    if engine == 'hbm':
        monkeypatch.setenv('MTSGPU_NO_SCENE_LDS', '1')
    else:
        monkeypatch.delenv('MTSGPU_NO_SCENE_LDS', raising=False)
    gpu_ctx.upload(sc)
    film, smp, st = gpu_ctx.render(it, samples=samples, engine='wavefront' if engine == 'wavefront' else None, **kw)
    word = gpu_ctx.debug_counters()[15]
    assert word & VARIANT_DELTA, hex(word)
    if engine == 'wavefront':
        assert word & (1 << 16), hex(word)
    else:
        assert bool(word & (1 << 12)) == (engine == 'lds'), hex(word)
    return film, smp, st


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_records(smp, want_li, base, what):
    bad = np.nonzero(np.any(_bits(smp[:, 0:3]) != _bits(want_li), 1))[0]
    assert bad.size == 0, (what, bad.size, bad[:4], smp[bad[:4], 0:3], want_li[bad[:4]])
    # sample positions and alpha: the oracle's render of the twin
    assert np.array_equal(_bits(smp[:, 3:6]), _bits(base['smp'][:, 3:6])), what


# ---- 1. the first bounce, bit for bit -------------------------------------------------------
# (the direct integrator has no wavefront engine)
FIRST = [(c, k, e) for c in ('point', 'spot', 'dir_direction', 'dir_toworld') for k in KINDS for e in ENGINES
         if not (e == 'wavefront' and k.startswith('direct'))]


@pytest.mark.parametrize('case,kind,engine', FIRST, ids=['-'.join(f) for f in FIRST])
def test_first_bounce_restatement(gpu_ctx, oracle, monkeypatch, base, case, kind, engine):
    strict = case in ('spot', 'dir_toworld')      # the strictNormals test on two of the four
    em = _emitters()[case]
    sc, _, twin = dr.delta_scene([em], width=SIZE, height=SIZE, spp=SPP)
    it = KINDS[kind](strict)
    key = (case, kind)
    if key not in base['cache']:
        base['cache'][key] = dr.first_bounce(sc, twin, oracle, base['H'], 'direct' if kind.startswith('direct') else kind,
                                             em=em, strict=strict, lum_samples=4 if kind == 'direct42' else 1)
    want, info = base['cache'][key]
    # the case shows what it is about: lit and shadowed samples, and for the spot all three zones
    assert info['lit'].sum() > 200 and (info['use'] & ~info['lit']).sum() > 20, (info['lit'].sum(), info['use'].sum())
    if case == 'spot':
        ct = dr.cos_theta_map(em, sc, base['H'])[base['H']['valid']]
        cb, cc = dr.cosf(dr.deg_to_rad(em.beamWidth)), dr.cosf(dr.deg_to_rad(em.cutoffAngle))
        assert (ct >= cb).sum() > 50 and ((ct < cb) & (ct > cc)).sum() > 50 and (ct <= cc).sum() > 50
    _, smp, _ = _render(gpu_ctx, monkeypatch, sc, it, engine)
    _assert_records(smp, want, base, (case, kind, engine))


# the smooth-materials box (conductor, dielectric, plastic with a checkerboard, twosided with one
# and two nested BSDFs, roughplastic inside twosided) under the point light: vertices without a
# smooth component take no emitter sample, twosided evaluates the nested BSDF of wi's side
@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('kind', ['path', 'direct11'])
def test_first_bounce_smooth_materials(gpu_ctx, oracle, monkeypatch, kind, engine):
    if engine == 'wavefront' and kind == 'direct11':
        engine = 'hbm'          # (the direct integrator has no wavefront engine: its HBM kernel once more)
    em = _emitters()['point']
    sc, it0, twin = dr.delta_scene([em], materials='smooth', width=SIZE, height=SIZE, spp=SPP)
    it = KINDS[kind](False)
    _, osmp, _ = oracle.render(twin, it0, samples=True, libm_mode=0)
    H = dr.first_hits(sc, twin, oracle, osmp[:, 4], osmp[:, 5])
    want, info = dr.first_bounce(sc, twin, oracle, H, 'direct' if kind == 'direct11' else kind, em=em)
    assert info['lit'].sum() > 200 and (H['valid'] & ~info['use']).sum() > 200      # lit ones, and delta surfaces
    _, smp, _ = _render(gpu_ctx, monkeypatch, sc, it, engine)
    _assert_records(smp, want, dict(smp=osmp), ('smooth', kind, engine))


# ---- 2. the emitter choice ------------------------------------------------------------------
@pytest.mark.parametrize('engine', ENGINES)
def test_emitter_choice(gpu_ctx, oracle, monkeypatch, base, engine):
    E = _emitters()
    pt, sp = E['point'], E['spot']
    pt.samplingWeight, sp.samplingWeight = 1.0, 3.0
    sc, _, twin = dr.delta_scene([pt, sp], width=SIZE, height=SIZE, spp=SPP)
    it = KINDS['path'](False)
    if 'choice' not in base['cache']:
        L = oracle.lib()
        smp = base['smp']
        pix = np.repeat(np.arange(SIZE * SIZE), SPP)      # records: pixel-major, sample-minor
        px, py = pix % SIZE, pix // SIZE
        j = np.tile(np.arange(SPP), SIZE * SIZE)
        m = int(np.log2(SIZE))
        # Sobol dimension 2 of the sample: Scene::sampleEmitterDirect's sample.x (path.cpp:176)
        u = np.array([L.oracle_sobol_sample(L.oracle_sobol_lookup(m, int(jj), int(x), int(y), 0), 2, 0)
                      for x, y, jj in zip(px, py, j)], np.float32)
        # DiscretePDF::sampleReuse over the normalised CDF of the weights {1, 3} (pmf.h)
        f32 = np.float32
        norm = f32(f32(1) / f32(f32(1) + f32(3)))
        cdf = np.array([0, f32(f32(1) * norm), 1], f32)
        pick = np.where(u <= cdf[1], 0, 1)            # lower_bound(u) - 1, u > 0
        pick = np.where(u == 0, 0, pick)
        em_pdf = (cdf[pick + 1] - cdf[pick]).astype(f32)
        base['cache']['choice'] = dr.first_bounce(sc, twin, oracle, base['H'], 'path', em=[pt, sp], em_pdf=em_pdf,
                                                  pick=pick) + (pick,)
    want, info, pick = base['cache']['choice']
    assert (pick == 0).sum() > 500 and (pick == 1).sum() > 2000
    _, smp, _ = _render(gpu_ctx, monkeypatch, sc, it, engine)
    _assert_records(smp, want, base, ('choice', engine))


# ---- 3. path(maxDepth = 2) is direct(1, 1) --------------------------------------------------
@pytest.mark.parametrize('case', ['point', 'spot', 'dir_direction'])
def test_path_depth2_is_direct(gpu_ctx, monkeypatch, case):
    sc, _, _ = dr.delta_scene([_emitters()[case]], width=SIZE, height=SIZE, spp=SPP)
    fp, sp, _ = _render(gpu_ctx, monkeypatch, sc, KINDS['path'](False), 'lds')
    fd, sd, _ = _render(gpu_ctx, monkeypatch, sc, KINDS['direct11'](False), 'lds')
    assert np.array_equal(_bits(sp[:, 0:6]), _bits(sd[:, 0:6]))
    assert np.array_equal(_bits(fp), _bits(fd))
    assert sp[:, 0:3].max() > 0


# ---- 4. the engines agree at full depth -----------------------------------------------------
def _mixed(which):
    E = _emitters()
    if which == 'point+area':
        return dr.delta_scene([E['point']], keep_area=True, width=SIZE, height=SIZE, spp=SPP, max_depth=-1)
    sc, it, twin = dr.delta_scene([E['dir_direction'], Emitter('constant', radiance=(0.4, 0.5, 0.7))],
                                  width=SIZE, height=SIZE, spp=SPP, max_depth=-1)
    return sc, it, twin


@pytest.mark.parametrize('which', ['point+area', 'directional+constant'])
def test_engines_agree(gpu_ctx, monkeypatch, which):
    sc, it, _ = _mixed(which)
    it.rfilter = 'box'
    ref_film, ref_smp, st = _render(gpu_ctx, monkeypatch, sc, it, 'lds')
    assert np.isfinite(ref_smp).all() and ref_smp[:, 0:3].max() > 0 and ref_smp[:, 6].max() > 3
    runs = {
        'hbm': lambda: _render(gpu_ctx, monkeypatch, sc, it, 'hbm'),
        'wavefront': lambda: _render(gpu_ctx, monkeypatch, sc, it, 'wavefront'),
        'plain': lambda: _render(gpu_ctx, monkeypatch, sc, it, 'lds', samples=False),
        'plain-hbm': lambda: _render(gpu_ctx, monkeypatch, sc, it, 'hbm', samples=False),
    }
    for name, run in runs.items():
        film, smp, _ = run()
        assert np.array_equal(_bits(film), _bits(ref_film)), (which, name)
        if smp is not None:
            assert np.array_equal(_bits(smp), _bits(ref_smp)), (which, name)
    # three launches: 1 MiB of records holds 2 of the 6 samples of 192 x 128 pixels (16 B each)
    big_sc, big_it, _ = (dr.delta_scene([_emitters()['point']], keep_area=True, width=192, height=128, spp=6, max_depth=-1)
                         if which == 'point+area' else
                         dr.delta_scene([_emitters()['dir_direction'], Emitter('constant', radiance=(0.4, 0.5, 0.7))],
                                        width=192, height=128, spp=6, max_depth=-1))
    big_it.rfilter = 'box'
    one_film, one_smp, _ = _render(gpu_ctx, monkeypatch, big_sc, big_it, 'lds')
    monkeypatch.setenv('MTSGPU_CONTRIB_BYTES', str(BUDGET))
    film, smp, _ = _render(gpu_ctx, monkeypatch, big_sc, big_it, 'lds')
    assert gpu_ctx.launch_chunks() == 3, gpu_ctx.launch_chunks()
    monkeypatch.delenv('MTSGPU_CONTRIB_BYTES')
    assert np.array_equal(_bits(film), _bits(one_film)) and np.array_equal(_bits(smp), _bits(one_smp))
    # a tile shard: every other 8x8 tile, whose records equal the whole render's there
    film, smp, _ = _render(gpu_ctx, monkeypatch, sc, it, 'lds', row=(0, 2, 1), tile_shard=True)
    tiles_x = SIZE // 8
    pix = np.arange(SIZE * SIZE)
    tile = (pix // SIZE // 8) * tiles_x + (pix % SIZE) // 8
    mine = np.repeat(tile % 2 == 1, SPP)
    assert mine.sum() == SIZE * SIZE * SPP // 2
    assert np.array_equal(_bits(smp[mine]), _bits(ref_smp[mine])), which


# ---- multichannel over a delta scene (the field pass has no NEE) ----------------------------
def test_multichannel_delta_scene(gpu_ctx, monkeypatch):
    from mitsuba_amd.scene import FieldIntegrator, MultiChannelIntegrator
    sc, it, _ = dr.delta_scene([_emitters()['point']], width=SIZE, height=SIZE, spp=SPP)
    it.rfilter = 'box'
    film, _, _ = _render(gpu_ctx, monkeypatch, sc, it, 'lds', samples=False)
    mc = MultiChannelIntegrator(children=[it, FieldIntegrator('distance')], sampleCount=SPP, rfilter='box')
    gpu_ctx.upload(sc)
    films, _, _ = gpu_ctx.render(mc)
    assert np.array_equal(_bits(films[0][..., 0:3]), _bits(film[..., 0:3]))
    assert films[1][..., 0].max() > 0


# ---- 5. energy against the oracle's proxy sphere --------------------------------------------
def test_energy_against_proxy(gpu_ctx, oracle, monkeypatch):
    """Per-channel image means of the GPU's point-light render and of the oracle's render of the
    proxy sphere (delta_ref.proxy_scene; the diffuse C1 at full depth, 32 x 32, another
    scramble), the pixels whose primary ray can hit the proxy left out (4 of 1024), within 4
    standard errors of the difference formed from the two renders' per-sample records.
    44 spp: the smallest count (multiples of 4) at which, on the CPU with the oracle alone,
    proxy r against proxy r / 2 gives z = 0.50 / 0.22 / 0.32 and a 5% intensity error
    z = 8.19 / 8.66 / 8.08 (tests/test_delta_emitters_host.py::test_proxy_calibration).
    Measured here on the MI355X: see DESIGN.md 2."""
    spp, r = dr.PROXY_SPP, dr.PROXY_R
    sc, it = dr.point_scene(spp)
    _, smp, _ = _render(gpu_ctx, monkeypatch, sc, it, 'lds')
    psc, pit = dr.proxy_scene(r, spp, scramble=0x1234567)
    keep = dr.proxy_mask(psc, oracle, r)
    assert 0 < (~keep).sum() <= keep.size // 100
    g = dr.image_mean(smp, keep, spp)
    o = dr.image_mean(oracle.render(psc, pit, samples=True, libm_mode=0)[1], keep, spp)
    z = dr.z_score(g, o)
    print('means', g[0], o[0], 'z', z, 'z at a 5% error', dr.z_score(g, o, 1.05))
    assert (z <= 4).all(), (z, g, o)
