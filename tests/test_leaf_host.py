"""difftrans, roughdiffuse and phong without a GPU: what configure() derives
(mtsgpu_leaf_host against leaf_ref.configure), the refusals with their messages, the plan
(such a scene takes the MTSG_FEAT_SET_LEAF2 kernels, 15367, and no other scene does), XML load
and save, and the numpy restatement checked against itself.

On the parent commit the library has no mtsgpu_leaf_host and every such scene is refused with
'unsupported BSDF type'."""
import os

import numpy as np
import pytest

import leaf_ref as lr
from mitsuba_amd import abi, scenes
from mitsuba_amd.integrator import (VARIANT_COMBO, VARIANT_LEAF2, MtsgpuError, albedo_factors_host, check_scene,
                                    leaf_host, plan_host)
from mitsuba_amd.scene import BSDF, Checkerboard, DirectIntegrator, VolpathIntegrator
from mitsuba_amd.xmlscene import SceneError, load_scene, save_scene

f32 = np.float32
ENV_KEYS = ('MTSGPU_NO_SCENE_LDS', 'MTSGPU_ENGINE', 'MTSGPU_WAVES', 'MTSGPU_NO_DIFF_VARIANT', 'MTSGPU_NO_BSDF_SETS',
            'MTSGPU_NO_REFN_SPEC')


def _scene(bsdf, **kw):
    sc, it = scenes.build('C1', width=32, height=32, spp=4, **kw)
    sc.bsdfs = [bsdf] + list(sc.bsdfs[1:])
    return sc, it


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- 1. configure ----------------------------------------------------------------------------
CONFIGS = {
    'difftrans_default': BSDF('difftrans'),
    'difftrans_scaled': BSDF('difftrans', transmittance=(0.4, 1.6, 0.2)),
    'difftrans_chk': BSDF('difftrans', transmittance=lr.checker((0.1, 0.2, 0.3), (1.3, 0.5, 0.4))),
    'rdiff_default': BSDF('roughdiffuse'),
    'rdiff_scaled': BSDF('roughdiffuse', reflectance=(1.5, 0.5, 0.3), alpha=0.35, useFastApprox=True),
    'rdiff_chk': BSDF('roughdiffuse', reflectance=lr.checker((0.1, 0.2, 0.3), (0.9, 1.1, 0.4)), alpha=lr.checker(0.1, 0.7)),
    'phong_default': BSDF('phong'),
    'phong_pair': BSDF('phong', diffuseReflectance=(0.7, 0.6, 0.2), specularReflectance=(0.5, 0.3, 0.9), exponent=7.5),
    'phong_pair_unscaled': BSDF('phong', diffuseReflectance=(0.7, 0.6, 0.2), specularReflectance=(0.5, 0.3, 0.9),
                                ensureEnergyConservation=False),
    'phong_chk': BSDF('phong', diffuseReflectance=lr.checker((0.1, 0.2, 0.3), (0.6, 0.5, 0.4)),
                      specularReflectance=(0.3, 0.3, 0.3)),
    'phong_chk_pair': BSDF('phong', diffuseReflectance=lr.checker((0.1, 0.2, 0.3), (0.8, 0.9, 0.4)),
                           specularReflectance=(0.3, 0.35, 0.3)),
}


@pytest.mark.parametrize('name', list(CONFIGS))
def test_leaf_host_matches_the_restatement(name):
    b = CONFIGS[name]
    got = leaf_host(_scene(b, materials='smooth')[0], 0)
    want = lr.configure(b)
    assert got['flags'] == want['flags'], (hex(got['flags']), hex(want['flags']))
    if 'refl' in want:
        assert np.array_equal(_bits(got['reflectance']), _bits(want['refl'][0])), (got['reflectance'], want['refl'])
        assert np.array_equal(_bits(got['reflectance1']), _bits(want['refl'][1]))
    if 'spec_r' in want:
        assert np.array_equal(_bits(got['specularReflectance']), _bits(want['spec_r'])), (got, want['spec_r'])
    if b.type == 'phong':
        assert _bits(got['specularSamplingWeight']) == _bits(want['weight']), (got['specularSamplingWeight'], want['weight'])
        assert got['alpha'] == f32(b.exponent)
    if b.type == 'roughdiffuse':
        assert got['useFastApprox'] == want['fast']
        if not isinstance(b.alpha, Checkerboard):
            assert _bits(got['alpha']) == _bits(want['alpha'])


def test_configure_values():
    """The restated configure() against figures worked by hand, so that it does not merely agree
    with the library: the scale 0.99f / max, the pair form's common scale, the plugins' defaults."""
    c = lr.configure(CONFIGS['difftrans_scaled'])
    assert np.array_equal(c['refl'][0], (np.array([0.4, 1.6, 0.2], f32) * f32(f32(0.99) * f32(f32(1) / f32(1.6)))).astype(f32))
    c = lr.configure(CONFIGS['phong_pair'])      # maxima's sum: (1.2, 0.9, 1.1)
    sc = f32(f32(0.99) * f32(f32(1) / f32(f32(0.7) + f32(0.5))))
    assert np.array_equal(c['spec_r'], (np.array([0.5, 0.3, 0.9], f32) * sc).astype(f32))
    assert np.array_equal(c['refl'][0], (np.array([0.7, 0.6, 0.2], f32) * sc).astype(f32))
    c = lr.configure(CONFIGS['phong_default'])   # 0.2 / (0.5 + 0.2) of the luminances (weights sum to 1)
    assert abs(float(c['weight']) - 0.2 / 0.7) < 1e-6 and c['exponent'] == 30 and np.all(c['spec_r'] == f32(0.2))
    c = lr.configure(CONFIGS['phong_chk'])       # the checkerboard's average (0.35, 0.35, 0.35) against 0.3
    assert abs(float(c['weight']) - 0.3 / 0.65) < 1e-6
    assert lr.configure(CONFIGS['rdiff_default'])['alpha'] == f32(0.2)
    assert np.all(lr.configure(CONFIGS['difftrans_default'])['refl'][0] == f32(0.5))


def test_leaf_host_refuses_other_types():
    with pytest.raises(MtsgpuError, match='not a difftrans'):
        leaf_host(_scene(BSDF('diffuse'))[0], 0)


# ---- 2. refusals -----------------------------------------------------------------------------
TRANSMIT = {'difftrans': BSDF('difftrans')}


@pytest.mark.parametrize('leaf', list(TRANSMIT))
@pytest.mark.parametrize('wrapper', ['twosided', 'mixturebsdf', 'blendbsdf', 'mask'])
def test_transmissive_leaves_are_refused_below_wrappers(wrapper, leaf):
    c = TRANSMIT[leaf]
    b = {'twosided': BSDF('twosided', nested=[c]),
         'mixturebsdf': BSDF('mixturebsdf', weights=[0.5, 0.5], nested=[BSDF('diffuse'), c]),
         'blendbsdf': BSDF('blendbsdf', nested=[BSDF('diffuse'), c]),
         'mask': BSDF('mask', nested=[c])}[wrapper]
    with pytest.raises(MtsgpuError) as e:
        check_scene(_scene(b)[0])
    if wrapper == 'twosided':      # TwoSidedBRDF::configure's message (twosided.cpp:96-98)
        assert str(e.value).endswith('Only materials without a transmission component can be nested!'), str(e.value)
    else:
        assert str(e.value).endswith("%s: a nested '%s' BSDF is not supported" % (wrapper, leaf)), str(e.value)


@pytest.mark.parametrize('leaf', ['phong', 'roughdiffuse'])
@pytest.mark.parametrize('wrapper', ['twosided', 'mixturebsdf', 'blendbsdf', 'mask'])
def test_reflective_leaves_nest(wrapper, leaf):
    c = BSDF(leaf)
    b = {'twosided': BSDF('twosided', nested=[c]),
         'mixturebsdf': BSDF('mixturebsdf', weights=[0.5, 0.5], nested=[BSDF('diffuse'), c]),
         'blendbsdf': BSDF('blendbsdf', nested=[BSDF('diffuse'), c]),
         'mask': BSDF('mask', nested=[BSDF('twosided', nested=[c])])}[wrapper]
    sc, it = _scene(b)
    assert check_scene(sc) is None
    assert plan_host(sc, it)['variant_word'] & VARIANT_LEAF2


def test_textured_parameters_that_are_refused():
    with pytest.raises(NotImplementedError, match="phong: a textured 'exponent'"):
        BSDF('phong', exponent=lr.checker(2.0, 30.0)).to_desc()
    with pytest.raises(NotImplementedError, match="phong: a textured 'specularReflectance'"):
        BSDF('phong', specularReflectance=lr.checker(0.2, 0.3)).to_desc()


def test_ward_is_still_refused(tmp_path):
    with pytest.raises(NotImplementedError, match='BSDF plugin "ward" is not on the GPU path'):
        BSDF('ward').to_desc()
    with pytest.raises(NotImplementedError, match='BSDF plugin "ward" is not on the GPU path'):
        load_scene(_write(tmp_path, '<shape type="cube"><bsdf type="ward"/></shape>'))


def test_thindielectric_is_still_refused(tmp_path):
    """Not implemented: its null lobe needs volpath's shadow segments to pass the pane
    (Scene::evalTransmittance), which the shadow rays here do not.  Type 11 is kept free for it."""
    with pytest.raises(NotImplementedError, match='BSDF plugin "thindielectric" is not on the GPU path'):
        BSDF('thindielectric').to_desc()
    with pytest.raises(NotImplementedError, match='BSDF plugin "thindielectric" is not on the GPU path'):
        load_scene(_write(tmp_path, '<shape type="cube"><bsdf type="thindielectric"/></shape>'))
    sc, _ = _scene(BSDF('phong'))
    d = sc.desc()
    d.bsdfs[0].type = 11
    import ctypes as C
    from mitsuba_amd.integrator import load_library
    buf = C.create_string_buffer(512)
    assert load_library().mtsgpu_check_scene(C.byref(d), buf, 512) == abi.EINVAL and b'unsupported BSDF type' in buf.value
    assert plan_host(_scene(BSDF('phong'))[0], VolpathIntegrator(sampleCount=4))['variant']['feat'] == 15367


def test_albedo_factors():
    """getDiffuseReflectance: phong's diffuseReflectance and roughdiffuse's reflectance as they are
    (factor 1); difftrans falls to BSDF's default (bsdf.cpp:82-86), eval at wi = wo = (0, 0, 1)
    with typeMask = EDiffuseReflection, which it rejects by its type mask and same-side test: 0."""
    for t, f in (('phong', 1.0), ('roughdiffuse', 1.0), ('difftrans', 0.0)):
        fac = albedo_factors_host(_scene(BSDF(t))[0])
        assert fac[0] == f, (t, fac)
    two = albedo_factors_host(_scene(BSDF('twosided', nested=[BSDF('phong')]))[0])
    assert two[-1] == 1.0


# ---- 3. the plan and XML ---------------------------------------------------------------------
@pytest.mark.parametrize('case', list(lr.cases()))
def test_leaf_scene_takes_the_leaf2_set(monkeypatch, case):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    b = lr.cases()[case]
    sc, it = _scene(b, materials='smooth')
    p = plan_host(sc, it)
    combo = any(x.type in ('mixturebsdf', 'blendbsdf', 'mask') for x in sc.flat_bsdfs()[0])
    assert p['variant_word'] & VARIANT_LEAF2 and p['variant']['leaf2'] and p['variant']['feat'] == 15367
    assert bool(p['variant_word'] & VARIANT_COMBO) == combo
    assert p['variant']['name'] == 'path_kernel<false, true, 15367, 3>' and p['scene_lds'] and not p['start_queue']
    assert plan_host(sc, it, engine='wavefront')['variant_word'] & ~VARIANT_COMBO == (1 << 16) | VARIANT_LEAF2
    assert plan_host(sc, DirectIntegrator(sampleCount=4))['variant_word'] & VARIANT_LEAF2
    monkeypatch.setenv('MTSGPU_NO_SCENE_LDS', '1')
    v = plan_host(sc, it)['variant']
    assert v['leaf2'] and not v['scene_lds'] and v['name'] == 'path_kernel<false, false, 15367, %d>' % v['waves']


@pytest.mark.parametrize('materials', ['diffuse', 'smooth', 'plastic'])
def test_plain_scenes_do_not(monkeypatch, materials):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    sc, it = scenes.build('C1', width=32, height=32, spp=4, materials=materials)
    for e in (None, 'wavefront'):
        p = plan_host(sc, it, engine=e)
        assert not p['variant_word'] & VARIANT_LEAF2


XML = '''<scene version="0.6.0">
  <integrator type="path"><integer name="maxDepth" value="3"/></integrator>
  <sensor type="perspective">
    <transform name="toWorld"><lookat origin="0, 1, -4" target="0, 1, 0" up="0, 1, 0"/></transform>
    <sampler type="sobol"><integer name="sampleCount" value="4"/></sampler>
    <film type="hdrfilm"><integer name="width" value="16"/><integer name="height" value="16"/>
      <rfilter type="box"/></film>
  </sensor>
  %s
  <emitter type="constant"/>
</scene>
'''
GOOD = '''<shape type="cube"><bsdf type="difftrans">
      <texture type="checkerboard" name="transmittance"><float name="uvscale" value="3"/></texture></bsdf></shape>
  <shape type="cube"><bsdf type="roughdiffuse"><rgb name="reflectance" value="0.6, 0.5, 0.3"/>
      <texture type="checkerboard" name="alpha"/><boolean name="useFastApprox" value="true"/></bsdf></shape>
  <shape type="cube"><bsdf type="phong"><float name="exponent" value="2.5"/>
      <texture type="checkerboard" name="diffuseReflectance"/></bsdf></shape>
  <shape type="cube"><bsdf type="twosided"><bsdf type="phong"/></bsdf></shape>
  <shape type="cube"><bsdf type="roughdiffuse"/></shape>'''


def _write(tmp_path, body):
    p = tmp_path / 'scene.xml'
    p.write_text(XML % body)
    return str(p)


def test_xml_load_desc_and_round_trip(tmp_path):
    sc, it = load_scene(_write(tmp_path, GOOD))
    dt, rd, ph, two, rd2 = [sc.bsdfs[m.bsdf] for m in sc.meshes]
    assert dt.type == 'difftrans' and isinstance(dt.transmittance, Checkerboard) and dt.transmittance.uscale == 3.0
    assert rd.type == 'roughdiffuse' and isinstance(rd.alpha, Checkerboard) and rd.useFastApprox is True
    assert ph.type == 'phong' and ph.exponent == 2.5 and isinstance(ph.diffuseReflectance, Checkerboard)
    assert tuple(ph.specularReflectance) == (0.2, 0.2, 0.2)
    assert two.nested[0].type == 'phong' and two.nested[0].exponent == 30.0
    assert rd2.alpha == 0.2 and rd2.useFastApprox is False
    assert check_scene(sc) is None
    assert plan_host(sc, it)['variant_word'] & VARIANT_LEAF2
    flat, _ = sc.flat_bsdfs()
    d = sc.desc()
    by = {id(b): i for i, b in enumerate(flat)}
    assert d.bsdfs[by[id(dt)]].type == abi.BSDF_DIFFTRANS and d.bsdfs[by[id(dt)]].transmittance_tex.type == abi.TEX_CHECKERBOARD
    dr_ = d.bsdfs[by[id(rd)]]
    assert dr_.type == abi.BSDF_ROUGHDIFFUSE and dr_.alpha_tex.type == abi.TEX_CHECKERBOARD and dr_.use_fast_approx == 1
    dp = d.bsdfs[by[id(ph)]]
    assert dp.type == abi.BSDF_PHONG and dp.exponent == 2.5 and dp.reflectance_tex.type == abi.TEX_CHECKERBOARD
    assert list(dp.specular_reflectance) == [f32(0.2)] * 3
    assert d.bsdfs[by[id(rd2)]].alpha_u == f32(0.2)
    out = tmp_path / 'saved'
    os.makedirs(out)
    sc2, _ = load_scene(save_scene(sc, it, str(out)))
    d2 = sc2.desc()
    assert d2.num_bsdfs == d.num_bsdfs and [m.bsdf for m in sc2.meshes] == [m.bsdf for m in sc.meshes]
    for i in range(d.num_bsdfs):
        assert bytes(d.bsdfs[i]) == bytes(d2.bsdfs[i]), (i, flat[i].type)


@pytest.mark.parametrize('body,exc,text', [
    ('<bsdf type="phong"><texture type="checkerboard" name="exponent"/></bsdf>', NotImplementedError,
     'phong: a textured "exponent"'),
    ('<bsdf type="phong"><texture type="checkerboard" name="specularReflectance"/></bsdf>', NotImplementedError,
     'phong: a textured "specularReflectance"'),
    ('<bsdf type="twosided"><bsdf type="difftrans"/></bsdf>', SceneError,
     'Only materials without a transmission component can be nested!'),
    ('<bsdf type="mask"><bsdf type="difftrans"/></bsdf>', NotImplementedError, 'mask: a nested "difftrans"'),
    ('<bsdf type="blendbsdf"><bsdf type="diffuse"/><bsdf type="difftrans"/></bsdf>', NotImplementedError,
     'blendbsdf: a nested "difftrans"'),
])
def test_xml_refuses(tmp_path, body, exc, text):
    with pytest.raises(exc, match=text):
        load_scene(_write(tmp_path, '<shape type="cube">%s</shape>' % body))


# ---- 4. the restatement against itself --------------------------------------------------------
N = 1 << 16
SELF = ['phong30', 'phong2.5', 'rdiff_fast', 'rdiff_full', 'difftrans']
WI = {'normal': np.array([0.0, 0.0, 1.0], f32),
      'sixty': np.array([np.sin(np.pi / 3) * np.cos(0.7), np.sin(np.pi / 3) * np.sin(0.7), 0.5], f32)}


@pytest.fixture(scope='module')
def draws():
    rng = np.random.RandomState(1234)
    return rng.random_sample((N, 2)).astype(f32)


@pytest.mark.parametrize('incidence', list(WI))
@pytest.mark.parametrize('case', SELF)
def test_restatement_is_consistent(draws, case, incidence):
    """2^16 draws at one incidence.  Bit for bit wherever pdf > 0: sample()'s pdf is pdf() at the
    sampled direction, and its weight is eval() there times the reciprocal of that pdf (Spectrum's
    division), the transmittance itself for difftrans.  And the draws follow that pdf: the mean
    of g(wo) / pdf(wo) over the samples on the lobe's side, g the cosine density (integral 1
    over the hemisphere, bounded where 1 / pdf alone is not), is 1 within 4 standard errors
    computed from the samples; a lobe sample below the horizon counts 0, as sample() fails there."""
    b = lr.cases()[case]
    wi = np.broadcast_to(WI[incidence], (N, 3)).astype(f32)
    uv = np.zeros((N, 2), f32)
    wo, w, pdf, eta, st, lobe = lr.sample(b, wi, draws[:, 0], draws[:, 1], uv)
    val, pdf2 = lr.eval_pdf(b, wi, wo, uv)
    ok = pdf > 0
    assert ok.mean() > 0.5 and (eta == 1).all()
    # sample()'s pdf is pdf() at the sampled direction
    assert np.array_equal(_bits(pdf[ok]), _bits(pdf2[ok]))
    if b.type == 'difftrans':      # sample() returns the transmittance itself: eval / pdf in exact terms
        assert np.array_equal(_bits(w[ok]), _bits(np.broadcast_to(lr.configure(b)['refl'][0], w[ok].shape)))
    else:                          # eval * (1 / pdf), the Spectrum division
        inv = (f32(1) / pdf[ok]).astype(f32)
        assert np.array_equal(_bits(w[ok]), _bits((val[ok] * inv[:, None]).astype(f32)))
    # the density integrates to one: E[g / pdf] for the cosine density g over the sampled side
    g = (np.abs(wo[:, 2]) * lr.INV_PI).astype(np.float64)
    side = wo[:, 2] < 0 if b.type == 'difftrans' else wo[:, 2] > 0
    est = np.where(ok & side, g / np.where(ok, pdf, 1).astype(np.float64), 0.0)
    mean, se = est.mean(), est.std(ddof=1) / np.sqrt(N)
    print(case, incidence, 'mean', mean, 'se', se, 'z', abs(mean - 1) / max(se, 1e-300))
    if se == 0:
        assert abs(mean - 1) < 1e-6          # the cosine-sampled leaves: g / pdf is 1 up to rounding
    else:
        assert abs(mean - 1) <= 4 * se, (mean, se)
    if b.type == 'phong':
        share = (lobe == 0).mean()
        assert 0.05 < share < 0.95, share
