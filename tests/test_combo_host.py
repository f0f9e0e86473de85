"""mixturebsdf, blendbsdf and mask, host side: the render plan picks the combinator feature set
(7175) for a scene with one of them and the set it picked before for every other scene; every
nesting the device chain does not cover is refused by mtsgpu_check_scene (MTSGPU_EINVAL) and by
the XML loader, with a message naming the plugin; the reference's own configure() errors are
reproduced; an XML file with each plugin round-trips; and MixtureBSDF::configure's weights and
m_pdf equal a float32 numpy restatement of pmf.h (combo_ref.mixture_configure).

None of this exists on the parent commit: BSDF('mixturebsdf') has no descriptor type there.
"""
import ctypes as C
import os

import numpy as np
import pytest

import combo_ref as cr
from mitsuba_amd import abi, scenes
from mitsuba_amd.integrator import (VARIANT_COMBO, MtsgpuError, albedo_factors_host, check_scene, combo_host,
                                    kernel_variant_of, load_library, plan_host)
from mitsuba_amd.scene import BSDF, Checkerboard, DirectIntegrator, VolpathIntegrator
from mitsuba_amd.xmlscene import SceneError, load_scene, save_scene

f32 = np.float32
ENV_KEYS = ('MTSGPU_NO_SCENE_LDS', 'MTSGPU_ENGINE', 'MTSGPU_WAVES', 'MTSGPU_NO_DIFF_VARIANT', 'MTSGPU_NO_BSDF_SETS',
            'MTSGPU_NO_REFN_SPEC')


def _scene(bsdf, **kw):
    sc, it = scenes.build('C1', width=32, height=32, spp=4, **kw)
    sc.bsdfs = [bsdf] + list(sc.bsdfs[1:])
    return sc, it


# ---- the plan -------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(cr.cases()))
def test_combinator_scene_takes_the_combo_set(monkeypatch, case):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    b = cr.cases()[case]
    sc, it = _scene(b)
    has = any(x.type in ('mixturebsdf', 'blendbsdf', 'mask') for x in sc.flat_bsdfs()[0])
    assert has
    p = plan_host(sc, it)
    assert p['variant_word'] & VARIANT_COMBO and p['variant']['combo'] and p['variant']['feat'] == 7175
    assert p['variant']['name'] == 'path_kernel<false, true, 7175, 3>' and p['scene_lds'] and not p['start_queue']
    assert plan_host(sc, it, samples=True)['variant']['name'] == 'path_kernel<true, true, 7175, 3>'
    assert plan_host(sc, it, engine='wavefront')['variant_word'] == (1 << 16) | VARIANT_COMBO
    assert plan_host(sc, DirectIntegrator(sampleCount=4))['variant_word'] & VARIANT_COMBO
    assert plan_host(sc, VolpathIntegrator(sampleCount=4))['variant']['feat'] == 7175
    monkeypatch.setenv('MTSGPU_NO_SCENE_LDS', '1')
    v = plan_host(sc, it)['variant']
    assert v['combo'] and not v['scene_lds'] and v['name'] == 'path_kernel<false, false, 7175, %d>' % v['waves']


# variant words of the parent commit (no combinators in the library) at 64 x 48, 4 spp, read
# from a run of mtsgpu_plan_host on that commit: (plain, plain wavefront, instrumented,
# instrumented wavefront, direct).  C1-C5 are test_delta_emitters_host.PARENT_WORDS'.
PARENT_WORDS = {
    'C1': (0x1408, 0x10000, 0x3408, 0x10000, 0x1408),
    'C2': (0x1408, 0x10000, 0x3408, 0x10000, 0x1408),
    'C3': (0xc431, 0x10000, 0xe431, 0x10000, 0x401),
    'C4': (0x4450, 0x10000, 0x6450, 0x10000, 0x400),
    'C5': (0xc473, 0x10000, 0xe473, 0x10000, 0x403),
}


@pytest.mark.parametrize('cfg', list(PARENT_WORDS))
def test_other_scenes_keep_their_variant(monkeypatch, cfg):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    sc, it = scenes.build(cfg, width=64, height=48, spp=4)
    got = tuple(plan_host(sc, it, samples=s, engine=e)['variant_word'] for s in (False, True) for e in (None, 'wavefront'))
    got += (plan_host(sc, DirectIntegrator(sampleCount=4))['variant_word'],)
    assert got == PARENT_WORDS[cfg], [hex(w) for w in got]
    assert not any(w & VARIANT_COMBO for w in got)
    assert not kernel_variant_of(got[0])['combo']


@pytest.mark.parametrize('materials', ['rough', 'plastic', 'smooth', 'shapes'])
def test_material_sets_without_combinators_keep_their_set(monkeypatch, materials):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    sc, it = scenes.build('C1', width=32, height=32, spp=4, materials=materials)
    p = plan_host(sc, it)
    assert not p['variant_word'] & VARIANT_COMBO
    assert p['variant']['feat'] == (6 if materials == 'shapes' else 0 if materials == 'rough' else 2)


# ---- refusals -------------------------------------------------------------------------------
def _leaf():
    return BSDF('diffuse', reflectance=(0.5, 0.4, 0.3))


def _refused():
    d, rc = _leaf(), BSDF('roughconductor', distribution='ggx', alpha=0.2, material='Au')
    rd = BSDF('roughdielectric', distribution='ggx', alpha=0.2)
    mix = lambda *n, w=None: BSDF('mixturebsdf', weights=list(w or [1.0 / len(n)] * len(n)), nested=list(n))
    blend = lambda a, b: BSDF('blendbsdf', weight=0.4, nested=[a, b])
    mask = lambda x: BSDF('mask', opacity=0.5, nested=[x])
    return {
        'mixture in mixture': (mix(d, mix(d, rc)), "mixturebsdf: nesting a 'mixturebsdf' BSDF is not supported"),
        'blend in mixture': (mix(d, blend(d, rc)), "mixturebsdf: nesting a 'blendbsdf' BSDF is not supported"),
        'twosided in blend': (blend(d, BSDF('twosided', nested=[rc])), "blendbsdf: nesting a 'twosided' BSDF is not supported"),
        'mixture in blend': (blend(mix(d, rc), d), "blendbsdf: nesting a 'mixturebsdf' BSDF is not supported"),
        'mask in mixture': (mix(d, mask(d)), "mixturebsdf: nesting a 'mask' BSDF is not supported"),
        'mask in blend': (blend(mask(d), d), "blendbsdf: nesting a 'mask' BSDF is not supported"),
        'mask in twosided': (BSDF('twosided', nested=[mask(d)]), 'twosided: nesting a mask BSDF is not supported'),
        'mask in mask': (mask(mask(d)), "mask: nesting a 'mask' BSDF is not supported"),
        'roughdielectric in mixture': (mix(d, rd), "mixturebsdf: a nested 'roughdielectric' BSDF is not supported"),
        'roughdielectric in blend': (blend(rd, d), "blendbsdf: a nested 'roughdielectric' BSDF is not supported"),
        'roughdielectric in mask': (mask(rd), "mask: a nested 'roughdielectric' BSDF is not supported"),
        'roughdielectric below mask': (mask(blend(rd, d)), "a nested 'roughdielectric' BSDF is not supported"),
        'two delta children': (mix(d, BSDF('conductor'), BSDF('plastic')), 'more than one nested BSDF with a delta lobe'),
        # the reference's own errors
        'weight count': (BSDF('mixturebsdf', weights=[0.5], nested=[d, rc]), 'BSDF count mismatch: 2 bsdfs, but specified 1 weights'),
        'weight sum': (BSDF('mixturebsdf', weights=[0.0, 0.0], nested=[d, rc]), 'The weights must sum to a value greater than zero!'),
        'no weights': (BSDF('mixturebsdf', weights=[], nested=[d]), 'No weights were supplied!'),
        'negative weight': (BSDF('mixturebsdf', weights=[0.5, -0.1], nested=[d, rc]), 'Invalid BSDF weight!'),
        'transmission below twosided': (BSDF('twosided', nested=[blend(d, BSDF('dielectric'))]),
                                        'Only materials without a transmission component can be nested!'),
    }


@pytest.mark.parametrize('what', list(_refused()))
def test_check_scene_refuses(what):
    b, text = _refused()[what]
    with pytest.raises(MtsgpuError) as e:
        check_scene(_scene(b)[0])
    assert e.value.code == abi.EINVAL and text in str(e.value), str(e.value)


def test_check_scene_refuses_nine_children_and_bad_blend():
    """A caller that bypasses the Python classes: the descriptor's own counts."""
    L = load_library()
    sc, _ = _scene(BSDF('mixturebsdf', weights=[0.1] * 8, nested=[_leaf() for _ in range(8)]))
    assert check_scene(sc) is None
    d = sc.desc()
    buf = C.create_string_buffer(512)
    d.bsdfs[0].num_children = d.bsdfs[0].num_weights = 9
    assert L.mtsgpu_check_scene(C.byref(d), buf, 512) == abi.EINVAL
    assert b'mixturebsdf: more than 8 nested BSDFs are not supported' in buf.value
    with pytest.raises(NotImplementedError, match='mixturebsdf: more than 8'):
        BSDF('mixturebsdf', weights=[0.1] * 9, nested=[_leaf() for _ in range(9)]).to_desc()
    sc, _ = _scene(BSDF('blendbsdf', weight=0.5, nested=[_leaf(), _leaf()]))
    d = sc.desc()
    d.bsdfs[0].nested[1] = -1
    assert L.mtsgpu_check_scene(C.byref(d), buf, 512) == abi.EINVAL
    assert b'blendbsdf: BSDF count mismatch: expected two nested BSDF instances!' in buf.value
    sc, _ = _scene(BSDF('mask', nested=[_leaf()]))
    d = sc.desc()
    d.bsdfs[0].nested[0] = -1
    assert L.mtsgpu_check_scene(C.byref(d), buf, 512) == abi.EINVAL and b'mask: A child BSDF is required' in buf.value


def test_anisotropic_leaf_below_a_combinator_needs_texcoords():
    """computeUVTangents' error (trimesh.cpp:685-691) reaches through the chain, as through twosided."""
    aniso = BSDF('roughconductor', distribution='ggx', alphaU=0.05, alphaV=0.4, material='Au')
    b = BSDF('mask', opacity=0.5, nested=[BSDF('twosided', nested=[BSDF('blendbsdf', weight=0.5, nested=[_leaf(), aniso])])])
    with pytest.raises(MtsgpuError, match='texture coordinates are required to generate tangent vectors'):
        check_scene(_scene(b)[0])                           # the diffuse C1's meshes carry no texcoords
    assert check_scene(_scene(b, materials='smooth')[0]) is None


@pytest.mark.parametrize('case', list(cr.cases()))
def test_check_scene_accepts_the_chain(case):
    assert check_scene(_scene(cr.cases()[case], materials='smooth')[0]) is None


def test_flags_are_the_childrens():
    """BSDF::EBSDFType bits (layout.h MTSG_F_*): the union of the children's; mask adds
    ENull | EFrontSide | EBackSide."""
    NULL, DIFF, GLOSSY, DELTA, FRONT, BACK = 0x1, 0x2, 0x8, 0x20, 0x1000, 0x2000
    C_ = cr.cases()
    sc, _ = _scene(C_['blend_rc_plastic'])
    assert combo_host(sc, 0)['flags'] == GLOSSY | DELTA | DIFF | FRONT
    sc, _ = _scene(C_['mask'])
    assert combo_host(sc, 0)['flags'] == NULL | DIFF | FRONT | BACK
    sc, _ = _scene(C_['mask_twosided_blend'])
    assert combo_host(sc, 0)['flags'] == NULL | DIFF | GLOSSY | FRONT | BACK
    assert np.array_equal(combo_host(sc, 0)['value'], np.full(3, 0.7, f32))
    # ESpatiallyVarying (here 0x4000): a mask whose opacity is a texture (mask.cpp:98-106); a blend's
    # textured weight adds nothing to its children's types (blendbsdf.cpp:119-131)
    sc, _ = _scene(C_['mask_chk'])
    assert combo_host(sc, 0)['flags'] == NULL | GLOSSY | FRONT | BACK | 0x4000
    sc, _ = _scene(C_['blend_chk'])
    assert combo_host(sc, 0)['flags'] == DIFF | GLOSSY | FRONT
    # ensureEnergyConservation(opacity, "opacity", 1.0f): an opacity above 1 is scaled to 0.99 of its maximum
    sc, _ = _scene(BSDF('mask', opacity=(2.0, 1.0, 0.5), nested=[_leaf()]))
    s = f32(f32(0.99) * f32(f32(1) / f32(2)))
    assert np.array_equal(combo_host(sc, 0)['value'], (np.array([2.0, 1.0, 0.5], f32) * s).astype(f32))
    with pytest.raises(MtsgpuError, match='not a mixturebsdf'):
        combo_host(sc, 1)


# ---- MixtureBSDF::configure against pmf.h ----------------------------------------------------
@pytest.mark.parametrize('weights,rescaled', [((0.5, 0.9, 0.6), True), ((0.2, 0.3), False)])
def test_mixture_weights_and_pdf(weights, rescaled):
    d = _leaf()
    sc, _ = _scene(BSDF('mixturebsdf', weights=list(weights), nested=[d] * len(weights)))
    got = combo_host(sc, 0)
    w, cdf = cr.mixture_configure(weights)
    assert got['n'] == len(weights)
    assert np.array_equal(got['weights'].view(np.uint32), w.view(np.uint32))
    assert np.array_equal(got['cdf'].view(np.uint32), cdf.view(np.uint32))
    assert np.array_equal(got['pdf'].view(np.uint32), (cdf[1:] - cdf[:-1]).astype(f32).view(np.uint32))
    assert (not np.array_equal(w, np.asarray(weights, f32))) == rescaled and cdf[-1] == 1
    # ensureEnergyConservation = false keeps the weights; m_pdf is normalised all the same
    sc, _ = _scene(BSDF('mixturebsdf', weights=list(weights), nested=[d] * len(weights), ensureEnergyConservation=False))
    got = combo_host(sc, 0)
    w, cdf = cr.mixture_configure(weights, ensure=False)
    assert np.array_equal(got['weights'], np.asarray(weights, f32)) and np.array_equal(got['cdf'].view(np.uint32), cdf.view(np.uint32))


def test_sample_reuse_restatement():
    _, cdf = cr.mixture_configure((0.5, 0.9, 0.6))
    assert cr.sample_reuse(cdf, f32(0.0))[0] == 0 and cr.sample_reuse(cdf, cdf[1])[0] == 0
    assert cr.sample_reuse(cdf, np.nextafter(cdf[1], f32(1)))[0] == 1 and cr.sample_reuse(cdf, f32(0.99))[0] == 2
    i, u, p = cr.sample_reuse(cdf, f32(0.5))
    assert i == 1 and p == f32(cdf[2] - cdf[1]) and u == f32(f32(f32(0.5) - cdf[1]) / p)


# ---- the energy test's sample count (tests/test_gpu_combo.py::test_energy_under_area_light) ----
def test_energy_calibration(oracle):
    """With the oracle alone at combo_ref.ENERGY_SPP = 896: the plain diffuse C1 against itself
    under another scramble gives z <= 2 in every channel, against itself with every reflectance
    scaled by 1.05 z >= 6 in every channel (measured: z = 0.125 / 0.131 / 0.113 and
    13.43 / 10.43 / 6.05); four samples fewer, the 5% error's z falls below 6 in blue (5.96), as
    it does at every smaller multiple of 4 (a scan from 4 spp up, run once; 396 spp: 4.18)."""
    import delta_ref as dr
    keep = np.ones(32 * 32, bool)

    def mean(spp, scramble, scale=1.0):
        sc, it = cr.energy_plain(spp, scramble, scale)
        return dr.image_mean(oracle.render(sc, it, samples=True, libm_mode=0)[1], keep, spp)

    spp = cr.ENERGY_SPP
    a = mean(spp, 0)
    z = dr.z_score(a, mean(spp, cr.ENERGY_SCRAMBLE))
    z5 = dr.z_score(a, mean(spp, cr.ENERGY_SCRAMBLE, 1.05))
    below = dr.z_score(mean(spp - 4, 0), mean(spp - 4, cr.ENERGY_SCRAMBLE, 1.05))
    print('z', z, 'z at a 5% error', z5, 'at 4 spp fewer', below)
    assert spp % 4 == 0 and (z <= 2).all() and (z5 >= 6).all(), (z, z5)
    assert not (below >= 6).all(), below


# ---- fields ---------------------------------------------------------------------------------
def test_albedo_is_refused():
    sc, _ = _scene(cr.cases()['mix2'])
    with pytest.raises(MtsgpuError, match="'albedo' field is not supported"):
        albedo_factors_host(sc)
    assert albedo_factors_host(scenes.build('C1', width=32, height=32, spp=4)[0]).tolist() == [1.0, 1.0, 1.0]


# ---- XML ------------------------------------------------------------------------------------
XML = '''<scene version="0.6.0">
  <integrator type="path"><integer name="maxDepth" value="3"/></integrator>
  <sensor type="perspective">
    <transform name="toWorld"><lookat origin="0, 1, -4" target="0, 1, 0" up="0, 1, 0"/></transform>
    <sampler type="sobol"><integer name="sampleCount" value="4"/></sampler>
    <film type="hdrfilm"><integer name="width" value="16"/><integer name="height" value="16"/>
      <rfilter type="box"/></film>
  </sensor>
  <bsdf type="roughconductor" id="gold"><string name="material" value="Au"/><float name="alpha" value="0.2"/></bsdf>
  %s
  <emitter type="constant"/>
</scene>
'''
GOOD = '''<shape type="cube"><bsdf type="mixturebsdf"><string name="weights" value="0.5, 0.9; 0.6"/>
      <bsdf type="diffuse"><rgb name="reflectance" value="0.5, 0.4, 0.3"/></bsdf><ref id="gold"/>
      <bsdf type="plastic"/></bsdf></shape>
  <shape type="cube"><bsdf type="blendbsdf">
      <texture type="checkerboard" name="weight"><float name="uvscale" value="3"/></texture>
      <bsdf type="diffuse"/><ref id="gold"/></bsdf></shape>
  <shape type="cube"><bsdf type="mask"><rgb name="opacity" value="0.2, 0.5, 0.8"/>
      <bsdf type="twosided"><bsdf type="blendbsdf"><float name="weight" value="0.3"/>
        <bsdf type="diffuse"/><ref id="gold"/></bsdf></bsdf></bsdf></shape>
  <shape type="cube"><bsdf type="mask"><texture type="checkerboard" name="opacity"/><bsdf type="diffuse"/></bsdf></shape>'''


def _write(tmp_path, body):
    p = tmp_path / 'scene.xml'
    p.write_text(XML % body)
    return str(p)


def _shape_bsdfs(sc):
    return [sc.bsdfs[m.bsdf] for m in sc.meshes]


def test_xml_load_desc_and_round_trip(tmp_path):
    sc, it = load_scene(_write(tmp_path, GOOD))
    mix, blend, mask, mask2 = _shape_bsdfs(sc)
    assert mix.type == 'mixturebsdf' and mix.weights == [0.5, 0.9, 0.6]
    assert [b.type for b in mix.nested] == ['diffuse', 'roughconductor', 'plastic'] and mix.nested[1].material == 'Au'
    assert blend.type == 'blendbsdf' and isinstance(blend.weight, Checkerboard) and blend.weight.uscale == 3.0
    assert mask.type == 'mask' and np.array_equal(np.asarray(mask.opacity, f32), np.array([0.2, 0.5, 0.8], f32))
    assert mask.nested[0].type == 'twosided' and mask.nested[0].nested[0].type == 'blendbsdf'
    assert f32(mask.nested[0].nested[0].weight) == f32(0.3) and isinstance(mask2.opacity, Checkerboard)
    assert check_scene(sc) is None
    # the descriptor: children / nested point at the flattened list, the new fields are filled
    flat, idx = sc.flat_bsdfs()
    d = sc.desc()
    by = {id(b): i for i, b in enumerate(flat)}
    dm = d.bsdfs[by[id(mix)]]
    assert dm.type == abi.BSDF_MIXTURE and dm.num_children == 3 and dm.num_weights == 3
    assert [flat[dm.children[k]].type for k in range(3)] == ['diffuse', 'roughconductor', 'plastic']
    assert list(dm.weights)[:3] == [f32(0.5), f32(0.9), f32(0.6)]
    db = d.bsdfs[by[id(blend)]]
    assert db.type == abi.BSDF_BLEND and db.weight_tex.type == abi.TEX_CHECKERBOARD and db.weight_tex.uscale == 3.0
    assert [flat[db.nested[k]].type for k in range(2)] == ['diffuse', 'roughconductor']
    dk = d.bsdfs[by[id(mask)]]
    assert dk.type == abi.BSDF_MASK and list(dk.opacity) == [f32(0.2), f32(0.5), f32(0.8)] and dk.nested[1] == -1
    two = flat[dk.nested[0]]
    assert two.type == 'twosided' and flat[d.bsdfs[dk.nested[0]].nested[0]].type == 'blendbsdf'
    assert d.bsdfs[d.bsdfs[dk.nested[0]].nested[0]].weight == f32(0.3)
    assert d.bsdfs[by[id(mask2)]].opacity_tex.type == abi.TEX_CHECKERBOARD
    # save and load again
    out = tmp_path / 'saved'
    os.makedirs(out)
    sc2, _ = load_scene(save_scene(sc, it, str(out)))
    d2 = sc2.desc()      # (no roughplastic here: the descriptors hold no pointer)
    assert d2.num_bsdfs == d.num_bsdfs and [m.bsdf for m in sc2.meshes] == [m.bsdf for m in sc.meshes]
    for i in range(d.num_bsdfs):
        assert bytes(d.bsdfs[i]) == bytes(d2.bsdfs[i]), (i, flat[i].type)


@pytest.mark.parametrize('body,exc,text', [
    ('<bsdf type="mixturebsdf"><string name="weights" value="1, 1"/><bsdf type="diffuse"/>'
     '<bsdf type="blendbsdf"><bsdf type="diffuse"/><bsdf type="diffuse"/></bsdf></bsdf>', NotImplementedError,
     'mixturebsdf: a nested "blendbsdf"'),
    ('<bsdf type="blendbsdf"><bsdf type="diffuse"/><bsdf type="twosided"><bsdf type="diffuse"/></bsdf></bsdf>',
     NotImplementedError, 'blendbsdf: a nested "twosided"'),
    ('<bsdf type="twosided"><bsdf type="mask"><bsdf type="diffuse"/></bsdf></bsdf>', NotImplementedError,
     'twosided: a nested "mask"'),
    ('<bsdf type="mask"><bsdf type="mask"><bsdf type="diffuse"/></bsdf></bsdf>', NotImplementedError, 'mask: a nested "mask"'),
    ('<bsdf type="mask"><bsdf type="roughdielectric"/></bsdf>', NotImplementedError, 'mask: a nested "roughdielectric"'),
    ('<bsdf type="mask"><bsdf type="twosided"><bsdf type="blendbsdf"><bsdf type="diffuse"/><bsdf type="roughdielectric"/>'
     '</bsdf></bsdf></bsdf>', NotImplementedError, 'a nested "roughdielectric"'),
    ('<bsdf type="mixturebsdf"><string name="weights" value="%s"/>%s</bsdf>' % (', '.join(['0.1'] * 9), '<bsdf type="diffuse"/>' * 9),
     NotImplementedError, 'mixturebsdf: more than 8'),
    ('<bsdf type="mixturebsdf"><string name="weights" value="0.5"/><bsdf type="diffuse"/><bsdf type="diffuse"/></bsdf>',
     SceneError, 'BSDF count mismatch: 2 bsdfs, but specified 1 weights'),
    ('<bsdf type="mixturebsdf"><string name="weights" value="0, 0"/><bsdf type="diffuse"/><bsdf type="diffuse"/></bsdf>',
     SceneError, 'The weights must sum to a value greater than zero!'),
    ('<bsdf type="mixturebsdf"><bsdf type="diffuse"/></bsdf>', SceneError, 'No weights were supplied!'),
    ('<bsdf type="blendbsdf"><bsdf type="diffuse"/></bsdf>', SceneError, 'expected two nested BSDF instances'),
    ('<bsdf type="mask"/>', SceneError, 'A child BSDF is required'),
    ('<bsdf type="coating"><bsdf type="diffuse"/></bsdf>', NotImplementedError, 'coating'),
])
def test_xml_refuses(tmp_path, body, exc, text):
    with pytest.raises(exc, match=text):
        load_scene(_write(tmp_path, '<shape type="cube">%s</shape>' % body))
