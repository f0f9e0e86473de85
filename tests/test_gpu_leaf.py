"""difftrans, roughdiffuse and phong on the GPU (dleaf2.h, the MTSG_FEAT_SET_LEAF2 kernels).

The oracle has none of the three, so leaf_ref.py restates them in numpy float32 and the
per-sample records are compared bit for bit:

1. eval(): the first bounce under a point light (path / volpath at maxDepth 2, direct);
2. sample(): two vertices under a point light (path / volpath at maxDepth 3);
3. checks that do not rest on the restatement: roughdiffuse(alpha = 0, useFastApprox) against
   the oracle's plain diffuse, the difftrans mirror (a quad with the light behind it against
   the oracle's diffuse with the light mirrored), the difftrans furnace;
4. the engines agree at full depth on a scene with all three (LDS, HBM, wavefront, plain
   kernels, the kd-tree flag, chunks, a tile shard);
and multichannel renders with `distance` and `albedo` fields: the albedo of the three leaves
against mtsgpu_albedo_factors_host's values (a scene that also holds a combinator still raises).

C1 at 32 x 32, 4 spp, box filter, Sobol.  Debug counter 15 must show VARIANT_LEAF2 for every
render.  On the parent commit every upload here fails with 'unsupported BSDF type'.
"""
import copy

import numpy as np
import pytest

import combo_ref as cr
import delta_ref as dr
import leaf_ref as lr
from mitsuba_amd.integrator import VARIANT_LEAF2, MtsgpuError
from mitsuba_amd.scene import (BSDF, DirectIntegrator, Emitter, FieldIntegrator, MultiChannelIntegrator, PathIntegrator,
                               VolpathIntegrator)

pytestmark = pytest.mark.gpu

SPP, SIZE = 4, 32
BUDGET = 1 << 20      # the smallest MTSGPU_CONTRIB_BYTES the library takes
ENGINES = ('lds', 'hbm', 'wavefront')


def _integrator(kind, max_depth, spp=SPP, rr=5):
    if kind == 'path':
        return PathIntegrator(maxDepth=max_depth, rrDepth=rr, sampleCount=spp, rfilter='box')
    if kind == 'volpath':
        return VolpathIntegrator(maxDepth=max_depth, rrDepth=rr, sampleCount=spp, rfilter='box')
    return DirectIntegrator(sampleCount=spp, rfilter='box')


def _render(gpu_ctx, monkeypatch, sc, it, engine, samples=True, **kw):
    if engine == 'hbm':
        monkeypatch.setenv('MTSGPU_NO_SCENE_LDS', '1')
    else:
        monkeypatch.delenv('MTSGPU_NO_SCENE_LDS', raising=False)
    gpu_ctx.upload(sc)
    film, smp, st = gpu_ctx.render(it, samples=samples, engine='wavefront' if engine == 'wavefront' else None, **kw)
    word = gpu_ctx.debug_counters()[15]
    assert word & VARIANT_LEAF2, hex(word)
    if engine == 'wavefront':
        assert word & (1 << 16), hex(word)
    else:
        assert bool(word & (1 << 12)) == (engine == 'lds'), hex(word)
    return film, smp, st


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_li(smp, want, what):
    bad = np.nonzero(np.any(_bits(smp[:, 0:3]) != _bits(want), 1))[0]
    assert bad.size == 0, (what, bad.size, bad[:4], smp[bad[:4], 0:3], want[bad[:4]])


def _kinds_engines(case, kinds):
    return [(k, e) for k in kinds for e in ENGINES if not (k == 'direct' and e == 'wavefront')]


# ---- 1 / 2. eval and sample against the restatement -------------------------------------------
@pytest.fixture(scope='module')
def base(oracle):
    """The oracle's view of the shared geometry (sample positions, first vertices) and the
    samples' BSDF draw at the first vertex, Sobol dimensions 5 and 6 (test_gpu_combo.py's
    fixture says why), and the restatements computed so far."""
    sc, twin = cr.point_scene(BSDF('diffuse'), 2, SIZE, SPP)
    _, smp, _ = oracle.render(twin, _integrator('path', 2), samples=True, libm_mode=0)
    H = dr.first_hits(sc, twin, oracle, smp[:, 4], smp[:, 5])
    return dict(smp=smp, H=H, u45=cr.sobol_2d(oracle, SIZE, SPP, 5), cache={})


def _checker_split(b, uv):
    """Samples on each colour of the case's checkerboard (None: the case has none)."""
    from mitsuba_amd.scene import Checkerboard
    import fields_ref as fr
    tex = [v for x in [b] + list(b.nested) for v in (x.diffuseReflectance, x.alpha, x.opacity, x.transmittance)
           if isinstance(v, Checkerboard)]
    if not tex:
        return None
    ok = ~np.isnan(uv[:, 0])
    is0 = fr.checker_is_color0(tex[0], uv[ok, 0], uv[ok, 1])
    return int(is0.sum()), int((~is0).sum())


EVAL = [(c, k, e) for c in lr.cases() for k, e in _kinds_engines(c, ('path', 'volpath', 'direct'))]


@pytest.mark.parametrize('case,kind,engine', EVAL, ids=['-'.join(f) for f in EVAL])
def test_eval_first_bounce(gpu_ctx, oracle, monkeypatch, base, case, kind, engine):
    b = lr.cases()[case]
    sc, twin = lr.case_scene(case, 2, 'eval', SIZE, SPP)
    key = ('eval', case, kind)
    if key not in base['cache']:
        base['cache'][key] = lr.nee(sc, twin, oracle, base['H'], kind)
    want, info = base['cache'][key]
    assert info['lit'].sum() > 200 and (info['use'] & ~info['lit']).sum() > 20, (info['lit'].sum(), info['use'].sum())
    split = _checker_split(b, base['H']['uv'])
    assert split is None or min(split) > 50, split
    _, smp, _ = _render(gpu_ctx, monkeypatch, sc, _integrator(kind, 2), engine)
    _assert_li(smp, want, (case, kind, engine))
    assert np.array_equal(_bits(smp[:, 3:6]), _bits(base['smp'][:, 3:6]))


SAMPLE = [(c, k, e) for c in lr.cases() for k, e in _kinds_engines(c, ('path', 'volpath'))]


def _leaf_lobes(choices):
    out = {}
    for ch in choices:
        for c in ch or ():
            if isinstance(c, str) and c.startswith('lobe'):
                out[c] = out.get(c, 0) + 1
    return out


@pytest.mark.parametrize('case,kind,engine', SAMPLE, ids=['-'.join(f) for f in SAMPLE])
def test_sample_two_vertices(gpu_ctx, oracle, monkeypatch, base, case, kind, engine):
    """Li = NEE_1 + thr * NEE_2 at maxDepth 3 (no ray can hit a point light): the BSDF sample at
    the first vertex restated from the sample's Sobol dimensions 5 and 6, the second vertex from
    oracle_intersect."""
    b = lr.cases()[case]
    sc, twin = lr.case_scene(case, 3, 'sample', SIZE, SPP)
    key = ('sample', case, kind)
    if key not in base['cache']:
        base['cache'][key] = lr.two_vertices(sc, twin, oracle, base['H'], base['u45'], kind)
    want, info = base['cache'][key]
    if 'phong' in case:
        # both lobes of phong
        shape = base['H']['shape']
        mine = [ch for i, ch in enumerate(info['choices'])
                if ch and sc.bsdfs[sc.meshes[shape[i]].bsdf].type != 'diffuse']
        lobes = _leaf_lobes(mine)
        total = sum(lobes.values())
        assert len(lobes) == 2 and min(lobes.values()) >= 0.05 * total, (case, lobes)
    assert np.any(info['c2'] != 0, 1).sum() >= 100, np.any(info['c2'] != 0, 1).sum()
    _, smp, _ = _render(gpu_ctx, monkeypatch, sc, _integrator(kind, 3), engine)
    _assert_li(smp, want, (case, kind, engine))


# ---- 3. checks that do not rest on the restatement --------------------------------------------
_plain = {}


@pytest.mark.parametrize('kind,engine', [(k, e) for k in ('path', 'volpath', 'direct') for e in ENGINES
                                         if not (k == 'direct' and e == 'wavefront')])
def test_roughdiffuse_alpha_zero_is_diffuse(gpu_ctx, oracle, monkeypatch, base, kind, engine):
    """sigma = 0: A = 1 - 0 / 0.33 = 1 and B = 0, so the value is rho * ((INV_PI * cos) * (1 + 0 *
    ...)), the plain diffuse value, unless tanBeta is not finite (0 * inf).  maxDepth 2 under the
    point light, where only eval() counts.  The oracle cannot configure a point light, so its
    diffuse eval() goes through delta_ref.first_bounce (the delta emitters' own reference, which
    takes the BSDF value, the hits and the occlusion from the oracle); the GPU's render of the
    plain diffuse scene, which runs none of the new code, must give the same records too."""
    refl = (0.5, 0.4, 0.3)
    sc, twin = cr.point_scene(BSDF('roughdiffuse', reflectance=refl, alpha=0.0, useFastApprox=True), 2, SIZE, SPP)
    it = _integrator(kind, 2)
    if kind not in _plain:
        plain, ptwin = cr.point_scene(BSDF('diffuse', reflectance=refl), 2, SIZE, SPP)
        li, info = dr.first_bounce(plain, ptwin, oracle, base['H'], kind, em=plain.emitters[0])
        gpu_ctx.upload(plain)
        rec = gpu_ctx.render(it, samples=True)[1]
        assert not gpu_ctx.debug_counters()[15] & VARIANT_LEAF2
        _plain[kind] = (li, rec, int(info['lit'].sum()))
    li, rec, lit = _plain[kind]
    assert lit > 200
    _, smp, _ = _render(gpu_ctx, monkeypatch, sc, it, engine)
    bad = np.nonzero(np.any(_bits(smp[:, 0:3]) != _bits(li), 1))[0]
    if bad.size:      # is it the restated tanBeta?  (0 * inf at a grazing vertex)
        V = base['H']
        with np.errstate(divide='ignore', invalid='ignore'):
            tb = lr.sin_theta(V['wi'][bad]) / V['wi'][bad][:, 2]
        print('differing samples', bad.size, 'of which tanBeta(wi) is not finite at', int((~np.isfinite(tb)).sum()))
    assert bad.size == 0, (kind, engine, bad.size, smp[bad[:4], 0:3], li[bad[:4]])
    assert np.array_equal(_bits(smp), _bits(rec))


def test_difftrans_furnace(gpu_ctx, monkeypatch):
    """Every surface difftrans(transmittance = 1) under a constant environment, full depth,
    rrDepth 64, 64 spp: each channel's image mean within 4 standard errors of the radiance
    (delta_ref.image_mean; the bound of the other energy tests).  Measured on the MI355X: means
    0.69996 / 1.09994 / 1.89990, z = 0.056 in every channel."""
    rad = np.array([0.7, 1.1, 1.9])
    spp = 64
    sc, _, _ = dr.delta_scene([Emitter('constant', radiance=tuple(rad))], width=SIZE, height=SIZE, spp=spp, max_depth=-1)
    cr.all_surfaces(sc, BSDF('difftrans', transmittance=1.0))
    _, smp, _ = _render(gpu_ctx, monkeypatch, sc, _integrator('path', -1, spp=spp, rr=64), 'lds')
    mean, se = dr.image_mean(smp, np.ones(SIZE * SIZE, bool), spp)
    z = np.abs(mean - rad) / np.maximum(se, 1e-300)
    print('difftrans furnace: mean', mean, 'se', se, 'z', z, 'max depth', smp[:, 6].max())
    assert (np.abs(mean - rad) <= 4 * se + 1e-6 * rad).all(), (mean, se, z)
    assert smp[:, 6].max() > 3 and np.isfinite(smp).all()


# ---- 4. the engines agree at full depth ---------------------------------------------------------
def _agree_scene(width=SIZE, height=SIZE, spp=SPP):
    sc, _, _ = dr.delta_scene([Emitter('constant', radiance=(0.4, 0.5, 0.7))], keep_area=True, materials='smooth',
                              width=width, height=height, spp=spp, max_depth=-1)
    C = lr.cases()
    sc.meshes = [copy.copy(m) for m in sc.meshes]
    sc.bsdfs = [C['phong_chk'], C['rdiff_chk'], C['difftrans'], C['phong30'], C['blend_phong_rdiff']]
    for i, m in enumerate(sc.meshes):
        if m.bsdf >= 0:
            m.bsdf = (0, 1, 0, 4, 1, 2, 3, 0)[i]      # floor, ceiling, back, left, right, the two boxes, the light quad
    return sc, _integrator('path', -1, spp=spp)


def test_engines_agree(gpu_ctx, monkeypatch):
    sc, it = _agree_scene()
    ref_film, ref_smp, _ = _render(gpu_ctx, monkeypatch, sc, it, 'lds')
    assert np.isfinite(ref_smp).all() and ref_smp[:, 0:3].max() > 0 and ref_smp[:, 6].max() > 3
    runs = {
        'hbm': lambda: _render(gpu_ctx, monkeypatch, sc, it, 'hbm'),
        'wavefront': lambda: _render(gpu_ctx, monkeypatch, sc, it, 'wavefront'),
        'plain': lambda: _render(gpu_ctx, monkeypatch, sc, it, 'lds', samples=False),
        'plain-hbm': lambda: _render(gpu_ctx, monkeypatch, sc, it, 'hbm', samples=False),
        'plain-wavefront': lambda: _render(gpu_ctx, monkeypatch, sc, it, 'wavefront', samples=False),
    }
    for name, run in runs.items():
        film, smp, _ = run()
        assert np.array_equal(_bits(film), _bits(ref_film)), name
        if smp is not None:
            assert np.array_equal(_bits(smp), _bits(ref_smp)), name
    gpu_ctx.upload(sc)
    film, smp, _ = gpu_ctx.render(it, samples=True, engine='kdtree')
    assert gpu_ctx.debug_counters()[15] & VARIANT_LEAF2
    assert np.array_equal(_bits(smp), _bits(ref_smp)) and np.array_equal(_bits(film), _bits(ref_film))
    # three launches: 1 MiB of records holds 2 of the 6 samples of 192 x 128 pixels (16 B each)
    big_sc, big_it = _agree_scene(192, 128, 6)
    one_film, one_smp, _ = _render(gpu_ctx, monkeypatch, big_sc, big_it, 'lds')
    monkeypatch.setenv('MTSGPU_CONTRIB_BYTES', str(BUDGET))
    film, smp, _ = _render(gpu_ctx, monkeypatch, big_sc, big_it, 'lds')
    assert gpu_ctx.launch_chunks() == 3, gpu_ctx.launch_chunks()
    monkeypatch.delenv('MTSGPU_CONTRIB_BYTES')
    assert np.array_equal(_bits(film), _bits(one_film)) and np.array_equal(_bits(smp), _bits(one_smp))
    # a tile shard: every other 8x8 tile, whose records equal the whole render's there
    film, smp, _ = _render(gpu_ctx, monkeypatch, sc, it, 'lds', row=(0, 2, 1), tile_shard=True)
    pix = np.arange(SIZE * SIZE)
    tile = (pix // SIZE // 8) * (SIZE // 8) + (pix % SIZE) // 8
    mine = np.repeat(tile % 2 == 1, SPP)
    assert np.array_equal(_bits(smp[mine]), _bits(ref_smp[mine]))


# ---- fields ----------------------------------------------------------------------------------
def test_fields_over_the_leaves(gpu_ctx, monkeypatch):
    sc, it = _agree_scene()
    film, _, _ = _render(gpu_ctx, monkeypatch, sc, it, 'lds', samples=False)
    mc = MultiChannelIntegrator(children=[it, FieldIntegrator('distance')], sampleCount=SPP, rfilter='box')
    gpu_ctx.upload(sc)
    films, _, _ = gpu_ctx.render(mc)
    assert np.array_equal(_bits(films[0][..., 0:3]), _bits(film[..., 0:3]))
    plain = cr.all_surfaces(copy.copy(sc), BSDF('diffuse'))
    gpu_ctx.upload(plain)
    want, _, _ = gpu_ctx.render(MultiChannelIntegrator(children=[FieldIntegrator('distance')], sampleCount=SPP,
                                                        rfilter='box'))
    assert np.array_equal(_bits(films[1]), _bits(want[0])) and films[1][..., 0].max() > 0
    gpu_ctx.upload(sc)      # (the scene has a blendbsdf: the combinators' refusal stands)
    with pytest.raises((NotImplementedError, MtsgpuError), match='albedo'):
        gpu_ctx.render(MultiChannelIntegrator(children=[FieldIntegrator('albedo')], sampleCount=SPP, rfilter='box'))


def _leaf_scene():
    """_agree_scene without a combinator: the left wall is twosided(phong)."""
    sc, it = _agree_scene()
    sc.bsdfs = list(sc.bsdfs[:4]) + [lr.cases()['twosided_phong']]
    return sc, it


def test_albedo_of_the_leaves(gpu_ctx, oracle, monkeypatch):
    """A multichannel render with `distance` and `albedo` over the three-type scene: the radiance
    film is the plain render's, and every sample's albedo is the BSDF's diffuse reflectance at the
    hit's uv (phong's diffuseReflectance, a checkerboard here; roughdiffuse's reflectance) times
    mtsgpu_albedo_factors_host's value: 1 for the two, 0 for difftrans."""
    import fields_ref as fr
    from mitsuba_amd.integrator import albedo_factors_host
    from mitsuba_amd.scene import Checkerboard
    sc, it = _leaf_scene()
    film, _, _ = _render(gpu_ctx, monkeypatch, sc, it, 'lds', samples=False)
    mc = MultiChannelIntegrator(children=[it, FieldIntegrator('distance'), FieldIntegrator('albedo')], sampleCount=SPP,
                                rfilter='box')
    gpu_ctx.upload(sc)
    films, _, _ = gpu_ctx.render(mc)
    assert np.array_equal(_bits(films[0][..., 0:3]), _bits(film[..., 0:3]))
    _, rec, _ = gpu_ctx.render_fields(it, [FieldIntegrator('albedo'), FieldIntegrator('uv')], samples=True)
    assert gpu_ctx.debug_counters()[15] & VARIANT_LEAF2
    flat, _ = sc.flat_bsdfs()
    factors = albedo_factors_host(sc)
    want_f = {'phong': 1.0, 'roughdiffuse': 1.0, 'difftrans': 0.0, 'twosided': 0.0}
    assert [float(f) for f in factors] == [want_f[b.type] for b in flat], factors
    o, d, mint, maxt = fr.primary_rays(sc, oracle, rec[:, 0], rec[:, 1])
    geo = cr.all_surfaces(copy.copy(sc), BSDF('diffuse'))      # (the oracle has none of the three: geometry only)
    hits = oracle.trace_rays(geo, o, d, mint, maxt)
    hit = np.isfinite(hits[:, 0])
    assert np.array_equal(rec[:, 3] != 0, hit)
    uv = fr.hit_uv(sc, hits)
    shape, _ = fr.prim_tables(sc)
    mesh = shape[np.minimum(hits[:, 3].view(np.uint32).astype(np.int64), len(shape) - 1)]
    exp = np.zeros((hit.size, 3), np.float32)
    seen = set()
    for mi, m in enumerate(sc.meshes):
        sel = hit & (mesh == mi)
        if not sel.any() or m.bsdf < 0:
            continue
        b = sc.bsdfs[m.bsdf]
        leaf = b.nested[0] if b.type == 'twosided' else b      # (one nested BSDF: both sides are it)
        fac = np.float32(factors[flat.index(leaf)])
        v = leaf.diffuseReflectance if leaf.type == 'phong' else leaf.reflectance
        if isinstance(v, Checkerboard):
            is0 = fr.checker_is_color0(v, uv[sel, 0], uv[sel, 1])
            c = np.where(is0[:, None], fr._spec3(v.color0)[None, :], fr._spec3(v.color1)[None, :]).astype(np.float32)
        else:
            c = np.repeat(np.asarray(fr._spec3(v), np.float32)[None, :], int(sel.sum()), 0)
        exp[sel] = (c * fac).astype(np.float32)
        seen.add(b.type)
    assert {'phong', 'roughdiffuse', 'difftrans', 'twosided'} <= seen, seen
    got = rec[:, 4:7]
    bad = np.nonzero(hit & np.any(_bits(got) != _bits(exp), 1))[0]
    assert bad.size == 0, (bad.size, got[bad[:4]], exp[bad[:4]], mesh[bad[:4]])
    assert (exp[hit] != 0).any(1).sum() > 500 and (exp[hit] == 0).all(1).sum() > 100


# ---- the difftrans mirror --------------------------------------------------------------------
_mirror = {}


@pytest.mark.parametrize('kind,engine', [(k, e) for k in ('path', 'volpath', 'direct') for e in ENGINES
                                         if not (k == 'direct' and e == 'wavefront')])
def test_difftrans_mirror(gpu_ctx, oracle, monkeypatch, base, kind, engine):
    """A quad in z = 0 as difftrans(T) with the point light at (x, y, +h) behind it, against the
    same quad as diffuse(T) with the light mirrored to (x, y, -h), maxDepth 2: the hit points have
    z = 0 exactly (barycentric sums of zeros), so the mirrored light's direction is the other one
    with z negated, |cos| replaces cos, and the records agree bit for bit.  The oracle has no point
    light; its diffuse eval(), hits and occlusion go through delta_ref.first_bounce."""
    T = (0.7, 0.5, 0.3)
    dt, df, twin = lr.mirror_scenes(T, 3.0, SIZE, SPP)
    if kind not in _mirror:
        H = dr.first_hits(df, twin, oracle, base['smp'][:, 4], base['smp'][:, 5])
        on_quad = H['valid'] & (H['shape'] == 0)
        assert (H['p'][on_quad][:, 2] == 0).all()
        li, info = dr.first_bounce(df, twin, oracle, H, kind, em=df.emitters[0])
        _mirror[kind] = (li, int(info['lit'].sum()))
    li, lit = _mirror[kind]
    assert lit > 200
    _, smp, _ = _render(gpu_ctx, monkeypatch, dt, _integrator(kind, 2), engine)
    _assert_li(smp, li, (kind, engine))
