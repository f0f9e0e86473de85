"""mixturebsdf, blendbsdf and mask on the GPU (dcombo.h, the MTSG_FEAT_SET_COMBO kernels).

The oracle has no combinator BSDF, so only the identity test compares against an oracle
render.  The rest (combo_ref.py) restates the combinators in numpy float32 over the oracle's
leaf entry points and compares per-sample records bit for bit:

1. mask(opacity = 1) over X is X: records and film of the oracle's render of the unwrapped
   scene, every material set without a roughdielectric, full depth, every engine;
2. the null lobe in closed form: mask(opacity = 0) everywhere under a constant environment;
3. eval(): the first bounce under a point light (path / volpath at maxDepth 2, direct);
4. sample(): two vertices under a point light (path / volpath at maxDepth 3);
5. the engines agree at full depth (LDS, HBM, wavefront, plain kernels, chunks, a tile shard,
   the kd-tree flag);
6. energy under the area light: blend(0.5, A, A) and mixture("0.25, 0.75", A, A) against the
   oracle's plain A (the combinators' pdf() inside NEE's MIS), at the calibrated 896 spp;
and a multichannel render with a `distance` field over a combinator scene; `albedo` raises.

C1 at 32 x 32, 4 spp, box filter, Sobol.  Debug counter 15 must show VARIANT_COMBO for every
render.  On the parent commit every upload here fails with 'unsupported BSDF type'.
"""
import copy

import numpy as np
import pytest

import combo_ref as cr
import delta_ref as dr
from mitsuba_amd import scenes
from mitsuba_amd.integrator import VARIANT_COMBO, MtsgpuError
from mitsuba_amd.scene import (BSDF, DirectIntegrator, Emitter, FieldIntegrator, MultiChannelIntegrator, PathIntegrator,
                               VolpathIntegrator)

pytestmark = pytest.mark.gpu

SPP, SIZE = 4, 32
BUDGET = 1 << 20      # the smallest MTSGPU_CONTRIB_BYTES the library takes
ENGINES = ('lds', 'hbm', 'wavefront')


def _integrator(kind, max_depth, strict=False, spp=SPP, rr=5):
    if kind == 'path':
        return PathIntegrator(maxDepth=max_depth, rrDepth=rr, sampleCount=spp, rfilter='box', strictNormals=strict)
    if kind == 'volpath':
        return VolpathIntegrator(maxDepth=max_depth, rrDepth=rr, sampleCount=spp, rfilter='box', strictNormals=strict)
    return DirectIntegrator(sampleCount=spp, rfilter='box', strictNormals=strict)


def _render(gpu_ctx, monkeypatch, sc, it, engine, samples=True, **kw):
    if engine == 'hbm':
        monkeypatch.setenv('MTSGPU_NO_SCENE_LDS', '1')
    else:
        monkeypatch.delenv('MTSGPU_NO_SCENE_LDS', raising=False)
    gpu_ctx.upload(sc)
    film, smp, st = gpu_ctx.render(it, samples=samples, engine='wavefront' if engine == 'wavefront' else None, **kw)
    word = gpu_ctx.debug_counters()[15]
    assert word & VARIANT_COMBO, hex(word)
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


def _kinds_engines(kinds):
    return [(k, e) for k in kinds for e in ENGINES if not (k == 'direct' and e == 'wavefront')]


# ---- 1. mask(opacity = 1) is the identity ----------------------------------------------------
SETS = ('diffuse', 'plastic', 'smooth', 'shapes')      # scenes.build's material sets without a roughdielectric
_oracle_cache = {}


def _wrapped(materials):
    sc, _ = scenes.build('C1', width=SIZE, height=SIZE, spp=SPP, materials=materials, max_depth=-1)
    wr = copy.copy(sc)
    wr.bsdfs = [BSDF('mask', opacity=1.0, nested=[b]) for b in sc.bsdfs]
    return sc, wr


@pytest.mark.parametrize('kind,engine', _kinds_engines(('path', 'volpath', 'direct')))
@pytest.mark.parametrize('materials', SETS)
def test_mask_identity(gpu_ctx, oracle, monkeypatch, materials, kind, engine):
    """prob = (1 * 0.212671f + 1 * 0.715160f) + 1 * 0.072169f == 1.0f, every product and
    quotient by 1 is exact and sample.x < 1 always: the wrapped scene renders the plain one's
    records bit for bit, through the combinator code (VARIANT_COMBO)."""
    sc, wr = _wrapped(materials)
    it = _integrator(kind, -1)
    key = (materials, kind)
    if key not in _oracle_cache:
        _oracle_cache[key] = oracle.render(sc, it, samples=True, libm_mode=0)[:2]
    film_o, smp_o = _oracle_cache[key]
    film, smp, _ = _render(gpu_ctx, monkeypatch, wr, it, engine)
    same = np.all(_bits(smp) == _bits(smp_o), axis=1)
    bad = np.nonzero(~same)[0]
    assert same.all(), (materials, kind, engine, bad.size, bad[:3], smp[bad[:3]], smp_o[bad[:3]])
    # The film: the oracle sums a pixel's samples in its own order (as in test_gpu_parity.py, where
    # a few words of the film differ in the last bit from the GPU's ordered reduction), so against
    # the oracle it is held as there, and bit for bit against the GPU's own film of the plain scene
    np.testing.assert_allclose(film, film_o, rtol=1e-6, atol=1e-7)
    assert np.mean(_bits(film) == _bits(film_o)) > 0.999
    gpu_ctx.upload(sc)
    film_p, smp_p, _ = gpu_ctx.render(it, samples=True, engine='wavefront' if engine == 'wavefront' else None)
    assert not gpu_ctx.debug_counters()[15] & VARIANT_COMBO
    assert np.array_equal(_bits(film), _bits(film_p)) and np.array_equal(_bits(smp), _bits(smp_p))
    assert smp[:, 6].max() > 3 or kind == 'direct'


# ---- 2. the null lobe in closed form ---------------------------------------------------------
@pytest.mark.parametrize('kind,engine', _kinds_engines(('path', 'volpath')))
def test_null_lobe_closed_form(gpu_ctx, monkeypatch, kind, engine):
    """Every mesh is mask(opacity = 0, diffuse) under a constant environment: the throughput is
    (1 - 0) / (1 - 0) at every vertex and the MIS weight of the environment 1 / (1 + 0), so
    every sample's Li is the radiance bit for bit, alpha is 1 where the camera ray hit, and
    paths run through several surfaces."""
    rad = (0.7, 1.1, 1.9)
    sc, _, _ = dr.delta_scene([Emitter('constant', radiance=rad)], width=SIZE, height=SIZE, spp=SPP, max_depth=-1)
    cr.all_surfaces(sc, BSDF('mask', opacity=0.0, nested=[BSDF('diffuse', reflectance=(0.5, 0.4, 0.3))]))
    _, smp, _ = _render(gpu_ctx, monkeypatch, sc, _integrator(kind, -1, rr=64), engine)
    # (a camera ray that misses sees the environment itself: every sample has that Li.  The depth
    # record counts the surfaces a path went through before it left the scene)
    want = np.broadcast_to(np.asarray(rad, np.float32), (smp.shape[0], 3))
    _assert_li(smp, want, (kind, engine))
    through = smp[:, 6] > 1
    assert through.sum() > 500 and (smp[through, 3] == 1).all() and (smp[:, 7] == 0).all()
    assert (smp[:, 6] > 2).any()


# ---- 3 / 4. eval and sample against the restatement -------------------------------------------
@pytest.fixture(scope='module')
def base(oracle):
    """The oracle's view of the shared geometry (sample positions, first vertices), the
    samples' BSDF draw at the first vertex, and the restatements computed so far.  The draw is
    Sobol dimensions 5 and 6: the film position took 0, 1, the emitter sample 2, 3, and a 2D
    draw at dimension 4 moves past the sampler's (empty) array range [5, 5) first
    (SobolSampler::next2D, sobol.cpp:233-235: m_dimension + 1 >= m_arrayStartDim)."""
    sc, twin = cr.point_scene(BSDF('diffuse'), 2, SIZE, SPP)
    _, smp, _ = oracle.render(twin, _integrator('path', 2), samples=True, libm_mode=0)
    H = dr.first_hits(sc, twin, oracle, smp[:, 4], smp[:, 5])
    return dict(smp=smp, H=H, u45=cr.sobol_2d(oracle, SIZE, SPP, 5), cache={})


def _checker_split(b, uv):
    """Samples on each colour of the case's checkerboard (None: the case has none)."""
    from mitsuba_amd.scene import Checkerboard
    import fields_ref as fr
    tex = b.weight if b.type == 'blendbsdf' else b.opacity if b.type == 'mask' else None
    if not isinstance(tex, Checkerboard):
        return None
    ok = ~np.isnan(uv[:, 0])
    is0 = fr.checker_is_color0(tex, uv[ok, 0], uv[ok, 1])
    return int(is0.sum()), int((~is0).sum())


EVAL = [(c, k, e) for c in cr.cases() for k, e in _kinds_engines(('path', 'volpath', 'direct'))]


@pytest.mark.parametrize('case,kind,engine', EVAL, ids=['-'.join(f) for f in EVAL])
def test_eval_first_bounce(gpu_ctx, oracle, monkeypatch, base, case, kind, engine):
    b = cr.cases()[case]
    strict = case in cr.STRICT_CASES
    sc, twin = cr.point_scene(b, 2, SIZE, SPP)
    key = ('eval', case, kind)
    if key not in base['cache']:
        base['cache'][key] = cr.nee(sc, twin, oracle, base['H'], kind, strict)
    want, info = base['cache'][key]
    assert info['lit'].sum() > 200 and (info['use'] & ~info['lit']).sum() > 20, (info['lit'].sum(), info['use'].sum())
    split = _checker_split(b, base['H']['uv'])
    assert split is None or min(split) > 50, split
    _, smp, _ = _render(gpu_ctx, monkeypatch, sc, _integrator(kind, 2, strict), engine)
    _assert_li(smp, want, (case, kind, engine))
    assert np.array_equal(_bits(smp[:, 3:6]), _bits(base['smp'][:, 3:6]))


SAMPLE = [(c, k, e) for c in cr.cases() for k, e in _kinds_engines(('path', 'volpath'))]


def _shares(b, choices):
    """Per level of the chain, the share of the samples that took each branch."""
    out = {}
    for ch in choices:
        if ch:
            for lvl, c in enumerate(ch):
                out.setdefault(lvl, {}).setdefault(c, 0)
                out[lvl][c] += 1
    return out


@pytest.mark.parametrize('case,kind,engine', SAMPLE, ids=['-'.join(f) for f in SAMPLE])
def test_sample_two_vertices(gpu_ctx, oracle, monkeypatch, base, case, kind, engine):
    """Li = NEE_1 + thr * NEE_2 at maxDepth 3 (no ray can hit a point light): the BSDF sample at
    the first vertex restated from the sample's Sobol dimensions 5 and 6, sampleReuse or the
    blend's / mask's rescaling, oracle_bsdf_sample on the chosen leaf and oracle_bsdf_eval on
    its siblings; the second vertex from oracle_intersect."""
    b = cr.cases()[case]
    strict = case in cr.STRICT_CASES
    sc, twin = cr.point_scene(b, 3, SIZE, SPP)
    key = ('sample', case, kind)
    if key not in base['cache']:
        base['cache'][key] = cr.two_vertices(sc, twin, oracle, base['H'], base['u45'], kind, strict)
    want, info = base['cache'][key]
    shares = _shares(b, info['choices'])
    # every branch of every level of the chain: both of a mask, every child of a mixture or blend
    want_branches, lvl_b = [], b
    while lvl_b.type in ('mask', 'twosided', 'mixturebsdf', 'blendbsdf'):
        if lvl_b.type != 'twosided':
            want_branches.append(2 if lvl_b.type == 'mask' else len(lvl_b.nested))
        if lvl_b.type in ('mixturebsdf', 'blendbsdf'):
            break
        lvl_b = lvl_b.nested[0]
    assert len(want_branches) >= 1 and sorted(shares) == list(range(len(want_branches))), (case, shares)
    for lvl, counts in shares.items():
        total = sum(counts.values())
        assert len(counts) == want_branches[lvl] and min(counts.values()) >= 0.05 * total, (case, lvl, counts)
    assert np.any(info['c2'] != 0, 1).sum() >= 100, np.any(info['c2'] != 0, 1).sum()
    _, smp, _ = _render(gpu_ctx, monkeypatch, sc, _integrator(kind, 3, strict), engine)
    _assert_li(smp, want, (case, kind, engine))


# ---- 5. the engines agree at full depth -------------------------------------------------------
def _agree_scene(width=SIZE, height=SIZE, spp=SPP):
    sc, _, _ = dr.delta_scene([Emitter('constant', radiance=(0.4, 0.5, 0.7))], keep_area=True, materials='smooth',
                              width=width, height=height, spp=spp, max_depth=-1)
    C = cr.cases()
    sc.meshes = [copy.copy(m) for m in sc.meshes]
    sc.bsdfs = [C['mask_twosided_blend'], C['mix3']]
    for i, m in enumerate(sc.meshes):
        if m.bsdf >= 0:
            m.bsdf = 0 if i < 5 else 1      # the room's five quads; the two boxes (and the light quad)
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
    # the kd-tree flag (the wavefront engine's other traversal; the scene is triangles only)
    gpu_ctx.upload(sc)
    film, smp, _ = gpu_ctx.render(it, samples=True, engine='kdtree')
    assert gpu_ctx.debug_counters()[15] & VARIANT_COMBO
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


# ---- 6. energy under the area light ------------------------------------------------------------
_energy_oracle = {}


@pytest.mark.parametrize('kind', ['blend', 'mixture'])
def test_energy_under_area_light(gpu_ctx, oracle, monkeypatch, kind):
    """blendbsdf(0.5, A, A) and mixturebsdf("0.25, 0.75", A, A) in place of every BSDF A of the
    diffuse C1, full depth, 32 x 32: the per-channel image means against the oracle's render of
    plain A under another scramble, within 4 standard errors of the difference (delta_ref.image_mean,
    z_score; the bound of the delta-emitter energy test: a margin over sampling noise).  This is
    the combinators' pdf() inside NEE's MIS under an area light, which nothing else restates.
    896 spp: the smallest multiple of 4 at which, with the oracle alone, A against A under two
    scrambles gives z = 0.125 / 0.131 / 0.113 (<= 2) and A against A with its reflectance scaled
    by 1.05 z = 13.43 / 10.43 / 6.05 (>= 6) (tests/test_combo_host.py::test_energy_calibration).
    Measured on the MI355X: blend z = 0.10 / 0.18 / 0.10, mixture z = 0.10 / 0.10 / 0.12."""
    spp = cr.ENERGY_SPP
    sc, it = cr.energy_wrapped(kind, spp)
    _, smp, _ = _render(gpu_ctx, monkeypatch, sc, it, 'lds')
    if 'plain' not in _energy_oracle:
        psc, pit = cr.energy_plain(spp, cr.ENERGY_SCRAMBLE)
        _energy_oracle['plain'] = oracle.render(psc, pit, samples=True, libm_mode=0)[1]
    keep = np.ones(SIZE * SIZE, bool)
    g, o = dr.image_mean(smp, keep, spp), dr.image_mean(_energy_oracle['plain'], keep, spp)
    z = dr.z_score(g, o)
    print(kind, 'means', g[0], o[0], 'z', z, 'z at a 5% error', dr.z_score(g, o, 1.05))
    assert (z <= 4).all(), (kind, z, g, o)


# ---- fields ----------------------------------------------------------------------------------
def test_fields_over_combinators(gpu_ctx, monkeypatch):
    sc, it = _agree_scene()
    film, _, _ = _render(gpu_ctx, monkeypatch, sc, it, 'lds', samples=False)
    mc = MultiChannelIntegrator(children=[it, FieldIntegrator('distance')], sampleCount=SPP, rfilter='box')
    gpu_ctx.upload(sc)
    films, _, _ = gpu_ctx.render(mc)
    assert np.array_equal(_bits(films[0][..., 0:3]), _bits(film[..., 0:3]))
    # the geometry's distances: the same scene with plain diffuse surfaces
    plain = cr.all_surfaces(copy.copy(sc), BSDF('diffuse'))
    gpu_ctx.upload(plain)
    want, _, _ = gpu_ctx.render(MultiChannelIntegrator(children=[FieldIntegrator('distance')], sampleCount=SPP,
                                                        rfilter='box'))
    assert np.array_equal(_bits(films[1]), _bits(want[0])) and films[1][..., 0].max() > 0
    gpu_ctx.upload(sc)
    with pytest.raises((NotImplementedError, MtsgpuError), match='albedo'):
        gpu_ctx.render(MultiChannelIntegrator(children=[FieldIntegrator('albedo')], sampleCount=SPP, rfilter='box'))
