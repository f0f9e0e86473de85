"""The field / multichannel integrators on the GPU (field_kernel.hip, mtsgpu_render_fields,
mtsgpu_develop_multi) against the CPU oracle's hit records and numpy restatements of the
film order.  Every comparison is on uint32 views (bit for bit)."""
import numpy as np
import pytest

import fields_ref as fr
from mitsuba_amd import abi, scenes
from mitsuba_amd.film import HDRFilm
from mitsuba_amd.integrator import MtsgpuError, albedo_factors_host
from mitsuba_amd.scene import (Checkerboard, FieldIntegrator, Mesh, MultiChannelIntegrator, PathIntegrator,
                               film_border, lookup_ior)

pytestmark = pytest.mark.gpu
f32 = np.float32
UNDEF = (-3.0, 0.25, 7.5)                 # a non-zero 'undefined': misses must carry it
NO_TRIANGLE = f32(4294967295.0)           # (float) KNoTriangleFlag


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def assert_bits(a, b, what=''):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.argwhere(bits(a) != bits(b))
    assert bad.size == 0, (what, len(bad), bad[:3].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


def fields_of(names):
    return [FieldIntegrator(n, undefined=UNDEF) for n in names]


def column(rec, k):
    return rec[:, 4 + 3 * k:7 + 3 * k]


# ---- 1. per-sample fields against the oracle's hit record ------------------------------
@pytest.mark.parametrize('materials', ['diffuse', 'shapes'])
def test_fields_equal_oracle_hit_record(gpu_ctx, oracle, materials):
    """Cornell C1 (the tiny-scene scan) and the analytic-shape box (LDS BVH; sphere, disk,
    rectangle): samplePos and alpha equal the oracle path render's records, and every
    field equals oracle_intersect of the helper's ray; misses carry `undefined`."""
    sc, it = scenes.build('C1', width=32, height=32, spp=4, materials=materials)
    it.hasAlpha = True
    names = ['position', 'distance', 'geoNormal', 'shNormal', 'shapeIndex', 'primIndex']
    gpu_ctx.upload(sc)
    films, rec, st = gpu_ctx.render_fields(it, fields_of(names), samples=True)
    assert st['samples'] == 32 * 32 * 4 == st['rays'] and films.shape[0] == 6
    assert gpu_ctx.debug_counters()[15] == (1 << 17) | (1 << 12)        # field_kernel, scene in LDS
    _, smp, _ = oracle.render(sc, it, samples=True)
    assert_bits(rec[:, 0:2], smp[:, 4:6], 'samplePos')
    assert_bits(rec[:, 2], smp[:, 3], 'alpha')
    o, d, _, _ = fr.primary_rays(sc, oracle, rec[:, 0], rec[:, 1])
    its = fr.oracle_intersect(sc, oracle, o, d)
    hit = its[:, 0] == 1.0
    assert_bits(rec[:, 3], hit.astype(f32), 'hit')
    assert 0 < hit.sum() < hit.size
    analytic = np.array([m.analytic for m in sc.meshes])[its[:, 14].astype(np.int64)]
    t3 = np.repeat(its[:, 1:2], 3, 1)
    prim = np.where(analytic, NO_TRIANGLE, its[:, 15]).astype(f32)
    want = {'position': its[:, 2:5], 'distance': t3, 'geoNormal': its[:, 5:8], 'shNormal': its[:, 8:11],
            'shapeIndex': np.repeat(its[:, 14:15], 3, 1), 'primIndex': np.repeat(prim[:, None], 3, 1)}
    for k, n in enumerate(names):
        exp = np.where(hit[:, None], want[n], np.asarray(UNDEF, f32)[None, :])
        assert_bits(column(rec, k), exp, n)
    if materials == 'shapes':
        assert analytic[hit].any() and (~analytic[hit]).any()


# ---- 2. a scene on the HBM BVH path ----------------------------------------------------
def test_fields_on_hbm_bvh_band(gpu_ctx, oracle):
    """A row band of C3 (the ~69k-triangle object, here with texture coordinates, on the HBM
    BVH): distance, primIndex and shapeIndex equal batch oracle_trace_rays; uv equals the
    barycentric restatement of skdtree.h's interpolation from the oracle's (u, v, prim)."""
    p, i, tc = scenes.blob_mesh(236, 148, uv=True)
    sc, it = scenes.build('C3', width=64, height=36, spp=4, env_size=(128, 64),
                          object_mesh=Mesh(p, i, texcoords=tc, name='object'))
    window = (0, 16, 64, 4)
    gpu_ctx.upload(sc)
    names = ['distance', 'primIndex', 'shapeIndex', 'uv']
    _, rec, st = gpu_ctx.render_fields(it, fields_of(names), window=window, samples=True)
    assert st['samples'] == 64 * 4 * 4
    assert gpu_ctx.debug_counters()[15] == 1 << 17                      # field_kernel, scene in HBM
    o, d, mint, maxt = fr.primary_rays(sc, oracle, rec[:, 0], rec[:, 1])
    hits = oracle.trace_rays(sc, o, d, mint, maxt)
    hit = np.isfinite(hits[:, 0])
    assert_bits(rec[:, 3], hit.astype(f32), 'hit')
    shape, local = fr.prim_tables(sc)
    prim = np.minimum(hits[:, 3].view(np.uint32).astype(np.int64), len(shape) - 1)
    uv = fr.hit_uv(sc, hits)
    want = [np.repeat(hits[:, 0:1], 3, 1), np.repeat(local[prim].astype(f32)[:, None], 3, 1),
            np.repeat(shape[prim].astype(f32)[:, None], 3, 1), np.concatenate([uv, np.zeros_like(uv[:, :1])], 1)]
    for k, n in enumerate(names):
        exp = np.where(hit[:, None], want[k], np.asarray(UNDEF, f32)[None, :])
        assert_bits(column(rec, k), exp, n)
    assert (shape[prim][hit] == 0).any() and (shape[prim][hit] > 0).any()   # the object and the ground


# ---- 3. albedo -------------------------------------------------------------------------
def _refl(v, uv):
    """A constant or checkerboard spectrum at uv (n, 3)."""
    if isinstance(v, Checkerboard):
        c0 = fr.checker_is_color0(v, uv[:, 0], uv[:, 1])
        return np.where(c0[:, None], fr._spec3(v.color0)[None, :], fr._spec3(v.color1)[None, :]).astype(f32)
    return np.repeat(fr._spec3(v)[None, :], uv.shape[0], 0)


def _albedo(sc, b, flat_index, uv, front, factors, oracle):
    """getDiffuseReflectance of BSDF `b` per sample; NaN rows: not checked here."""
    n = uv.shape[0]
    if b.type == 'diffuse':
        return _refl(b.reflectance, uv)
    if b.type == 'plastic':           # diffuseReflectance * (1 - fdrExt) (plastic.cpp:219-221)
        eta = f32(f32(lookup_ior(b.int_ior())) / f32(lookup_ior(b.extIOR)))
        k = f32(1) - f32(oracle.lib().oracle_fresnel_diffuse_reflectance(eta))
        return (_refl(b.diffuseReflectance, uv) * k).astype(f32)
    if b.type == 'roughplastic':
        if isinstance(b.alpha, Checkerboard):
            return np.full((n, 3), np.nan, f32)      # textured alpha: evaluated per hit, not pinned here
        # a self-consistency check: the factor is the host's own mtsg_rtrans_eval_diffuse value
        # (mtsgpu_albedo_factors_host), not an independent restatement of the table lookup
        return (_refl(b.diffuseReflectance, uv) * f32(factors[flat_index])).astype(f32)
    if b.type == 'twosided':          # dispatches on its.wi.z > 0 (twosided.cpp:198-203)
        flat, nested = sc.flat_bsdfs()
        idx = nested[flat_index]
        fi, bi = idx[0], idx[-1]
        a = _albedo(sc, flat[fi], fi, uv, front, factors, oracle)
        c = _albedo(sc, flat[bi], bi, uv, front, factors, oracle)
        return np.where(front[:, None], a, c)
    return np.zeros((n, 3), f32)      # conductors and dielectrics reject EDiffuseReflection (bsdf.cpp:82-86)


@pytest.mark.parametrize('materials', ['plastic', 'smooth'])
def test_albedo(gpu_ctx, oracle, materials):
    """The checkerboard C1 variant (textured diffuse, roughplastic) and the smooth-BSDF box
    (plastic, conductor, dielectric, twosided with one and with two nested BSDFs)."""
    sc, it = scenes.build('C1', width=32, height=32, spp=4, materials=materials)
    gpu_ctx.upload(sc)
    _, rec, _ = gpu_ctx.render_fields(it, fields_of(['albedo', 'uv']), samples=True)
    o, d, mint, maxt = fr.primary_rays(sc, oracle, rec[:, 0], rec[:, 1])
    hits = oracle.trace_rays(sc, o, d, mint, maxt)
    hit = np.isfinite(hits[:, 0])
    assert_bits(rec[:, 3], hit.astype(f32), 'hit')
    uv = fr.hit_uv(sc, hits)
    assert_bits(column(rec, 1)[hit, :2], uv[hit], 'uv')
    shape, _ = fr.prim_tables(sc)
    mesh = shape[np.minimum(hits[:, 3].view(np.uint32).astype(np.int64), len(shape) - 1)]
    # wi.z = dot(-d, shFrame.n) (Frame::toLocal), for the samples on a twosided BSDF: the
    # shading normal is the oracle's hit record's (one oracle_intersect per such sample)
    two_sided = np.array([m.bsdf >= 0 and sc.bsdfs[m.bsdf].type == 'twosided' for m in sc.meshes])
    ts = np.nonzero(hit & two_sided[mesh])[0]
    front = np.zeros(hit.size, bool)
    if ts.size:
        n = fr.oracle_intersect(sc, oracle, o[ts], d[ts])[:, 8:11]
        dd = d[ts]
        front[ts] = (((-dd[:, 0] * n[:, 0]).astype(f32) + (-dd[:, 1] * n[:, 1]).astype(f32)).astype(f32)
                     + (-dd[:, 2] * n[:, 2]).astype(f32)).astype(f32) > 0
    factors = albedo_factors_host(sc)
    exp = np.repeat(np.asarray(UNDEF, f32)[None, :], hit.size, 0)
    seen = set()
    for mi, m in enumerate(sc.meshes):
        sel = hit & (mesh == mi)
        if not sel.any():
            continue
        if m.bsdf < 0:                 # Shape::configure's default diffuse: black on an emitter (shape.cpp:48-70)
            exp[sel] = 0.0 if m.emitter >= 0 else 0.5
            continue
        b = sc.bsdfs[m.bsdf]
        seen.add(b.type)
        exp[sel] = _albedo(sc, b, m.bsdf, uv[sel], front[sel], factors, oracle)
    check = ~np.isnan(exp).any(1)
    assert_bits(column(rec, 0)[check], exp[check], 'albedo')
    if materials == 'smooth':
        assert {'plastic', 'conductor', 'twosided'} <= seen
        two = [i for i, b in enumerate(sc.bsdfs) if b.type == 'twosided' and len(b.nested) == 2]
        assert any((hit & (mesh == mi)).any() for mi, m in enumerate(sc.meshes) if m.bsdf in two)
    else:
        assert {'diffuse', 'roughplastic'} <= seen and check[hit].sum() > hit.sum() // 2


# ---- 4. relPosition --------------------------------------------------------------------
def test_rel_position(gpu_ctx, oracle):
    """A camera whose to_world is an axis permutation with sign flips and a dyadic translation
    (its inverse is exact by any method): relPosition equals the float32 affine product of
    the inverse with its.p in Transform::operator()(Point)'s order."""
    sc, it = scenes.build('C1', width=32, height=32, spp=4)
    tw = np.array([[0, 0, 1, -9.5], [0, 1, 0, 2.75], [-1, 0, 0, 2.5], [0, 0, 0, 1]], f32)   # looks along +x
    sc.sensor.toWorld = tw
    inv = np.eye(4, dtype=np.float64)
    inv[:3, :3] = tw[:3, :3].T
    inv[:3, 3] = -tw[:3, :3].T.astype(np.float64) @ tw[:3, 3].astype(np.float64)
    assert np.array_equal(inv @ tw.astype(np.float64), np.eye(4))
    gpu_ctx.upload(sc)
    _, rec, _ = gpu_ctx.render_fields(it, fields_of(['position', 'relPosition']), samples=True)
    hit = rec[:, 3] == 1.0
    assert 0 < hit.sum() < hit.size
    exp = fr.xf_point(inv.astype(f32), column(rec, 0))
    assert_bits(column(rec, 1)[hit], exp[hit], 'relPosition')
    assert_bits(column(rec, 1)[~hit], np.repeat(np.asarray(UNDEF, f32)[None], (~hit).sum(), 0), 'undefined')
    # and the position itself is the oracle's hit point for this camera
    o, d, _, _ = fr.primary_rays(sc, oracle, rec[:, 0], rec[:, 1])
    its = fr.oracle_intersect(sc, oracle, o, d)
    assert_bits(column(rec, 0)[hit], its[hit, 2:5], 'position')


# ---- 5. films --------------------------------------------------------------------------
FILM_FIELDS = ['shNormal', 'distance', 'position']


@pytest.mark.parametrize('window', [None, (5, 3, 20, 17)])
def test_box_films_equal_ordered_sum(gpu_ctx, oracle, window):
    sc, it = scenes.build('C1', width=32, height=32, spp=4)
    it.hasAlpha = True
    gpu_ctx.upload(sc)
    win = window or (0, 0, 32, 32)
    films, rec, _ = gpu_ctx.render_fields(it, fields_of(FILM_FIELDS), window=win, samples=True)
    ref = fr.box_film_ref(rec, 3, 4, win, 32, 32, oracle)
    assert_bits(films, ref, 'box films')
    assert (films[0][..., :3] < 0).any()              # negative normals are kept
    colour, _, _ = gpu_ctx.render(it, window=win)
    for f in range(3):                                # alpha and weight: the colour film's
        assert_bits(films[f][..., 3:5], colour[..., 3:5], 'alpha/weight %d' % f)
    if window is None:                                # the two tile shards sum to the whole film
        parts = [gpu_ctx.render_fields(it, fields_of(FILM_FIELDS), row=(0, 2, k), tile_shard=True)[0] for k in (0, 1)]
        assert np.count_nonzero(parts[0][0][..., 4]) and np.count_nonzero(parts[1][0][..., 4])
        assert_bits(parts[0] + parts[1], films, 'tile shards')


@pytest.mark.parametrize('window', [None, (5, 3, 20, 17)])
def test_gaussian_films_equal_gather_order(gpu_ctx, oracle, window):
    sc, it = scenes.build('C1', width=32, height=32, spp=4, rfilter='gaussian')
    it.hasAlpha = True
    gpu_ctx.upload(sc)
    win = window or (0, 0, 32, 32)
    films, rec, _ = gpu_ctx.render_fields(it, fields_of(FILM_FIELDS), window=win, samples=True)
    for f in range(3):
        ref = fr.gather_film_ref(rec, f, 4, win, 32, 32, 'gaussian', 0.5, oracle)
        assert_bits(films[f], ref, 'gather film %d' % f)
    colour, _, _ = gpu_ctx.render(it, window=win)
    for f in range(3):
        assert_bits(films[f][..., 3:5], colour[..., 3:5], 'alpha/weight %d' % f)


# ---- 6. multichannel end to end --------------------------------------------------------
@pytest.mark.parametrize('sampler', ['sobol', 'independent'])
def test_multichannel_end_to_end(gpu_ctx, oracle, sampler):
    sc, path = scenes.build('C1', width=32, height=32, spp=4)
    path.sampler = sampler
    hf = HDRFilm(pixelFormat='rgb, rgb, luminance', channelNames='color, normal, distance', componentFormat='float32')
    mc = MultiChannelIntegrator([path, FieldIntegrator('shNormal', UNDEF), FieldIntegrator('distance', UNDEF)], film=hf)
    gpu_ctx.upload(sc)
    plain, _, _ = gpu_ctx.render(path)
    films, (smp_c, rec), st = gpu_ctx.render(mc, samples=True)
    assert films.shape == (3,) + plain.shape and 'field_kernel_ms' in st
    assert_bits(films[0][..., :3], plain[..., :3], 'colour rgb')
    assert_bits(rec[:, 0:2], smp_c[:, 4:6], 'samplePos')
    assert_bits(rec[:, 2], smp_c[:, 3], 'alpha')
    ref = fr.box_film_ref(rec, 2, 4, (0, 0, 32, 32), 32, 32, oracle)
    assert_bits(films[1:], ref, 'field films')
    assert_bits(films[0][..., 3:5], films[1][..., 3:5], 'alpha/weight')
    b = film_border(mc.rfilter, mc.rfilterParam)
    films = films.copy()
    films[:, b + 3, b + 5, :] = 0.0                   # a zero-weight pixel: invWeight = 0
    for comp in ('float16', 'float32', 'uint32'):
        hf.componentFormat = comp
        img = hf.develop(gpu_ctx, films, b)
        ref = fr.develop_multi_ref(films, b, hf.pixel_formats, comp)
        assert img.dtype == ref.dtype and img.shape == (32, 32, 7)
        assert np.array_equal(img.view(np.uint16 if comp == 'float16' else np.uint32),
                              ref.view(np.uint16 if comp == 'float16' else np.uint32)), comp
    assert not img[3, 5].any()


def test_sfmt_replay_is_refused(gpu_ctx):
    sc, path = scenes.build('C1', width=32, height=32, spp=4)
    path.sampler = 'independent-sfmt'
    gpu_ctx.upload(sc)
    with pytest.raises(MtsgpuError) as e:
        gpu_ctx.render_fields(path, fields_of(['distance']))
    assert e.value.code == abi.EINVAL and 'SFMT' in str(e.value)
    path.sampler = 'sobol'
    for bad in ([], fields_of(['distance'] * 9)):
        with pytest.raises(MtsgpuError) as e:
            gpu_ctx.render_fields(path, bad)
        assert e.value.code == abi.EINVAL
    d = FieldIntegrator('distance')
    d.field = 'position'
    desc = d.to_desc()
    desc.field = 9                                    # an unknown field
    import ctypes as C
    st, p = abi.Stats(), path.params(32, 32)
    film = np.zeros((34, 34, 5), f32)
    rc = gpu_ctx.L.mtsgpu_render_fields(gpu_ctx.h, C.byref(p), C.byref(desc), 1, abi.fptr(film), None, C.byref(st))
    assert rc == abi.EINVAL


# ---- 7. existing behaviour -------------------------------------------------------------
def test_path_render_unchanged_after_field_pass(gpu_ctx):
    sc, it = scenes.build('C1', width=32, height=32, spp=4)
    gpu_ctx.upload(sc)
    before, _, _ = gpu_ctx.render(it)
    variant = gpu_ctx.kernel_variant()
    gpu_ctx.render_fields(it, fields_of(['albedo', 'primIndex']))
    assert gpu_ctx.kernel_variant() is None
    after, _, _ = gpu_ctx.render(it)
    assert gpu_ctx.kernel_variant() == variant and variant is not None
    assert_bits(after, before, 'path film')
