"""Film reconstruction at every gather width and on the atomic fallback.

Every other GPU test with a gaussian uses stddev 0.5 (H = 2, film_gather<2>).  Here:

a. film_gather<1>, <3> and <4> (stddev 0.2, 0.8, 1.0): two rows per thread with other LDS
   shapes, and the one-row code with the 40-pixel block bitmap.  Records, film and counters
   equal the oracle's bit for bit, and the film equals the numpy restatement of the gather
   order (tests/test_film_gather.py gather_ref) -- which differs from the other order in most
   pixels (tests/test_film_spill.py), so equality shows which kernel ran.
b. MTSGPU_NO_GATHER takes the same filter through the fallback.
c. The fallback (dfilm.h film_splat's double atomics + film_finalize): gaussians with H = 0,
   5, 6 and boxes of radius 0.3 and 1.5, against tests/film_ref.py spill_film_ref of the
   oracle's records.  Film values whose spill sum is certified exact are compared bit for
   bit; the others within 3 * 2^-23 of the larger value: the two double totals round to
   float32 values at most one ulp of the spill sum apart (2^-23 * sum|c|), the last float32
   add rounds each side by half an ulp of the result, together 2^-22 (1 + 2^-23) of the
   larger value for the non-negative path films.
d. The field pass: every field's own film, gathered and through its own spill film
   (signed values: the bound is 2^-22 (|own| + sum|c|) (1 + 2^-23)).

Base shape: C1 at 40 x 36, spp 3: two 32-pixel blocks each way, a partial 8x8 tile row,
3 x 2 gather workgroups at H = 3 and 3 x 3 at H = 4, partial ones included.
"""
import os

import numpy as np
import pytest

import fields_ref as fr
from film_ref import Rendered, spill_film_ref
from mitsuba_amd import scenes
from mitsuba_amd.scene import FieldIntegrator
from test_film_gather import gather_ref
from test_gpu_hoisted import SHARD_IDS, SHARDS
from test_gpu_spp_chunks import BUDGET, ENV, chunk_plan

pytestmark = pytest.mark.gpu

W, H, SPP = 40, 36, 3
FULL = (0, 0, W, H)
EDGE_CROP = (0, 5, 37, 29)      # the film's left edge (the gx0 clip), across x = 32
INNER_CROP = (6, 3, 27, 22)     # interior, off the tile grid
SPARSE = ((8, 13, 4), True)     # tiles 4 and 17 of 25
THREADS = min(16, os.cpu_count() or 1)
COUNTERS = ('samples', 'rays', 'shadow_rays', 'path_length_sum')
GATHER_H = {0.2: 1, 0.8: 3, 1.0: 4}
UNDEF = (-3.0, 0.25, 7.5)
FIELDS = ['shNormal', 'distance', 'position']      # (the normal and the position are signed)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _scene(rfilter, param, crop=None, size=(W, H), spp=SPP, materials='diffuse'):
    sc, it = scenes.build('C1', width=size[0], height=size[1], spp=spp, rfilter=rfilter, materials=materials)
    it.rfilterParam = param
    it.crop = crop
    return sc, it


_REF = {}


def _cached(key, make):
    """A case's reference, made once per session and shared read-only."""
    if key not in _REF:
        _REF[key] = make()
        for a in _REF[key] if isinstance(_REF[key], tuple) else (_REF[key],):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _REF[key]


def _oracle(oracle, sc, it, key, row=(0, 1, 0), tile_shard=False):
    return _cached(('oracle',) + key + (row, tile_shard),
                   lambda: oracle.render(sc, it, samples=True, libm_mode=0, threads=THREADS, row=row, tile_shard=tile_shard))


def _records_equal(a, b, what):
    same = np.all(_bits(a) == _bits(b), axis=1)
    bad = np.nonzero(~same)[0]
    assert same.all(), '%s: %d of %d records differ, first %d: %s vs %s' % (
        what, bad.size, same.size, bad[0], a[bad[0]].tolist(), b[bad[0]].tolist())


def _films_equal(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.argwhere(np.any(_bits(a) != _bits(b), axis=-1))
    assert bad.size == 0, '%s: %d film pixels differ, first %s: %s vs %s' % (
        what, len(bad), bad[:3].tolist(), a[tuple(bad[0])].tolist(), b[tuple(bad[0])].tolist())


def _counters_equal(a, b, what):
    for k in COUNTERS:
        assert a[k] == b[k], (what, k, a[k], b[k])


# ---- a. the gather widths ------------------------------------------------------------------
def _gather_case(gpu_ctx, oracle, param, instr, crop=None, row=(0, 1, 0), tile_shard=False, engine=None,
                 materials='diffuse'):
    """One render at gaussian stddev `param` against the oracle and the numpy gather order."""
    sc, it = _scene('gaussian', param, crop, materials=materials)
    win = crop or FULL
    key = ('gaussian', param, crop, materials)
    film_o, smp_o, st_o = _oracle(oracle, sc, it, key, row, tile_shard)
    shard = Rendered(row, tile_shard)
    ref = _cached(('gather',) + key + (row, tile_shard),
                  lambda: gather_ref(smp_o, SPP, win, W, H, 'gaussian', param, oracle, shard=shard))
    gpu_ctx.upload(sc)
    film, smp, st = gpu_ctx.render(it, samples=instr, row=row, tile_shard=tile_shard, engine=engine)
    what = 'gaussian %g %s' % (param, (crop, row, tile_shard, engine))
    if instr:
        _records_equal(smp, smp_o, what)
    _films_equal(film, film_o, what + ': vs oracle')
    _films_equal(film, ref, what + ': vs the numpy gather order')
    _counters_equal(st, st_o, what)
    b = (film.shape[0] - H) // 2
    assert b == GATHER_H[param]
    return film, shard.pixels(win[2], win[3]), b


@pytest.mark.parametrize('instr', [True, False], ids=['instr', 'plain'])
@pytest.mark.parametrize('crop', [None, EDGE_CROP, INNER_CROP], ids=['full', 'edge_crop', 'inner_crop'])
@pytest.mark.parametrize('param', sorted(GATHER_H))
def test_gather_width_windows(gpu_ctx, oracle, param, crop, instr):
    film, _, b = _gather_case(gpu_ctx, oracle, param, instr, crop=crop)
    x0, y0, w, h = crop or FULL
    reach = np.zeros(film.shape[:2], bool)
    reach[max(0, y0):y0 + h + 2 * b, max(0, x0):x0 + w + 2 * b] = True
    assert not film[~reach].any() and np.count_nonzero(film[..., 4]) > w * h
    v = gpu_ctx.kernel_variant()
    assert v is not None and v['scene_lds'] and v['instr'] == instr, v


@pytest.mark.parametrize('instr', [True, False], ids=['instr', 'plain'])
@pytest.mark.parametrize('row,tile_shard', SHARDS, ids=SHARD_IDS)
@pytest.mark.parametrize('param', sorted(GATHER_H))
def test_gather_width_shards(gpu_ctx, oracle, param, row, tile_shard, instr):
    film, _, _ = _gather_case(gpu_ctx, oracle, param, instr, row=row, tile_shard=tile_shard)
    assert np.count_nonzero(film[..., 4])


@pytest.mark.parametrize('instr', [True, False], ids=['instr', 'plain'])
@pytest.mark.parametrize('param', sorted(GATHER_H))
def test_gather_width_sparse_tiles(gpu_ctx, oracle, param, instr):
    """Two of the 25 tiles are rendered: most gather workgroups find no rendered source and
    leave before their first barrier; the film stays zero beyond the two tiles' reach."""
    film, rendered, b = _gather_case(gpu_ctx, oracle, param, instr, row=SPARSE[0], tile_shard=SPARSE[1])
    assert rendered.sum() == 2 * 64                     # tiles 4 (the last column) and 17
    reach = np.zeros(film.shape[:2], bool)
    for y, x in np.argwhere(rendered):
        reach[y:y + 2 * b + 1, x:x + 2 * b + 1] = True
    assert not film[~reach].any() and np.count_nonzero(film[..., 4]) > rendered.sum()


@pytest.mark.parametrize('instr', [True, False], ids=['instr', 'plain'])
@pytest.mark.parametrize('param', [0.8, 1.0])
def test_gather_width_scene_in_hbm(gpu_ctx, oracle, monkeypatch, param, instr):
    monkeypatch.setenv('MTSGPU_NO_SCENE_LDS', '1')
    _gather_case(gpu_ctx, oracle, param, instr)
    v = gpu_ctx.kernel_variant()
    assert v is not None and not v['scene_lds'] and v['instr'] == instr, v


@pytest.mark.parametrize('param', [0.8, 1.0])
def test_gather_width_wavefront(gpu_ctx, oracle, param):
    _gather_case(gpu_ctx, oracle, param, True, engine='wavefront', materials='rough')
    assert gpu_ctx.kernel_variant() is None and gpu_ctx.debug_counters()[15] == 1 << 16


@pytest.mark.parametrize('param', [0.8, 1.0])
def test_gather_width_running_sums_between_launches(gpu_ctx, oracle, monkeypatch, param):
    """96 x 80 at spp 9 under the smallest record budget: launches of 4 + 4 + 1 samples, the
    later ones continuing the sums film_gather<H> left in the film."""
    size, spp = (96, 80), 9
    assert chunk_plan(size, spp, True) == (4, 3, 7680)
    sc, it = _scene('gaussian', param, size=size, spp=spp)
    film_o, smp_o, st_o = _oracle(oracle, sc, it, ('gaussian', param, size, spp))
    gpu_ctx.upload(sc)
    monkeypatch.setenv(ENV, str(BUDGET))
    film_c, smp_c, st_c = gpu_ctx.render(it, samples=True)
    assert gpu_ctx.launch_chunks() == 3
    monkeypatch.delenv(ENV)
    film_1, _, st_1 = gpu_ctx.render(it)
    assert gpu_ctx.launch_chunks() == 1
    _records_equal(smp_c, smp_o, 'chunked vs oracle')
    _films_equal(film_c, film_o, 'chunked vs oracle')
    _films_equal(film_c, film_1, 'chunked vs one launch')
    _counters_equal(st_c, st_o, 'chunked vs oracle')
    _counters_equal(st_c, st_1, 'chunked vs one launch')


# ---- c. the rule of the fallback ------------------------------------------------------------
def _check_spill_rule(film, ref, what):
    """Certified values bit for bit, every other one within 3 * 2^-23 of the larger value
    (non-negative films).  Returns the number of values that differ at all."""
    mine = ref.film()
    assert film.shape == mine.shape, (what, film.shape, mine.shape)
    differ = _bits(film) != _bits(mine)
    bad = np.argwhere(differ & ref.certified)
    assert bad.size == 0, '%s: %d certified film values differ, first %s: %r vs %r' % (
        what, len(bad), bad[:3].tolist(), film[tuple(bad[0])], mine[tuple(bad[0])])
    assert (film >= 0).all() and (mine >= 0).all()
    g, r = film.astype(np.float64), mine.astype(np.float64)
    over = np.argwhere(np.abs(g - r) > 3.0 * 2.0 ** -23 * np.maximum(g, r))
    assert over.size == 0, '%s: %d film values beyond the bound, first %s: %r vs %r' % (
        what, len(over), over[:3].tolist(), film[tuple(over[0])], mine[tuple(over[0])])
    n = int(differ.sum())
    print('%s: %d of %d film values differ from the exact-sum film (%d uncertified)' % (
        what, n, differ.size, int((~ref.certified).sum())))
    return n


def _fallback_case(gpu_ctx, oracle, rfilter, param, spp, crop, instr):
    sc, it = _scene(rfilter, param, crop, spp=spp)
    key = (rfilter, param, crop, spp)
    film_o, smp_o, st_o = _oracle(oracle, sc, it, key)
    ref = _cached(('spill',) + key, lambda: spill_film_ref(smp_o, spp, crop or FULL, W, H, rfilter, param, oracle))
    gpu_ctx.upload(sc)
    film, smp, st = gpu_ctx.render(it, samples=instr)
    what = '%s %g %s' % (rfilter, param, 'crop' if crop else 'full')
    if instr:
        _records_equal(smp, smp_o, what)
    _counters_equal(st, st_o, what)
    _check_spill_rule(film, ref, what)
    return film, film_o, ref


# ---- b. the switch -------------------------------------------------------------------------
def test_no_gather_switch(gpu_ctx, oracle, monkeypatch):
    """stddev 0.8 is gathered (above); with MTSGPU_NO_GATHER the same records go through
    film_splat, and the film is the other order's: it differs from the gathered film."""
    monkeypatch.setenv('MTSGPU_NO_GATHER', '1')
    film, film_gathered, ref = _fallback_case(gpu_ctx, oracle, 'gaussian', 0.8, SPP, None, True)
    assert np.count_nonzero(_bits(film) != _bits(film_gathered)) >= 1
    assert np.allclose(film, film_gathered, rtol=1e-5, atol=0)
    monkeypatch.delenv('MTSGPU_NO_GATHER')
    again, _, _ = gpu_ctx.render(_scene('gaussian', 0.8)[1])
    _films_equal(again, film_gathered, 'gathered again with the variable unset')


# ---- c. the fallback -----------------------------------------------------------------------
FALLBACK = [('gaussian', 0.1, 3), ('gaussian', 1.13, 3), ('gaussian', 1.5, 2), ('box', 0.3, 3), ('box', 1.5, 3)]


@pytest.mark.parametrize('instr', [True, False], ids=['instr', 'plain'])
@pytest.mark.parametrize('crop', [None, EDGE_CROP], ids=['full', 'edge_crop'])
@pytest.mark.parametrize('rfilter,param,spp', FALLBACK, ids=['%s_%g' % c[:2] for c in FALLBACK])
def test_fallback(gpu_ctx, oracle, rfilter, param, spp, crop, instr):
    """Differing values measured on an MI355X (full frame; gaussian 1.13: 0 of 11500,
    gaussian 1.5: 0 of 12480 -- see DESIGN.md's film section); the count is printed, not asserted."""
    film, film_o, ref = _fallback_case(gpu_ctx, oracle, rfilter, param, spp, crop, instr)
    if rfilter == 'box' or param == 0.1:
        assert ref.certified.all()
        _films_equal(film, film_o, 'a wholly certified film vs oracle')
    else:
        px = ref.certified.all(axis=-1)
        assert crop is not None or 4 * px.sum() >= 3 * px.size


def test_fallback_between_launches(gpu_ctx, oracle, monkeypatch):
    """gaussian 1.13 (H = 5) at 160 x 112, spp 7, 16 B records: launches of 3 + 3 + 1 samples
    whose paired record sectors (film_slot) and spills carry on in one film."""
    size, spp, param = (160, 112), 7, 1.13
    assert chunk_plan(size, spp, False) == (3, 3, 17920)
    sc, it = _scene('gaussian', param, size=size, spp=spp)
    film_o, smp_o, st_o = _oracle(oracle, sc, it, ('gaussian', param, size, spp))
    gpu_ctx.upload(sc)
    monkeypatch.setenv(ENV, str(BUDGET))
    film_c, smp_c, st_c = gpu_ctx.render(it, samples=True)
    assert gpu_ctx.launch_chunks() == 3
    monkeypatch.delenv(ENV)
    film_1, smp_1, st_1 = gpu_ctx.render(it, samples=True)
    assert gpu_ctx.launch_chunks() == 1
    _records_equal(smp_c, smp_o, 'chunked vs oracle')
    _records_equal(smp_c, smp_1, 'chunked vs one launch')
    _counters_equal(st_c, st_o, 'chunked vs oracle')
    _counters_equal(st_c, st_1, 'chunked vs one launch')
    assert (film_c >= 0).all() and (film_1 >= 0).all() and (film_o >= 0).all()
    c = film_c.astype(np.float64)
    for other, what in ((film_1, 'one launch'), (film_o, 'oracle')):
        o = other.astype(np.float64)
        over = np.argwhere(np.abs(c - o) > 3.0 * 2.0 ** -23 * np.maximum(c, o))
        print('chunked vs %s: %d of %d film values differ' % (what, int((_bits(film_c) != _bits(other)).sum()), c.size))
        assert over.size == 0, (what, len(over), over[:3].tolist(), film_c[tuple(over[0])], other[tuple(over[0])])


# ---- d. the field pass ---------------------------------------------------------------------
def _field_render(gpu_ctx, rfilter, param):
    sc, it = _scene(rfilter, param)
    it.hasAlpha = True
    gpu_ctx.upload(sc)
    films, rec, st = gpu_ctx.render_fields(it, [FieldIntegrator(n, undefined=UNDEF) for n in FIELDS], samples=True)
    assert gpu_ctx.debug_counters()[15] == (1 << 17) | (1 << 12)
    assert st['samples'] == W * H * SPP and films.shape[0] == len(FIELDS)
    assert (rec[:, 4:7] < 0).any()                       # the normal field is signed
    return films, rec


@pytest.mark.parametrize('param', [0.8, 1.0])
def test_field_pass_gather_widths(gpu_ctx, oracle, param):
    films, rec = _field_render(gpu_ctx, 'gaussian', param)
    for f in range(len(FIELDS)):
        _films_equal(films[f], fr.gather_film_ref(rec, f, SPP, FULL, W, H, 'gaussian', param, oracle),
                     'field %s at gaussian %g vs the gather order' % (FIELDS[f], param))


@pytest.mark.parametrize('rfilter,param', [('box', 1.0), ('gaussian', 1.13)], ids=['box_1', 'gaussian_1.13'])
def test_field_pass_spill_films(gpu_ctx, oracle, rfilter, param):
    """Every sample splats into its neighbours, so every field's own spill film
    (FA.spill[f]) takes real traffic; a field's film holds no other field's values."""
    films, rec = _field_render(gpu_ctx, rfilter, param)
    refs = [spill_film_ref(rec, SPP, FULL, W, H, rfilter, param, oracle, field=f) for f in range(len(FIELDS))]
    for f, ref in enumerate(refs):
        what = 'field %s at %s %g' % (FIELDS[f], rfilter, param)
        mine = ref.film()
        differ = _bits(films[f]) != _bits(mine)
        bad = np.argwhere(differ & ref.certified)
        assert bad.size == 0, '%s: %d certified film values differ, first %s: %r vs %r' % (
            what, len(bad), bad[:3].tolist(), films[f][tuple(bad[0])], mine[tuple(bad[0])])
        lim = 2.0 ** -22 * (np.abs(ref.own.astype(np.float64)) + ref.sumabs) * (1.0 + 2.0 ** -23)
        over = np.argwhere(np.abs(films[f].astype(np.float64) - mine.astype(np.float64)) > lim)
        assert over.size == 0, '%s: %d film values beyond the bound, first %s: %r vs %r' % (
            what, len(over), over[:3].tolist(), films[f][tuple(over[0])], mine[tuple(over[0])])
        print('%s: %d of %d film values differ from the exact-sum film (%d uncertified)' % (
            what, int(differ.sum()), differ.size, int((~ref.certified).sum())))
        # real traffic: a box 1.0 sample covers 2 x 2 pixels (3 spills, so an interior pixel takes
        # 3 spp on average), a gaussian 1.13 sample 11 x 11
        assert ref.count[..., 4].max() >= (3 if rfilter == 'box' else 60) * SPP
        if rfilter == 'box':
            assert ref.certified[..., 3:].all()
        for g, other in enumerate(refs):
            if g != f:
                lim_g = 2.0 ** -22 * (np.abs(other.own.astype(np.float64)) + other.sumabs) * (1.0 + 2.0 ** -23)
                off = np.abs(films[f][..., :3].astype(np.float64) - other.film()[..., :3]) > lim_g[..., :3]
                assert off.sum() > W * H, (what, FIELDS[g], int(off.sum()))
