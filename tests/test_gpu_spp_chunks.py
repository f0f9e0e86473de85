"""Renders whose sample count is split into several launches (csrc/render_plan.cpp, capi.cpp render_impl).

plan_render sizes the per-sample record buffer against a budget and, when the
frame's samples do not fit, loops over chunks of the sample count: L.j0,
L.chunk_spp and L.num_items change per launch, the run shift is chosen per chunk,
and film_reduce / film_gather continue the running float32 sums of the launches
before.  MTSGPU_CONTRIB_BYTES = 1 MiB (the smallest budget the library takes) makes
frames of 60k-350k samples take that path; every chunked render here

* reports the launch count that `chunk_plan` restates from the code (debug
  counter 8, Context.launch_chunks), at least 3 launches;
* equals the CPU oracle, which has no notion of chunks: per-sample records where
  the instrumented kernels run, the film and the counters, on uint32 views;
* equals the same render with the variable unset (one launch): film and counters.

A record's index is pixel * spp + j, so a mismatch names the sample j and with it
the launch j // chunk it belongs to (see `_records_equal`).
"""
import ctypes as C
import os

import numpy as np
import pytest

import fields_ref as fr
from mitsuba_amd import abi, scenes
from mitsuba_amd.film import HDRFilm
from mitsuba_amd.integrator import MtsgpuError
from mitsuba_amd.scene import (DirectIntegrator, FieldIntegrator, MultiChannelIntegrator, PathIntegrator,
                               VolpathIntegrator, film_border)

pytestmark = pytest.mark.gpu

ENV = 'MTSGPU_CONTRIB_BYTES'
BUDGET = 1 << 20                          # the library raises any smaller value to this
THREADS = min(16, os.cpu_count() or 1)
COUNTERS = ('samples', 'rays', 'shadow_rays', 'path_length_sum')
UNDEF = (-3.0, 0.25, 7.5)


def _ceil_div(a, b):
    return (a + b - 1) // b


def chunk_plan(size, spp, gaussian, n_films=1, row=(0, 1, 0), tile_shard=False):
    """(chunk, launches, compact pixels) of a render of a size = (w, h) window: render_plan.cpp's
    launch_geometry and the budget arithmetic of plan_render, restated."""
    w, h = size
    block, stride = row[0] or 1, row[1] or 1
    tiles_x = _ceil_div(w, 8)
    if tile_shard:
        num_pixels = _ceil_div(tiles_x * _ceil_div(h, 8), stride) * 64
    else:
        rows_compact = _ceil_div(_ceil_div(h, block), stride) * block
        num_pixels = tiles_x * _ceil_div(rows_compact, 8) * 64
    per_sample = num_pixels * (32 if gaussian else 16)
    chunk = max(1, min(spp, BUDGET // (per_sample * n_films)))
    return chunk, _ceil_div(spp, chunk), num_pixels


def test_chunk_plan_of_the_smallest_shapes():
    """The frames the cases below use: (compact pixels, chunk, launches)."""
    table = [((160, 112), 7, False, 1, (17920, 3, 3)),       # odd chunk (padded to 4), a tail of one sample
             ((192, 128), 5, False, 1, (24576, 2, 3)),
             ((96, 80), 9, True, 1, (7680, 4, 3)),
             ((160, 112), 3, True, 1, (17920, 1, 3)),
             ((96, 80), 5, False, 3, (7680, 2, 3)),
             ((96, 80), 3, True, 3, (7680, 1, 3)),
             ((96, 80), 3, False, 8, (7680, 1, 3))]
    for size, spp, gaussian, films, (pixels, chunk, launches) in table:
        assert chunk_plan(size, spp, gaussian, films) == (chunk, launches, pixels), (size, spp, gaussian, films)
    # every third 8x8 tile / every third block of 8 rows of 192 x 260 (33 tile rows, the last one partial)
    assert chunk_plan((192, 260), 7, False, row=(0, 3, 1), tile_shard=True) == (3, 3, 16896)
    assert chunk_plan((192, 260), 7, False, row=(8, 3, 2)) == (3, 3, 16896)
    assert chunk_plan((192, 260), 7, False) == (1, 7, 50688)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _records_equal(a, b, spp, chunk, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    same = np.all(_bits(a) == _bits(b), axis=1)
    bad = np.nonzero(~same)[0]
    assert same.all(), '%s: %d of %d records differ; first record %d = pixel %d, sample j = %d (launch %d): %s vs %s' % (
        what, bad.size, same.size, bad[0], bad[0] // spp, bad[0] % spp, (bad[0] % spp) // chunk,
        a[bad[0]].tolist(), b[bad[0]].tolist())


def _films_equal(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.argwhere(np.any(_bits(a) != _bits(b), axis=-1))
    assert bad.size == 0, '%s: %d film pixels differ, first %s: %s vs %s' % (
        what, len(bad), bad[:3].tolist(), a[tuple(bad[0])].tolist(), b[tuple(bad[0])].tolist())


_REF = {}


def _oracle(oracle, key, sc, it, **kw):
    """The oracle's render of a case, made once per session and shared (read-only)."""
    if key not in _REF:
        film, smp, st = oracle.render(sc, it, samples=True, libm_mode=0, threads=THREADS, **kw)
        film.setflags(write=False)
        smp.setflags(write=False)
        _REF[key] = (film, smp, st)
    return _REF[key]


def _window(sc, it):
    return it.crop or (0, 0, sc.sensor.width, sc.sensor.height)


def _check(gpu_ctx, oracle, monkeypatch, key, sc, it, instr=True, engine=None, row=(0, 1, 0), tile_shard=False,
           expect=None, oracle_kw=None):
    """One chunked render against the oracle and against the one-launch render.
    instr: the instrumented kernels (per-sample records compared), else the kernels the
    benchmark times.  expect: the (chunk, launches) the case was chosen for."""
    win = _window(sc, it)
    spp = it.sampleCount
    chunk, launches, _ = chunk_plan(win[2:], spp, it.rfilter != 'box', row=row, tile_shard=tile_shard)
    assert launches >= 3 and chunk < spp
    if expect is not None:
        assert (chunk, launches) == expect
    gpu_ctx.upload(sc)
    if oracle_kw is None:
        oracle_kw = {}
    film_o, smp_o, st_o = _oracle(oracle, key, sc, it, row=row, tile_shard=tile_shard, **oracle_kw)
    monkeypatch.setenv(ENV, str(BUDGET))
    film_c, smp_c, st_c = gpu_ctx.render(it, samples=instr, row=row, tile_shard=tile_shard, engine=engine)
    assert gpu_ctx.launch_chunks() == launches, (gpu_ctx.launch_chunks(), launches)
    variant = gpu_ctx.kernel_variant()
    monkeypatch.delenv(ENV)
    film_1, smp_1, st_1 = gpu_ctx.render(it, samples=instr, row=row, tile_shard=tile_shard, engine=engine)
    assert gpu_ctx.launch_chunks() == 1
    assert gpu_ctx.kernel_variant() == variant
    if instr:
        _records_equal(smp_c, smp_o, spp, chunk, key + ': chunked vs oracle')
    _films_equal(film_c, film_o, key + ': chunked vs oracle')
    _films_equal(film_c, film_1, key + ': chunked vs one launch')
    for k in COUNTERS:
        assert st_c[k] == st_o[k] == st_1[k], (key, k, st_c[k], st_o[k], st_1[k])
    return film_c, variant


# ---- the megakernel on the tiny LDS scene (C1) ---------------------------------------------
def _c1(name, materials='diffuse'):
    """name -> (scene, integrator, (chunk, launches))."""
    if name == 'box_odd':           # chunk 3: the record buffer is padded to 4, the last launch holds 1 sample
        sc, it = scenes.build('C1', width=160, height=112, spp=7, rfilter='box', materials=materials)
        return sc, it, (3, 3)
    if name == 'box_even':
        sc, it = scenes.build('C1', width=192, height=128, spp=5, rfilter='box', materials=materials)
        return sc, it, (2, 3)
    if name == 'gauss_4':
        sc, it = scenes.build('C1', width=96, height=80, spp=9, rfilter='gaussian', materials=materials)
        return sc, it, (4, 3)
    if name == 'gauss_1':
        sc, it = scenes.build('C1', width=160, height=112, spp=3, rfilter='gaussian', materials=materials)
        return sc, it, (1, 3)
    if name == 'box_crop':          # a window off the origin with partial 8x8 tiles: 20 x 14 tiles
        sc, it = scenes.build('C1', width=168, height=120, spp=7, rfilter='box', materials=materials)
        it.crop = (5, 4, 155, 107)
        return sc, it, (3, 3)
    assert name == 'gauss_crop'     # 12 x 10 tiles
    sc, it = scenes.build('C1', width=104, height=88, spp=9, rfilter='gaussian', materials=materials)
    it.crop = (6, 3, 91, 75)
    return sc, it, (4, 3)


@pytest.mark.parametrize('instr', [True, False], ids=['instr', 'plain'])
@pytest.mark.parametrize('name', ['box_odd', 'box_even', 'gauss_4', 'gauss_1', 'box_crop', 'gauss_crop'])
def test_megakernel_lds_scene(gpu_ctx, oracle, monkeypatch, name, instr):
    sc, it, expect = _c1(name)
    _, v = _check(gpu_ctx, oracle, monkeypatch, 'c1_' + name, sc, it, instr=instr, expect=expect)
    assert v is not None and v['scene_lds'] and v['instr'] == instr, v


@pytest.mark.parametrize('instr', [True, False], ids=['instr', 'plain'])
@pytest.mark.parametrize('shift', [0, 1, 2])
def test_sample_runs_against_chunks(gpu_ctx, oracle, monkeypatch, shift, instr):
    """Runs of 1, 2 and 4 samples over chunks of 3 + 3 + 1: with shift 2 the run is longer
    than every chunk; with shift 1 the second run of a chunk lacks its second sample (the
    held splat pair is stored alone) and the last chunk's only run lacks it too."""
    monkeypatch.setenv('MTSGPU_ROUND_SHIFT', str(shift))
    sc, it, expect = _c1('box_odd')
    _check(gpu_ctx, oracle, monkeypatch, 'c1_box_odd', sc, it, instr=instr, expect=expect)


# ---- the megakernel over an HBM BVH (C3 small) ---------------------------------------------
def _c3(rfilter):
    w, h, spp = (160, 112, 7) if rfilter == 'box' else (96, 80, 9)
    return scenes.build('C3', width=w, height=h, spp=spp, rfilter=rfilter, env_size=(128, 64), blob=(48, 30))


@pytest.mark.parametrize('shift', [None, 2], ids=['default_runs', 'runs_of_4'])
@pytest.mark.parametrize('rfilter', ['box', 'gaussian'])
def test_megakernel_hbm_bvh(gpu_ctx, oracle, monkeypatch, rfilter, shift):
    """The latency-bound kernels' own run lengths (chosen per chunk, so the one-sample tail
    takes another shift than the chunks before it), and runs of 4 forced."""
    if shift is not None:
        monkeypatch.setenv('MTSGPU_ROUND_SHIFT', str(shift))
    sc, it = _c3(rfilter)
    expect = (3, 3) if rfilter == 'box' else (4, 3)
    _, v = _check(gpu_ctx, oracle, monkeypatch, 'c3_' + rfilter, sc, it, instr=True, expect=expect)
    assert v is not None and not v['scene_lds'], v
    _, v = _check(gpu_ctx, oracle, monkeypatch, 'c3_' + rfilter, sc, it, instr=False, expect=expect)
    assert v is not None and not v['scene_lds'] and not v['instr'], v


# ---- the wavefront engine ------------------------------------------------------------------
@pytest.mark.parametrize('name', ['box_odd', 'gauss_4'])
def test_wavefront(gpu_ctx, oracle, monkeypatch, name):
    sc, it, expect = _c1(name, 'rough')
    _, v = _check(gpu_ctx, oracle, monkeypatch, 'c1_rough_' + name, sc, it, engine='wavefront', expect=expect)
    assert v is None and gpu_ctx.debug_counters()[15] == 1 << 16


def test_wavefront_slot_regeneration_inside_chunks(gpu_ctx, oracle, monkeypatch):
    """2048 path slots for chunks of 3 x 17920 items: every slot takes its next item from
    (sampleIndex - j0) * num_pixels + pix + slots, in launches with j0 = 3 and 6 as well."""
    monkeypatch.setenv('MTSGPU_WF_SLOTS', '2048')
    sc, it, expect = _c1('box_odd', 'rough')
    assert chunk_plan((160, 112), 7, False)[2] * expect[0] > 8 * 2048
    _check(gpu_ctx, oracle, monkeypatch, 'c1_rough_box_odd', sc, it, engine='wavefront', expect=expect)
    assert gpu_ctx.debug_counters()[15] == 1 << 16


def test_wavefront_over_kdtree(gpu_ctx, oracle, monkeypatch):
    sc, it, expect = _c1('gauss_4', 'rough')
    gpu_ctx.upload(sc)
    nodes, idx, _ = gpu_ctx.kdtree()
    _check(gpu_ctx, oracle, monkeypatch, 'c1_rough_gauss_4_kd', sc, it, engine='kdtree', expect=expect,
           oracle_kw={'kdtree': (nodes, idx)})
    assert gpu_ctx.debug_counters()[15] == 1 << 16


# ---- other integrators and samplers --------------------------------------------------------
def test_direct_integrator(gpu_ctx, oracle, monkeypatch):
    """path_kernel.hip's direct kernel: its own j = j0 + jj, 2D sample arrays of 2 and 3."""
    sc, _, expect = _c1('box_odd', 'smooth')
    it = DirectIntegrator(sampleCount=7, rfilter='box', emitterSamples=2, bsdfSamples=3)
    _check(gpu_ctx, oracle, monkeypatch, 'c1_smooth_direct', sc, it, expect=expect)


def test_volpath(gpu_ctx, oracle, monkeypatch):
    sc, _, expect = _c1('box_even', 'shapes')
    it = VolpathIntegrator(sampleCount=5, rfilter='box', strictNormals=True)
    _check(gpu_ctx, oracle, monkeypatch, 'c1_shapes_volpath', sc, it, expect=expect)


def test_independent_sampler(gpu_ctx, oracle, monkeypatch):
    """The stream key holds the global sample index (indep_key(px, py, j))."""
    sc, _, expect = _c1('gauss_4', 'shapes')
    it = PathIntegrator(sampleCount=9, rfilter='gaussian', sampler='independent')
    _check(gpu_ctx, oracle, monkeypatch, 'c1_shapes_independent', sc, it, expect=expect)


# ---- shards --------------------------------------------------------------------------------
@pytest.mark.parametrize('row,tile_shard', [((0, 3), True), ((8, 3), False)], ids=['tiles3', 'row8of3'])
def test_shards(gpu_ctx, oracle, monkeypatch, row, tile_shard):
    """Every third 8x8 tile / every third block of 8 rows of a 192 x 260 frame: each shard
    runs as 3 + 3 + 1 samples and equals the oracle's shard; the shards sum to the unsharded
    frame, which runs as 7 launches of one sample."""
    sc, it = scenes.build('C1', width=192, height=260, spp=7, rfilter='box')
    acc = None
    for k in range(3):
        r = (row[0], row[1], k)
        film, _ = _check(gpu_ctx, oracle, monkeypatch, 'c1_shard_%d_%d_%d_%d' % (r + (tile_shard,)), sc, it,
                         instr=(k == 1), row=r, tile_shard=tile_shard, expect=(3, 3))
        assert np.count_nonzero(film[..., 4])
        acc = film.copy() if acc is None else acc + film
    monkeypatch.setenv(ENV, str(BUDGET))
    full, _, _ = gpu_ctx.render(it)
    assert gpu_ctx.launch_chunks() == 7 == chunk_plan((192, 260), 7, False)[1]
    _films_equal(acc, full, 'the shards\' sum vs the unsharded chunked film')


# ---- the field pass ------------------------------------------------------------------------
def _fields(names):
    return [FieldIntegrator(n, undefined=UNDEF) for n in names]


FIELDS8 = ['shNormal', 'distance', 'position', 'geoNormal', 'relPosition', 'primIndex', 'shapeIndex', 'uv']


@pytest.mark.parametrize('rfilter,spp,names', [('box', 5, FIELDS8[:3]), ('gaussian', 3, FIELDS8[:3]), ('box', 3, FIELDS8)],
                         ids=['box_3', 'gaussian_3', 'box_8'])
def test_field_pass(gpu_ctx, oracle, monkeypatch, rfilter, spp, names):
    """One record array per field under the one budget: contrib_stride and the fields'
    offsets follow the chunk; with 8 fields (MTSGPU_MAX_FIELDS) the chunk is one sample."""
    n = len(names)
    assert n == 3 or n == abi.MAX_FIELDS
    W, H = 96, 80
    sc, it = scenes.build('C1', width=W, height=H, spp=spp, rfilter=rfilter)
    it.hasAlpha = True
    win = (0, 0, W, H)
    chunk, launches, _ = chunk_plan((W, H), spp, rfilter != 'box', n_films=n)
    assert launches >= 3 and (chunk, launches) == ((2, 3) if (rfilter, n) == ('box', 3) else (1, 3))
    gpu_ctx.upload(sc)
    monkeypatch.setenv(ENV, str(BUDGET))
    films_c, rec_c, st_c = gpu_ctx.render_fields(it, _fields(names), samples=True)
    assert gpu_ctx.launch_chunks() == launches
    assert gpu_ctx.debug_counters()[15] == (1 << 17) | (1 << 12)
    # (the colour render's records are 1 / n of the field pass's: it takes the launches of its own plan)
    colour, _, _ = gpu_ctx.render(it)
    assert gpu_ctx.launch_chunks() == chunk_plan((W, H), spp, rfilter != 'box')[1]
    monkeypatch.delenv(ENV)
    films_1, rec_1, st_1 = gpu_ctx.render_fields(it, _fields(names), samples=True)
    assert gpu_ctx.launch_chunks() == 1
    _records_equal(rec_c, rec_1, spp, chunk, 'field records: chunked vs one launch')
    _films_equal(films_c, films_1, 'field films: chunked vs one launch')
    if rfilter == 'box':
        _films_equal(films_c, fr.box_film_ref(rec_1, n, spp, win, W, H, oracle), 'box field films vs the ordered sum')
    else:
        for f in range(n):
            _films_equal(films_c[f], fr.gather_film_ref(rec_1, f, spp, win, W, H, rfilter, it.rfilterParam, oracle),
                         'gather field film %d vs the gather order' % f)
    for f in range(n):
        _films_equal(films_c[f][..., 3:5], colour[..., 3:5], 'alpha / weight of field film %d' % f)
    for k in COUNTERS:
        assert st_c[k] == st_1[k], (k, st_c[k], st_1[k])
    assert st_c['samples'] == W * H * spp == st_c['rays']


def test_multichannel_end_to_end(gpu_ctx, oracle, monkeypatch):
    """The colour pass (3 launches) and the field pass (two films: 7 launches) of one
    multichannel render, both chunked."""
    sc, path, expect = _c1('box_odd')
    W, H, spp = 160, 112, 7
    hf = HDRFilm(pixelFormat='rgb, rgb, luminance', channelNames='color, normal, distance', componentFormat='float32')
    mc = MultiChannelIntegrator([path, FieldIntegrator('shNormal', UNDEF), FieldIntegrator('distance', UNDEF)], film=hf)
    gpu_ctx.upload(sc)
    monkeypatch.setenv(ENV, str(BUDGET))
    plain, _, _ = gpu_ctx.render(path)
    assert gpu_ctx.launch_chunks() == expect[1]
    _films_equal(plain, _oracle(oracle, 'c1_box_odd', sc, path)[0], 'plain chunked path render vs oracle')
    films_c, (smp_c, rec_c), _ = gpu_ctx.render(mc, samples=True)
    assert gpu_ctx.launch_chunks() == 7 == chunk_plan((W, H), spp, False, n_films=2)[1]     # (the field pass)
    monkeypatch.delenv(ENV)
    films_1, (smp_1, rec_1), _ = gpu_ctx.render(mc, samples=True)
    assert gpu_ctx.launch_chunks() == 1
    _films_equal(films_c[0][..., :3], plain[..., :3], 'colour rgb vs the plain chunked path render')
    _films_equal(films_c, films_1, 'multichannel films: chunked vs one launch')
    _records_equal(smp_c, smp_1, spp, expect[0], 'colour records')
    _records_equal(rec_c, rec_1, spp, 1, 'field records')
    _records_equal(rec_c[:, 0:2], smp_c[:, 4:6], spp, 1, 'samplePos')
    _films_equal(films_c[1:], fr.box_film_ref(rec_1, 2, spp, (0, 0, W, H), W, H, oracle), 'field films')
    _films_equal(films_c[0][..., 3:5], films_c[1][..., 3:5], 'alpha / weight')


# ---- render_device -------------------------------------------------------------------------
def test_render_device_on_torch_stream(gpu_ctx, oracle, monkeypatch):
    """The call the benchmark makes: a torch film on torch's stream, no records."""
    import torch
    sc, it, expect = _c1('box_odd')
    gpu_ctx.upload(sc)
    b = film_border(it.rfilter, it.rfilterParam)
    shape = (112 + 2 * b, 160 + 2 * b, 5)
    monkeypatch.setenv(ENV, str(BUDGET))
    host, _, st_h = gpu_ctx.render(it)
    assert gpu_ctx.launch_chunks() == expect[1]
    film = torch.zeros(shape, dtype=torch.float32, device='cuda')
    st_d = gpu_ctx.render_device(it, film.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert gpu_ctx.launch_chunks() == expect[1]
    v = gpu_ctx.kernel_variant()
    assert v is not None and not v['instr']
    dev = film.cpu().numpy()
    _films_equal(dev, host, 'device film vs host-buffer film')
    film_o, _, st_o = _oracle(oracle, 'c1_box_odd', sc, it)
    _films_equal(dev, film_o, 'device film vs oracle')
    for k in COUNTERS:
        assert st_d[k] == st_h[k] == st_o[k], (k, st_d[k], st_h[k], st_o[k])


# ---- between chunks ------------------------------------------------------------------------
@pytest.mark.parametrize('sampler', ['independent-sfmt', 'independent-sfmt-blocks'])
def test_sfmt_replay_refuses_a_chunked_render(gpu_ctx, monkeypatch, sampler):
    """One lane renders a replay unit's whole SFMT stream: the samplers cannot stop between
    chunks.  40 x 32 (1280 compact pixels): 51 samples fit the budget, 64 do not."""
    sc, sobol = scenes.build('C1', width=40, height=32, spp=4, rfilter='box')
    assert chunk_plan((40, 32), 64, False)[0] == 51
    gpu_ctx.upload(sc)
    monkeypatch.setenv(ENV, str(BUDGET))
    before, _, _ = gpu_ctx.render(sobol)
    with pytest.raises(MtsgpuError) as e:
        gpu_ctx.render(PathIntegrator(sampleCount=64, rfilter='box', sampler=sampler))
    assert e.value.code == abi.EINVAL and 'sampleCount' in str(e.value), str(e.value)
    after, _, _ = gpu_ctx.render(sobol)
    _films_equal(after, before, 'the Sobol render after the refusal')


def test_cancel_before_the_first_launch(gpu_ctx, oracle, monkeypatch):
    """A cancel word set before the call: MTSGPU_ECANCEL; with the word cleared the same
    context renders the uncancelled film, chunked and in one launch."""
    sc, it, expect = _c1('box_odd')
    gpu_ctx.upload(sc)
    film_o = _oracle(oracle, 'c1_box_odd', sc, it)[0]
    word = C.c_int32(0)
    for budget in (str(BUDGET), None):
        if budget is None:
            monkeypatch.delenv(ENV)
        else:
            monkeypatch.setenv(ENV, budget)
        launches = expect[1] if budget else 1
        ref, _, st_ref = gpu_ctx.render(it)
        assert gpu_ctx.launch_chunks() == launches
        word.value = 1
        with pytest.raises(MtsgpuError) as e:
            gpu_ctx.render(it, cancel=word)
        assert e.value.code == abi.ECANCEL
        word.value = 0
        film, _, st = gpu_ctx.render(it, cancel=word)
        assert gpu_ctx.launch_chunks() == launches
        _films_equal(film, ref, 'after a cancelled call')
        _films_equal(film, film_o, 'after a cancelled call vs oracle')
        for k in COUNTERS:
            assert st[k] == st_ref[k], (k, st[k], st_ref[k])
