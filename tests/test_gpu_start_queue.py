"""The tiny-scene megakernel starts its paths a wave at a time from an LDS queue
(dmega.h): production passes, in which all 64 lanes run one step of their item
stream and the real samples' start records are compacted into the wave's buffer,
and pops, in which the lanes whose path ended take the next records.  Which lane
renders which of the wave's items must not change a bit.

Each test is one small render compared with the oracle as tests/test_gpu_hoisted.py
does (per-sample records where instrumented, film, the four counters, on uint32
views), at the smallest shapes at which the queue can go wrong: partial and empty
batches, refills while most lanes are busy, whole-batch consumption, every record
mode, chunked launches, the other samplers, and a launch that does not take the queue.

Debug counter 11 (Context.debug_counters) holds the production passes of the last
render.  `queue_plan` restates their number from the launch geometry: a wave runs one
pass per step of its first lane (the lane of a wave with the most items) and one more
in which every lane finds its stream exhausted.  Every test asserts at least that
many, so none can pass by taking the loop without the queue.
"""
import os

import numpy as np
import pytest

from mitsuba_amd import scenes
from mitsuba_amd.scene import BSDF, Mesh, PathIntegrator, VolpathIntegrator, film_border, look_at
from test_gpu_hoisted import COUNTERS, SHARD_IDS, SHARDS, _bits, _check

pytestmark = pytest.mark.gpu

PASSES = 11           # debug counter: production passes
BUDGET = 1 << 20      # the smallest MTSGPU_CONTRIB_BYTES the library takes
INSTR = pytest.mark.parametrize('instr', [True, False], ids=['instr', 'plain'])


def _ceil_div(a, b):
    return (a + b - 1) // b


def compact_pixels(size, row=(0, 1, 0), tile_shard=False):
    """Compact pixels (padding included) of a size = (w, h) window: render_plan.cpp launch_geometry."""
    w, h = size
    block, stride = row[0] or 1, row[1] or 1
    tiles_x = _ceil_div(w, 8)
    if tile_shard:
        return _ceil_div(tiles_x * _ceil_div(h, 8), stride) * 64
    return tiles_x * _ceil_div(_ceil_div(_ceil_div(h, block), stride) * block, 8) * 64


def queue_plan(num_pixels, spp, cus, shift=None, chunk=None):
    """Production passes of a render: per launch, over the waves of its grid, the
    steps of the wave's first lane plus the pass that finds every lane exhausted
    (render_plan.cpp plan_launch and run_shift, layout.h mtsg_run_step, restated)."""
    chunk = chunk or spp
    total = 0
    for j0 in range(0, spp, chunk):
        cs = min(chunk, spp - j0)
        items = cs * num_pixels
        blocks = max(1, _ceil_div(items, 256))
        assert blocks <= cus       # the grid is not capped by the resident blocks
        lanes = blocks * 256
        if shift is None:
            s = 1
            while s > 0 and ((1 << s) > cs or ((items // lanes) >> s) < 100):
                s -= 1
        else:
            s = shift
        runs = _ceil_div(cs, 1 << s) * num_pixels
        for g0 in range(0, lanes, 64):
            total += ((_ceil_div(runs - g0, lanes) if g0 < runs else 0) << s) + 1
    return total


def test_queue_plan():
    # one tile, one sample: 4 waves; the first steps once and fails once, the others fail once
    assert queue_plan(64, 1, 256) == 2 + 3
    # runs of two with one sample: the run's second step is its missing sample
    assert queue_plan(64, 1, 256, shift=1) == 3 + 3
    # 384 pixels x 5 samples = 1920 items in 8 blocks (32 waves): 30 waves hold one item per lane
    assert queue_plan(384, 5, 256, shift=0) == 30 * 2 + 2
    # runs of two: 3 runs per pixel = 1152 runs over 2048 lanes: 18 waves with a run of two steps
    assert queue_plan(384, 5, 256, shift=1) == 18 * 3 + 14
    # two launches of 3 and 2 samples
    assert queue_plan(384, 5, 256, shift=0, chunk=3) == (18 * 2 + 2) + (12 * 2)


def _window(sc, it):
    return it.crop or (0, 0, sc.sensor.width, sc.sensor.height)


def _passes(gpu_ctx, sc, it, row=(0, 1, 0), tile_shard=False, shift=None, chunk=None):
    """Asserts the last render's production passes against the plan; returns them."""
    n = compact_pixels(_window(sc, it)[2:], row, tile_shard)
    plan = queue_plan(n, it.sampleCount, gpu_ctx.scene_info()['cus'], shift, chunk)
    got = gpu_ctx.debug_counters()[PASSES]
    assert got >= plan > 0, (got, plan)
    return got


def _queued(gpu_ctx, oracle, sc, it, instr, row=(1, 1, 0), tile_shard=False, shift=None):
    st = _check(gpu_ctx, oracle, sc, it, instr, row, tile_shard)
    v = gpu_ctx.kernel_variant()
    assert v is not None and v['scene_lds'] and v['instr'] == instr
    _passes(gpu_ctx, sc, it, row, tile_shard, shift)
    return st


# ---- partial and empty batches -------------------------------------------------------------
@INSTR
@pytest.mark.parametrize('shift', [0, 1])
@pytest.mark.parametrize('spp', [1, 3, 5])
@pytest.mark.parametrize('size,crop', [((24, 16), (0, 0, 21, 13)), ((40, 24), (0, 0, 37, 19))], ids=['24x16', '40x24'])
def test_windows_with_padding(gpu_ctx, oracle, monkeypatch, size, crop, spp, shift, instr):
    monkeypatch.setenv('MTSGPU_ROUND_SHIFT', str(shift))
    sc, it = scenes.build('C1', width=size[0], height=size[1], spp=spp, rfilter='box')
    it.crop = crop
    _queued(gpu_ctx, oracle, sc, it, instr, shift=shift)


@INSTR
@pytest.mark.parametrize('shift', [0, 1])
def test_fewer_items_than_a_wave(gpu_ctx, oracle, monkeypatch, shift, instr):
    """15 pixels of one tile, one sample: one wave produces a first batch of 15, three nothing."""
    monkeypatch.setenv('MTSGPU_ROUND_SHIFT', str(shift))
    sc, it = scenes.build('C1', width=24, height=16, spp=1, rfilter='box')
    it.crop = (9, 6, 5, 3)
    st = _queued(gpu_ctx, oracle, sc, it, instr, shift=shift)
    assert st['samples'] == 15


@INSTR
@pytest.mark.parametrize('spp', [3, 5])
def test_crop_off_the_origin(gpu_ctx, oracle, monkeypatch, spp, instr):
    monkeypatch.setenv('MTSGPU_ROUND_SHIFT', '1')
    sc, it = scenes.build('C1', width=24, height=20, spp=spp, rfilter='box')
    it.crop = (5, 4, 13, 11)
    _queued(gpu_ctx, oracle, sc, it, instr, shift=1)


@INSTR
@pytest.mark.parametrize('row,tile_shard', SHARDS, ids=SHARD_IDS)
def test_every_shard_setting(gpu_ctx, oracle, monkeypatch, row, tile_shard, instr):
    """(rows 8 of 4, phase 3: every compact pixel is padding -- passes that produce nothing)"""
    monkeypatch.setenv('MTSGPU_ROUND_SHIFT', '1')
    sc, it = scenes.build('C1', width=24, height=20, spp=3, rfilter='box')
    it.crop = (5, 4, 13, 11)
    _queued(gpu_ctx, oracle, sc, it, instr, row, tile_shard, shift=1)


# ---- refill while most lanes are busy ------------------------------------------------------
def _closed_bright_box(spp):
    """The Cornell room closed by a front wall, every albedo 0.9, seen from inside: path
    lengths spread out up to maxDepth 30, so pops meet a buffer with fewer entries than
    needy lanes, and refills happen while most lanes of the wave are mid-path."""
    sc, _ = scenes.build('C1', width=32, height=24, spp=spp, rfilter='box')
    sc.bsdfs = [BSDF('diffuse', reflectance=(0.9, 0.9, 0.9)) for _ in sc.bsdfs]
    p, i = scenes._quads_mesh([[(0, 0, 0), (552.8, 0, 0), (556, 548.8, 0), (0, 548.8, 0)]], inward=True)
    sc.meshes = list(sc.meshes) + [Mesh(p, i, bsdf=0)]
    sc.sensor.toWorld = look_at(np.array([2.78, 2.73, 0.2]), np.array([2.78, 2.5, 3.0]), (0, 1, 0))
    sc.sensor.fov = 90.0
    sc.sensor.nearClip = 0.01
    it = PathIntegrator(maxDepth=30, rrDepth=20, sampleCount=spp, rfilter='box', rfilterParam=0.5)
    return sc, it


@INSTR
@pytest.mark.parametrize('shift', [0, 1])
def test_refill_while_lanes_are_busy(gpu_ctx, oracle, monkeypatch, shift, instr):
    monkeypatch.setenv('MTSGPU_ROUND_SHIFT', str(shift))
    sc, it = _closed_bright_box(6)
    assert sc.num_triangles <= 64
    st = _queued(gpu_ctx, oracle, sc, it, instr, shift=shift)
    assert st['path_length_sum'] > 8 * st['samples']   # long paths of spread-out lengths


# ---- whole-batch consumption ---------------------------------------------------------------
@INSTR
def test_wide_camera_mostly_misses(gpu_ctx, oracle, instr):
    sc, it = scenes.build('C1', width=40, height=24, spp=4, rfilter='box')
    sc.sensor.fov = 120.0
    st = _queued(gpu_ctx, oracle, sc, it, instr)
    assert st['rays'] < 2 * st['samples']    # most paths are their primary ray


@INSTR
def test_every_primary_ray_misses(gpu_ctx, oracle, instr):
    sc, it = scenes.build('C1', width=24, height=16, spp=3, rfilter='box')
    sc.sensor.toWorld = look_at(np.array([2.78, 2.73, -8.0]), np.array([2.78, 2.73, -9.0]), (0, 1, 0))
    st = _queued(gpu_ctx, oracle, sc, it, instr)
    assert st['rays'] == st['samples'] == 24 * 16 * 3 and st['shadow_rays'] == 0


# ---- other record modes --------------------------------------------------------------------
@INSTR
@pytest.mark.parametrize('spp', [3, 4])
def test_gaussian_gather(gpu_ctx, oracle, spp, instr):
    sc, it = scenes.build('C1', width=32, height=24, spp=spp, rfilter='gaussian')
    it.crop = (6, 3, 20, 12)
    _queued(gpu_ctx, oracle, sc, it, instr)


@INSTR
def test_box_of_radius_one_spills(gpu_ctx, oracle, monkeypatch, instr):
    monkeypatch.setenv('MTSGPU_ROUND_SHIFT', '1')
    sc, it = scenes.build('C1', width=24, height=16, spp=3, rfilter='box')
    it.rfilterParam = 1.0
    it.crop = (3, 2, 19, 13)
    _queued(gpu_ctx, oracle, sc, it, instr, shift=1)


def test_render_device(gpu_ctx, oracle):
    import torch
    sc, it = scenes.build('C1', width=40, height=24, spp=5, rfilter='box')
    gpu_ctx.upload(sc)
    b = film_border(it.rfilter, it.rfilterParam)
    film = torch.zeros((24 + 2 * b, 40 + 2 * b, 5), dtype=torch.float32, device='cuda')
    st_d = gpu_ctx.render_device(it, film.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _passes(gpu_ctx, sc, it)
    film_o, _, st_o = oracle.render(sc, it, samples=True, libm_mode=0)
    assert np.array_equal(_bits(film.cpu().numpy()), _bits(film_o))
    for k in COUNTERS:
        assert st_d[k] == st_o[k], (k, st_d[k], st_o[k])


# ---- chunked launches ----------------------------------------------------------------------
@INSTR
@pytest.mark.parametrize('rfilter,size,spp,chunk', [('box', (160, 112), 7, 3), ('gaussian', (96, 80), 9, 4)])
def test_chunked_launches(gpu_ctx, oracle, monkeypatch, rfilter, size, spp, chunk, instr):
    monkeypatch.setenv('MTSGPU_CONTRIB_BYTES', str(BUDGET))
    sc, it = scenes.build('C1', width=size[0], height=size[1], spp=spp, rfilter=rfilter)
    n = compact_pixels(size)
    assert chunk == BUDGET // (n * (32 if rfilter == 'gaussian' else 16)) and _ceil_div(spp, chunk) == 3
    _check(gpu_ctx, oracle, sc, it, instr)
    assert gpu_ctx.launch_chunks() == 3
    _passes(gpu_ctx, sc, it, chunk=chunk)


# ---- other samplers and integrators --------------------------------------------------------
@INSTR
def test_independent_sampler_through_the_queue(gpu_ctx, oracle, instr):
    sc, _ = scenes.build('C1', width=24, height=16, spp=4, rfilter='box')
    it = PathIntegrator(sampleCount=5, rfilter='box', sampler='independent')
    it.crop = (2, 1, 19, 13)
    _queued(gpu_ctx, oracle, sc, it, instr)


@INSTR
def test_volpath_through_the_queue(gpu_ctx, oracle, instr):
    sc, _ = scenes.build('C1', width=24, height=16, spp=4, rfilter='box')
    it = VolpathIntegrator(sampleCount=3, rfilter='box', strictNormals=True)
    _queued(gpu_ctx, oracle, sc, it, instr)


@INSTR
def test_sfmt_replay_keeps_its_loop(gpu_ctx, oracle, instr):
    """The replay's draws depend on the order in which a lane renders its unit: it
    keeps the loop without the queue (no production passes)."""
    sc, _ = scenes.build('C1', width=40, height=24, spp=4, rfilter='box')
    it = PathIntegrator(sampleCount=3, rfilter='box', sampler='independent-sfmt')
    _check(gpu_ctx, oracle, sc, it, instr)
    assert gpu_ctx.kernel_variant()['scene_lds']
    assert gpu_ctx.debug_counters()[PASSES] == 0


# ---- a launch that does not take the queue -------------------------------------------------
@INSTR
@pytest.mark.parametrize('rfilter', ['box', 'gaussian'])
def test_traversing_launch_equals_the_queued_one(gpu_ctx, oracle, monkeypatch, rfilter, instr):
    """MTSGPU_NO_SCAN=1: the LDS scene is traversed, its stacks lie where the queue would,
    and the kernel takes the loop without the queue.  Both renders equal the oracle's."""
    monkeypatch.setenv('MTSGPU_ROUND_SHIFT', '1')
    sc, it = scenes.build('C1', width=40, height=24, spp=5, rfilter=rfilter)
    it.crop = (3, 2, 35, 21)
    _queued(gpu_ctx, oracle, sc, it, instr, shift=1)
    film_q, smp_q, st_q = gpu_ctx.render(it, samples=instr)
    monkeypatch.setenv('MTSGPU_NO_SCAN', '1')
    _check(gpu_ctx, oracle, sc, it, instr)
    assert gpu_ctx.kernel_variant()['scene_lds']
    assert gpu_ctx.debug_counters()[PASSES] == 0
    film_t, smp_t, st_t = gpu_ctx.render(it, samples=instr)
    monkeypatch.delenv('MTSGPU_NO_SCAN')
    assert np.array_equal(_bits(film_q), _bits(film_t))
    if instr:
        assert np.array_equal(_bits(smp_q), _bits(smp_t))
    for k in COUNTERS:
        assert st_q[k] == st_t[k], (k, st_q[k], st_t[k])
    # the A/B library built with -DMTSG_START_QUEUE=0 (make variant V=no_queue), where present
    from mitsuba_amd import LIB_PATH
    from mitsuba_amd.integrator import Context
    lib = os.path.join(os.path.dirname(LIB_PATH), 'variants', 'libmtsgpu_no_queue.so')
    if os.path.exists(lib):
        ctx = Context(lib_path=lib)
        ctx.upload(sc)
        film_v, smp_v, st_v = ctx.render(it, samples=instr)
        assert ctx.debug_counters()[PASSES] == 0
        ctx.close()
        assert np.array_equal(_bits(film_q), _bits(film_v))
        for k in COUNTERS:
            assert st_q[k] == st_v[k], (k, st_q[k], st_v[k])
