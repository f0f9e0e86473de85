"""The tiny-scene megakernel's production passes retire the samples whose camera ray
fails section B's own ray_interval test (scene bounds and clip planes) in kernels
without an environment emitter (dmega.h, PathShader::retire): the pass writes the
black depth-1 record itself and the sample never takes a lane.  Nothing may change:
every test is one small render compared with the oracle as tests/test_gpu_hoisted.py
does (per-sample records where instrumented, film, the four counters, bit for bit).

Debug counter 12 (Context.debug_counters) holds the samples the passes retired.
`footprints` restates, in numpy, which pixels must and which must not lose their
samples this way: the C1 camera stands in front of the scene's bounding box, inside
the extent of its front face, so a camera ray meets the box exactly when it crosses
that face's rectangle.  A pixel whose footprint, grown by one pixel on every side,
misses the rectangle has all its samples retired (`outside`); one whose grown
footprint lies within it has none retired (`inside`: a margin of one pixel on the
safe side of either claim).  Every render asserts
    samples of `outside` pixels <= counter 12 <= samples - samples of `inside` pixels
and counter 12 <= the oracle's records with L == 0 and depth 1, so no test can pass
with a kernel that queues every sample, nor with one that retires a sample that
sees the box.

Windows: C1 in 40x16, 56x16 and 40x24 frames (fov on the smaller axis): whole 8x8
tiles outside the box, tiles across its edge, and (40x24) tiles inside it.
"""
import math
import os

import numpy as np
import pytest

from mitsuba_amd import scenes
from mitsuba_amd.scene import Emitter, PathIntegrator, VolpathIntegrator, film_border, look_at
from test_gpu_hoisted import COUNTERS, SHARD_IDS, SHARDS, _bits, _check

INSTR = pytest.mark.parametrize('instr', [True, False], ids=['instr', 'plain'])
gpu = pytest.mark.gpu

PASSES, RETIRED = 11, 12     # debug counters: production passes, samples retired in them
SOBOL_WORDS = 10             # debug counter: Sobol words read from HBM (instrumented kernels)
BUDGET = 1 << 20             # the smallest MTSGPU_CONTRIB_BYTES the library takes
WINDOWS = [(40, 16), (56, 16), (40, 24)]


# ---- the geometric restatement -------------------------------------------------------------
def bounds(sc):
    pos = np.concatenate([np.asarray(m.positions, np.float64).reshape(-1, 3) for m in sc.meshes])
    return pos.min(axis=0), pos.max(axis=0)


def film_to_front_face(sc, sx, sy):
    """World (x, y) at which the camera ray through film position (sx, sy) crosses the
    plane of the bounds' front face (perspective.cpp: fov on the smaller axis, film x
    towards the camera's left, film y downwards)."""
    s = sc.sensor
    cam = np.asarray(s.toWorld, np.float64)
    left, up, d, o = cam[:3, 0], cam[:3, 1], cam[:3, 2], cam[:3, 3]
    lo, hi = bounds(sc)
    assert np.allclose(d, (0, 0, 1)) and np.allclose(np.abs(left), (1, 0, 0)) and np.allclose(up, (0, 1, 0))
    assert o[2] < lo[2] and lo[0] < o[0] < hi[0] and lo[1] < o[1] < hi[1]   # in front of, and within, the face
    assert s.fovAxis == 'smaller' and s.width >= s.height
    ty = math.tan(math.radians(s.fov) / 2)
    tx = ty * s.width / s.height
    depth = lo[2] - o[2]
    xc = (1 - 2 * np.asarray(sx, np.float64) / s.width) * tx
    yc = (1 - 2 * np.asarray(sy, np.float64) / s.height) * ty
    return o[0] + depth * xc * left[0], o[1] + depth * yc * up[1]


def footprints(sc, margin=1.0):
    """(outside, inside): (height, width) masks of the film's pixels whose footprint, grown
    by `margin` pixels, misses / lies within the front face's rectangle."""
    s = sc.sensor
    lo, hi = bounds(sc)
    x, y = np.meshgrid(np.arange(s.width), np.arange(s.height))
    xa, ya = film_to_front_face(sc, x - margin, y - margin)
    xb, yb = film_to_front_face(sc, x + 1 + margin, y + 1 + margin)
    x0, x1, y0, y1 = np.minimum(xa, xb), np.maximum(xa, xb), np.minimum(ya, yb), np.maximum(ya, yb)
    outside = (x1 < lo[0]) | (x0 > hi[0]) | (y1 < lo[1]) | (y0 > hi[1])
    inside = (x0 >= lo[0]) & (x1 <= hi[0]) & (y0 >= lo[1]) & (y1 <= hi[1])
    return outside, inside


def retired_bounds(sc, smp_o):
    """(lower, upper, black, samples) for a render whose oracle records are smp_o: records
    of samples that were not rendered (other shards) have depth 0 and do not count."""
    outside, inside = footprints(sc)
    r = smp_o[smp_o[:, 6] >= 1]
    px = np.clip(np.floor(r[:, 4]).astype(int), 0, sc.sensor.width - 1)
    py = np.clip(np.floor(r[:, 5]).astype(int), 0, sc.sensor.height - 1)
    black = int(np.count_nonzero((r[:, :3] == 0).all(axis=1) & (r[:, 6] == 1)))
    return int(outside[py, px].sum()), len(r) - int(inside[py, px].sum()), black, len(r)


def test_footprints_restate_the_clip():
    """No GPU.  At C2's 16:9 frame 556/1015.8 x 548.8/571.4 = 52.6% of the film looks into
    the box; the windows of the GPU tests hold outside, mixed and (40x24) inside tiles."""
    sc, _ = scenes.build('C2')
    s = sc.sensor
    x, y = np.meshgrid(np.arange(s.width) + 0.5, np.arange(s.height) + 0.5)
    wx, wy = film_to_front_face(sc, x, y)
    lo, hi = bounds(sc)
    miss = ~((wx >= lo[0]) & (wx <= hi[0]) & (wy >= lo[1]) & (wy <= hi[1]))
    print('C2 1280x720: %.1f%% of the pixel centres miss the bounds' % (100 * miss.mean()))
    assert abs(miss.mean() - 0.474) < 0.005
    # the frame's top-left corner looks left of and above the box
    cx, cy = film_to_front_face(sc, 0.0, 0.0)
    assert cx > hi[0] and cy > hi[1]
    for w, h in WINDOWS:
        sc, _ = scenes.build('C1', width=w, height=h, spp=1)
        outside, inside = footprints(sc)
        o0, i0 = footprints(sc, margin=0.0)
        assert not (outside & inside).any() and (outside <= o0).all() and (inside <= i0).all()
        tiles = [(o0[ty:ty + 8, tx:tx + 8].all(), i0[ty:ty + 8, tx:tx + 8].all())
                 for ty in range(0, h, 8) for tx in range(0, w, 8)]
        n_out, n_in = sum(t[0] for t in tiles), sum(t[1] for t in tiles)
        print('%dx%d: %.1f%% of the pixels must be retired, %.1f%% must not; tiles outside %d, inside %d, mixed %d'
              % (w, h, 100 * outside.mean(), 100 * inside.mean(), n_out, n_in, len(tiles) - n_out - n_in))
        assert 0 < outside.sum() and 0 < inside.sum() and outside.sum() + inside.sum() < w * h
        assert n_out > 0 and len(tiles) - n_out - n_in > 0
        if (w, h) == (40, 24):
            assert n_in > 0


# ---- one render against the oracle, with the retired count bracketed -----------------------
class _Keep:
    """The oracle, keeping its last render (tests/test_gpu_hoisted._check calls it once)."""

    def __init__(self, oracle):
        self.oracle, self.last = oracle, None

    def render(self, *a, **kw):
        self.last = self.oracle.render(*a, **kw)
        return self.last


def _early(gpu_ctx, oracle, sc, it, instr, row=(1, 1, 0), tile_shard=False, geometric=True):
    """_check, then counter 12 between its bounds.  Returns (stats, retired, bounds)."""
    keep = _Keep(oracle)
    st = _check(gpu_ctx, keep, sc, it, instr, row, tile_shard)
    v = gpu_ctx.kernel_variant()
    assert v is not None and v['scene_lds'] and v['instr'] == instr
    c = gpu_ctx.debug_counters()
    assert c[PASSES] > 0                      # the launch took the start queue
    lower, upper, black, n = retired_bounds(sc, keep.last[1]) if geometric else (0, st['samples'], None, st['samples'])
    if not geometric:
        smp = keep.last[1]
        black = int(np.count_nonzero((smp[:, :3] == 0).all(axis=1) & (smp[:, 6] == 1)))
    assert n == st['samples']
    print('retired %d of %d samples (%.1f%%): bounds [%d, %d], black depth-1 records %d'
          % (c[RETIRED], n, 100.0 * c[RETIRED] / max(n, 1), lower, upper, black))
    assert lower <= c[RETIRED] <= upper, (lower, c[RETIRED], upper)
    assert c[RETIRED] <= black, (c[RETIRED], black)
    return st, c[RETIRED], (lower, upper, black, n)


@gpu
@INSTR
@pytest.mark.parametrize('shift', [0, 1])
@pytest.mark.parametrize('spp', [1, 3, 5])
@pytest.mark.parametrize('size', WINDOWS, ids=['40x16', '56x16', '40x24'])
def test_wide_windows(gpu_ctx, oracle, monkeypatch, size, spp, shift, instr):
    """Outside, mixed and inside tiles; odd sample counts under runs of two: passes in
    which a lane's item is padding or a missing sample beside a retired neighbour."""
    monkeypatch.setenv('MTSGPU_ROUND_SHIFT', str(shift))
    sc, it = scenes.build('C1', width=size[0], height=size[1], spp=spp, rfilter='box')
    _, _, (lower, upper, _, n) = _early(gpu_ctx, oracle, sc, it, instr)
    assert 0 < lower and upper < n


@gpu
@INSTR
def test_window_with_padding_pixels(gpu_ctx, oracle, monkeypatch, instr):
    monkeypatch.setenv('MTSGPU_ROUND_SHIFT', '1')
    sc, it = scenes.build('C1', width=56, height=16, spp=3, rfilter='box')
    it.crop = (3, 1, 43, 13)
    _, _, (lower, upper, _, n) = _early(gpu_ctx, oracle, sc, it, instr)
    assert 0 < lower and upper < n


# ---- everything retired, nothing retired ---------------------------------------------------
@gpu
@INSTR
def test_crop_outside_the_box(gpu_ctx, oracle, instr):
    """Every sample is retired: the batch is never filled."""
    sc, it = scenes.build('C1', width=56, height=16, spp=3, rfilter='box')
    it.crop = (0, 0, 16, 16)
    st, retired, _ = _early(gpu_ctx, oracle, sc, it, instr)
    assert retired == st['samples'] == st['rays'] == 16 * 16 * 3 and st['shadow_rays'] == 0


@gpu
@INSTR
def test_camera_that_sees_nothing(gpu_ctx, oracle, instr):
    sc, it = scenes.build('C1', width=24, height=16, spp=3, rfilter='box')
    sc.sensor.toWorld = look_at(np.array([2.78, 2.73, -8.0]), np.array([2.78, 2.73, -9.0]), (0, 1, 0))
    st, retired, _ = _early(gpu_ctx, oracle, sc, it, instr, geometric=False)
    assert retired == st['samples'] == st['rays'] == 24 * 16 * 3 and st['shadow_rays'] == 0


@gpu
@INSTR
def test_far_clip_in_front_of_the_box(gpu_ctx, oracle, instr):
    """The bounds clip succeeds and maxt > mint fails: retired by ray_interval, not by
    aabb_clip's answer."""
    sc, it = scenes.build('C1', width=40, height=16, spp=3, rfilter='box')
    sc.sensor.farClip = 5.0          # the box begins 8 units from the camera
    st, retired, _ = _early(gpu_ctx, oracle, sc, it, instr, geometric=False)
    assert retired == st['samples'] == st['rays'] == 40 * 16 * 3


@gpu
@INSTR
def test_crop_inside_the_box(gpu_ctx, oracle, instr):
    # (the window ends below the sampler's resolution of 32: film positions are not wrapped)
    sc, it = scenes.build('C1', width=40, height=24, spp=3, rfilter='box')
    it.crop = (10, 2, 20, 20)
    st, retired, (lower, upper, _, _) = _early(gpu_ctx, oracle, sc, it, instr)
    assert upper == 0 and retired == 0 and st['rays'] > st['samples']


# ---- record modes --------------------------------------------------------------------------
@gpu
@INSTR
def test_alpha_output(gpu_ctx, oracle, instr):
    """L.has_alpha: a retired record carries alpha 0 (1 without it)."""
    sc, _ = scenes.build('C1', width=40, height=16, spp=3, rfilter='box')
    it = PathIntegrator(sampleCount=3, rfilter='box', hasAlpha=True)
    keep = _Keep(oracle)
    _check(gpu_ctx, keep, sc, it, instr)
    smp = keep.last[1]
    black = (smp[:, :3] == 0).all(axis=1) & (smp[:, 6] == 1)
    assert gpu_ctx.debug_counters()[RETIRED] > 0
    assert (smp[black, 3] == 0).sum() >= gpu_ctx.debug_counters()[RETIRED]   # the misses among them: alpha 0
    _early(gpu_ctx, oracle, sc, it, instr)


@gpu
@INSTR
@pytest.mark.parametrize('spp', [3, 4])
def test_gaussian_gather(gpu_ctx, oracle, spp, instr):
    sc, it = scenes.build('C1', width=40, height=16, spp=spp, rfilter='gaussian')
    _, _, (lower, upper, _, n) = _early(gpu_ctx, oracle, sc, it, instr)
    assert 0 < lower and upper < n


@gpu
@INSTR
def test_box_of_radius_one_spills(gpu_ctx, oracle, monkeypatch, instr):
    """Every retired sample still adds its weight to its neighbours' spill film."""
    monkeypatch.setenv('MTSGPU_ROUND_SHIFT', '1')
    sc, it = scenes.build('C1', width=40, height=16, spp=3, rfilter='box')
    it.rfilterParam = 1.0
    it.crop = (3, 1, 35, 14)
    _, _, (lower, upper, _, n) = _early(gpu_ctx, oracle, sc, it, instr)
    assert 0 < lower and upper < n


@gpu
def test_render_device(gpu_ctx, oracle):
    import torch
    sc, it = scenes.build('C1', width=40, height=16, spp=5, rfilter='box')
    gpu_ctx.upload(sc)
    b = film_border(it.rfilter, it.rfilterParam)
    film = torch.zeros((16 + 2 * b, 40 + 2 * b, 5), dtype=torch.float32, device='cuda')
    st_d = gpu_ctx.render_device(it, film.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    c = gpu_ctx.debug_counters()
    film_o, smp_o, st_o = oracle.render(sc, it, samples=True, libm_mode=0)
    lower, upper, black, n = retired_bounds(sc, smp_o)
    assert c[PASSES] > 0 and 0 < lower <= c[RETIRED] <= min(upper, black) and upper < n
    assert np.array_equal(_bits(film.cpu().numpy()), _bits(film_o))
    for k in COUNTERS:
        assert st_d[k] == st_o[k], (k, st_d[k], st_o[k])


# ---- integrators, samplers, launch settings ------------------------------------------------
@gpu
@INSTR
def test_volpath(gpu_ctx, oracle, instr):
    sc, _ = scenes.build('C1', width=40, height=16, spp=3, rfilter='box')
    it = VolpathIntegrator(sampleCount=3, rfilter='box', strictNormals=True)
    _early(gpu_ctx, oracle, sc, it, instr)


@gpu
@INSTR
def test_max_depth_one(gpu_ctx, oracle, instr):
    sc, it = scenes.build('C1', width=40, height=16, spp=3, rfilter='box', max_depth=1)
    st, _, (lower, _, _, _) = _early(gpu_ctx, oracle, sc, it, instr)
    assert lower > 0 and st['path_length_sum'] == st['samples']


@gpu
@INSTR
def test_independent_sampler(gpu_ctx, oracle, instr):
    sc, _ = scenes.build('C1', width=40, height=16, spp=4, rfilter='box')
    it = PathIntegrator(sampleCount=5, rfilter='box', sampler='independent')
    _, _, (lower, upper, _, n) = _early(gpu_ctx, oracle, sc, it, instr)
    assert 0 < lower and upper < n


@gpu
@pytest.mark.parametrize('lds_dims', [0, 1])
def test_sobol_reads_of_retired_samples(gpu_ctx, oracle, monkeypatch, lds_dims):
    """The film dimensions read from HBM (none, or only the first, staged in LDS): a
    retired sample counts the two it drew, as the loop without the queue counts them."""
    monkeypatch.setenv('MTSGPU_SOBOL_LDS_DIMS', str(lds_dims))
    sc, it = scenes.build('C1', width=40, height=16, spp=3, rfilter='box')
    _, retired, _ = _early(gpu_ctx, oracle, sc, it, True)
    reads = gpu_ctx.debug_counters()[SOBOL_WORDS]
    assert retired > 0 and reads > 0
    monkeypatch.setenv('MTSGPU_NO_SCAN', '1')
    gpu_ctx.render(it, samples=True)
    c = gpu_ctx.debug_counters()
    assert c[PASSES] == 0 and c[SOBOL_WORDS] == reads, (c[SOBOL_WORDS], reads)


@gpu
@INSTR
@pytest.mark.parametrize('rfilter,size,spp,chunk', [('box', (280, 64), 7, 3), ('gaussian', (192, 40), 9, 4)])
def test_three_launches(gpu_ctx, oracle, monkeypatch, rfilter, size, spp, chunk, instr):
    monkeypatch.setenv('MTSGPU_CONTRIB_BYTES', str(BUDGET))
    sc, it = scenes.build('C1', width=size[0], height=size[1], spp=spp, rfilter=rfilter)
    n = ((size[0] + 7) // 8) * ((size[1] + 7) // 8) * 64
    assert chunk == BUDGET // (n * (32 if rfilter == 'gaussian' else 16)) and (spp + chunk - 1) // chunk == 3
    _, _, (lower, upper, _, total) = _early(gpu_ctx, oracle, sc, it, instr)
    assert gpu_ctx.launch_chunks() == 3 and 0 < lower and upper < total


@gpu
@INSTR
@pytest.mark.parametrize('row,tile_shard', SHARDS, ids=SHARD_IDS)
def test_every_shard_setting(gpu_ctx, oracle, monkeypatch, row, tile_shard, instr):
    monkeypatch.setenv('MTSGPU_ROUND_SHIFT', '1')
    sc, it = scenes.build('C1', width=56, height=16, spp=3, rfilter='box')
    _early(gpu_ctx, oracle, sc, it, instr, row, tile_shard)


# ---- launches that retire nothing ----------------------------------------------------------
@gpu
@INSTR
def test_constant_emitter_retires_nothing(gpu_ctx, oracle, instr):
    """Under an environment emitter a camera miss is not black: the ENV kernel queues
    every real sample."""
    sc, it = scenes.build('C1', width=40, height=16, spp=3, rfilter='box')
    sc.emitters = list(sc.emitters) + [Emitter('constant', radiance=(0.3, 0.4, 0.5))]
    keep = _Keep(oracle)
    st = _check(gpu_ctx, keep, sc, it, instr)
    v, c = gpu_ctx.kernel_variant(), gpu_ctx.debug_counters()
    assert v['scene_lds'] and v['feat'] & 1 and c[PASSES] > 0 and c[RETIRED] == 0
    smp = keep.last[1]
    assert ((smp[:, 6] == 1) & (smp[:, :3] > 0).all(axis=1)).any()   # camera misses that see the emitter


@gpu
@INSTR
def test_launches_without_the_queue(gpu_ctx, oracle, monkeypatch, instr):
    """MTSGPU_NO_SCAN=1 and the SFMT replay keep the loop without the queue."""
    sc, it = scenes.build('C1', width=40, height=16, spp=3, rfilter='box')
    its = PathIntegrator(sampleCount=3, rfilter='box', sampler='independent-sfmt')
    _check(gpu_ctx, oracle, sc, its, instr)
    c = gpu_ctx.debug_counters()
    assert gpu_ctx.kernel_variant()['scene_lds'] and c[PASSES] == 0 and c[RETIRED] == 0
    monkeypatch.setenv('MTSGPU_NO_SCAN', '1')
    _check(gpu_ctx, oracle, sc, it, instr)
    c = gpu_ctx.debug_counters()
    assert gpu_ctx.kernel_variant()['scene_lds'] and c[PASSES] == 0 and c[RETIRED] == 0


@gpu
@INSTR
def test_variant_without_early_miss(gpu_ctx, oracle, instr):
    """The A/B library built with -DMTSG_EARLY_MISS=0 (make variant V=no_early), where
    present: the same film and counters, nothing retired."""
    from mitsuba_amd import LIB_PATH
    from mitsuba_amd.integrator import Context
    sc, it = scenes.build('C1', width=40, height=16, spp=3, rfilter='box')
    gpu_ctx.upload(sc)
    film_q, smp_q, st_q = gpu_ctx.render(it, samples=instr)
    assert gpu_ctx.debug_counters()[RETIRED] > 0
    lib = os.path.join(os.path.dirname(LIB_PATH), 'variants', 'libmtsgpu_no_early.so')
    if os.path.exists(lib):
        ctx = Context(lib_path=lib)
        ctx.upload(sc)
        film_v, smp_v, st_v = ctx.render(it, samples=instr)
        c = ctx.debug_counters()
        ctx.close()
        assert c[PASSES] > 0 and c[RETIRED] == 0
        assert np.array_equal(_bits(film_q), _bits(film_v))
        if instr:
            assert np.array_equal(_bits(smp_q), _bits(smp_v))
        for k in COUNTERS:
            assert st_q[k] == st_v[k], (k, st_q[k], st_v[k])
