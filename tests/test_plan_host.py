"""The render plan without a device (mtsgpu_plan_host, integrator.plan_host): which kernel
runs, how many launches a render takes and which run length a launch gets, decided by
the functions the renders themselves run (csrc/render_plan.cpp plan_render, plan_launch,
plan_wavefront) and compared here with the restatements the GPU tests keep:

* the chunk arithmetic against tests/test_gpu_spp_chunks.py::chunk_plan;
* a launch's samples, grid and run length against tests/test_gpu_start_queue.py::queue_plan;
* the kernels of the benchmark configurations against
  tests/test_gpu_bench_kernels.py::KERNELS, decoded as Context.kernel_variant decodes
  debug counter 15;
* every environment switch that changes a decision; the parameter checks' codes and texts.

The issue's run-length case "384 px x 5 spp split as 3 + 2 through the budget" cannot be
formed: the library raises MTSGPU_CONTRIB_BYTES to 1 MiB, which holds 170 samples of 384
pixels.  The split is checked on the smallest frame the budget splits 3 + 2, 160 x 112
(17920 compact pixels, 65536 // 17920 = 3), by the same rule; 384 x 5 as one launch.

C4 and C5 configure in well under 10 s each on the host, so nothing is cached beyond the
scene objects (built once per configuration, read-only).
"""

import pytest

import bench
from mitsuba_amd import abi, scenes
from mitsuba_amd.integrator import MtsgpuError, kernel_variant_of, plan_host
from mitsuba_amd.scene import FIELDS, DirectIntegrator, PathIntegrator
from test_gpu_bench_kernels import KERNELS
from test_gpu_spp_chunks import BUDGET, chunk_plan
from test_gpu_start_queue import queue_plan

ENV = 'MTSGPU_CONTRIB_BYTES'
SWITCHES = ('MTSGPU_WF_HITREC', 'MTSGPU_NO_SCAN_PAIRS', 'MTSGPU_WF_SHADE_LDS_DIMS', 'MTSGPU_WF_GENERIC',
            'MTSGPU_ROUND_SHIFT', 'MTSGPU_NO_ONE_EMITTER', 'MTSGPU_NO_SCENE_LDS', 'MTSGPU_NO_SCAN',
            'MTSGPU_NO_DIFF_VARIANT', 'MTSGPU_NO_BSDF_SETS', 'MTSGPU_NO_REFN_SPEC', 'MTSGPU_WAVES', 'MTSGPU_NO_GATHER',
            'MTSGPU_SOBOL_LDS_DIMS', 'MTSGPU_CONTRIB_BYTES', 'MTSGPU_ENGINE', 'MTSGPU_WF_SLOTS')
SET_BITS = 16 | 32 | 64 | 256 | 512   # MTSG_FEAT_GGX | NORD | NORC | NOSTRICT | NOREFN (csrc/layout.h)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


_BENCH = {}


def _bench_scene(cfg):
    if cfg not in _BENCH:
        _BENCH[cfg] = bench.build_scene(cfg)
    return _BENCH[cfg]


def _cornell(size, spp, gaussian=False):
    return scenes.build('C1', width=size[0], height=size[1], spp=spp, rfilter='gaussian' if gaussian else 'box')


# ---- chunk arithmetic ----------------------------------------------------------------------
CHUNK_ROWS = [((160, 112), 7, False, 1), ((192, 128), 5, False, 1), ((96, 80), 9, True, 1), ((160, 112), 3, True, 1),
              ((96, 80), 5, False, 3), ((96, 80), 3, True, 3), ((96, 80), 3, False, 8)]
SHARD_ROWS = [((0, 3, 1), True), ((8, 3, 2), False), ((0, 1, 0), False)]


@pytest.mark.parametrize('size,spp,gaussian,films', CHUNK_ROWS)
def test_chunks_match_chunk_plan(monkeypatch, size, spp, gaussian, films):
    sc, it = _cornell(size, spp, gaussian)
    fields = list(FIELDS[:films]) if films > 1 else None
    chunk, launches, pixels = chunk_plan(size, spp, gaussian, films)
    monkeypatch.setenv(ENV, str(BUDGET))
    p = plan_host(sc, it, fields=fields)
    assert (p['pixels'], p['chunk'], p['launches']) == (pixels, chunk, launches)
    assert p['engine'] == ('fields' if fields else 'megakernel') and p['gather'] == gaussian
    assert [cs for cs, _, _ in p['launch']] == [min(chunk, spp - j0) for j0 in range(0, spp, chunk)]
    monkeypatch.delenv(ENV)
    p = plan_host(sc, it, fields=fields, free_bytes=0)
    assert (p['pixels'], p['chunk'], p['launches']) == (pixels, spp, 1)


@pytest.mark.parametrize('row,tile_shard', SHARD_ROWS, ids=['tiles', 'rows', 'whole'])
def test_sharded_chunks_match_chunk_plan(monkeypatch, row, tile_shard):
    sc, it = _cornell((192, 260), 7)
    chunk, launches, pixels = chunk_plan((192, 260), 7, False, row=row, tile_shard=tile_shard)
    monkeypatch.setenv(ENV, str(BUDGET))
    p = plan_host(sc, it, row=row, tile_shard=tile_shard)
    assert (p['pixels'], p['chunk'], p['launches']) == (pixels, chunk, launches)
    monkeypatch.delenv(ENV)
    assert plan_host(sc, it, row=row, tile_shard=tile_shard)['launches'] == 1


def test_free_memory_sets_the_budget():
    """A quarter of the free bytes above 8 GiB, at most 32 GiB; C5's 15 GB of records: one launch."""
    sc, it = _bench_scene('C5')
    per_sample = 1280 * 720 * 16
    assert plan_host(sc, it)['chunk'] == (8 << 30) // per_sample
    assert plan_host(sc, it, free_bytes=200 << 30)['launches'] == 1
    assert plan_host(sc, it, free_bytes=40 << 30)['chunk'] == (10 << 30) // per_sample


# ---- run length and grid -------------------------------------------------------------------
def _rule_shift(cs, items, lanes, lds=True):
    """queue_plan's run-length rule (its `shift is None` branch), large scenes start at 6."""
    s = 1 if lds else 6
    while s > 0 and ((1 << s) > cs or ((items // lanes) >> s) < 100):
        s -= 1
    return s


def _check_launches(p, n, spp, chunk, cus=256, shift=None):
    assert p['pixels'] == n and p['chunk'] == chunk and p['start_queue']
    total = 0
    for i, j0 in enumerate(range(0, spp, chunk)):
        cs, grid, s = p['launch'][i]
        items = min(chunk, spp - j0) * n
        blocks = max(1, -(-items // 256))
        assert blocks <= cus and (cs, grid) == (min(chunk, spp - j0), blocks)
        assert s == (_rule_shift(cs, items, blocks * 256) if shift is None else shift)
        total += queue_plan(n, cs, cus, shift=s)
    assert len(p['launch']) == i + 1 == p['launches']
    assert total == queue_plan(n, spp, cus, shift=shift, chunk=chunk)   # the production passes of the whole render


@pytest.mark.parametrize('size,spp', [((8, 8), 1), ((24, 16), 5)], ids=['64x1', '384x5'])
def test_launches_match_queue_plan(monkeypatch, size, spp):
    sc, it = _cornell(size, spp)
    n = size[0] * size[1]
    _check_launches(plan_host(sc, it, cus=256), n, spp, spp)
    for env, shift in (('0', 0), ('1', 1), ('9', 6)):   # 9 clamps to 6
        monkeypatch.setenv('MTSGPU_ROUND_SHIFT', env)
        _check_launches(plan_host(sc, it, cus=256), n, spp, spp, shift=shift)


def test_split_launches_match_queue_plan(monkeypatch):
    """5 spp split as 3 + 2 through the 1 MiB budget (the module docstring has the frame's choice)."""
    sc, it = _cornell((160, 112), 5)
    monkeypatch.setenv(ENV, str(BUDGET))
    p = plan_host(sc, it, cus=256)
    assert [cs for cs, _, _ in p['launch']] == [3, 2]
    _check_launches(p, 17920, 5, 3)
    monkeypatch.setenv('MTSGPU_ROUND_SHIFT', '1')
    _check_launches(plan_host(sc, it, cus=256), 17920, 5, 3, shift=1)


def test_grid_is_capped_by_the_resident_blocks():
    sc, it = _cornell((160, 112), 7)
    p = plan_host(sc, it, cus=8)
    assert p['launch'] == [(7, 8 * p['waves'], p['launch'][0][2])]
    assert plan_host(sc, it, cus=8, blocks_per_cu=2)['launch'][0][1] == 16


# ---- the bench kernels ---------------------------------------------------------------------
# DESIGN.md 4, render_plan.cpp run_shift.  The issue lists C1 with C2 and C2g at 1; by the rule as it
# stood before the planner (unchanged here) C1 gets 0: 512 x 512 x 64 samples over 256 CUs x 4 blocks x
# 256 lanes are 64 per lane, and runs of two would leave 32 < MTSG_MIN_RUNS = 100 of them.  The 1 was
# tools/prof_run.py's restatement (full_frame_shift named C1 an LDS scene and stopped there).
FULL_FRAME_SHIFT = {'C1': 0, 'C2': 1, 'C2g': 1, 'C3': 4, 'C5': 5}


@pytest.mark.parametrize('cfg', ['C1', 'C2', 'C2g', 'C3', 'C4', 'C5'])
def test_bench_kernels(cfg):
    sc, it = _bench_scene(cfg)
    p = plan_host(sc, it, row=(8, 1, 0), tile_shard=True, cus=256, free_bytes=200 << 30)
    assert p['engine'] == 'megakernel' and p['variant']['name'] == KERNELS[cfg]
    assert p['variant'] == kernel_variant_of(p['variant_word']) and not p['variant']['instr']
    assert p['launches'] == 1 and p['waves'] == 4
    if cfg in FULL_FRAME_SHIFT:
        assert p['launch'][0][2] == FULL_FRAME_SHIFT[cfg]
    q = plan_host(sc, it, row=(8, 1, 0), tile_shard=True, cus=256, samples=True, free_bytes=200 << 30)
    assert q['variant']['name'] == KERNELS[cfg].replace('<false', '<true', 1)


# ---- switches ------------------------------------------------------------------------------
def test_no_scene_lds(monkeypatch):
    sc, it = _cornell((40, 24), 4)
    p = plan_host(sc, it)
    assert p['scene_lds'] and p['variant']['scene_lds'] and p['scan'] and p['start_queue']
    monkeypatch.setenv('MTSGPU_NO_SCENE_LDS', '1')
    q = plan_host(sc, it)
    assert not q['scene_lds'] and not q['variant']['scene_lds'] and not q['scan'] and not q['start_queue']


def test_no_scan(monkeypatch):
    sc, it = _cornell((40, 24), 4)
    monkeypatch.setenv('MTSGPU_NO_SCAN', '1')
    q = plan_host(sc, it)
    assert q['scene_lds'] and not q['scan'] and not q['start_queue']


def test_no_bsdf_sets(monkeypatch):
    sc, it = _bench_scene('C4')
    assert plan_host(sc, it)['variant']['feat'] & SET_BITS
    monkeypatch.setenv('MTSGPU_NO_BSDF_SETS', '1')
    assert plan_host(sc, it)['variant']['feat'] & SET_BITS == 0


def test_no_gather(monkeypatch):
    sc, it = _cornell((40, 24), 4, gaussian=True)
    p = plan_host(sc, it)
    assert p['gather'] and p['gather_h'] == 2
    monkeypatch.setenv('MTSGPU_NO_GATHER', '1')
    q = plan_host(sc, it)
    assert not q['gather'] and q['gather_h'] == 0


def test_waves_and_sobol_lds_dims(monkeypatch):
    sc, it = _cornell((40, 24), 4)
    assert plan_host(sc, it)['waves'] == 4 and plan_host(sc, it)['lds_dims'] == 32
    monkeypatch.setenv('MTSGPU_WAVES', '3')
    p = plan_host(sc, it)
    assert p['waves'] == 3 and p['variant']['waves'] == 3
    monkeypatch.setenv('MTSGPU_SOBOL_LDS_DIMS', '5000')
    assert plan_host(sc, it)['lds_dims'] == 1024


def test_engines(monkeypatch):
    sc, it = _cornell((40, 24), 4)
    monkeypatch.setenv('MTSGPU_ENGINE', 'wavefront')
    p = plan_host(sc, it)
    assert p['engine'] == 'wavefront' and p['variant_word'] == 1 << 16 and p['variant'] is None
    assert p['wf_slots'] == 40 * 24 * 4 and p['launch'] == [(4, 0, 0)]
    assert plan_host(sc, it, engine='megakernel')['engine'] == 'megakernel'   # the flag wins
    monkeypatch.setenv('MTSGPU_ENGINE', 'megakernel')
    assert plan_host(sc, it)['engine'] == 'megakernel'
    assert plan_host(sc, it, engine='wavefront')['engine'] == 'wavefront'
    monkeypatch.setenv('MTSGPU_WF_SLOTS', '1000')
    assert plan_host(sc, it, engine='wavefront')['wf_slots'] == 1024   # whole blocks
    for lds in (True, False):
        if not lds:
            monkeypatch.setenv('MTSGPU_NO_SCENE_LDS', '1')
        f = plan_host(sc, it, fields=['position', 'uv', 'albedo'])
        assert f['engine'] == 'fields' and f['variant_word'] == (1 << 17) | (int(lds) << 12) and f['scene_lds'] == lds


# ---- errors --------------------------------------------------------------------------------
def _params(sc, it, window=None):
    W, H = sc.sensor.width, sc.sensor.height
    x0, y0, w, h = window or (0, 0, W, H)
    return it.params(W, H, x0, y0, w, h, 0, 1, 0)


def _fails(sc, p, text, fields=None):
    with pytest.raises(MtsgpuError) as e:
        plan_host(sc, None, fields=fields, params=p)
    assert e.value.code == abi.EINVAL and str(e.value) == 'EINVAL (-1): ' + text


def test_errors_are_the_renders():
    sc, it = _cornell((40, 24), 4)
    p = _params(sc, it)
    p.spp = 0
    _fails(sc, p, 'sampleCount must be positive')
    p = _params(sc, it)
    p.rr_depth = 0
    _fails(sc, p, "'rrDepth' must be set to a value greater than zero!")
    _fails(sc, _params(sc, it, (8, 0, 40, 24)), 'render window exceeds the film')
    p = _params(sc, it)
    p.sampler = 99
    _fails(sc, p, 'unknown sampler')
    _fails(sc, _params(sc, PathIntegrator(sampleCount=4, rfilter='box', sampler='independent-sfmt')),
           "field pass: the SFMT replay samplers' draw positions depend on how many numbers the radiance "
           "integrator consumed; a separate pass cannot reproduce the sample positions", fields=['position'])
    p = _params(sc, DirectIntegrator(sampleCount=4, rfilter='box'))
    p.emitter_samples = p.bsdf_samples = 0
    _fails(sc, p, 'direct: emitterSamples + bsdfSamples must be positive')
    big, itb = scenes.build('C1', width=65536, height=65536, spp=1 << 21, rfilter='box')
    _fails(big, _params(big, itb), 'sample index exceeds the 52-bit Sobol direction numbers')
    # the order of the checks: the sample count before the window, the window before the sampler
    p = _params(sc, it, (8, 0, 40, 24))
    p.sampler = 99
    _fails(sc, p, 'render window exceeds the film')
    p.spp = 0
    _fails(sc, p, 'sampleCount must be positive')
