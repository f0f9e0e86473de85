"""Launch- and triangle-invariant work hoisted out of the megakernel's loop must not
change a bit (dmega.h, dpath.h, layout.h):

* the sample-run index carried from run to run and pixel_of's multiply-high
  divisions, at windows with padding pixels, every row / tile shard setting, odd
  sample counts under runs of two (the held splat pair) and a crop off the origin;
* sobol::look_up through the folded tables (megakernel, wavefront engine, `direct`);
* the unit face normals staged with an LDS scene (hits, the flip against opposing
  vertex normals, the area-light sample, a degenerate triangle);
* the one-emitter shortcut, and that two lights do not take it.

Each test is one small render compared with the oracle: per-sample records
(value, alpha, sx, sy, depth, flags), film and counters, bit for bit.
"""
import numpy as np
import pytest

from mitsuba_amd import scenes
from mitsuba_amd.scene import BSDF, DirectIntegrator, Emitter, Mesh

pytestmark = pytest.mark.gpu

COUNTERS = ('samples', 'rays', 'shadow_rays', 'path_length_sum')
# (row_block, row_stride, row_phase), tile shards
SHARDS = [((1, 1, 0), False), ((8, 4, 3), False), ((2, 3, 1), False), ((8, 3, 2), True)]
SHARD_IDS = ['rows', 'row8of4', 'row2of3', 'tiles3']


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(gpu_ctx, oracle, sc, it, instr, row=(1, 1, 0), tile_shard=False, engine=None):
    """One GPU render against the oracle's.  instr: the instrumented kernels, whose
    per-sample records are compared too; else the kernels the benchmark times."""
    gpu_ctx.upload(sc)
    film_g, smp_g, st_g = gpu_ctx.render(it, samples=instr, row=row, tile_shard=tile_shard, engine=engine)
    film_o, smp_o, st_o = oracle.render(sc, it, samples=True, libm_mode=0, row=row, tile_shard=tile_shard)
    if instr:
        same = np.all(_bits(smp_g) == _bits(smp_o), axis=1)
        bad = np.nonzero(~same)[0]
        assert same.all(), (bad.size, same.size, bad[:3], smp_g[bad[:2]], smp_o[bad[:2]])
    diff = np.argwhere(_bits(film_g) != _bits(film_o))
    assert diff.size == 0, (len(diff), diff[:4])
    for k in COUNTERS:
        assert st_g[k] == st_o[k], (k, st_g[k], st_o[k])
    return st_g   # (rows 8 of 4, phase 3 of these windows: every compact pixel is padding, nothing is rendered)


@pytest.fixture
def runs_of_two(monkeypatch):
    """Sample runs of two (tiny scenes take them only with many runs per lane): the
    held splat pair, and with an odd sample count a run's missing second sample."""
    monkeypatch.setenv('MTSGPU_ROUND_SHIFT', '1')


@pytest.mark.parametrize('instr', [True, False], ids=['instr', 'plain'])
@pytest.mark.parametrize('spp', [3, 5])
@pytest.mark.parametrize('row,tile_shard', SHARDS, ids=SHARD_IDS)
def test_box_window_with_padding(gpu_ctx, oracle, runs_of_two, row, tile_shard, spp, instr):
    sc, it = scenes.build('C1', width=24, height=20, spp=spp, rfilter='box')
    it.crop = (5, 4, 13, 11)
    _check(gpu_ctx, oracle, sc, it, instr, row, tile_shard)


@pytest.mark.parametrize('instr', [True, False], ids=['instr', 'plain'])
@pytest.mark.parametrize('spp', [3, 5])
@pytest.mark.parametrize('row,tile_shard', SHARDS, ids=SHARD_IDS)
def test_gaussian_window_gather(gpu_ctx, oracle, row, tile_shard, spp, instr):
    sc, it = scenes.build('C1', width=32, height=24, spp=spp, rfilter='gaussian')
    it.crop = (6, 3, 20, 12)
    _check(gpu_ctx, oracle, sc, it, instr, row, tile_shard)


def _tie_scene(it_cls=None):
    """The Cornell box with every face of the short block twice (exact-t ties) and a
    degenerate triangle, as tests/test_gpu_scan.py builds it; 16 x 16, 4 spp."""
    sc, it = scenes.build('C1', width=16, height=16, spp=4, rfilter='box')
    short = sc.meshes[5]
    sc.bsdfs = list(sc.bsdfs) + [BSDF('diffuse', reflectance=(0.1, 0.3, 0.9))]
    dup = Mesh(short.positions.copy(), short.indices.copy(), bsdf=len(sc.bsdfs) - 1, faceNormals=True)
    p = np.array([[0.5, 0.5, 0.5], [1.0, 1.0, 1.0], [1.5, 1.5, 1.5]], np.float32)
    degen = Mesh(p, np.array([[0, 1, 2]], np.uint32), bsdf=0, faceNormals=True)
    sc.meshes = list(sc.meshes) + [dup, degen]
    return sc, it


def _opposed_normals_scene():
    """The back wall with vertex normals that oppose its face normal: fill_hit flips
    the geometric normal towards the shading normal."""
    sc, it = scenes.build('C1', width=16, height=16, spp=4, rfilter='box')
    back = sc.meshes[2]
    P, I = np.asarray(back.positions, np.float32), np.asarray(back.indices, np.uint32)
    n = np.cross(P[I[0, 1]] - P[I[0, 0]], P[I[0, 2]] - P[I[0, 0]])
    n = (-n / np.linalg.norm(n)).astype(np.float32)
    sc.meshes = list(sc.meshes)
    sc.meshes[2] = Mesh(P.copy(), I.copy(), normals=np.tile(n, (P.shape[0], 1)), bsdf=back.bsdf)
    return sc, it


def _two_lights_scene():
    sc, it = scenes.build('C1', width=16, height=16, spp=4, rfilter='box')
    light = sc.meshes[-1]
    P = np.asarray(light.positions, np.float32)
    ext = P.max(0) - P.min(0)
    P2 = (P + np.array([1.2 * ext[0], 0.0, 0.0], np.float32)) * np.array([1.0, 0.98, 1.0], np.float32)
    sc.emitters = list(sc.emitters) + [Emitter('area', radiance=(3.0, 5.0, 9.0))]
    sc.meshes = list(sc.meshes) + [Mesh(P2.astype(np.float32), np.asarray(light.indices, np.uint32).copy(), bsdf=-1,
                                        emitter=1, faceNormals=True)]
    return sc, it


SCENES = {'ties_degenerate': _tie_scene, 'opposed_normals': _opposed_normals_scene, 'two_lights': _two_lights_scene}


@pytest.mark.parametrize('instr', [True, False], ids=['instr', 'plain'])
@pytest.mark.parametrize('name', sorted(SCENES))
def test_lds_scene_face_normals_and_emitters(gpu_ctx, oracle, name, instr):
    sc, it = SCENES[name]()
    assert sc.num_triangles <= 64   # staged in LDS and scanned
    _check(gpu_ctx, oracle, sc, it, instr)
    assert gpu_ctx.kernel_variant()['scene_lds']


def test_wavefront_engine_shares_the_lookup(gpu_ctx, oracle):
    sc, it = _tie_scene()
    _check(gpu_ctx, oracle, sc, it, True, engine='wavefront')
    assert gpu_ctx.kernel_variant() is None


def test_direct_integrator_shares_the_lookup(gpu_ctx, oracle):
    sc, _ = _tie_scene()
    it = DirectIntegrator(sampleCount=4, rfilter='box', rfilterParam=0.5, shadingSamples=2)
    _check(gpu_ctx, oracle, sc, it, True)
