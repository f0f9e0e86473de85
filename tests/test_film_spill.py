"""The film order taken when gather mode is off, and the gather order at other widths, on
the CPU: the numpy restatements the GPU tests compare with (tests/film_ref.py
spill_film_ref, tests/test_film_gather.py gather_ref) must equal the oracle's film bit for
bit, and the exactness certificate of spill_film_ref must cover the share of the film that
tests/test_gpu_filter_widths.py compares bit for bit.

C1 at 40 x 36: two 32-pixel blocks in each direction, so footprints are clipped by the
block bitmap (imageblock.h:124-204) inside the frame as well as at its edge."""
import numpy as np
import pytest

from film_ref import Rendered, spill_film_ref
from mitsuba_amd import scenes
from test_film_gather import gather_ref

W, H = 40, 36
EDGE_CROP = (0, 5, 37, 29)
# (rfilter, box radius / gaussian stddev, spp)
FALLBACK = [('gaussian', 0.1, 3), ('gaussian', 1.13, 3), ('gaussian', 1.5, 2),
            ('box', 0.3, 3), ('box', 1.0, 3), ('box', 1.5, 3)]
IDS = ['%s_%g' % c[:2] for c in FALLBACK]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _scene(rfilter, param, spp, crop=None):
    sc, it = scenes.build('C1', width=W, height=H, spp=spp, rfilter=rfilter)
    it.rfilterParam = param
    it.crop = crop
    return sc, it


_REF = {}


def _case(oracle, rfilter, param, spp, crop):
    """(oracle film, spill_film_ref of the oracle's records), made once per session."""
    key = (rfilter, param, spp, crop)
    if key not in _REF:
        sc, it = _scene(rfilter, param, spp, crop)
        film, smp, _ = oracle.render(sc, it, samples=True, threads=8)
        ref = spill_film_ref(smp, spp, crop or (0, 0, W, H), W, H, rfilter, param, oracle)
        film.setflags(write=False)
        _REF[key] = (film, ref)
    return _REF[key]


@pytest.mark.parametrize('crop', [None, EDGE_CROP], ids=['full', 'edge_crop'])
@pytest.mark.parametrize('rfilter,param,spp', FALLBACK, ids=IDS)
def test_oracle_film_equals_spill_order(oracle, rfilter, param, spp, crop):
    film, ref = _case(oracle, rfilter, param, spp, crop)
    mine = ref.film()
    assert mine.shape == film.shape
    bad = np.argwhere(_bits(film) != _bits(mine))
    assert bad.size == 0, (len(bad), bad[:4].tolist(), film[tuple(bad[0])], mine[tuple(bad[0])])
    assert np.count_nonzero(film[..., 4]) > 0


@pytest.mark.parametrize('row,tile_shard', [((2, 3, 1), False), ((8, 3, 2), True)], ids=['row2of3', 'tiles3'])
@pytest.mark.parametrize('rfilter,param', [('box', 1.5), ('gaussian', 1.13)])
def test_oracle_shard_film_equals_spill_order(oracle, rfilter, param, row, tile_shard):
    """Row blocks and 8x8 tiles of a shard: the other pixels' records contribute nothing."""
    sc, it = _scene(rfilter, param, 3)
    film, smp, _ = oracle.render(sc, it, samples=True, threads=8, row=row, tile_shard=tile_shard)
    ref = spill_film_ref(smp, 3, (0, 0, W, H), W, H, rfilter, param, oracle, shard=Rendered(row, tile_shard))
    assert np.array_equal(_bits(film), _bits(ref.film()))
    whole = _case(oracle, rfilter, param, 3, None)[0]
    assert 0 < film[..., 4].sum() < 0.6 * whole[..., 4].sum()


def test_the_cases_are_the_ones_meant(oracle):
    """H = max(border, floor(radius + 1/2)) of each filter, and what it implies."""
    def hb(rfilter, param):
        radius, _, b, _ = oracle.filter_table(rfilter, param)
        return max(b, int(np.floor(np.float32(radius) + np.float32(0.5)))), b
    assert [hb('gaussian', s) for s in (0.1, 0.2, 0.5, 0.8, 1.0, 1.13, 1.5)] == \
        [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (6, 6)]
    assert [hb('box', r)[1] for r in (0.3, 0.5, 1.0, 1.5)] == [0, 1, 1, 2]
    # box 0.3 covers no pixel centre for some samples, and then the sample leaves no weight
    film, ref = _case(oracle, 'box', 0.3, 3, None)
    assert film.shape == (H, W, 5) and 0 < np.count_nonzero(film[..., 4] == 0) < W * H and not ref.count.any()
    # the wide gaussians send most of their weight through the spill film
    for param, spp, fp in ((1.13, 3, 121), (1.5, 2, 169)):
        _, ref = _case(oracle, 'gaussian', param, spp, None)
        assert ref.count[..., 4].max() > spp * fp // 2


@pytest.mark.parametrize('rfilter,param,spp', [c for c in FALLBACK if c[0] == 'box' or c[1] == 0.1],
                         ids=[i for c, i in zip(FALLBACK, IDS) if c[0] == 'box' or c[1] == 0.1])
def test_certificate_covers_narrow_filters(oracle, rfilter, param, spp):
    for crop in (None, EDGE_CROP):
        _, ref = _case(oracle, rfilter, param, spp, crop)
        assert ref.certified.all()


@pytest.mark.parametrize('param,spp', [(1.13, 3), (1.5, 2)])
def test_certificate_covers_most_of_a_wide_gaussian(oracle, param, spp):
    """Not a tolerance: the share of film pixels that the GPU test compares bit for bit
    must not shrink to nothing.  (Measured: 1920 of 2300 and 2021 of 2496.)"""
    _, ref = _case(oracle, 'gaussian', param, spp, None)
    pixels = ref.certified.all(axis=-1)
    assert 4 * pixels.sum() >= 3 * pixels.size, (int(pixels.sum()), pixels.size)
    assert not pixels.all()     # and the uncertified rest is there to be checked with the bound


def test_certificate_arithmetic():
    """Three contributions 1, 2^-30 and 2^-52: q = -52 and the sum is below 2^1, certified
    (the sum has 53 significant bits); with 2^-54 the bound 2^-1 fails, and the exact sum
    is no double."""
    class Table:
        @staticmethod
        def filter_table(rfilter, param):
            v = np.zeros(32, np.float32)
            v[:] = 1.0
            return 1.5, np.float32(32 / 1.5), 1, v
    for tiny, ok in ((2.0 ** -52, True), (2.0 ** -54, False)):
        rec = np.zeros((9 * 1, 8), np.float32)
        rec[:, 4] = np.tile(np.arange(3), 3) + 0.5
        rec[:, 5] = np.repeat(np.arange(3), 3) + 0.5
        rec[0, 0], rec[1, 0], rec[2, 0] = 1.0, 2.0 ** -30, tiny
        ref = spill_film_ref(rec, 1, (0, 0, 3, 3), 3, 3, 'box', 1.0, Table)
        # film pixel (2, 2) = image pixel (1, 1) takes all nine samples, eight of them as spills
        assert ref.count[2, 2, 4] == 8 and ref.count[2, 2, 0] == 3
        assert bool(ref.certified[2, 2, 0]) == ok
        assert ref.spill[2, 2, 0] == 1.0 + 2.0 ** -30 + (tiny if ok else 0.0)   # the exact sum, rounded to double
        assert ref.certified[..., 4].all()


@pytest.mark.parametrize('crop', [None, EDGE_CROP], ids=['full', 'edge_crop'])
@pytest.mark.parametrize('param', [0.2, 1.0])
def test_oracle_gather_equals_numpy_order_at_other_widths(oracle, param, crop):
    """H = 1 and H = 4 (H = 2 and 3: tests/test_film_gather.py)."""
    sc, it = _scene('gaussian', param, 3, crop)
    win = crop or (0, 0, W, H)
    film, smp, _ = oracle.render(sc, it, samples=True, threads=8)
    ref = gather_ref(smp, 3, win, W, H, 'gaussian', param, oracle)
    bad = np.argwhere(_bits(film) != _bits(ref))
    assert bad.size == 0, (len(bad), bad[:4].tolist())


def test_spill_order_differs_from_gather_order(oracle):
    """What lets a film tell which order it was summed in (stddev 0.8, H = 3)."""
    sc, it = _scene('gaussian', 0.8, 3)
    film, smp, _ = oracle.render(sc, it, samples=True, threads=8)
    other = spill_film_ref(smp, 3, (0, 0, W, H), W, H, 'gaussian', 0.8, oracle).film()
    assert np.count_nonzero(np.any(_bits(film) != _bits(other), axis=-1)) > film.shape[0] * film.shape[1] // 2
    assert np.allclose(film, other, rtol=1e-5, atol=0)
