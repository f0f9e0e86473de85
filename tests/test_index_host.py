"""The index arithmetic the kernels share with the host (csrc/layout.h), run on the
host through mtsgpu_index_host / mtsgpu_lookup_host (no device):

* the megakernel carries (sample run, compact pixel) from run to run instead of
  dividing the item index (mtsg_run_init / mtsg_run_step), and pixel_of divides by
  the launch's tiles_x and row_block with a multiply-high and one correction
  (mtsg_divmod).  Both must give what Python's divmod gives, for every (lane, round).
* sobol::look_up through tables that hold the GF(2) inverse already applied
  (mtsg_lut_word / sobol_lookup_lds) must give the oracle's index.
"""
import itertools
import json
import os

import numpy as np
import pytest

from mitsuba_amd.integrator import index_host, lookup_host

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the item -> pixel rule restated with Python integers -------------------------------
def geometry(window, row, tile_shard):
    """(compact pixels, tiles across) of a launch (render_plan.cpp launch_geometry)."""
    _, _, w, h = window
    rb, rs_, _ = max(row[0], 1), max(row[1], 1), row[2]
    tiles_x = (w + 7) // 8
    if tile_shard:
        tiles = tiles_x * ((h + 7) // 8)
        return (tiles + rs_ - 1) // rs_ * 64, tiles_x
    rows = ((h + rb - 1) // rb + rs_ - 1) // rs_ * rb
    return tiles_x * ((rows + 7) // 8) * 64, tiles_x


def pixel_of(window, row, tile_shard, pix):
    """(px, py) of compact pixel pix, or None for a padding pixel."""
    x0, y0, w, h = window
    rb, rstride = max(row[0], 1), max(row[1], 1)
    phase = row[2] % rstride
    tiles_x = (w + 7) // 8
    tile, inn = pix >> 6, pix & 63
    if tile_shard:
        ty, tx = divmod(tile * rstride + phase, tiles_x)
        lx, ly = tx * 8 + (inn & 7), ty * 8 + (inn >> 3)
    else:
        ty, tx = divmod(tile, tiles_x)
        lx, r = tx * 8 + (inn & 7), ty * 8 + (inn >> 3)
        blk, off = divmod(r, rb)
        ly = (blk * rstride + phase) * rb + off
    if lx >= w or ly >= h:
        return None
    return x0 + lx, y0 + ly


def expected(window, row, tile_shard, spp, shift, lanes, lane, rnd):
    """The row mtsgpu_index_host must return for item `rnd` of `lane`."""
    P, _ = geometry(window, row, tile_shard)
    jq, pix = divmod(lane + (rnd >> shift) * lanes, P)
    if (jq << shift) >= spp:
        return (0, 0, 0, 0, 0, 0)
    jj = (jq << shift) + (rnd & ((1 << shift) - 1))
    xy = pixel_of(window, row, tile_shard, pix) if jj < spp else None
    return (1, jj, pix) + ((xy[0], xy[1], 1) if xy else (0, 0, 0))


WINDOWS = [(3, 5, 13, 11), (16, 8, 8, 8)]
ROWS = [((1, 1, 0), False), ((8, 4, 3), False), ((2, 3, 1), False), ((8, 3, 2), True)]
LANES = [192, 200, 256, 2048]   # 192, 200: lanes % num_pixels != 0; 2048: more lanes than items


@pytest.mark.parametrize('window', WINDOWS)
@pytest.mark.parametrize('row,tile_shard', ROWS)
def test_every_lane_and_round_matches_divmod(window, row, tile_shard):
    P, tiles_x = geometry(window, row, tile_shard)
    inside = sum(pixel_of(window, row, tile_shard, p) is not None for p in range(P))   # the shard's window pixels
    for spp, shift, lanes in itertools.product((1, 3, 5), (0, 1, 2), LANES):
        runs = -(-spp // (1 << shift))                       # sample runs per pixel
        rounds = (-(-P * runs // lanes) + 1) << shift         # past every lane's last item
        lr = np.array([(g, r) for g in range(lanes) for r in range(rounds + 1)], np.uint32)
        got, info = index_host(window, lr, row=row, tile_shard=tile_shard, spp=spp, run_shift=shift, lanes=lanes)
        assert info == (P, tiles_x)
        want = np.array([expected(window, row, tile_shard, spp, shift, lanes, int(g), int(r)) for g, r in lr],
                        np.uint32)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (spp, shift, lanes, lr[bad[:3]], got[bad[:3]], want[bad[:3]])
        # every (pixel, sample) of the window is rendered exactly once
        done = got[got[:, 5] == 1]
        keys = (done[:, 1].astype(np.int64) * 65536 + done[:, 4]) * 65536 + done[:, 3]
        assert np.unique(keys).size == keys.size == inside * spp
        if row[1] == 1:
            assert inside == window[2] * window[3]


# two launches no GPU has to render: item indices beyond 2^32, and num_pixels = 2^26 + 64
BIG = [
    # 4096 x 4096: P = 2^24; 2^22 lanes, 1024 spp: q = lane + round * lanes reaches 2^34
    dict(window=(7, 9, 4096, 4096), row=(1, 1, 0), spp=1024, shift=0, lanes=1 << 22, rounds=4200, pixels=1 << 24,
         qmin=1 << 32),
    # 17 x 61681 tiles: P = 2^26 + 64; 2^19 lanes, runs of 2
    dict(window=(1, 2, 136, 493448), row=(1, 1, 0), spp=8, shift=1, lanes=1 << 19, rounds=1100,
         pixels=(1 << 26) + 64, qmin=0),
]


@pytest.mark.parametrize('g', BIG, ids=['q_beyond_2^32', 'pixels_2^26+64'])
def test_random_lanes_and_rounds_of_large_launches(g):
    P, _ = geometry(g['window'], g['row'], False)
    assert P == g['pixels']
    rng = np.random.RandomState(0x5EED)
    n = 100000
    lr = np.stack([rng.randint(0, g['lanes'], n), rng.randint(0, g['rounds'], n)], axis=1).astype(np.uint32)
    lr[:4] = [(0, 0), (g['lanes'] - 1, 0), (g['lanes'] - 1, g['rounds'] - 1), (0, g['rounds'] - 1)]
    got, _ = index_host(g['window'], lr, row=g['row'], spp=g['spp'], run_shift=g['shift'], lanes=g['lanes'])
    q = lr[:, 0].astype(np.uint64) + (lr[:, 1].astype(np.uint64) >> g['shift']) * g['lanes']
    assert int(q.max()) >= g['qmin']
    bad = []
    for i in range(n):
        want = expected(g['window'], g['row'], False, g['spp'], g['shift'], g['lanes'], int(lr[i, 0]), int(lr[i, 1]))
        if tuple(int(v) for v in got[i]) != want:
            bad.append((tuple(lr[i]), tuple(got[i]), want))
    assert not bad, bad[:3]
    assert got[:, 0].min() == 0 and got[:, 5].max() == 1   # some lanes had finished, some items render


# ---- sobol::look_up through the folded tables -------------------------------------------
SCRAMBLES = [0, 0x9E3779B97F4A7C15, 0x0123456789ABCDEF ^ 0xF0F0F0F00F0F0F0F]


@pytest.mark.parametrize('m', range(1, 13))
def test_folded_lookup_matches_oracle(oracle, m):
    L = oracle.lib()
    rng = np.random.RandomState(1000 + m)
    res = 1 << m
    if m <= 5:
        q = np.array([(x, y, j) for y in range(res) for x in range(res) for j in (0, 1, 2, 3, 7, 100, 65535, (1 << 20) + 5)],
                     np.uint32)
    else:
        q = np.stack([rng.randint(0, res, 100000), rng.randint(0, res, 100000), rng.randint(0, 1 << 20, 100000)],
                     axis=1).astype(np.uint32)
    for scr in SCRAMBLES:
        got = lookup_host(m, scr, q)
        want = np.array([L.oracle_sobol_lookup(m, int(j), int(x), int(y), scr) for x, y, j in q], np.uint64)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (m, hex(scr), q[bad[:3]], got[bad[:3]], want[bad[:3]])


def test_folded_lookup_matches_recorded_indices():
    gold = json.load(open(os.path.join(HERE, 'golden', 'sobol_golden.json')))['lookups']
    assert len(gold) > 1000
    for m, frame, px, py, scr, value in gold:
        assert int(lookup_host(m, scr, [(px, py, frame)])[0]) == value, (m, frame, px, py, scr)


# ---- the unit face normals staged with an LDS scene -------------------------------------
def _face_normal_f32(c):
    """fill_hit's operation sequence (dhit.h) in numpy float32: cross as dmath.h forms it,
    the length by a correctly rounded sqrt, its reciprocal, three products; zero stays zero."""
    f = np.float32
    a, b = c[1] - c[0], c[2] - c[0]
    n = np.array([f(a[1] * b[2]) - f(a[2] * b[1]), f(a[2] * b[0]) - f(a[0] * b[2]), f(a[0] * b[1]) - f(a[1] * b[0])], f)
    length = np.sqrt(f(f(f(n[0] * n[0]) + f(n[1] * n[1])) + f(n[2] * n[2])))
    if not (n == 0).all():
        with np.errstate(divide='ignore', over='ignore', invalid='ignore'):
            n = n * f(f(1.0) / length)
    return n.astype(f)


def _degenerate_and_sliver_scene():
    from mitsuba_amd import scenes
    from mitsuba_amd.scene import Mesh
    sc, _ = scenes.build('C1', width=8, height=8, spp=1)
    degen = Mesh(np.array([[0.5, 0.5, 0.5], [1.0, 1.0, 1.0], [1.5, 1.5, 1.5]], np.float32),
                 np.array([[0, 1, 2]], np.uint32), bsdf=0, faceNormals=True)
    sliver = Mesh(np.array([[0.25, 0.3, 0.4], [0.252, 0.3, 0.4], [0.25, 0.301, 0.4]], np.float32),   # area 1e-6
                  np.array([[0, 1, 2]], np.uint32), bsdf=0, faceNormals=True)
    sc.meshes = list(sc.meshes[:-1]) + [degen, sliver, sc.meshes[-1]]
    return sc


def test_face_normal_table_is_fill_hits_operation_sequence():
    from mitsuba_amd import scenes
    from mitsuba_amd.integrator import face_normals_host
    c1, _ = scenes.build('C1', width=8, height=8, spp=1)
    sc = _degenerate_and_sliver_scene()
    for scene in (c1, sc):
        nrm, cor = face_normals_host(scene)
        assert nrm.shape[0] == scene.num_triangles >= 30
        want = np.array([_face_normal_f32(c) for c in cor], np.float32)
        assert np.array_equal(nrm.view(np.uint32), want.view(np.uint32)), np.argwhere(nrm.view(np.uint32) != want.view(np.uint32))[:4]
    # the degenerate triangle (collinear, dyadic coordinates: its cross product is exactly zero)
    zero = np.nonzero((nrm == 0).all(axis=1))[0]
    assert zero.size == 1 and np.array_equal(cor[zero[0], 0], np.float32([0.5, 0.5, 0.5]))
    sliver = np.nonzero(np.isclose(cor[:, 0, 0], 0.25) & np.isclose(cor[:, 0, 1], 0.3))[0]
    assert sliver.size == 1 and abs(np.linalg.norm(nrm[sliver[0]].astype(np.float64)) - 1.0) < 1e-6
