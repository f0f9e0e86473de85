"""numpy restatement of the film order taken when gather mode is off (box filters, gaussians
with H = 0 or H > MTSG_GATHER_HMAX, MTSGPU_NO_GATHER): dfilm.h film_splat + film_reduce +
film_finalize on the GPU, film_put in the oracle.

Per film value the sum has two parts:

* own: the contributions of the pixel's own samples, summed in float32 in sample order;
* spill: every other contribution, summed in double in whatever order the atomics land
  and rounded to float32 once; here the exact sum (math.fsum).

The film is float32(own + float32(spill)).  A double total does not depend on the order
only while every partial sum is exact; `certified` marks the film values for which that is
proven: with q the smallest exponent of a lowest set mantissa bit over the value's non-zero
contributions, sum|c| < 2^(q + 53) makes every partial sum of every order a multiple of 2^q
below 2^(q + 53), hence exact.

Footprint and weights as ImageBlock::put (imageblock.h:124-204) with the discretised
filter of rfilter.cpp:37-55; everything here is float32 unless it says double.
"""
import math

import numpy as np

f32 = np.float32
BLOCK = 32


class Rendered:
    """The pixels of a w x h window that a (row_block, row_stride, row_phase) shard renders
    (row blocks, or 8x8 tiles t % stride == phase with tile_shard): the `shard` argument of
    gather_ref (tests/test_film_gather.py) and of spill_film_ref."""

    def __init__(self, row=(0, 1, 0), tile_shard=False):
        self.block, self.stride, self.phase = row[0] or 1, row[1] or 1, row[2]
        self.tile_shard = tile_shard

    def pixels(self, w, h):
        ly, lx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
        if self.tile_shard:
            return ((ly // 8) * (-(-w // 8)) + lx // 8) % self.stride == self.phase
        return (ly // self.block) % self.stride == self.phase


class SpillFilm:
    """spill_film_ref's result, each array (H + 2b, W + 2b, 5): own float32, spill float64 (the
    exact sum, rounded to double once), sumabs float64 (sum |c| of the spill contributions),
    count (their number) and the boolean certificate."""

    def __init__(self, own, spill, sumabs, count, certified, border):
        self.own, self.spill, self.sumabs, self.count, self.certified, self.border = own, spill, sumabs, count, certified, border
        for a in (own, spill, sumabs, count, certified):
            a.setflags(write=False)

    def film(self):
        return (self.own + self.spill.astype(f32)).astype(f32)


def _lowest_bit_exponent(c):
    """Per float32 c != 0 the exponent e of its lowest set mantissa bit (c is an odd multiple of 2^e)."""
    bits = np.ascontiguousarray(c, f32).view(np.uint32).astype(np.int64)
    exp, man = (bits >> 23) & 0xff, bits & 0x7fffff
    m = np.where(exp == 0, man, man | 0x800000)
    e = np.where(exp == 0, -149, exp - 150)
    low = m & -m
    return e + np.round(np.log2(np.maximum(low, 1).astype(np.float64))).astype(np.int64)


def spill_film_ref(rec, spp, window, W, H, rfilter, param, ob, field=None, shard=None):
    """rec: the records of `window` = (x0, y0, w, h), row-major pixels, sample-minor.
    field None: path records (n, 8) {L.rgb, alpha, sx, sy, ..}; a sample with a negative or
    non-finite value is dropped whole, as ImageBlock::put does.  field f: field records
    (n, 4 + 3 nf) {sx, sy, alpha, hit, f0.rgb, ..}; nothing is dropped (the multichannel
    block does not warn).  shard: an object with pixels(w, h) (Rendered, TileSharding)."""
    radius, scale, b, values = ob.filter_table(rfilter, param)
    r32 = f32(radius)
    x0, y0, w, h = window
    fw, fh = W + 2 * b, H + 2 * b
    n = w * h * spp
    rec = np.asarray(rec, f32)
    assert rec.shape[0] == n, (rec.shape, n)
    py, px = np.meshgrid(np.arange(y0, y0 + h), np.arange(x0, x0 + w), indexing='ij')
    px, py = np.repeat(px.reshape(-1), spp), np.repeat(py.reshape(-1), spp)
    live = np.ones(n, bool) if shard is None else np.repeat(shard.pixels(w, h).reshape(-1), spp)
    one = np.ones((n, 1), f32)
    if field is None:
        val = np.concatenate([rec[:, 0:4], one], 1).astype(f32)
        sx, sy = rec[:, 4], rec[:, 5]
        live = live & np.all(np.isfinite(val) & (val >= 0), axis=1)
    else:
        val = np.concatenate([rec[:, 4 + 3 * field:7 + 3 * field], rec[:, 2:3], one], 1).astype(f32)
        sx, sy = rec[:, 0], rec[:, 1]
    bx, by = (px // BLOCK) * BLOCK, (py // BLOCK) * BLOCK
    bw = BLOCK + 2 * b
    posx = ((sx - f32(0.5)).astype(f32) - (bx - b).astype(f32)).astype(f32)
    posy = ((sy - f32(0.5)).astype(f32) - (by - b).astype(f32)).astype(f32)
    minx = np.maximum(np.ceil(posx - r32).astype(np.int64), 0)
    miny = np.maximum(np.ceil(posy - r32).astype(np.int64), 0)
    maxx = np.minimum(np.floor(posx + r32).astype(np.int64), bw - 1)
    maxy = np.minimum(np.floor(posy + r32).astype(np.int64), bw - 1)

    def disc(x):
        i = np.abs((x * scale).astype(f32)).astype(np.int64)
        return values[np.minimum(i, 31)]

    own = np.zeros((fh, fw, 5), f32)
    idx, con = [], []
    reach = int(math.floor(radius + 0.5)) + 1      # |film x - (px + b)| <= floor(radius + 1/2)
    for dy in range(-reach, reach + 1):
        for dx in range(-reach, reach + 1):
            gx, gy = px + b + dx, py + b + dy
            x, y = gx - bx, gy - by
            m = live & (x >= minx) & (x <= maxx) & (y >= miny) & (y <= maxy) & (gx < fw) & (gy < fh)
            if not m.any():
                continue
            assert abs(dx) < reach and abs(dy) < reach
            wgt = (disc(x.astype(f32) - posx) * disc(y.astype(f32) - posy)).astype(f32)
            c = (wgt[:, None] * val).astype(f32)
            if dx == 0 and dy == 0:
                for j in range(spp):               # sample order within each pixel
                    s = np.nonzero(m[j::spp])[0] * spp + j
                    own[gy[s], gx[s]] = (own[gy[s], gx[s]] + c[s]).astype(f32)
            else:
                s = np.nonzero(m)[0]
                idx.append(gy[s] * fw + gx[s])
                con.append(c[s])
    spill = np.zeros((fh * fw, 5), np.float64)
    sumabs = np.zeros((fh * fw, 5), np.float64)
    count = np.zeros((fh * fw, 5), np.int64)
    q = np.full((fh * fw, 5), 1 << 20, np.int64)
    if idx:
        idx = np.concatenate(idx)
        con = np.concatenate(con)
        order = np.argsort(idx, kind='stable')
        idx, con = idx[order], con[order]
        c64 = con.astype(np.float64)
        np.add.at(sumabs, idx, np.abs(c64))
        np.add.at(count, idx, (con != 0).astype(np.int64))
        np.minimum.at(q, idx, np.where(con != 0, _lowest_bit_exponent(np.where(con != 0, con, f32(1))), 1 << 20))
        starts = np.nonzero(np.diff(idx, prepend=-1))[0]
        ends = np.append(starts[1:], idx.size)
        for s, e in zip(starts, ends):
            seg = c64[s:e]
            spill[idx[s]] = [math.fsum(seg[:, k].tolist()) for k in range(5)]
    # (sumabs itself is a rounded double sum: 2^-40 covers its error many times over)
    certified = (count == 0) | (sumabs * (1.0 + 2.0 ** -40) < np.ldexp(1.0, np.minimum(q, 900) + 53))
    shape = (fh, fw, 5)
    return SpillFilm(own, spill.reshape(shape), sumabs.reshape(shape), count.reshape(shape), certified.reshape(shape), b)
