"""Shared numpy restatements for the field / multichannel tests (test_fields_host.py,
test_gpu_fields.py).  Everything is float32 with the reference's operation order; numpy
float32 arithmetic is IEEE single precision without contraction."""
import ctypes as C

import numpy as np

f32 = np.float32
BLOCK = 32


def _affine(m, x, y, z):
    """m00*x + m01*y + m02*z + m03 per row, left to right (transform.h:108-125)."""
    return [(((m[4 * r] * x).astype(f32) + (m[4 * r + 1] * y).astype(f32)).astype(f32)
             + (m[4 * r + 2] * z).astype(f32)).astype(f32) + m[4 * r + 3] for r in range(4)]


def xf_point(m16, p):
    """Transform::operator()(Point): the affine product, divided by w unless w == 1."""
    m = np.asarray(m16, f32).reshape(16)
    x, y, z = (np.asarray(p[..., i], f32) for i in range(3))
    X, Y, Z, Wc = (v.astype(f32) for v in _affine(m, x, y, z))
    with np.errstate(divide='ignore', invalid='ignore'):
        r = (f32(1) / Wc).astype(f32)
    one = Wc == f32(1)
    return np.stack([np.where(one, X, (X * r).astype(f32)), np.where(one, Y, (Y * r).astype(f32)),
                     np.where(one, Z, (Z * r).astype(f32))], -1).astype(f32)


def sample_to_camera(sc, ob):
    d = sc.desc()
    m = np.zeros(16, f32)
    dxdy = np.zeros(6, f32)
    fp = C.POINTER(C.c_float)
    assert ob.lib().oracle_camera(C.byref(d.sensor), m.ctypes.data_as(fp), dxdy.ctypes.data_as(fp)) == 0
    return m


def primary_rays(sc, ob, sx, sy):
    """PerspectiveCameraImpl::sampleRayDifferential (perspective.cpp:271-298) for the film
    positions (sx, sy): (o (n, 3), d (n, 3), mint (n,), maxt (n,)) float32."""
    s = sc.sensor
    m = sample_to_camera(sc, ob)
    sx, sy = np.asarray(sx, f32), np.asarray(sy, f32)
    irx, iry = f32(1) / f32(s.width), f32(1) / f32(s.height)
    near = xf_point(m, np.stack([(sx * irx).astype(f32), (sy * iry).astype(f32), np.zeros_like(sx)], -1))
    x, y, z = near[:, 0], near[:, 1], near[:, 2]
    ln = np.sqrt((((x * x).astype(f32) + (y * y).astype(f32)).astype(f32) + (z * z).astype(f32)).astype(f32)).astype(f32)
    r = (f32(1) / ln).astype(f32)                        # normalize = v / length: v * (1 / length)
    dl = np.stack([(x * r).astype(f32), (y * r).astype(f32), (z * r).astype(f32)], -1)
    inv_z = (f32(1) / dl[:, 2]).astype(f32)
    mint, maxt = (f32(s.nearClip) * inv_z).astype(f32), (f32(s.farClip) * inv_z).astype(f32)
    W = np.asarray(s.toWorld, f32).reshape(16)
    zero = np.zeros_like(sx)
    o = np.stack([v.astype(f32) for v in _affine(W, zero, zero, zero)[:3]], -1)
    d = np.stack([(((W[4 * k] * dl[:, 0]).astype(f32) + (W[4 * k + 1] * dl[:, 1]).astype(f32)).astype(f32)
                   + (W[4 * k + 2] * dl[:, 2]).astype(f32)).astype(f32) for k in range(3)], -1)
    return o.astype(f32), d.astype(f32), mint, maxt


def oracle_intersect(sc, ob, o, d):
    """oracle_intersect per ray: (n, 16) {valid, t, p, geoN, shN, s, shape, tri}."""
    desc = sc.desc()
    L = ob.lib()
    fp = C.POINTER(C.c_float)
    out = np.zeros((o.shape[0], 16), f32)
    o = np.ascontiguousarray(o, f32)
    d = np.ascontiguousarray(d, f32)
    for i in range(o.shape[0]):
        rc = L.oracle_intersect(C.byref(desc), o[i].ctypes.data_as(fp), d[i].ctypes.data_as(fp),
                                out[i].ctypes.data_as(fp))
        assert rc == 0
    return out


def prim_tables(sc):
    """Global primitive -> (shape index, index within the shape); analytic shapes are one primitive."""
    shape, local = [], []
    for i, m in enumerate(sc.meshes):
        n = 1 if m.analytic else len(m.indices)
        shape += [i] * n
        local += list(range(n))
    return np.asarray(shape, np.int64), np.asarray(local, np.int64)


def hit_uv(sc, hits):
    """its.uv of triangle hits {t, u, v, prim} (skdtree.h:398-405): t0*b.x + t1*b.y + t2*b.z
    with b = (1 - u - v, u, v), or (b.y, b.z) for a mesh without texcoords.  Rows of misses
    and of analytic shapes are NaN."""
    shape, local = prim_tables(sc)
    prim = hits[:, 3].view(np.uint32).astype(np.int64)
    uv = np.full((hits.shape[0], 2), np.nan, f32)
    u, v = hits[:, 1].astype(f32), hits[:, 2].astype(f32)
    bx = ((f32(1) - u).astype(f32) - v).astype(f32)
    for i, m in enumerate(sc.meshes):
        if m.analytic:
            continue
        sel = np.nonzero((prim < len(shape)) & (shape[np.minimum(prim, len(shape) - 1)] == i))[0]
        if not sel.size:
            continue
        if m.texcoords is None:
            uv[sel, 0], uv[sel, 1] = u[sel], v[sel]
            continue
        tri = np.asarray(m.indices)[local[prim[sel]]]
        tc = np.asarray(m.texcoords, f32)
        for c in range(2):
            t0, t1, t2 = tc[tri[:, 0], c], tc[tri[:, 1], c], tc[tri[:, 2], c]
            uv[sel, c] = (((t0 * bx[sel]).astype(f32) + (t1 * u[sel]).astype(f32)).astype(f32)
                          + (t2 * v[sel]).astype(f32)).astype(f32)
    return uv


def checker_is_color0(tex, u, v):
    """Checkerboard::eval (checkerboard.cpp) after Texture2D's uv transform (texture.cpp:112-121)."""
    uu = ((u * f32(tex.uscale)).astype(f32) + f32(tex.uoffset)).astype(f32)
    vv = ((v * f32(tex.vscale)).astype(f32) + f32(tex.voffset)).astype(f32)
    x = 2 * (np.trunc((uu * f32(2)).astype(f32)).astype(np.int64) % 2) - 1
    y = 2 * (np.trunc((vv * f32(2)).astype(f32)).astype(np.int64) % 2) - 1
    return x * y == 1


def _spec3(v):
    return np.asarray((v,) * 3 if np.isscalar(v) else v, f32)


def window_pixels(window, spp):
    """(px, py) of every record of a window render (row-major pixels, sample-minor)."""
    x0, y0, w, h = window
    py, px = np.meshgrid(np.arange(y0, y0 + h), np.arange(x0, x0 + w), indexing='ij')
    return np.repeat(px.reshape(-1), spp), np.repeat(py.reshape(-1), spp)


def box_film_ref(rec, nf, spp, window, W, H, ob, rendered=None):
    """The box-filter films of field records (n, 4 + 3 nf): per field a (H+2b, W+2b, 5) film
    {f.rgb, alpha, 1} * weight, each pixel's own samples summed in float32 in sample order
    (film_reduce), the rare splats into neighbouring pixels summed in double and rounded
    once (film_finalize).  Footprint and weights as ImageBlock::put (imageblock.h:124-204)."""
    radius, scale, b, values = ob.filter_table('box', 0.5)
    r32 = f32(radius)
    fw, fh = W + 2 * b, H + 2 * b
    px, py = window_pixels(window, spp)
    sx, sy, alpha = rec[:, 0], rec[:, 1], rec[:, 2]
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

    live = np.ones(px.shape, bool) if rendered is None else rendered
    own = np.zeros((nf, fh, fw, 5), f32)
    spill = np.zeros((nf, fh, fw, 5), np.float64)
    n = px.size
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            gx, gy = px + b + dx, py + b + dy
            x, y = gx - bx, gy - by
            m = live & (x >= minx) & (x <= maxx) & (y >= miny) & (y <= maxy) & (gx < fw) & (gy < fh)
            wgt = (disc(x.astype(f32) - posx) * disc(y.astype(f32) - posy)).astype(f32)
            for f in range(nf):
                val = np.concatenate([rec[:, 4 + 3 * f:7 + 3 * f], alpha[:, None], np.ones((n, 1), f32)], 1).astype(f32)
                c = (wgt[:, None] * val).astype(f32)
                if dx == 0 and dy == 0:
                    for j in range(spp):      # sample order within each pixel
                        s = np.nonzero(m[j::spp])[0] * spp + j
                        own[f, gy[s], gx[s]] = (own[f, gy[s], gx[s]] + c[s]).astype(f32)
                else:
                    s = np.nonzero(m)[0]
                    np.add.at(spill[f], (gy[s], gx[s]), c[s].astype(np.float64))
    return (own + spill.astype(f32)).astype(f32)


def gather_film_ref(rec, f, spp, window, W, H, rfilter, param, ob):
    """film_gather's order (tests/test_film_gather.py gather_ref) over the records of field f:
    for each sample index ascending, the (2H+1)^2 neighbourhood's source pixels in row-major
    order; no value is dropped (the multichannel block does not warn on negative values)."""
    radius, scale, b, values = ob.filter_table(rfilter, param)
    r32 = f32(radius)
    Hh = max(b, int(np.floor(f32(radius) + f32(0.5))))
    x0, y0, w, h = window
    fw, fh = W + 2 * b, H + 2 * b
    film = np.zeros((fh, fw, 5), f32)
    r = rec.reshape(h, w, spp, rec.shape[1])
    gy, gx = np.meshgrid(np.arange(max(0, y0 + b - Hh), min(fh, y0 + h + b + Hh)),
                         np.arange(max(0, x0 + b - Hh), min(fw, x0 + w + b + Hh)), indexing='ij')
    acc = np.zeros(gx.shape + (5,), f32)
    bw = BLOCK + 2 * b

    def disc(x):
        i = np.abs((x * scale).astype(f32)).astype(np.int64)
        return values[np.minimum(i, 31)]

    for j in range(spp):
        for dy in range(-Hh, Hh + 1):
            for dx in range(-Hh, Hh + 1):
                qx, qy = gx - b + dx, gy - b + dy
                lx, ly = qx - x0, qy - y0
                m = (lx >= 0) & (ly >= 0) & (lx < w) & (ly < h)
                q = r[np.clip(ly, 0, h - 1), np.clip(lx, 0, w - 1), j]
                sx, sy = q[..., 0].astype(f32), q[..., 1].astype(f32)
                bx, by = (np.maximum(qx, 0) // BLOCK) * BLOCK, (np.maximum(qy, 0) // BLOCK) * BLOCK
                posx = (sx - f32(0.5)) - (bx - b).astype(f32)
                posy = (sy - f32(0.5)) - (by - b).astype(f32)
                minx = np.maximum(np.ceil(posx - r32).astype(np.int64), 0)
                miny = np.maximum(np.ceil(posy - r32).astype(np.int64), 0)
                maxx = np.minimum(np.floor(posx + r32).astype(np.int64), bw - 1)
                maxy = np.minimum(np.floor(posy + r32).astype(np.int64), bw - 1)
                x, y = gx - bx, gy - by
                m &= (x >= minx) & (x <= maxx) & (y >= miny) & (y <= maxy)
                wgt = (disc(x.astype(f32) - posx) * disc(y.astype(f32) - posy)).astype(f32)
                val = np.concatenate([q[..., 4 + 3 * f:7 + 3 * f], q[..., 2:3], np.ones_like(q[..., :1])], -1).astype(f32)
                acc = np.where(m[..., None], acc + wgt[..., None] * val, acc)
    film[gy, gx] = acc
    return film


def develop_multi_ref(films, border, formats, component_format):
    """Bitmap::convertMultiSpectrumAlphaWeight (bitmap.cpp:1617-1673) + the component
    conversion (oracle/film_oracle.py _conv): (N, H+2b, W+2b, 5) -> (H, W, C)."""
    from oracle.film_oracle import _conv
    b = int(border)
    fl = np.asarray(films, f32)[:, b:films.shape[1] - b, b:films.shape[2] - b]
    w = fl[0, ..., 4]
    with np.errstate(divide='ignore', invalid='ignore'):
        inv = np.where(w == 0, f32(0), f32(1) / w).astype(f32)
    alpha = (fl[0, ..., 3] * inv).astype(f32)
    out = []
    for i, fmt in enumerate(formats):
        v = [(fl[i, ..., k] * inv).astype(f32) for k in range(3)]
        if fmt in ('luminance', 'luminancealpha'):
            out.append(((v[0] * f32(0.212671)).astype(f32) + (v[1] * f32(0.715160)).astype(f32)).astype(f32)
                       + (v[2] * f32(0.072169)).astype(f32))
        elif fmt in ('rgb', 'rgba'):
            out += v
        else:
            for c0, c1, c2 in ((0.412453, 0.357580, 0.180423), (0.212671, 0.715160, 0.072169),
                               (0.019334, 0.119193, 0.950227)):
                out.append(((v[0] * f32(c0)).astype(f32) + (v[1] * f32(c1)).astype(f32)).astype(f32)
                           + (v[2] * f32(c2)).astype(f32))
        if fmt in ('luminancealpha', 'rgba', 'xyza'):
            out.append(alpha)
    with np.errstate(over='ignore', invalid='ignore'):
        return np.stack([_conv(c.astype(f32), component_format) for c in out], -1)
