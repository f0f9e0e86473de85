"""Shared pieces of the delta-emitter tests (test_delta_emitters_host.py,
test_gpu_delta_emitters.py): the test scenes, and float32 numpy restatements of
PointEmitter / SpotEmitter / DirectionalEmitter::sampleDirect and of the first
bounce of `path`, `volpath` and `direct` under one of them.

Everything is float32 in the reference's operation order (numpy float32 arithmetic is
IEEE single precision without contraction); cosf and acosf are glibc's, through ctypes."""
import copy
import ctypes as C
import ctypes.util

import numpy as np

import fields_ref as fr
from mitsuba_amd import scenes
from mitsuba_amd.scene import Emitter
from mitsuba_amd.transform import deg_to_rad

f32 = np.float32
EPSILON, SHADOW_EPSILON = f32(1e-4), f32(1e-3)      # constants.h:28-29

_libm = C.CDLL(ctypes.util.find_library('m') or 'libm.so.6')
for _n in ('cosf', 'acosf'):
    getattr(_libm, _n).restype = C.c_float
    getattr(_libm, _n).argtypes = [C.c_float]


def cosf(x):
    return f32(_libm.cosf(float(f32(x))))


def acosf(x):
    return np.array([_libm.acosf(float(v)) for v in np.asarray(x, f32).reshape(-1)], f32).reshape(np.shape(x))


def dot(a, b):
    return (((a[..., 0] * b[..., 0]).astype(f32) + (a[..., 1] * b[..., 1]).astype(f32)).astype(f32)
            + (a[..., 2] * b[..., 2]).astype(f32)).astype(f32)


def cross(a, b):
    return np.stack([((a[..., 1] * b[..., 2]).astype(f32) - (a[..., 2] * b[..., 1]).astype(f32)).astype(f32),
                     ((a[..., 2] * b[..., 0]).astype(f32) - (a[..., 0] * b[..., 2]).astype(f32)).astype(f32),
                     ((a[..., 0] * b[..., 1]).astype(f32) - (a[..., 1] * b[..., 0]).astype(f32)).astype(f32)], -1)


def length(a):
    return np.sqrt(dot(a, a)).astype(f32)


# ---- scenes ---------------------------------------------------------------------------------
def delta_scene(emitters, keep_area=False, materials='diffuse', width=32, height=32, spp=4, max_depth=2):
    """C1 with the ceiling light quad kept as geometry (white diffuse, emitter -1 unless
    keep_area) and `emitters` appended.  Returns (scene, integrator, twin): the twin is the
    same geometry with the quad emitting and no other emitter -- what the oracle, which
    cannot configure a delta emitter, intersects and traces (hits and occlusion do not
    depend on emission)."""
    sc, it = scenes.build('C1', width=width, height=height, spp=spp, materials=materials, max_depth=max_depth)
    sc.meshes[-1].bsdf = 0
    twin = copy.copy(sc)
    twin.meshes = list(sc.meshes)
    twin.emitters = list(sc.emitters)
    sc.meshes = [copy.copy(m) for m in sc.meshes]
    if keep_area:
        sc.emitters = list(sc.emitters) + list(emitters)
    else:
        sc.meshes[-1].emitter = -1
        sc.emitters = list(emitters)
    return sc, it, twin


def scene_bounds(sc):
    """The kd-tree AABB (gkdtree.h:1211-1217: the vertex bounds, slightly enlarged)."""
    p = np.concatenate([np.asarray(m.positions, f32).reshape(-1, 3) for m in sc.meshes])
    lo, hi = p.min(0).astype(f32), p.max(0).astype(f32)
    eps = f32(1e-3)
    d = (hi - lo).astype(f32)
    lo2 = (lo - ((d * eps).astype(f32) + eps).astype(f32)).astype(f32)
    d2 = (hi - lo2).astype(f32)                            # (min is moved before max is)
    hi2 = (hi + ((d2 * eps).astype(f32) + eps).astype(f32)).astype(f32)
    return lo2, hi2


# ---- sampleDirect ---------------------------------------------------------------------------
def sample_direct(em, sc, ref):
    """(value (n, 3), d (n, 3), dist (n,), pdf (n,), p (n, 3)) of em.sampleDirect at the points ref."""
    ref = np.asarray(ref, f32)
    n = ref.shape[0]
    I = np.asarray(em.radiance, f32)
    T = np.eye(4, dtype=f32) if em.toWorld is None else np.asarray(em.toWorld.m, f32)
    Ti = np.eye(4, dtype=f32) if em.toWorld is None else np.asarray(em.toWorld.inv, f32)
    if em.type == 'directional':                      # directional.cpp:159-180
        d = np.array([f32(f32(f32(T[r, 0] * f32(0)) + f32(T[r, 1] * f32(0))) + f32(T[r, 2] * f32(1))) for r in range(3)], f32)
        lo, hi = scene_bounds(sc)
        center = ((hi + lo).astype(f32) * f32(0.5)).astype(f32)
        radius = f32(length(center - hi) * f32(1.1))
        disk = (center - (d * radius).astype(f32)).astype(f32)
        distance = dot((ref - disk).astype(f32), np.broadcast_to(d, ref.shape))
        ok = ~(distance < 0)
        value = np.where(ok[:, None], I[None, :], f32(0)).astype(f32)
        p = (ref - (d[None, :] * distance[:, None]).astype(f32)).astype(f32)
        return value, np.broadcast_to(-d, ref.shape).astype(f32), distance, ok.astype(f32), p
    # point.cpp:131-147, spot.cpp:184-200: trafo.transformAffine(Point(0))
    pos = np.array([f32(f32(f32(f32(T[r, 0] * f32(0)) + f32(T[r, 1] * f32(0))) + f32(T[r, 2] * f32(0))) + T[r, 3])
                    for r in range(3)], f32)
    d = (pos[None, :] - ref).astype(f32)
    dist = length(d)
    inv = (f32(1) / dist).astype(f32)
    d = (d * inv[:, None]).astype(f32)
    inv2 = (inv * inv).astype(f32)
    if em.type == 'point':
        value = (I[None, :] * inv2[:, None]).astype(f32)
    else:
        nd = -d
        cos_t = (((Ti[2, 0] * nd[:, 0]).astype(f32) + (Ti[2, 1] * nd[:, 1]).astype(f32)).astype(f32)
                 + (Ti[2, 2] * nd[:, 2]).astype(f32)).astype(f32)
        beam, cutoff = deg_to_rad(em.beamWidth), deg_to_rad(em.cutoffAngle)     # spot.cpp:70-94
        cos_beam, cos_cut = cosf(beam), cosf(cutoff)
        inv_tw = f32(f32(1) / f32(cutoff - beam))
        trans = ((cutoff - acosf(cos_t)).astype(f32) * inv_tw).astype(f32)
        fall = np.where(cos_t <= cos_cut, f32(0), np.where(cos_t >= cos_beam, f32(1), (f32(1) * trans).astype(f32)))
        value = ((I[None, :] * fall[:, None].astype(f32)).astype(f32) * inv2[:, None]).astype(f32)
    return value, d, dist, np.ones(n, f32), np.broadcast_to(pos, ref.shape).astype(f32)


# ---- first bounce ---------------------------------------------------------------------------
def bsdf_eval(ob, desc, wi, wo):
    fp = C.POINTER(C.c_float)
    val = np.zeros((wi.shape[0], 3), f32)
    pdf = C.c_float(0)
    wi, wo = np.ascontiguousarray(wi, f32), np.ascontiguousarray(wo, f32)
    for i in range(wi.shape[0]):
        rc = ob.lib().oracle_bsdf_eval(C.byref(desc), wi[i].ctypes.data_as(fp), wo[i].ctypes.data_as(fp),
                                       val[i].ctypes.data_as(fp), C.byref(pdf), 0)
        assert rc == 0
    return val


def first_hits(sc, twin, ob, sx, sy):
    """The camera rays' first vertices from the oracle: dict of rd, valid, p, geoN, n, s, t, wi, shape."""
    from mitsuba_amd.scene import BSDF
    o, d, mint, maxt = fr.primary_rays(sc, ob, sx, sy)
    # oracle_intersect configures the scene for every ray: hand it the geometry alone (the hit
    # record, UV tangents included, does not depend on the BSDFs; roughplastic would load its
    # tables 4096 times)
    geo = copy.copy(twin)
    geo.bsdfs = [BSDF('diffuse') for _ in twin.bsdfs]
    h = fr.oracle_intersect(geo, ob, o, d)
    uv = fr.hit_uv(geo, ob.trace_rays(geo, o, d, mint, maxt))      # its.uv, for textured BSDFs
    n, s = h[:, 8:11].copy(), h[:, 11:14].copy()
    t = cross(n, s)                                        # skdtree.h:425-427
    nd = -d
    wi = np.stack([dot(nd, s), dot(nd, t), dot(nd, n)], -1)
    return dict(rd=d, valid=h[:, 0] != 0, p=h[:, 2:5].copy(), geoN=h[:, 5:8].copy(), n=n, s=s, t=t, wi=wi,
                shape=h[:, 14].astype(np.int64), uv=uv)


def mesh_bsdf_eval(ob, b, wi, wo, uv):
    """bsdf->eval(bRec) of BSDF object `b` for rows (wi, wo, uv), and whether it has a smooth
    component (BSDF::ESmooth: only then is an emitter sampled, path.cpp:171).  twosided
    (twosided.cpp:105-131): the nested BSDF of wi's side, both directions mirrored on the back;
    a checkerboard diffuseReflectance is resolved per row to its colour (checkerboard.cpp)."""
    import dataclasses
    from mitsuba_amd.scene import Checkerboard
    n = wi.shape[0]
    val = np.zeros((n, 3), f32)
    if b.type == 'twosided':
        flip = ~(wi[:, 2] > 0)
        smooth = np.zeros(n, bool)
        for side in (0, 1):
            m = flip == bool(side)
            if not m.any():
                continue
            nb = b.nested[min(side, len(b.nested) - 1)]
            sgn = np.array([1, 1, -1 if side else 1], f32)
            val[m], smooth[m] = mesh_bsdf_eval(ob, nb, (wi[m] * sgn).astype(f32), (wo[m] * sgn).astype(f32), uv[m])
        # (the wrapper's flags are the union of its nested BSDFs': smooth if either is)
        any_smooth = any(x.type not in ('conductor', 'dielectric') for x in b.nested)
        return val, np.full(n, any_smooth)
    if b.type in ('conductor', 'dielectric'):
        return val, np.zeros(n, bool)
    tex = getattr(b, 'diffuseReflectance', None) if b.type in ('plastic', 'roughplastic') else getattr(b, 'reflectance', None)
    if isinstance(tex, Checkerboard):
        is0 = fr.checker_is_color0(tex, uv[:, 0], uv[:, 1])
        key = 'diffuseReflectance' if b.type in ('plastic', 'roughplastic') else 'reflectance'
        for flag, col in ((True, tex.color0), (False, tex.color1)):
            m = is0 == flag
            if m.any():
                val[m] = bsdf_eval(ob, dataclasses.replace(b, **{key: tuple(fr._spec3(col))}).to_desc(), wi[m], wo[m])
        return val, np.ones(n, bool)
    return bsdf_eval(ob, b.to_desc(), wi, wo), np.ones(n, bool)


def first_bounce(sc, twin, ob, H, kind, em=None, em_pdf=None, pick=None, strict=False, lum_samples=1):
    """Li of every sample after the first vertex's emitter sample alone: `path` / `volpath` at
    maxDepth 2 and `direct` in a scene whose only emitters are delta emitters (no ray can hit
    one, so nothing else contributes).  em: the emitter, or with `pick` (n,) the emitters
    list indexed by it, em_pdf (n,) the pick's probability."""
    nS = H['p'].shape[0]
    ems = [em] if pick is None else em
    pick = np.zeros(nS, np.int64) if pick is None else pick
    value, d, dist, pdf, lp = (np.zeros((nS, 3), f32), np.zeros((nS, 3), f32), np.zeros(nS, f32), np.zeros(nS, f32),
                               np.zeros((nS, 3), f32))
    for k, e in enumerate(ems):
        m = pick == k
        if m.any():
            value[m], d[m], dist[m], pdf[m], lp[m] = sample_direct(e, sc, H['p'][m])
    if em_pdf is not None:                                 # scene.cpp:846-847: value /= emPdf
        value = (value * (f32(1) / em_pdf).astype(f32)[:, None]).astype(f32)
        dpdf = (pdf * em_pdf).astype(f32)
    else:
        dpdf = pdf
    wo = np.stack([dot(d, H['s']), dot(d, H['t']), dot(d, H['n'])], -1)
    bval = np.zeros((nS, 3), f32)
    smooth = np.zeros(nS, bool)
    for si, m in enumerate(sc.meshes):
        sel = np.nonzero(H['valid'] & (H['shape'] == si))[0]
        if sel.size:
            bval[sel], smooth[sel] = mesh_bsdf_eval(ob, sc.bsdfs[m.bsdf], H['wi'][sel], wo[sel], H['uv'][sel])
    snp = (dot(H['rd'], H['geoN']) * H['wi'][:, 2]).astype(f32)
    go = H['valid'].copy()
    if strict:                                             # path.cpp:164-166, volpath.cpp:214-221, direct.cpp:186-188
        go &= ~(snp > 0 if kind == 'volpath' else snp >= 0)
    use = go & smooth & (pdf != 0) & np.any(value != 0, 1) & np.any(bval != 0, 1)
    if strict:
        use &= (dot(H['geoN'], d) * wo[:, 2]).astype(f32) > 0
    if kind == 'direct':
        nl = lum_samples
        frac = f32(f32(nl) / f32(nl + (1 if nl == 1 else 2)))      # the tests' (1, 1) and (4, 2)
        pa = (dpdf * frac).astype(f32)
        with np.errstate(invalid='ignore', divide='ignore'):
            w = (((pa * pa).astype(f32) / ((pa * pa).astype(f32) + f32(0)).astype(f32)).astype(f32)
                 * f32(f32(1) / f32(nl))).astype(f32)
    else:
        pa = (dpdf * dpdf).astype(f32)
        with np.errstate(invalid='ignore', divide='ignore'):
            w = (pa / (pa + f32(0)).astype(f32)).astype(f32)
    c = (((value * bval).astype(f32)) * w[:, None]).astype(f32)
    # the shadow ray (scene.cpp:839-840), or volpath's segment to dRec.p (scene.cpp:619-626, p2OnSurface false)
    if kind == 'volpath':
        v = (lp - H['p']).astype(f32)
        rem = length(v)
        with np.errstate(invalid='ignore', divide='ignore'):
            sd = (v * (f32(1) / rem).astype(f32)[:, None]).astype(f32)
        maxt = (rem * f32(1)).astype(f32)
    else:
        sd, maxt = d, (dist * f32(f32(1) - SHADOW_EPSILON)).astype(f32)
    rays = np.zeros((nS, 8), f32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = H['p'], EPSILON, np.where(use[:, None], sd, f32(1)), maxt
    hits = np.zeros((nS, 4), f32)
    desc = twin.desc()
    fp = C.POINTER(C.c_float)
    sel = np.nonzero(use)[0]
    if sel.size:
        r = np.ascontiguousarray(rays[sel])
        h = np.zeros((sel.size, 4), f32)
        assert ob.lib().oracle_trace_rays(C.byref(desc), r.ctypes.data_as(fp), sel.size, 1, h.ctypes.data_as(fp)) == 0
        hits[sel] = h
    lit = use & (hits[:, 0] == 0)
    Li = np.zeros((nS, 3), f32)
    for _ in range(lum_samples if kind == 'direct' else 1):
        Li = np.where(lit[:, None], (Li + c).astype(f32), Li)
    return Li, dict(use=use, lit=lit, value=value, d=d, dist=dist, wo=wo, bval=bval)


def cos_theta_map(em, sc, H):
    """cosTheta of the spot's local direction at every first vertex (to place the beam and cutoff edges)."""
    _, d, _, _, _ = sample_direct(Emitter('point', intensity=(1, 1, 1), toWorld=em.toWorld), sc, H['p'])
    Ti = np.asarray(em.toWorld.inv, f32)
    nd = -d
    return (((Ti[2, 0] * nd[:, 0]).astype(f32) + (Ti[2, 1] * nd[:, 1]).astype(f32)).astype(f32)
            + (Ti[2, 2] * nd[:, 2]).astype(f32)).astype(f32)


# ---- energy against the oracle's proxy sphere -----------------------------------------------
# A uniformly radiant sphere of radius r and radiance I / (pi r^2) gives a receiver that sees
# all of it the irradiance of a point source I at its centre; the oracle renders that proxy
# (emitting sphere, cone sampling) where it cannot configure the point emitter.
PROXY_POS, PROXY_I, PROXY_R = (2.1, 4.4, 2.4), (30.0, 24.0, 12.0), 0.15
# The smallest sample count (multiples of 4 tried, 32 x 32 pixels, full depth) at which, with
# the oracle alone, proxy r against proxy r/2 under another scramble stays within 4 standard
# errors and a 5% intensity error misses by at least 8: z = 0.50 / 0.22 / 0.32 and
# 8.19 / 8.66 / 8.08 per channel (40 spp: 7.59 / 8.25 / 7.58 for the 5% error)
PROXY_SPP = 44


def point_scene(spp=PROXY_SPP, size=32, scramble=0):
    from mitsuba_amd.scene import Emitter as E
    sc, it, _ = delta_scene([E('point', intensity=PROXY_I, position=PROXY_POS)], width=size, height=size, spp=spp,
                            max_depth=-1)
    it.rfilter, it.scramble = 'box', scramble
    return sc, it


def proxy_scene(r, spp=PROXY_SPP, size=32, scramble=0):
    from mitsuba_amd.scene import Emitter as E, Mesh
    sc, it = point_scene(spp, size, scramble)
    k = float(f32(1) / f32(f32(np.pi) * f32(f32(r) * f32(r))))
    sc.emitters = [E('area', radiance=tuple(x * k for x in PROXY_I))]
    sc.meshes = sc.meshes + [Mesh(shape='sphere', center=PROXY_POS, radius=r, bsdf=-1, emitter=0)]
    return sc, it


def proxy_mask(sc, ob, r, size=32):
    """Pixels none of whose primary rays (a 9 x 9 grid over the pixel) passes within 1.1 r of the proxy's centre."""
    g = np.arange(9) / 8.0
    hit = np.zeros(size * size, bool)
    py, px = np.meshgrid(np.arange(size), np.arange(size), indexing='ij')
    for gy in g:
        for gx in g:
            o, d, _, _ = fr.primary_rays(sc, ob, (px.reshape(-1) + gx).astype(f32), (py.reshape(-1) + gy).astype(f32))
            oc = np.asarray(PROXY_POS, np.float64)[None, :] - o.astype(np.float64)
            t = (oc * d).sum(1)
            hit |= (oc * oc).sum(1) - t * t <= (1.1 * r) ** 2
    return ~hit


def image_mean(smp, keep, spp):
    """Per-channel mean over the kept pixels and its standard error from the per-sample records:
    the pixels are strata, each with its own sample variance."""
    v = smp[:, 0:3].astype(np.float64).reshape(keep.size, spp, 3)[keep]
    return v.mean((0, 1)), np.sqrt((v.var(1, ddof=1) / spp).sum(0)) / v.shape[0]


def z_score(a, b, scale=1.0):
    (ma, ea), (mb, eb) = a, b
    return np.abs(scale * ma - mb) / np.sqrt((scale * ea) ** 2 + eb ** 2)
