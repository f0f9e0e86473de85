"""Shared pieces of the combinator-BSDF tests (test_combo_host.py, test_gpu_combo.py): the test
materials and scenes, and float32 numpy restatements of mixturebsdf / blendbsdf / mask / twosided
eval(), pdf() and sample(bRec, pdf, sample) composed from the oracle's leaf entry points
(oracle_bsdf_eval, oracle_bsdf_sample), of DiscreteDistribution (pmf.h), and of the first two
vertices of `path` / `volpath` under a point light.

Everything is float32 in the reference's operation order (mixturebsdf.cpp:115-277,
blendbsdf.cpp:101-270, mask.cpp:94-219, twosided.cpp:108-185); numpy float32 arithmetic is
IEEE single precision without contraction.  The leaves of the combinators here carry no
textures (oracle_bsdf_eval evaluates at uv = 0); the combinators' own weight / opacity may be
a checkerboard, resolved per row."""
import copy
import ctypes as C

import numpy as np

import delta_ref as dr
import fields_ref as fr
from mitsuba_amd.scene import BSDF, Checkerboard, Emitter

f32 = np.float32
F_NULL, F_DELTA = 0x1, 0x1 | 0x20 | 0x40      # BSDF::ENull, EDelta (bsdf.h)
EPSILON, SHADOW_EPSILON = dr.EPSILON, dr.SHADOW_EPSILON
POINT = dict(intensity=(30.0, 24.0, 12.0), position=(2.1, 4.4, 2.4))


# ---- materials ------------------------------------------------------------------------------
def leaves():
    return dict(d=BSDF('diffuse', reflectance=(0.5, 0.4, 0.3)),
                d2=BSDF('diffuse', reflectance=(0.2, 0.6, 0.7)),
                rc=BSDF('roughconductor', distribution='ggx', alpha=0.2, material='Au'),
                rp=BSDF('roughplastic', distribution='ggx', alpha=0.15, diffuseReflectance=(0.1, 0.3, 0.7)),
                pl=BSDF('plastic', diffuseReflectance=(0.7, 0.6, 0.2)))


def checker(lo, hi):
    return Checkerboard(color0=lo, color1=hi, uscale=3.0, vscale=3.0)


def cases():
    """The nine materials of the eval / sample restatements (the issue's list)."""
    L = leaves()
    mix3 = BSDF('mixturebsdf', weights=[0.5, 0.9, 0.6], nested=[L['d'], L['rc'], L['rp']])
    return {
        'blend03': BSDF('blendbsdf', weight=0.3, nested=[L['d'], L['rc']]),
        'blend_chk': BSDF('blendbsdf', weight=checker(0.2, 0.8), nested=[L['d2'], L['rc']]),
        'mix3': mix3,
        'mix2': BSDF('mixturebsdf', weights=[0.2, 0.3], nested=[L['d'], L['rc']]),
        'mask': BSDF('mask', opacity=(0.2, 0.5, 0.8), nested=[L['d']]),
        'mask_chk': BSDF('mask', opacity=checker((0.1, 0.2, 0.3), (0.9, 0.8, 0.7)), nested=[L['rc']]),
        'twosided_mix': BSDF('twosided', nested=[copy.deepcopy(mix3)]),
        'mask_twosided_blend': BSDF('mask', opacity=0.7, nested=[BSDF('twosided', nested=[
            BSDF('blendbsdf', weight=0.3, nested=[L['d2'], L['rc']])])]),
        'blend_rc_plastic': BSDF('blendbsdf', weight=0.54, nested=[L['rc'], L['pl']]),
    }


STRICT_CASES = ('mix3', 'mask_chk')      # strictNormals on for two of the nine


def all_surfaces(sc, bsdf):
    """Every mesh of the scene but the light quad carries `bsdf` (texture coordinates: the
    mesh's own, or the barycentrics)."""
    sc.bsdfs = [bsdf]
    sc.meshes = [copy.copy(m) for m in sc.meshes]
    for m in sc.meshes:
        if m.bsdf >= 0:
            m.bsdf = 0
    return sc


def point_scene(bsdf, max_depth, size=32, spp=4):
    """C1 (UV'd 'smooth' geometry: texture coordinates on the walls) under a point light, every
    surface `bsdf`; (scene, twin): the twin is the geometry the oracle intersects."""
    sc, _, twin = dr.delta_scene([Emitter('point', **POINT)], materials='smooth', width=size, height=size, spp=spp,
                                 max_depth=max_depth)
    all_surfaces(sc, bsdf)
    twin = all_surfaces(copy.copy(twin), BSDF('diffuse'))
    return sc, twin


# ---- DiscreteDistribution (pmf.h) and MixtureBSDF::configure ---------------------------------
def mixture_configure(weights, ensure=True):
    """(m_weights, m_pdf's CDF) as configure() leaves them (mixturebsdf.cpp:123-170, pmf.h:52-114)."""
    w = np.asarray(weights, f32).copy()
    total = f32(0)
    for x in w:
        total = f32(total + x)
    if ensure and total > 1:
        scale = f32(f32(1) / total)
        w = (w * scale).astype(f32)
    cdf = np.zeros(len(w) + 1, f32)
    for i, x in enumerate(w):
        cdf[i + 1] = f32(cdf[i] + x)
    norm = f32(f32(1) / cdf[-1])
    cdf[1:] = (cdf[1:] * norm).astype(f32)
    cdf[-1] = f32(1)
    return w, cdf


def sample_reuse(cdf, u):
    """DiscreteDistribution::sampleReuse (pmf.h:124-169): (index, reused sample, m_pdf[index])."""
    n = len(cdf) - 1
    idx = int(np.searchsorted(cdf, u, side='left')) - 1       # std::lower_bound
    idx = min(n - 1, max(0, idx))
    while f32(cdf[idx + 1] - cdf[idx]) == 0 and idx < n - 1:
        idx += 1
    p = f32(cdf[idx + 1] - cdf[idx])
    return idx, f32(f32(u - cdf[idx]) / p), p


# ---- leaves through the oracle ---------------------------------------------------------------
_FP = C.POINTER(C.c_float)
# The leaf queries are memoised on (BSDF, arguments): the integrators, and twosided_mix and
# mix3 on the front side, ask the same ones (a roughplastic query loads its tables anew each time)
_memo = {}


def leaf_eval_pdf(ob, b, wi, wo):
    """(eval (3,), pdf) of leaf `b` in the solid-angle measure."""
    key = ('e', repr(b), np.asarray(wi, f32).tobytes(), np.asarray(wo, f32).tobytes())
    if key not in _memo:
        _memo[key] = _leaf_eval_pdf(ob, b, wi, wo)
    return _memo[key]


def _leaf_eval_pdf(ob, b, wi, wo):
    val = np.zeros(3, f32)
    pdf = C.c_float(0)
    d = b.to_desc()
    wi, wo = np.ascontiguousarray(wi, f32), np.ascontiguousarray(wo, f32)
    assert ob.lib().oracle_bsdf_eval(C.byref(d), wi.ctypes.data_as(_FP), wo.ctypes.data_as(_FP), val.ctypes.data_as(_FP),
                                     C.byref(pdf), 0) == 0
    return val, f32(pdf.value)


def leaf_sample(ob, b, wi, sx, sy):
    """(wo, weight, pdf, eta, sampledType) of leaf `b`'s sample(bRec, pdf, sample)."""
    key = ('s', repr(b), np.asarray(wi, f32).tobytes(), float(sx), float(sy))
    if key not in _memo:
        _memo[key] = _leaf_sample(ob, b, wi, sx, sy)
    return _memo[key]


def _leaf_sample(ob, b, wi, sx, sy):
    L = ob.lib()
    L.oracle_bsdf_sample.restype = C.c_int
    wo, w = np.zeros(3, f32), np.zeros(3, f32)
    pdf, eta = C.c_float(0), C.c_float(1)
    d = b.to_desc()
    wi = np.ascontiguousarray(wi, f32)
    u3 = np.array([sx, sy, 0], f32)
    st = L.oracle_bsdf_sample(C.byref(d), wi.ctypes.data_as(_FP), u3.ctypes.data_as(_FP), wo.ctypes.data_as(_FP),
                              w.ctypes.data_as(_FP), C.byref(pdf), C.byref(eta), 0)
    return wo, w, f32(pdf.value), f32(eta.value), int(st)


def _tex(v, uv):
    """A spectrum-valued parameter at the hit: the constant, or the checkerboard's colour."""
    if isinstance(v, Checkerboard):
        is0 = bool(fr.checker_is_color0(v, np.asarray([uv[0]], f32), np.asarray([uv[1]], f32))[0])
        return fr._spec3(v.color0 if is0 else v.color1)
    return fr._spec3(float(v) if np.isscalar(v) else tuple(v))


def luminance(s):
    return f32(f32(f32(s[0] * f32(0.212671)) + f32(s[1] * f32(0.715160))) + f32(s[2] * f32(0.072169)))


def blend_weight(b, uv):
    s = _tex(b.weight, uv)
    r = f32(0)
    for x in s:
        r = f32(r + x)
    return min(f32(1), max(f32(0), f32(r * f32(f32(1) / f32(3)))))


def child_weights(b, uv):
    """Per child (weight, selection probability), and the mixture's CDF (None for a blend)."""
    if b.type == 'blendbsdf':
        w1 = blend_weight(b, uv)
        w = [f32(f32(1) - w1), w1]
        return w, w, None
    w, cdf = mixture_configure(b.weights, b.ensureEnergyConservation)
    return list(w), [f32(cdf[i + 1] - cdf[i]) for i in range(len(w))], cdf


def sibling_sum(ob, b, w, p, skip, val, pdf, wi, wo):
    """pdf += child.pdf * p[i]; val += child.eval * w[i] over the children but `skip`, in index order."""
    for i, c in enumerate(b.nested):
        if i == skip:
            continue
        cv, cp = leaf_eval_pdf(ob, c, wi, wo)
        pdf = f32(pdf + f32(cp * p[i]))
        val = (val + (cv * w[i]).astype(f32)).astype(f32)
    return val, pdf


# ---- eval / pdf / sample through the chain ---------------------------------------------------
def combo_eval_pdf(ob, b, wi, wo, uv):
    """(eval (3,), pdf) of `b` (any supported chain or leaf), solid-angle measure."""
    wi, wo = np.asarray(wi, f32).copy(), np.asarray(wo, f32).copy()
    if b.type == 'mask':
        op = _tex(b.opacity, uv)
        v, p = combo_eval_pdf(ob, b.nested[0], wi, wo, uv)
        return (v * op).astype(f32), f32(p * luminance(op))
    if b.type == 'twosided':
        side = 0 if wi[2] > 0 else 1
        if side:
            wi[2], wo[2] = -wi[2], -wo[2]
        return combo_eval_pdf(ob, b.nested[min(side, len(b.nested) - 1)], wi, wo, uv)
    if b.type in ('mixturebsdf', 'blendbsdf'):
        w, p, _ = child_weights(b, uv)
        return sibling_sum(ob, b, w, p, -1, np.zeros(3, f32), f32(0), wi, wo)
    return leaf_eval_pdf(ob, b, wi, wo)


def combo_sample(ob, b, wi, sx, sy, uv, choice=None):
    """(wo, weight, pdf, eta, sampledType) of `b`'s sample(bRec, pdf, sample); `choice` (a list)
    receives the branch taken at each level ('null' / 'nested', the child index)."""
    wi = np.asarray(wi, f32).copy()
    sx, sy = f32(sx), f32(sy)
    choice = [] if choice is None else choice
    if b.type == 'mask':
        op = _tex(b.opacity, uv)
        prob = luminance(op)
        if sx < prob:
            choice.append('nested')
            wo, w, pdf, eta, st = combo_sample(ob, b.nested[0], wi, f32(sx / prob), sy, uv, choice)
            inv = f32(f32(1) / prob)
            return wo, ((w * op).astype(f32) * inv).astype(f32), f32(pdf * prob), eta, st
        choice.append('null')
        pdf = f32(f32(1) - prob)
        return -wi, ((f32(1) - op).astype(f32) * f32(f32(1) / pdf)).astype(f32), pdf, f32(1), F_NULL
    if b.type == 'twosided':
        flip = wi[2] < 0
        if flip:
            wi[2] = -wi[2]
        wo, w, pdf, eta, st = combo_sample(ob, b.nested[min(int(flip), len(b.nested) - 1)], wi, sx, sy, uv, choice)
        if flip and np.any(w != 0) and pdf != 0:
            wo = wo.copy()
            wo[2] = -wo[2]
        return wo, w, pdf, eta, st
    if b.type in ('mixturebsdf', 'blendbsdf'):
        w, p, cdf = child_weights(b, uv)
        if cdf is None:
            if sx < w[0]:
                entry, sx = 0, f32(sx / w[0])
            else:
                entry, sx = 1, f32(f32(sx - w[0]) / w[1])
        else:
            entry, sx, _ = sample_reuse(cdf, sx)
        choice.append(entry)
        wo, cw, pdf, eta, st = leaf_sample(ob, b.nested[entry], wi, sx, sy)
        if not np.any(cw != 0):
            return wo, cw, pdf, eta, st
        val = (cw * f32(w[entry] * pdf)).astype(f32)
        pdf = f32(pdf * p[entry])
        if not st & F_DELTA:      # (a delta sample: the smooth siblings are exactly 0 in the discrete measure)
            val, pdf = sibling_sum(ob, b, w, p, entry, val, pdf, wi, wo)
        return wo, (val * f32(f32(1) / pdf)).astype(f32), pdf, eta, st
    return leaf_sample(ob, b, wi, sx, sy)


def has_smooth(b):
    if b.type in ('twosided', 'mixturebsdf', 'blendbsdf', 'mask'):
        return any(has_smooth(c) for c in b.nested)
    return b.type not in ('conductor', 'dielectric')


# ---- the emitter sample at a set of vertices -------------------------------------------------
def nee(sc, twin, ob, V, kind, strict=False, thr=None):
    """The point light's NEE term at the vertices V (delta_ref.first_hits' dict), times the
    throughput `thr` ((n, 3), default 1) in path.cpp's order ((thr * value) * bsdfVal) * weight,
    with the shadow ray traced by the oracle; `direct` with one emitter sample weighs the same
    way.  Returns (c (n, 3), info)."""
    em = sc.emitters[0]
    nS = V['p'].shape[0]
    thr = np.ones((nS, 3), f32) if thr is None else thr
    value, d, dist, pdf, lp = dr.sample_direct(em, sc, V['p'])
    wo = np.stack([dr.dot(d, V['s']), dr.dot(d, V['t']), dr.dot(d, V['n'])], -1)
    snp = (dr.dot(V['rd'], V['geoN']) * V['wi'][:, 2]).astype(f32)
    go = V['valid'].copy()
    if strict:
        go &= ~(snp > 0 if kind == 'volpath' else snp >= 0)
    go &= (pdf != 0) & np.any(value != 0, 1)
    bval = np.zeros((nS, 3), f32)
    for i in np.nonzero(go)[0]:
        b = sc.bsdfs[sc.meshes[V['shape'][i]].bsdf]
        if has_smooth(b):
            bval[i] = combo_eval_pdf(ob, b, V['wi'][i], wo[i], V['uv'][i])[0]
    use = go & np.any(bval != 0, 1)
    if strict:
        use &= (dr.dot(V['geoN'], d) * wo[:, 2]).astype(f32) > 0
    if kind == 'direct':
        pa = (pdf * f32(0.5)).astype(f32)                      # fracLum of (1, 1)
        with np.errstate(invalid='ignore', divide='ignore'):
            w = (((pa * pa).astype(f32) / ((pa * pa).astype(f32) + f32(0)).astype(f32)).astype(f32) * f32(1)).astype(f32)
        c = ((value * bval).astype(f32) * w[:, None]).astype(f32)
    else:
        pa = (pdf * pdf).astype(f32)
        with np.errstate(invalid='ignore', divide='ignore'):
            w = (pa / (pa + f32(0)).astype(f32)).astype(f32)
        c = (((thr * value).astype(f32) * bval).astype(f32) * w[:, None]).astype(f32)
    if kind == 'volpath':
        v = (lp - V['p']).astype(f32)
        rem = dr.length(v)
        with np.errstate(invalid='ignore', divide='ignore'):
            sd = (v * (f32(1) / rem).astype(f32)[:, None]).astype(f32)
        maxt = (rem * f32(1)).astype(f32)
    else:
        sd, maxt = d, (dist * f32(f32(1) - SHADOW_EPSILON)).astype(f32)
    sel = np.nonzero(use)[0]
    occl = np.zeros(nS, bool)
    if sel.size:
        rays = np.zeros((sel.size, 8), f32)
        rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = V['p'][sel], EPSILON, sd[sel], maxt[sel]
        h = np.zeros((sel.size, 4), f32)
        desc = twin.desc()
        assert ob.lib().oracle_trace_rays(C.byref(desc), rays.ctypes.data_as(_FP), sel.size, 1, h.ctypes.data_as(_FP)) == 0
        occl[sel] = h[:, 0] != 0
    lit = use & ~occl
    return np.where(lit[:, None], c, f32(0)).astype(f32), dict(use=use, lit=lit, wo=wo, uv=V['uv'])


# ---- the BSDF sample at the first vertex and the second vertex --------------------------------
def sobol_2d(ob, size, spp, dim, scramble=0):
    """Dimensions (dim, dim + 1) of every sample's Sobol point (records: pixel-major, sample-minor)."""
    L = ob.lib()
    L.oracle_sobol_sample.restype = C.c_float
    L.oracle_sobol_lookup.restype = C.c_uint64
    m = int(np.log2(size))
    out = np.zeros((size * size * spp, 2), f32)
    k = 0
    for pix in range(size * size):
        for j in range(spp):
            idx = L.oracle_sobol_lookup(C.c_uint32(m), C.c_uint32(j), C.c_uint32(pix % size), C.c_uint32(pix // size),
                                        C.c_uint64(scramble))
            out[k] = (L.oracle_sobol_sample(C.c_uint64(idx), C.c_uint32(dim), C.c_uint32(scramble)),
                      L.oracle_sobol_sample(C.c_uint64(idx), C.c_uint32(dim + 1), C.c_uint32(scramble)))
            k += 1
    return out


def to_world(V, i, w):
    """Frame::toWorld (frame.h:100-102): s * v.x + t * v.y + n * v.z."""
    return ((V['s'][i] * w[0]).astype(f32) + (V['t'][i] * w[1]).astype(f32)).astype(f32) + (V['n'][i] * w[2]).astype(f32)


def second_vertices(sc, twin, ob, V, u45, kind='path', strict=False):
    """The BSDF sample at every first vertex (u45: its 2D draw, Sobol dimensions 5, 6) and the vertex its ray
    reaches: (V2 (delta_ref.first_hits' dict), thr (n, 3) = the sample's weight, choices)."""
    nS = V['p'].shape[0]
    thr = np.zeros((nS, 3), f32)
    o, d = V['p'].copy(), np.zeros((nS, 3), f32)
    d[:, 2] = 1
    go = np.zeros(nS, bool)
    choices = [None] * nS
    snp = (dr.dot(V['rd'], V['geoN']) * V['wi'][:, 2]).astype(f32)
    for i in np.nonzero(V['valid'])[0]:
        if strict and (snp[i] > 0 if kind == 'volpath' else snp[i] >= 0):
            continue
        b = sc.bsdfs[sc.meshes[V['shape'][i]].bsdf]
        ch = []
        wo, w, pdf, eta, st = combo_sample(ob, b, V['wi'][i], u45[i, 0], u45[i, 1], V['uv'][i], ch)
        choices[i] = ch
        if not np.any(w != 0):
            continue
        wow = to_world(V, i, wo).astype(f32)
        if strict and not f32(dr.dot(V['geoN'][i], wow) * wo[2]) > 0:
            continue
        thr[i], d[i], go[i] = w, wow, True
    geo = copy.copy(twin)
    geo.bsdfs = [BSDF('diffuse') for _ in twin.bsdfs]
    sel = np.nonzero(go)[0]
    h = np.zeros((nS, 16), f32)
    uv = np.full((nS, 2), np.nan, f32)
    if sel.size:
        h[sel] = fr.oracle_intersect(geo, ob, o[sel], d[sel])
        uv[sel] = fr.hit_uv(geo, ob.trace_rays(geo, o[sel], d[sel], np.full(sel.size, EPSILON, f32),
                                                np.full(sel.size, np.inf, f32)))
    n, s = h[:, 8:11].copy(), h[:, 11:14].copy()
    t = dr.cross(n, s)
    nd = -d
    wi = np.stack([dr.dot(nd, s), dr.dot(nd, t), dr.dot(nd, n)], -1)
    V2 = dict(rd=d, valid=go & (h[:, 0] != 0), p=h[:, 2:5].copy(), geoN=h[:, 5:8].copy(), n=n, s=s, t=t, wi=wi,
              shape=h[:, 14].astype(np.int64), uv=uv)
    return V2, thr, choices


def two_vertices(sc, twin, ob, V, u45, kind, strict=False):
    """Li of `path` / `volpath` at maxDepth 3 under the point light: NEE_1 + thr * NEE_2."""
    c1, info1 = nee(sc, twin, ob, V, kind, strict)
    V2, thr, choices = second_vertices(sc, twin, ob, V, u45, kind, strict)
    c2, info2 = nee(sc, twin, ob, V2, kind, strict, thr=thr)
    return (c1 + c2).astype(f32), dict(c1=c1, c2=c2, choices=choices, info1=info1, info2=info2, V2=V2)


# ---- energy under the area light -------------------------------------------------------------
# The smallest sample count (every multiple of 4 from 4 up was tried, 32 x 32 pixels, the diffuse
# C1 at full depth, box filter) at which, with the oracle alone, the plain scene under scramble 0
# against itself under ENERGY_SCRAMBLE stays within z <= 2 in every channel and against itself
# with every reflectance scaled by 1.05 misses by z >= 6 in every channel:
#   z = 0.125 / 0.131 / 0.113 (R / G / B) and 13.43 / 10.43 / 6.05   at 896 spp
#   (892 spp: 13.31 / 10.33 / 5.96 for the 5% error: blue falls short)
ENERGY_SPP = 896
ENERGY_SCRAMBLE = 0x1234567


def energy_plain(spp=ENERGY_SPP, scramble=0, scale=1.0):
    """The diffuse C1 at 32 x 32, full depth, box filter; `scale` multiplies every reflectance."""
    import dataclasses
    from mitsuba_amd import scenes
    sc, it = scenes.build('C1', width=32, height=32, spp=spp, max_depth=-1)
    it.rfilter, it.scramble = 'box', scramble
    if scale != 1.0:
        sc.bsdfs = [dataclasses.replace(b, reflectance=tuple(x * scale for x in b.reflectance)) for b in sc.bsdfs]
    return sc, it


def energy_wrapped(kind, spp=ENERGY_SPP, scramble=0):
    """The same scene with every BSDF A replaced by blendbsdf(0.5, A, A) or
    mixturebsdf("0.25, 0.75", A, A): the same material, through the combinators' eval, pdf and sample."""
    sc, it = energy_plain(spp, scramble)
    if kind == 'blend':
        sc.bsdfs = [BSDF('blendbsdf', weight=0.5, nested=[b, copy.copy(b)]) for b in sc.bsdfs]
    else:
        sc.bsdfs = [BSDF('mixturebsdf', weights=[0.25, 0.75], nested=[b, copy.copy(b)]) for b in sc.bsdfs]
    return sc, it
