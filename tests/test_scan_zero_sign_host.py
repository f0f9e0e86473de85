"""The canonical zero of the tiny-scene scan's record copy (render_plan.cpp
mtsg_scan_layout, MTSG_SCAN_ZERO_SIGN): where a general record's n_u or n_v is
-0 and its n_d is not +-0, the copy the scans read gets +0, so that the two
triangles of a fan quad whose TriAccel construction left zeros of opposite sign
pair by the unchanged bit-equality rule.  No device.

(a) the layout through mtsgpu_scan_host: C2, and a synthetic scene of four fan
    quads with dyadic coordinates (every TriAccel field exact);
(b) the exactness argument as arithmetic: a float32 restatement of the TriAccel
    test, one operation per line (each rounded to float32 by itself), evaluated
    with the zero of either sign over a grid of rays and planes.  With n_d != 0 no accept decision and no accepted
    (t, u, v) differs; with n_d = -0 some do (+0 - (+-0) is +0 either way, but
    -0 - (+0) = -0 and -0 - (-0) = +0), which is why the rule leaves n_d = +-0
    alone and shows that the grid can see a difference."""
import itertools

import numpy as np
import pytest

from mitsuba_amd import scenes
from mitsuba_amd.integrator import scan_host
from mitsuba_amd.scene import Mesh

# MtsgTri words (csrc/layout.h)
K, N_U, N_V, N_D, A_U, A_V, B_NU, B_NV, C_NU, C_NV, PRIM, SHAPE = range(12)
SIGN = 0x80000000


def _tri_mesh(pts, idx, bsdf=0):
    return Mesh(np.asarray(pts, np.float32), np.asarray(idx, np.uint32), bsdf=bsdf, faceNormals=True)


FAN = [[0, 1, 2], [0, 2, 3]]
# Fan quads (A, B, C, D) -> (A, B, C), (A, C, D), dyadic coordinates, in the free space of
# C1's room above and in front of its blocks.
# TriAccel::load forms the normal as cross(B - A, C - A); a component that is zero
# comes out as a difference of two products, whose zero takes its sign from them:
#  NU: the plane y + 2 z = 6 (k = z, u = x, v = y): n_u is -0 in (A, B, C), +0 in (A, C, D)
#  NV: the plane x + 2 z = 6.5 (k = z): n_v is -0 in one, +0 in the other
#  ND: the NU quad moved into the plane y + 2 z = 0 through the origin, in front of the room's
#      open side (a plane through the origin that crosses the room leaves no such zero):
#      n_d = 0 and n_u = -+0, not rewritten
#  AL: a plane z = 1.5 (aligned group of k = z)
QUAD_NU = [[1.0, 2.0, 2.0], [2.0, 2.0, 2.0], [2.0, 3.0, 1.5], [1.0, 3.0, 1.5]]
QUAD_NV = [[3.5, 2.0, 1.5], [3.5, 3.0, 1.5], [2.5, 3.0, 2.0], [2.5, 2.0, 2.0]]
QUAD_ND = [[3.0, 2.0, -1.0], [4.0, 2.0, -1.0], [4.0, 3.0, -1.5], [3.0, 3.0, -1.5]]
QUAD_AL = [[1.0, 3.5, 1.5], [2.0, 3.5, 1.5], [2.0, 4.5, 1.5], [1.0, 4.5, 1.5]]
QUADS = {'nu': QUAD_NU, 'nv': QUAD_NV, 'nd': QUAD_ND, 'al': QUAD_AL}
ORDER = ('nu', 'nv', 'nd', 'al')


def zero_sign_scene(width=8, height=8, spp=1, room=False, bsdf=0):
    """C1's sensor, BSDFs and light with the four quads in place of (or, room=True:
    inside) the room; the quads' primitives are numbered in ORDER, two each, from
    first_prim(scene)."""
    sc, it = scenes.build('C1', width=width, height=height, spp=spp, rfilter='box')
    keep = sc.meshes[:-1] if room else []
    sc.meshes = list(keep) + [_tri_mesh(QUADS[q], FAN, bsdf) for q in ORDER] + [sc.meshes[-1]]
    return sc, it


def first_prim(sc):
    return sc.num_triangles - 2 - 2 * len(ORDER)


def source_records(sc):
    """the records as configured, by primitive: the layout without the rewrite is not
    exported, so they are re-formed here as TriAccel::load forms them (float32, the
    same operation order), for the quads' primitives only"""
    out = {}
    f = np.float32
    p = first_prim(sc)
    for q in ORDER:
        P = np.asarray(QUADS[q], f)
        for tri in FAN:
            A, B, C = P[tri[0]], P[tri[1]], P[tri[2]]
            b, c = C - A, B - A
            Nn = np.array([c[1] * b[2] - c[2] * b[1], c[2] * b[0] - c[0] * b[2], c[0] * b[1] - c[1] * b[0]], f)
            k = 0
            for j in range(3):
                if abs(Nn[j]) > abs(Nn[k]):
                    k = j
            u, w = (k + 1) % 3, (k + 2) % 3
            denom = f(b[u] * c[w]) - f(b[w] * c[u])
            dotA = f(f(f(A[0] * Nn[0]) + f(A[1] * Nn[1])) + f(A[2] * Nn[2]))
            rec = np.zeros(12, np.uint32)
            rec[K] = k
            rec[N_U:C_NV + 1] = np.array([Nn[u] / Nn[k], Nn[w] / Nn[k], dotA / Nn[k], A[u], A[w], b[u] / denom,
                                          -b[w] / denom, c[w] / denom, -c[u] / denom], f).view(np.uint32)
            rec[PRIM] = p
            out[p] = rec
            p += 1
    return out


def _where(rec, n):
    off = np.concatenate([[0], np.cumsum(n)])
    out = {}
    for i, r in enumerate(rec):
        g = int(np.searchsorted(off, i, side='right') - 1)
        out[int(r[PRIM])] = (g, i - int(off[g]), r)
    return out


def _paired(where, npairs, p, q):
    (g, i, _), (h, j, _) = where[p], where[q]
    return g == h and i // 2 == j // 2 and max(i, j) < 2 * npairs[g]


@pytest.mark.parametrize('no_pairs', [False, True], ids=['pairs', 'no_pairs'])
def test_synthetic_layout(monkeypatch, no_pairs):
    if no_pairs:
        monkeypatch.setenv('MTSGPU_NO_SCAN_PAIRS', '1')
    else:
        monkeypatch.delenv('MTSGPU_NO_SCAN_PAIRS', raising=False)
    sc, _ = zero_sign_scene()
    rec, n, npairs = scan_host(sc)
    assert len(rec) == sum(n) == sc.num_triangles == 10
    where, src, p0 = _where(rec, n), source_records(sc), first_prim(sc)
    prim = {q: (p0 + 2 * i, p0 + 2 * i + 1) for i, q in enumerate(ORDER)}
    # the construction: the partners differ in the sign of one zero and in nothing else
    # that pairing reads (their b_*, c_* differ, as any two triangles' do)
    for q, word in (('nu', N_U), ('nv', N_V), ('nd', N_U)):
        a, b = src[prim[q][0]], src[prim[q][1]]
        assert {int(a[word]), int(b[word])} == {0, SIGN}, (q, a, b)
        for w in (N_U, N_V, N_D, A_U, A_V):
            assert w == word or a[w] == b[w], (q, w)
    for p in prim['nd']:
        assert int(src[p][N_D]) & 0x7fffffff == 0
    for p in prim['nu'] + prim['nv']:
        assert int(src[p][N_D]) & 0x7fffffff != 0
    # every record of g is its source but for a rewritten sign bit: -0 -> +0 in n_u / n_v of
    # the nu and nv quads; the n_d = 0 quad and the aligned quad are copied as they are
    rewritten = 0
    for q in ORDER:
        for p in prim[q]:
            got, want = where[p][2], src[p]
            for w in range(PRIM):
                if got[w] != want[w]:
                    assert q in ('nu', 'nv') and w in (N_U, N_V) and want[w] == SIGN and got[w] == 0, (q, p, w)
                    rewritten += 1
    assert rewritten == 2
    for p in prim['nu'] + prim['nv']:
        assert where[p][0] == 4 and where[p][2][N_U] != SIGN and where[p][2][N_V] != SIGN   # general, k = z
    assert [where[p][0] for p in prim['nd']] == [4, 4] and [where[p][0] for p in prim['al']] == [5, 5]
    assert {int(where[p][2][N_U]) for p in prim['nd']} == {0, SIGN}
    if no_pairs:
        assert npairs == [0] * 6
        return
    assert _paired(where, npairs, *prim['nu']) and _paired(where, npairs, *prim['nv'])
    assert _paired(where, npairs, *prim['al'])
    assert not _paired(where, npairs, *prim['nd'])
    assert all(where[p][1] >= 2 * npairs[4] for p in prim['nd'])   # two singles
    assert npairs[4] == 2 and sum(npairs) == 4                       # and the light's aligned pair


def test_cornell_layout(monkeypatch):
    """C2: 32 records.  Before the rewrite 13 of its 16 quads paired; the two block faces
    whose records differ in the sign of a zero n_u / n_v pair now (15), and the red wall,
    which is not planar, keeps its two singles."""
    monkeypatch.delenv('MTSGPU_NO_SCAN_PAIRS', raising=False)
    sc = scenes.build('C2')[0]
    rec, n, npairs = scan_host(sc)
    assert sum(n) == 32 and sum(npairs) >= 13
    assert sum(npairs) == 15, (n, npairs)
    where = _where(rec, n)
    singles = sorted(p for p, (g, i, _) in where.items() if i >= 2 * npairs[g])
    assert len(singles) == 2 and singles[1] == singles[0] + 1, singles      # one mesh's two triangles
    a, b = where[singles[0]][2], where[singles[1]][2]
    assert where[singles[0]][0] == where[singles[1]][0]                      # one group, yet no pair:
    assert any(a[w] != b[w] for w in (N_U, N_V, N_D))                        # their planes differ
    red = sc.meshes[4]
    first = sum(len(m.indices) for m in sc.meshes[:4])
    assert singles == [first, first + 1] and len(red.indices) == 2
    for r in rec:   # no -0 is left in a general record with n_d != 0
        f = r.view(np.float32)
        if not (f[N_U] == 0 and f[N_V] == 0) and f[N_D] != 0:
            assert r[N_U] != SIGN and r[N_V] != SIGN


# ---- (b) the TriAccel test in float32, one operation per line ----------------------------
# The float32 values are held in float64 arrays and every single operation is rounded to
# float32 at once (rn32): +, -, * and / of two float32 values, formed in float64 and rounded
# again, are the correctly rounded float32 results (53 >= 2 * 24 + 2 bits), denormals, signed
# zeros and overflow included.  numpy's own float32 arithmetic gives the same bits, but only
# while the process honours denormals: a library loaded earlier in a test run can have set
# the CPU's flush-to-zero mode, and then a denormal n_d reads as the zero the rule excludes.
# test_restatement_is_float32 ties the two together where the process allows.

FLT_MAX = float(np.finfo(np.float32).max)


def rn32(x):
    """round a float64 array to the nearest float32 value (ties to even), kept in float64"""
    x = np.asarray(x, np.float64)
    m, e = np.frexp(x)
    normal = np.ldexp(np.rint(np.ldexp(m, 24)), e - 24)
    small = np.rint(x * 2.0 ** 149) * 2.0 ** -149          # the denormal grid; a zero keeps its sign
    r = np.where(np.abs(x) < 2.0 ** -126, small, normal)
    return np.where(np.abs(r) > FLT_MAX, np.copysign(np.inf, r), r)


def tri_test(n_u, n_v, n_d, a_u, a_v, b_nu, b_nv, c_nu, c_nv, o_u, o_v, o_k, d_u, d_v, d_k, rn=rn32):
    """TriAccel::rayIntersect as scan_k / scan_pair_k evaluate it (no fused operation), up to
    the interval test: (t, u, v, u + v).  rn rounds each operation's result to float32."""
    p1 = rn(o_u * n_u)
    s1 = rn(n_d - p1)
    p2 = rn(o_v * n_v)
    s2 = rn(s1 - p2)
    num = rn(s2 - o_k)
    q1 = rn(d_u * n_u)
    q2 = rn(d_v * n_v)
    q3 = rn(q1 + q2)
    den = rn(q3 + d_k)
    t = rn(num / den)
    m1 = rn(t * d_u)
    h1 = rn(o_u + m1)
    hu = rn(h1 - a_u)
    m2 = rn(t * d_v)
    h2 = rn(o_v + m2)
    hv = rn(h2 - a_v)
    u1 = rn(hv * b_nu)
    u2 = rn(hu * b_nv)
    u = rn(u1 + u2)
    v1 = rn(hu * c_nu)
    v2 = rn(hv * c_nv)
    v = rn(v1 + v2)
    w = rn(u + v)
    return t, u, v, w


def accept(t, u, v, w, mint, maxt):
    return ~((t < mint) | (t > maxt)) & (u >= 0) & (v >= 0) & (w <= 1.0)


DENORM = 2.0 ** -149
ORIGIN = np.array([0.0, -0.0, DENORM, -DENORM, 0.5, -1.25])
DIRECTION = np.array([0.0, -0.0, DENORM, -DENORM, 1.0, -0.375])
N_OTHER = [0.5, -2.0, DENORM, -DENORM]                               # the record's nonzero n_v (or n_u)
INTERVALS = [(mi, ma) for mi in (0.0, -1.0) for ma in (np.inf, -np.inf, 4.0)]   # mint 0 and -1: trace_rays
# vertex A at the origin (a zero hu / hv keeps a zero's sign alive) and elsewhere
RECORDS = [(0.0, 0.0, 1.0, 0.5, 0.5, 1.0), (0.25, -0.5, 0.75, -0.25, 0.5, 1.5)]


def _grid():
    o = np.array(list(itertools.product(ORIGIN, repeat=3)))
    d = np.array(list(itertools.product(DIRECTION, repeat=3)))
    oo, dd = np.repeat(o, len(d), axis=0), np.tile(d, (len(o), 1))
    return [oo[:, i] for i in range(3)] + [dd[:, i] for i in range(3)]


def _same(a, b):
    return (a == b) & (np.signbit(a) == np.signbit(b))    # (accepted values are never NaN)


def _differing(n_d, field):
    """how many grid points give another accept decision, or another accepted (t, u, v),
    with -0 than with +0 in `field` (0: n_u, 1: n_v)"""
    rays = _grid()
    assert (rays[5] == 0).any() and (rays[0] == 0).any()    # s_k = 0, zero origins
    n, accepted = 0, 0
    with np.errstate(all='ignore'):
        for rec in RECORDS:
            for other in N_OTHER:
                res = []
                for z in (0.0, -0.0):
                    nu, nv = (z, other) if field == 0 else (other, z)
                    res.append(tri_test(nu, nv, n_d, *rec, *rays))
                (t0, u0, v0, w0), (t1, u1, v1, w1) = res
                same = _same(t0, t1) & _same(u0, u1) & _same(v0, v1)
                for mint, maxt in INTERVALS:
                    a0, a1 = accept(t0, u0, v0, w0, mint, maxt), accept(t1, u1, v1, w1, mint, maxt)
                    both = a0 & a1
                    n += int((a0 != a1).sum()) + int((both & ~same).sum())
                    accepted += int(both.sum())
    assert accepted > 0 or not np.isfinite(n_d)     # the grid holds hits
    return n


def test_restatement_is_float32():
    """rn32 on the float32 grid: a value that is a float32 stays, a tie goes to even, the
    denormal grid and overflow; and, where this process honours float32 denormals, numpy's
    float32 arithmetic gives tri_test's bits"""
    x = np.array([1.0, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 2.0 ** -149, 2.0 ** -150, 3 * 2.0 ** -150, -2.0 ** -151,
                  FLT_MAX, FLT_MAX + 2.0 ** 102, FLT_MAX + 2.0 ** 103, -np.inf, -0.0])
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -22, 2.0 ** -149, 0.0, 2.0 ** -148, -0.0, FLT_MAX, FLT_MAX, np.inf, -np.inf, -0.0])
    assert _same(rn32(x), want).all(), rn32(x)
    f = np.float32
    if float(f(2.0 ** -149)) == 0.0 or float(f(2.0 ** -149) * f(1.0)) == 0.0 or float(f(2.0 ** -128) - f(0.0)) == 0.0:
        return      # flush-to-zero is on in this process: numpy's float32 is not IEEE here
    rays = _grid()
    native = lambda a: np.asarray(a, np.float32)
    check = lambda a: (a if a.dtype == np.float32 else 1 / 0)     # every intermediate is float32
    with np.errstate(all='ignore'):
        for n_d in (1.0, -2.0 ** -128, -0.0):
            for z in (0.0, -0.0):
                emu = tri_test(z, DENORM, n_d, *RECORDS[0], *rays)
                nat = tri_test(f(z), f(DENORM), f(n_d), *[f(r) for r in RECORDS[0]], *[native(r) for r in rays], rn=check)
                for a, b in zip(emu, nat):
                    b = b.astype(np.float64)
                    assert ((np.isnan(a) & np.isnan(b)) | _same(a, b)).all()


@pytest.mark.parametrize('field', [0, 1], ids=['n_u', 'n_v'])
@pytest.mark.parametrize('n_d', [1.0, -0.75, 2.0 ** -149, -2.0 ** -128, np.inf], ids=['1', '-0.75', 'denorm_min', '-2^-128', 'inf'])
def test_sign_of_zero_is_invisible_with_nonzero_n_d(n_d, field):
    assert _differing(n_d, field) == 0


@pytest.mark.parametrize('field', [0, 1], ids=['n_u', 'n_v'])
def test_sign_of_zero_is_visible_with_zero_n_d(field):
    """the exclusion is needed, and the grid can see a difference (it is n_d = -0 that
    shows it: +0 minus a zero of either sign is +0)"""
    neg, pos = _differing(-0.0, field), _differing(0.0, field)
    assert neg > 0 and neg + pos > 0
