"""ldrfilm output (film.LDRFilm) without a GPU: the constructor's property handling
(src/films/ldrfilm.cpp:130-196), the XML loader, the PNG writer against its reader and
against the format's published layout, the C ABI of mtsgpu_develop_ldr, and `ldr_ref`,
the numpy restatement of LDRFilm::develop that tests/test_gpu_ldrfilm.py holds the
device develop to, with its known answers worked by hand.

ldr_ref is float32 numpy in the reference's operation order (numpy float32 arithmetic
is IEEE single precision without contraction); std::pow on floats, math::fastlog and
math::fastexp are libm's powf, log and exp, called through ctypes."""
import ctypes as C
import ctypes.util
import math
import os
import struct
import subprocess
import warnings
import zlib

import numpy as np
import pytest

from mitsuba_amd import abi, integrator, xmlscene
from mitsuba_amd import film as F

f32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(REPO, 'include', 'mtsgpu.h')

# ---------------------------------------------------------------------------
# libm
# ---------------------------------------------------------------------------
_libm = None
_loop = False


def _lib():
    global _libm
    if _libm is None:
        _libm = C.CDLL(ctypes.util.find_library('m') or 'libm.so.6')
        _libm.powf.restype, _libm.powf.argtypes = C.c_float, [C.c_float, C.c_float]
        for fn in (_libm.log, _libm.exp):
            fn.restype, fn.argtypes = C.c_double, [C.c_double]
    return _libm


def _array_loop():
    """oracle/libm_check.c's glibc_eval: a C loop over an array that calls the same libm
    functions (powf; (float)exp((double)x); (float)log((double)x)) -- one ctypes call per
    array instead of one per element.  None where the oracle is not built."""
    global _loop
    if _loop is False:
        so = os.path.join(REPO, 'oracle', '_build', 'liblibm_check.so')
        _loop = None
        if os.path.exists(so):
            L = C.CDLL(so)
            P = C.POINTER(C.c_float)
            L.glibc_eval.argtypes = [C.c_int, P, P, P, C.c_long]
            L.glibc_eval.restype = None
            _loop = L
    return _loop


_FN = {'powf': 7, 'fastexp': 8, 'fastlog': 9}     # ids of oracle/libm_check.c


def _each(name, a, b):
    m = _lib()
    if name == 'powf':
        return np.array([m.powf(float(x), float(y)) for x, y in zip(a, b)], f32)
    fn = m.exp if name == 'fastexp' else m.log
    return np.array([fn(float(x)) for x in a], np.float64).astype(f32)


def libm_f32(name, a, b=None, loop=True):
    """libm's `name` over float32 arrays (b: a scalar or an array for powf)."""
    a = np.ascontiguousarray(a, f32)
    flat = a.reshape(-1)
    bb = None if b is None else np.ascontiguousarray(np.broadcast_to(f32(b), a.shape), f32).reshape(-1)
    L = _array_loop() if loop else None
    if L is None or flat.size < 8:
        return _each(name, flat, bb).reshape(a.shape)
    out = np.empty_like(flat)
    P = C.POINTER(C.c_float)
    L.glibc_eval(_FN[name], flat.ctypes.data_as(P), bb.ctypes.data_as(P) if bb is not None else P(),
                 out.ctypes.data_as(P), flat.size)
    return out.reshape(a.shape)


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def _smax(a, b):
    """std::max(a, b) = (a < b) ? b : a"""
    return np.where(np.less(a, b), b, a).astype(f32)


def _smin(a, b):
    """std::min(a, b) = (b < a) ? b : a"""
    return np.where(np.less(b, a), b, a).astype(f32)


def _apply_gamma(v, inv_gamma):
    """FormatConverterImpl::applyGamma (fmtconv.cpp:1104-1111)."""
    if inv_gamma == f32(-1):
        p = f32(1.055) * libm_f32('powf', v, f32(1.0 / 2.4)) - f32(0.055)
        return np.where(v <= f32(0.0031308), f32(12.92) * v, p).astype(f32)
    return libm_f32('powf', v, inv_gamma)


def _to_u8(v, mult=None, inv_gamma=None):
    """convertScalar<uint8_t> (fmtconv.cpp:1137-1160); alpha: no multiplier, no gamma."""
    v = np.asarray(v, f32)
    if mult is not None:
        v = v * f32(mult)
        if inv_gamma != f32(1):
            v = _apply_gamma(v, inv_gamma)
    t = v * f32(255) + f32(0.5)
    return _smin(f32(255), _smax(f32(0), t)).astype(np.uint8)     # in [0, 255]: the cast truncates


def max_luminance(lum):
    """The loop of bitmap.cpp:1743-1750 for maxLuminance, in closed form: the reset at a
    luminance of exactly 1024 leaves the maximum over the pixels from the last such pixel
    on; std::max(maxLuminance, luminance) from 0 takes a value only when it is greater,
    so NaN, negative values and zeros never enter and the result is the largest positive
    value (+0 if there is none).  test_max_luminance_closed_form checks this against the
    literal loop."""
    lum = np.asarray(lum, f32).reshape(-1)
    hit = np.nonzero(lum == f32(1024))[0]
    tail = lum[hit[-1]:] if hit.size else lum
    pos = tail[tail > 0]
    return f32(pos.max()) if pos.size else f32(0)


def ldr_ref(film, border, ldrfilm, info=False):
    """LDRFilm::develop (ldrfilm.cpp:300-321) of the (H+2b, W+2b, 5) float32 film:
    (H, W, C) uint8, and with info=True also float32 {logAvgLuminance, maxLuminance}."""
    film = np.asarray(film, f32)
    b = int(border)
    core = film[b:film.shape[0] - b, b:film.shape[1] - b]
    fmt = ldrfilm.pixel_format
    mono = fmt in ('luminance', 'luminancealpha')
    info2 = np.zeros(2, f32)
    with np.errstate(all='ignore'):
        # Bitmap::convert(pixelFormat, EFloat) (fmtconv.cpp:955-1005)
        s0, s1, s2, alpha, w = (core[..., i] for i in range(5))
        inv = np.where(w != 0, f32(1) / np.where(w != 0, w, f32(1)), w).astype(f32)
        if mono:
            vals = [((s0 * f32(0.212671) + s1 * f32(0.715160)) + s2 * f32(0.072169)) * inv]
        else:
            vals = [s0 * inv, s1 * inv, s2 * inv]
        a = alpha * inv
        mult = f32(1)
        if ldrfilm.tonemapMethod == 'reinhard':
            # Bitmap::tonemapReinhard (bitmap.cpp:1711-1854)
            lum = vals[0] if mono else (vals[0] * f32(0.212671) + vals[1] * f32(0.715160)) + vals[2] * f32(0.072169)
            lum = lum.reshape(-1)
            terms = libm_f32('fastlog', f32(1e-3) + lum)
            # the sequential Float sum, from 0, in pixel order
            total = np.add.accumulate(np.concatenate([np.zeros(1, f32), terms]), dtype=f32)[-1]
            max_lum = max_luminance(lum)
            log_avg = libm_f32('fastexp', np.array([total / f32(lum.size)], f32))[0]
            info2[:] = (log_avg, max_lum)
            if max_lum != 0:
                t = f32(1) - f32(ldrfilm.burn)
                t = t if f32(1e-8) < t else f32(1e-8)
                burn = t if t < f32(1) else f32(1)
                scale = f32(ldrfilm.key) / log_avg
                lwhite = max_lum * scale
                inv_wp2 = f32(1) / (lwhite * lwhite * libm_f32('powf', np.array([burn], f32), f32(4))[0])
                if mono:
                    lp = vals[0] * scale
                    vals = [lp * (f32(1) + lp * inv_wp2) / (f32(1) + lp)]
                else:
                    r, g, bl = vals
                    X = (r * f32(0.412453) + g * f32(0.357580)) + bl * f32(0.180423)
                    Y = (r * f32(0.212671) + g * f32(0.715160)) + bl * f32(0.072169)
                    Z = (r * f32(0.019334) + g * f32(0.119193)) + bl * f32(0.950227)
                    norm = f32(1) / ((X + Y) + Z)
                    x, y, lp = X * norm, Y * norm, Y * scale
                    Y = lp * (f32(1) + lp * inv_wp2) / (f32(1) + lp)
                    ratio = Y / y
                    X = ratio * x
                    Z = ratio * ((f32(1) - x) - y)
                    vals = [(f32(3.240479) * X + f32(-1.537150) * Y) + f32(-0.498535) * Z,
                            (f32(-0.969256) * X + f32(1.875991) * Y) + f32(0.041556) * Z,
                            (f32(0.055648) * X + f32(-0.204043) * Y) + f32(1.057311) * Z]
        else:
            mult = libm_f32('powf', np.array([2], f32), f32(ldrfilm.exposure))[0]      # ldrfilm.cpp:318
        inv_gamma = f32(1) / f32(ldrfilm.gamma)                                          # fmtconv.cpp:148
        chans = [_to_u8(v, mult, inv_gamma) for v in vals]
        if ldrfilm.hasAlpha:
            chans.append(_to_u8(a))
    out = np.stack(chans, -1)
    return (out, info2) if info else out


def _px(values, weight=1.0, alpha=1.0, border=1):
    """A film of len(values) pixels in one row: (r, g, b) each, with a border of zeros."""
    n = len(values)
    film = np.zeros((1 + 2 * border, n + 2 * border, 5), f32)
    for i, v in enumerate(values):
        film[border, border + i] = (v[0], v[1], v[2], alpha, weight)
    return film


def _ldr(**kw):
    kw.setdefault('banner', False)
    return F.LDRFilm(**kw)


# ---------------------------------------------------------------------------
# the constructor (ldrfilm.cpp:130-196)
# ---------------------------------------------------------------------------
def test_ldrfilm_defaults_and_overrides():
    l = F.LDRFilm()
    assert (l.fileFormat, l.pixel_format, l.tonemapMethod, l.banner) == ('png', 'rgb', 'gamma', True)
    assert (l.gamma, l.exposure, l.burn) == (-1.0, 0.0, 0.0) and f32(l.key) == f32(0.18)
    assert l.channel_names == ['R', 'G', 'B'] and not l.hasAlpha and l.componentFormat == 'uint8'
    l = F.LDRFilm(fileFormat='PNG', pixelFormat='luminanceAlpha', tonemapMethod='Reinhard', gamma=2.2, exposure=1.5,
                  key=0.5, burn=0.25, banner=False)
    assert (l.fileFormat, l.pixel_format, l.tonemapMethod, l.banner) == ('png', 'luminancealpha', 'reinhard', False)
    assert (f32(l.gamma), l.exposure, l.key, l.burn) == (f32(2.2), 1.5, 0.5, 0.25)
    assert l.channel_names == ['Y', 'A']
    p = l.develop_params((10, 12, 5), 2)
    assert (p.film_width, p.film_height, p.border) == (12, 10, 2)
    assert (p.pixel_format, p.tonemap_method) == (abi.PIX_LUMINANCE_ALPHA, abi.TONEMAP_REINHARD)
    assert (p.gamma, p.exposure, p.key, p.burn) == (f32(2.2), 1.5, 0.5, 0.25)
    assert l.output_array((10, 12, 5), 2).shape == (6, 8, 2) and l.output_array((10, 12, 5), 2).dtype == np.uint8
    assert F.LDRFilm().develop_params((4, 4, 5), 1).tonemap_method == abi.TONEMAP_GAMMA


@pytest.mark.parametrize('kw,msg', [
    (dict(fileFormat='openexr'), 'The "fileFormat" parameter must either be equal to "png" or "jpeg"!'),
    (dict(tonemapMethod='filmic'), 'The "method" parameter must either be equal to "gamma" or "reinhard"!'),
    (dict(pixelFormat='xyz'), 'The "pixelFormat" parameter must either be equal to "luminance", "luminanceAlpha", '
                              '"rgb", or "rgba"!'),
    (dict(pixelFormat='xyza'), '"rgb", or "rgba"!'),
    (dict(pixelFormat='spectrum'), '"rgb", or "rgba"!'),
])
def test_ldrfilm_errors(kw, msg):
    with pytest.raises(ValueError) as e:
        F.LDRFilm(**kw)
    assert msg in str(e.value)


@pytest.mark.parametrize('fmt,alpha', [('luminance', False), ('luminanceAlpha', True), ('rgb', False),
                                       ('rgba', True)])
def test_ldrfilm_has_alpha(fmt, alpha):
    l = F.LDRFilm(pixelFormat=fmt)
    assert l.hasAlpha is alpha and len(l.channel_names) == {'luminance': 1, 'luminanceAlpha': 2, 'rgb': 3,
                                                            'rgba': 4}[fmt]


def test_ldrfilm_output_path_extension():
    """ldrfilm.cpp:335-345: a wrong extension is replaced (compared in lower case)."""
    assert F.LDRFilm().output_path('/tmp/a.exr') == '/tmp/a.png'
    assert F.LDRFilm().output_path('/tmp/a.PNG') == '/tmp/a.PNG'
    assert F.LDRFilm().output_path('/tmp/a') == '/tmp/a.png'
    assert F.LDRFilm(fileFormat='jpeg').output_path('/tmp/a.png') == '/tmp/a.jpg'
    assert F.LDRFilm(fileFormat='jpg').output_path('/tmp/a.jpg') == '/tmp/a.jpg'


def test_ldrfilm_jpeg_drops_alpha_and_cannot_be_written(tmp_path):
    """ldrfilm.cpp:172-178; the package has no JPEG encoder."""
    with pytest.warns(UserWarning, match='JPEG format does not support it'):
        l = F.LDRFilm(fileFormat='jpeg', pixelFormat='rgba')
    assert (l.fileFormat, l.pixel_format, l.hasAlpha) == ('jpeg', 'rgb', False)
    with pytest.warns(UserWarning):
        assert F.LDRFilm(fileFormat='JPG', pixelFormat='luminanceAlpha').pixel_format == 'luminance'
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert F.LDRFilm(fileFormat='jpeg', pixelFormat='rgb').pixel_format == 'rgb'
    with pytest.raises(NotImplementedError, match='JPEG'):
        l.write(str(tmp_path / 'a.jpg'), np.zeros((2, 2, 3), np.uint8))
    assert not os.listdir(str(tmp_path))


def test_hdrfilm_is_untouched():
    with pytest.raises(ValueError):
        F.HDRFilm(fileFormat='png')
    with pytest.raises(ValueError):
        F.HDRFilm(componentFormat='uint8')


# ---------------------------------------------------------------------------
# the XML loader
# ---------------------------------------------------------------------------
SCENE = """<scene version="0.6.0">
    <integrator type="path"/>
    <sensor type="perspective">
        <sampler type="sobol"><integer name="sampleCount" value="8"/></sampler>
        <film type="ldrfilm">%s</film>
    </sensor>
    <shape type="cube"><emitter type="area"><rgb name="radiance" value="1, 1, 1"/></emitter></shape>
</scene>
"""


def test_xml_ldrfilm_defaults(tmp_path):
    src = tmp_path / 'a.xml'
    src.write_text(SCENE % '')
    sc, it = xmlscene.load_scene(str(src))
    assert isinstance(it.film, F.LDRFilm) and it.film == F.LDRFilm()
    assert (sc.sensor.width, sc.sensor.height) == (768, 576)            # film.cpp:27-33
    assert (it.rfilter, it.rfilterParam, it.hasAlpha) == ('gaussian', 0.5, False)


def test_xml_ldrfilm_all_properties_and_round_trip(tmp_path):
    props = ('<integer name="width" value="64"/><integer name="height" value="48"/>'
             '<string name="fileFormat" value="png"/><string name="pixelFormat" value="rgba"/>'
             '<string name="tonemapMethod" value="reinhard"/><float name="gamma" value="2.2"/>'
             '<float name="exposure" value="-1.5"/><float name="key" value="0.25"/><float name="burn" value="0.5"/>'
             '<boolean name="banner" value="false"/><rfilter type="box"/>')
    src = tmp_path / 'a.xml'
    src.write_text(SCENE % props)
    sc, it = xmlscene.load_scene(str(src))
    l = it.film
    assert isinstance(l, F.LDRFilm)
    assert (l.fileFormat, l.pixel_format, l.tonemapMethod, l.banner) == ('png', 'rgba', 'reinhard', False)
    assert (f32(l.gamma), l.exposure, l.key, l.burn) == (f32(2.2), -1.5, 0.25, 0.5)
    assert it.hasAlpha is True and (sc.sensor.width, sc.sensor.height) == (64, 48) and it.rfilter == 'box'
    sc2, it2 = xmlscene.load_scene(xmlscene.save_scene(sc, it, str(tmp_path / 'out')))
    assert isinstance(it2.film, F.LDRFilm) and it2.film == l and it2.hasAlpha is True
    src.write_text(SCENE % '<string name="pixelFormat" value="luminanceAlpha"/>')
    assert xmlscene.load_scene(str(src))[1].hasAlpha is True
    src.write_text(SCENE % '<string name="pixelFormat" value="luminance"/>')
    assert xmlscene.load_scene(str(src))[1].hasAlpha is False


def test_xml_ldrfilm_errors(tmp_path):
    src = tmp_path / 'a.xml'
    src.write_text(SCENE % '<string name="pixelFormat" value="xyz"/>')
    with pytest.raises(xmlscene.SceneError, match='"pixelFormat" parameter'):
        xmlscene.load_scene(str(src))
    src.write_text(SCENE % '<boolean name="highQualityEdges" value="true"/>')
    with pytest.raises(NotImplementedError, match='highQualityEdges'):
        xmlscene.load_scene(str(src))
    src.write_text((SCENE % '').replace('ldrfilm', 'tiledhdrfilm'))
    with pytest.raises(NotImplementedError, match='ldrfilm'):
        xmlscene.load_scene(str(src))


def test_banner_warns_once_and_is_not_stamped():
    class Ctx:
        def develop_ldr(self, film, border, l):
            return 'developed'
    F._banner_warned = False
    with pytest.warns(UserWarning, match='banner'):
        assert F.LDRFilm().develop(Ctx(), None, 1) == 'developed'
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        F.LDRFilm().develop(Ctx(), None, 1)
        F.LDRFilm(banner=False).develop(Ctx(), None, 1)


# ---------------------------------------------------------------------------
# the restatement's known answers
# ---------------------------------------------------------------------------
def test_libm_loop_equals_libm_call_by_call():
    rng = np.random.default_rng(5)
    a = (rng.random(500, dtype=np.float32) * f32(4)).astype(f32)
    a[:4] = (0.0, -1.0, np.nan, np.inf)
    for name, b in (('powf', f32(1.0 / 2.4)), ('powf', f32(1) / f32(2.2)), ('fastlog', None), ('fastexp', None)):
        x, y = libm_f32(name, a, b), libm_f32(name, a, b, loop=False)
        assert np.array_equal(x.view(np.uint32)[~np.isnan(x)], y.view(np.uint32)[~np.isnan(y)])
        assert np.array_equal(np.isnan(x), np.isnan(y))


def test_ref_linear_and_srgb_known_answers():
    one = ldr_ref(_px([(1.0, 0.0, 0.5)]), 1, _ldr(gamma=1.0))[0, 0]
    assert one.tolist() == [255, 0, 128]                   # 0.5 * 255 + 0.5 = 128.0
    # weight division: 3 / 4 = 0.75 -> 0.75 * 255 + 0.5 = 191.75 -> 191
    assert ldr_ref(_px([(3.0, 3.0, 3.0)], weight=4.0), 1, _ldr(gamma=1.0))[0, 0].tolist() == [191, 191, 191]
    # weight 0: invWeight = weight = 0 -> 0
    assert ldr_ref(_px([(3.0, 3.0, 3.0)], weight=0.0), 1, _ldr())[0, 0].tolist() == [0, 0, 0]
    # sRGB (gamma -1): 1 -> 1.055 * 1 - 0.055 = 1 -> 255; 0 -> 12.92 * 0 -> 0
    assert ldr_ref(_px([(1.0, 0.0, 1.0)]), 1, _ldr())[0, 0].tolist() == [255, 0, 255]
    # 0.0031308f is on the linear branch, the next float on the power branch
    t = f32(0.0031308)
    nxt = np.nextafter(t, f32(1))
    lin = f32(f32(12.92) * t)
    pw = f32(f32(1.055) * f32(_lib().powf(float(nxt), float(f32(1.0 / 2.4)))) - f32(0.055))
    assert lin != pw                                       # the curve's two pieces do not meet exactly
    out = ldr_ref(_px([(t, nxt, 0.0)]), 1, _ldr())[0, 0]
    assert out[0] == int(f32(lin * f32(255) + f32(0.5))) == 10
    assert out[1] == int(f32(pw * f32(255) + f32(0.5))) == 10
    # mid grey: 0.5 -> 1.055 * 0.5^(1/2.4) - 0.055 = 0.7354 -> 188.02 -> 188
    assert ldr_ref(_px([(0.5, 0.5, 0.5)]), 1, _ldr())[0, 0].tolist() == [188, 188, 188]
    # gamma 2.2: 0.5^(1/2.2) = 0.72974 -> 186.58 -> 186; clamps at 255
    assert ldr_ref(_px([(0.5, 2.0, 1e9)]), 1, _ldr(gamma=2.2))[0, 0].tolist() == [186, 255, 255]


def test_ref_negative_nan_inf():
    """pow of a negative value is NaN, and std::max(0, NaN) = 0; -inf and +inf clamp."""
    film = _px([(-0.5, np.nan, np.inf), (-np.inf, -0.0, 0.25)])
    for g in (2.2, -1.0):
        out = ldr_ref(film, 1, _ldr(gamma=g))
        assert out[0, 0].tolist() == [0, 0, 255]
        # pow(-inf, y) is +inf for a positive y that is no odd integer; the sRGB curve's linear
        # piece keeps -inf.  pow(-0, y) = +0.
        assert out[0, 1, :2].tolist() == [255 if g == 2.2 else 0, 0]
    # gamma 1 skips the power: a negative value is clamped, NaN * 255 + 0.5 = NaN -> 0
    assert ldr_ref(film, 1, _ldr(gamma=1.0))[0, 0].tolist() == [0, 0, 255]


def test_ref_gamma_one_skips_the_power(monkeypatch):
    """invDestGamma == 1: no pow at all -- powf(x, 1) would return x too, so the proof is
    that the restatement never calls it."""
    calls = []
    real = libm_f32

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)
    monkeypatch.setitem(ldr_ref.__globals__, 'libm_f32', spy)
    out = ldr_ref(_px([(0.25, 0.5, 1.0)]), 1, _ldr(gamma=1.0))
    assert out[0, 0].tolist() == [64, 128, 255]            # 0.25 * 255 + 0.5 = 64.25
    assert calls == ['powf']                               # powf(2, exposure) only


def test_ref_exposure_and_alpha():
    """multiplier = powf(2, exposure) on colour; alpha sees neither it nor gamma."""
    film = _px([(0.125, 0.25, 0.5)], alpha=0.5)
    out = ldr_ref(film, 1, _ldr(pixelFormat='rgba', gamma=1.0, exposure=1.0))[0, 0]
    assert out.tolist() == [64, 128, 255, 128]             # x2, alpha 0.5 -> 128
    out = ldr_ref(film, 1, _ldr(pixelFormat='rgba', gamma=2.2, exposure=-2.0))[0, 0]
    assert out[3] == 128
    # 0.5 / 4 = 0.125 -> 0.125^(1/2.2) = 0.38865 -> 99.6 -> 99
    assert out[2] == 99
    la = ldr_ref(film, 1, _ldr(pixelFormat='luminanceAlpha', gamma=1.0, exposure=1.0))[0, 0]
    lum = f32(f32(f32(0.125) * f32(0.212671) + f32(0.25) * f32(0.715160)) + f32(0.5) * f32(0.072169))
    assert la.tolist() == [int(f32(f32(lum * f32(2)) * f32(255) + f32(0.5))), 128]
    assert ldr_ref(film, 1, _ldr(pixelFormat='luminance', gamma=1.0, exposure=1.0)).shape == (1, 1, 1)
    # reinhard ignores exposure
    a = ldr_ref(film, 1, _ldr(tonemapMethod='reinhard', exposure=3.0))
    assert np.array_equal(a, ldr_ref(film, 1, _ldr(tonemapMethod='reinhard')))


def test_ref_reinhard_2x2_by_hand():
    """A 2x2 luminance film, every step of bitmap.cpp:1762-1784, 1845-1852 written out."""
    film = np.zeros((4, 4, 5), f32)
    grey = [0.25, 1.0, 4.0, 0.0]
    for i, v in enumerate(grey):
        film[1 + i // 2, 1 + i % 2] = (v, v, v, 1.0, 1.0)
    lums = [f32(f32(f32(f32(v) * f32(0.212671) + f32(v) * f32(0.715160)) + f32(v) * f32(0.072169)) * f32(1))
            for v in grey]
    total = f32(0)
    for l in lums:                                           # logAvgLuminance += fastlog(1e-3f + luminance)
        total = f32(total + f32(math.log(float(f32(f32(1e-3) + l)))))
    log_avg = f32(math.exp(float(f32(total / f32(4)))))
    max_lum = max(lums)
    assert max_lum == lums[2] and abs(float(max_lum) - 4.0) < 1e-6
    # exp((ln 0.251 + ln 1.001 + ln 4.001 + ln 0.001) / 4) = (0.251 * 1.001 * 4.001 * 0.001)^(1/4)
    assert abs(float(log_avg) - (0.251 * 1.001 * 4.001 * 0.001) ** 0.25) < 1e-6
    key, burn = f32(0.18), f32(1)                            # burn parameter 0 -> 1 - 0 = 1
    scale = f32(key / log_avg)
    lwhite = f32(max_lum * scale)
    inv_wp2 = f32(f32(1) / f32(f32(lwhite * lwhite) * f32(_lib().powf(float(burn), 4.0))))
    expect = []
    for l in lums:
        lp = f32(l * scale)
        v = f32(f32(lp * f32(f32(1) + f32(lp * inv_wp2))) / f32(f32(1) + lp))
        expect.append(int(min(f32(255), max(f32(0), f32(v * f32(255) + f32(0.5))))))
    out, info2 = ldr_ref(film, 1, _ldr(pixelFormat='luminance', tonemapMethod='reinhard', gamma=1.0), info=True)
    assert out.reshape(-1).tolist() == expect
    assert info2.view(np.uint32).tolist() == np.array([log_avg, max_lum], f32).view(np.uint32).tolist()
    # the brightest pixel maps to Lwhite * (1 + Lwhite / Lwhite^2) / (1 + Lwhite) = 1 -> 255, black stays 0
    assert expect[2] == 255 and expect[3] == 0 and 0 < expect[0] < expect[1] < 255
    # burn = 1 -> max(1e-8, 0): invWp2 = 1 / (Lwhite^2 * 1e-32), about 6e30 here -> every lit pixel saturates
    out = ldr_ref(film, 1, _ldr(pixelFormat='luminance', tonemapMethod='reinhard', gamma=1.0, burn=1.0))
    assert out.reshape(-1).tolist() == [255, 255, 255, 0]


def test_ref_reinhard_rgb_keeps_chromaticity_and_alpha():
    film = _px([(0.2, 0.4, 0.8), (2.0, 1.0, 0.5)], alpha=0.25)
    out = ldr_ref(film, 1, _ldr(pixelFormat='rgba', tonemapMethod='reinhard', gamma=1.0))
    assert out[0, :, 3].tolist() == [64, 64]               # alpha untouched: 0.25 * 255 + 0.5 = 64.25
    assert out[0, 0, 0] < out[0, 0, 1] < out[0, 0, 2] and out[0, 1, 0] > out[0, 1, 1] > out[0, 1, 2]
    # a black pixel in a lit image: 1 / (X + Y + Z) = inf, 0 * inf = NaN -> 0
    film = _px([(0.0, 0.0, 0.0), (1.0, 1.0, 1.0)])
    assert ldr_ref(film, 1, _ldr(tonemapMethod='reinhard'))[0, 0].tolist() == [0, 0, 0]


def test_ref_1024_rule():
    """bitmap.cpp:1745-1746: a luminance of exactly 1024 resets the running maximum."""
    l = _ldr(pixelFormat='luminance', tonemapMethod='reinhard', gamma=1.0)
    g = lambda v: (v, v, v)
    lum = lambda film: ldr_ref(film, 1, l, info=True)[1][1]
    # luminance of (v, v, v) is v * 1.0 up to rounding: pick 1024 exactly through the weights' sum
    c = f32(f32(f32(1024) * f32(0.212671) + f32(1024) * f32(0.715160)) + f32(1024) * f32(0.072169))
    assert c == f32(1024)
    assert lum(_px([g(3000.0), g(1024.0), g(7.0)])) == f32(1024)      # 1024 after the brightest: 3000 forgotten
    assert lum(_px([g(1024.0), g(3000.0), g(7.0)])) > f32(2999)       # 1024 before it: 3000 stays
    assert lum(_px([g(3000.0), g(1024.0), g(7.0), g(1024.0), g(0.5)])) == f32(1024)
    assert lum(_px([g(3000.0), g(1023.0), g(7.0)])) > f32(2999)


def test_max_luminance_closed_form():
    rng = np.random.default_rng(9)
    for trial in range(40):
        lum = (rng.random(50, dtype=np.float32) * f32(2000)).astype(f32)
        lum[rng.integers(0, 50, 6)] = (np.nan, -3.0, np.inf if trial % 5 == 0 else 5.0, 1024.0, -0.0, 0.0)
        if trial % 3 == 0:
            lum[rng.integers(0, 50)] = 1024.0
        if trial % 7 == 0:
            lum = -lum
        m = f32(0)
        for v in lum:                                        # the literal loop
            if v == f32(1024):
                m = f32(0)
            m = v if m < v else m
        got = max_luminance(lum)
        assert got.view(np.uint32) == f32(m).view(np.uint32)


def test_ref_all_black():
    """maxLuminance == 0: tonemapReinhard returns early, logAvgLuminance = fastexp(fastlog(1e-3f))."""
    film = np.zeros((4, 5, 5), f32)
    film[..., 4] = 1
    out, info2 = ldr_ref(film, 1, _ldr(pixelFormat='rgba', tonemapMethod='reinhard'), info=True)
    assert not out[..., :3].any() and out.shape == (2, 3, 4)
    # six terms of ln(0.001f) = -6.9: the sum's and the mean's rounding stay below 1e-5 of the
    # exponent, that is 1e-5 of the result
    assert info2[1] == 0 and abs(float(info2[0]) - 1e-3) < 1e-8


def test_ref_sum_is_sequential():
    """The float sum depends on its order; ldr_ref's is the pixel order."""
    rng = np.random.default_rng(3)
    film = (rng.random((40, 50, 5), dtype=np.float32) * f32(3)).astype(f32)
    l = _ldr(pixelFormat='luminance', tonemapMethod='reinhard')
    _, info2 = ldr_ref(film, 1, l, info=True)
    core = film[1:-1, 1:-1]
    lum = (((core[..., 0] * f32(0.212671) + core[..., 1] * f32(0.715160)) + core[..., 2] * f32(0.072169))
           * (f32(1) / core[..., 4])).reshape(-1)
    total = f32(0)
    for t in libm_f32('fastlog', f32(1e-3) + lum):
        total = f32(total + t)
    assert info2[0] == f32(math.exp(float(f32(total / f32(lum.size)))))


# ---------------------------------------------------------------------------
# PNG
# ---------------------------------------------------------------------------
def _chunks(raw):
    assert raw[:8] == b'\x89PNG\r\n\x1a\n'
    pos, out = 8, []
    while pos < len(raw):
        n, tag = struct.unpack_from('>I4s', raw, pos)
        body = raw[pos + 8:pos + 8 + n]
        crc = struct.unpack_from('>I', raw, pos + 8 + n)[0]
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        out.append((tag, body))
        pos += 12 + n
    return out


@pytest.mark.parametrize('c,color', [(1, 0), (2, 4), (3, 2), (4, 6)])
def test_png_round_trip_and_layout(tmp_path, c, color):
    rng = np.random.default_rng(c)
    img = rng.integers(0, 256, (7, 11, c), dtype=np.uint8)
    p = str(tmp_path / 'a.png')
    F.write_png(p, img)
    back, gamma = F.read_png(p)
    assert back.dtype == np.uint8 and np.array_equal(back, img) and gamma == -1.0
    ch = _chunks(open(p, 'rb').read())
    assert [t for t, _ in ch] == [b'IHDR', b'gAMA', b'sRGB', b'cHRM', b'IDAT', b'IEND']
    assert struct.unpack('>IIBBBBB', ch[0][1]) == (11, 7, 8, color, 0, 0, 0)
    assert struct.unpack('>I', ch[1][1]) == (45455,) and ch[2][1] == b'\x03'      # PNG_sRGB_INTENT_ABSOLUTE
    assert struct.unpack('>8I', ch[3][1]) == (31270, 32900, 64000, 33000, 30000, 60000, 15000, 6000)
    raw = zlib.decompress(ch[4][1])
    assert len(raw) == 7 * (1 + 11 * c) and ch[5][1] == b''
    rows = np.frombuffer(raw, np.uint8).reshape(7, 1 + 11 * c)
    assert not rows[:, 0].any() and np.array_equal(rows[:, 1:].reshape(7, 11, c), img)
    if c == 1:
        F.write_png(p, img[:, :, 0])
        assert np.array_equal(F.read_png(p)[0], img)


def test_png_gamma_chunk(tmp_path):
    img = np.arange(24, dtype=np.uint8).reshape(2, 4, 3)
    p = str(tmp_path / 'g.png')
    F.write_png(p, img, 2.2)
    ch = _chunks(open(p, 'rb').read())
    assert [t for t, _ in ch] == [b'IHDR', b'gAMA', b'IDAT', b'IEND']
    assert struct.unpack('>I', ch[1][1]) == (45455,)       # 1 / 2.2 = 0.454545 in 1e-5 units
    back, gamma = F.read_png(p)
    assert np.array_equal(back, img) and abs(gamma - 2.2) < 1e-4
    F.write_png(p, img, 1.0)
    assert struct.unpack('>I', _chunks(open(p, 'rb').read())[1][1]) == (100000,)
    assert F.read_png(p)[1] == 1.0
    with pytest.raises(ValueError):
        F.write_png(p, img.astype(np.float32))
    with pytest.raises(ValueError):
        F.write_png(p, np.zeros((2, 2, 5), np.uint8))


def test_png_reader_checks_crc_and_unfilters(tmp_path):
    img = np.random.default_rng(2).integers(0, 256, (5, 6, 3), dtype=np.uint8)
    p = str(tmp_path / 'a.png')
    F.write_png(p, img)
    raw = bytearray(open(p, 'rb').read())
    raw[-20] ^= 1                                           # inside IDAT
    open(p, 'wb').write(bytes(raw))
    with pytest.raises(ValueError, match='CRC'):
        F.read_png(p)
    # a file with every filter type, built here: Sub, Up, Average, Paeth, None
    s = img.astype(np.int32).reshape(5, 18)
    lines = []
    for y, ft in enumerate((1, 2, 3, 4, 0)):
        prev = s[y - 1] if y else np.zeros(18, np.int32)
        a = np.concatenate([np.zeros(3, np.int32), s[y, :-3]])
        cc = np.concatenate([np.zeros(3, np.int32), prev[:-3]])
        if ft == 0:
            pred = 0 * a
        elif ft == 1:
            pred = a
        elif ft == 2:
            pred = prev
        elif ft == 3:
            pred = (a + prev) >> 1
        else:
            pa, pb, pc = abs(prev - cc), abs(a - cc), abs(a + prev - 2 * cc)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, cc))
        lines.append(bytes([ft]) + ((s[y] - pred) & 0xFF).astype(np.uint8).tobytes())
    body = F._png_chunk(b'IHDR', struct.pack('>IIBBBBB', 6, 5, 8, 2, 0, 0, 0))
    body += F._png_chunk(b'IDAT', zlib.compress(b''.join(lines))) + F._png_chunk(b'IEND', b'')
    open(p, 'wb').write(F.PNG_MAGIC + body)
    back, gamma = F.read_png(p)
    assert np.array_equal(back, img) and gamma is None


@pytest.mark.parametrize('c', [1, 2, 3, 4])
def test_png_decodes_in_pillow(tmp_path, c):
    Image = pytest.importorskip('PIL.Image')
    img = np.random.default_rng(c).integers(0, 256, (9, 13, c), dtype=np.uint8)
    p = str(tmp_path / 'a.png')
    F.write_png(p, img, -1.0 if c % 2 else 2.2)
    with Image.open(p) as im:
        assert im.mode == {1: 'L', 2: 'LA', 3: 'RGB', 4: 'RGBA'}[c]
        assert np.array_equal(np.asarray(im).reshape(9, 13, c), img)


def test_ldrfilm_write_png(tmp_path):
    img = np.random.default_rng(4).integers(0, 256, (4, 5, 4), dtype=np.uint8)
    l = F.LDRFilm(pixelFormat='rgba', gamma=2.2)
    path = l.write(str(tmp_path / 'out.exr'), img)
    assert path.endswith('out.png')
    back, gamma = F.read_png(path)
    assert np.array_equal(back, img) and abs(gamma - 2.2) < 1e-4


# ---------------------------------------------------------------------------
# the C ABI, without a device
# ---------------------------------------------------------------------------
def test_abi_symbols_struct_and_null_arguments(tmp_path):
    L = integrator.load_library()
    src = open(HDR).read()
    for name in ('mtsgpu_develop_ldr', 'mtsgpu_develop_ldr_device'):
        assert hasattr(L, name) and name in integrator.EXPORTS
        assert ('int %s(' % name) in src
    assert L.mtsgpu_abi_version() == abi.ABI_VERSION == 8
    assert (abi.TONEMAP_GAMMA, abi.TONEMAP_REINHARD) == (0, 1)
    # sizeof / offsetof from the C compiler == the ctypes mirror
    py, cname = abi.DevelopLdrParams, 'mtsgpu_develop_ldr_params'
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, 'int main(void) {',
             'printf("size %%zu\\n", sizeof(%s));' % cname,
             'printf("enum %d %d\\n", MTSGPU_TONEMAP_GAMMA, MTSGPU_TONEMAP_REINHARD);']
    for f in py._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(%s, %s));' % (f[0], cname, f[0]))
    lines.append('return 0; }')
    c = tmp_path / 'layout.c'
    c.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-o', str(exe), str(c)], check=True)
    out = [l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                             text=True).stdout.splitlines()]
    got = {l[0]: l[1:] for l in out}
    assert int(got['size'][0]) == C.sizeof(py) == 36 and got['enum'] == ['0', '1']
    assert [f[0] for f in py._fields_] == ['film_width', 'film_height', 'border', 'pixel_format', 'tonemap_method',
                                           'gamma', 'exposure', 'key', 'burn']
    for f in py._fields_:
        assert int(got[f[0]][0]) == getattr(py, f[0]).offset, f[0]
    # NULL context or params: MTSGPU_EINVAL, no device needed
    p = F.LDRFilm().develop_params((4, 4, 5), 1)
    buf = (C.c_float * 80)()
    out8 = (C.c_uint8 * 12)()
    assert L.mtsgpu_develop_ldr(None, C.byref(p), buf, out8, None) == abi.EINVAL
    assert L.mtsgpu_develop_ldr(None, None, None, None, None) == abi.EINVAL
    assert L.mtsgpu_develop_ldr_device(None, C.byref(p), None, None, None, None) == abi.EINVAL
    assert L.mtsgpu_develop_ldr_device(None, None, None, None, None, None) == abi.EINVAL
