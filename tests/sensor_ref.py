"""Shared pieces of the sensor tests (test_sensors_host.py, test_gpu_sensors.py): numpy float32
restatements of ThinLens / OrthographicCamera / TelecentricLensCamera::sampleRayDifferential
(thinlens.cpp:324-361, orthographic.cpp:157-179, telecentric.cpp:224-255) in the reference's
operation order, and the first vertices of their rays in delta_ref.first_hits' form.

The oracle cannot configure these sensors: it reads the descriptor's old fields and renders the
scene as the pinhole of the same fov (the twin).  From it come the sample positions, the
aperture sample (oracle_sobol_sample of dimensions 2 and 3 of the sample's index), thinlens'
sampleToCamera and dx / dy (oracle_camera: perspective's, thinlens.cpp:180-193 builds the same
product) and the intersections of the restated rays.  The orthographic matrices are restated
here from mitsuba_amd.transform; the disk warp's sincosf is glibc's, through ctypes."""
import copy
import ctypes as C
import ctypes.util

import numpy as np

import delta_ref as dr
import fields_ref as fr
from mitsuba_amd.transform import Transform

f32 = np.float32
_libm = C.CDLL(ctypes.util.find_library('m') or 'libm.so.6')
_libm.sincosf.restype = None
_libm.sincosf.argtypes = [C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]


def sincosf(x):
    s, c = np.zeros(x.shape, f32), np.zeros(x.shape, f32)
    a, b = C.c_float(0), C.c_float(0)
    for i, v in enumerate(np.asarray(x, f32).reshape(-1)):
        _libm.sincosf(float(v), C.byref(a), C.byref(b))
        s.reshape(-1)[i], c.reshape(-1)[i] = a.value, b.value
    return s, c


def disk_concentric(u, v):
    """warp::squareToUniformDiskConcentric (warp.cpp:81-102)."""
    u, v = np.asarray(u, f32), np.asarray(v, f32)
    r1 = ((f32(2) * u).astype(f32) - f32(1)).astype(f32)
    r2 = ((f32(2) * v).astype(f32) - f32(1)).astype(f32)
    pi4, pi2 = f32(f32(np.pi) / f32(4)), f32(f32(np.pi) / f32(2))
    with np.errstate(divide='ignore', invalid='ignore'):
        a = (pi4 * (r2 / r1).astype(f32)).astype(f32)
        b = (pi2 - ((r1 / r2).astype(f32) * pi4).astype(f32)).astype(f32)
    first = (r1 * r1).astype(f32) > (r2 * r2).astype(f32)
    zero = (r1 == 0) & (r2 == 0)
    r = np.where(zero, f32(0), np.where(first, r1, r2)).astype(f32)
    phi = np.where(zero, f32(0), np.where(first, a, b)).astype(f32)
    s, c = sincosf(phi)
    return (r * c).astype(f32), (r * s).astype(f32)


def _vec(W, x, y, z):
    """Transform::operator()(Vector): the 3 x 3 product, left to right."""
    return np.stack([(((W[k, 0] * x).astype(f32) + (W[k, 1] * y).astype(f32)).astype(f32)
                      + (W[k, 2] * z).astype(f32)).astype(f32) for k in range(3)], -1)


def _affine(W, x, y, z):
    """Transform::transformAffine(Point) (transform.h:108-121): no division by w."""
    return np.stack([v.astype(f32) for v in fr._affine(np.asarray(W, f32).reshape(16), x, y, z)[:3]], -1)


def _normalize(v):
    ln = dr.length(v)
    return (v * (f32(1) / ln).astype(f32)[..., None]).astype(f32)


def ortho_matrices(s):
    """sampleToCamera, dx, dy of orthographic / telecentric configure() (crop = film)."""
    aspect = f32(f32(s.width) / f32(s.height))
    near, far = f32(s.nearClip), f32(s.farClip)
    ortho = Transform.scale_(f32(1), f32(1), f32(f32(1) / f32(far - near))) * Transform.translate_(f32(0), f32(0), -near)
    t = (Transform.scale_(f32(1), f32(1), f32(1)) * Transform.translate_(f32(-0.0), f32(-0.0), f32(0))
         * Transform.scale_(f32(-0.5), f32(f32(-0.5) * aspect), f32(1))
         * Transform.translate_(f32(-1), f32(f32(-1) / aspect), f32(0)) * ortho)
    m = np.asarray(t.inv, f32).reshape(16)
    irx, iry = f32(1) / f32(s.width), f32(1) / f32(s.height)
    p0 = fr.xf_point(m, np.array([[0, 0, 0]], f32))[0]
    dx = (fr.xf_point(m, np.array([[irx, 0, 0]], f32))[0] - p0).astype(f32)
    dy = (fr.xf_point(m, np.array([[0, iry, 0]], f32))[0] - p0).astype(f32)
    return m, dx, dy


def aperture_samples(ob, size, spp, scramble=0):
    """Sobol dimensions 2, 3 of every sample (records: pixel-major, sample-minor)."""
    L = ob.lib()
    pix = np.repeat(np.arange(size * size), spp)
    px, py = pix % size, pix // size
    j = np.tile(np.arange(spp), size * size)
    m = int(np.log2(size))
    idx = [L.oracle_sobol_lookup(m, int(jj), int(x), int(y), scramble) for x, y, jj in zip(px, py, j)]
    return (np.array([L.oracle_sobol_sample(i, 2, scramble) for i in idx], f32),
            np.array([L.oracle_sobol_sample(i, 3, scramble) for i in idx], f32))


def sensor_rays(sc, ob, sx, sy, ax=None, ay=None):
    """(o, d, mint, maxt) of sc.sensor's rays through film positions (sx, sy) with aperture
    samples (ax, ay) (thinlens, telecentric)."""
    s = sc.sensor
    sx, sy = np.asarray(sx, f32), np.asarray(sy, f32)
    W = np.asarray(s.toWorld, f32).reshape(4, 4)
    irx, iry = f32(1) / f32(s.width), f32(1) / f32(s.height)
    film = np.stack([(sx * irx).astype(f32), (sy * iry).astype(f32), np.zeros_like(sx)], -1)
    zero = np.zeros_like(sx)
    near, far = f32(s.nearClip), f32(s.farClip)
    if s.type == 'thinlens':
        m = fr.sample_to_camera(sc, ob)
        tx, ty = disk_concentric(ax, ay)
        tx, ty = (tx * f32(s.apertureRadius)).astype(f32), (ty * f32(s.apertureRadius)).astype(f32)
        nearP = fr.xf_point(m, film)
        fdist = (f32(s.focusDistance) / nearP[:, 2]).astype(f32)
        focus = (nearP * fdist[:, None]).astype(f32)
        ap = np.stack([tx, ty, zero], -1)
        dl = _normalize((focus - ap).astype(f32))
        inv_z = (f32(1) / dl[:, 2]).astype(f32)
        return (_affine(W, tx, ty, zero), _vec(W, dl[:, 0], dl[:, 1], dl[:, 2]), (near * inv_z).astype(f32),
                (far * inv_z).astype(f32))
    m, _, _ = ortho_matrices(s)
    p = np.stack([v.astype(f32) for v in fr._affine(m, film[:, 0], film[:, 1], film[:, 2])[:3]], -1)
    mint, maxt = np.full(sx.shape, near, f32), np.full(sx.shape, far, f32)
    if s.type == 'orthographic':
        d = _normalize(_vec(W, np.zeros(1, f32), np.zeros(1, f32), np.ones(1, f32)))[0]
        return _affine(W, p[:, 0], p[:, 1], zero), np.broadcast_to(d, p.shape).astype(f32).copy(), mint, maxt
    assert s.type == 'telecentric'
    scale_x = dr.length(_vec(W, np.ones(1, f32), np.zeros(1, f32), np.zeros(1, f32)))[0]
    scale_z = dr.length(_vec(W, np.zeros(1, f32), np.zeros(1, f32), np.ones(1, f32)))[0]
    tx, ty = disk_concentric(ax, ay)
    rad = f32(f32(s.apertureRadius) / scale_x)
    tx, ty = (tx * rad).astype(f32), (ty * rad).astype(f32)
    fz = np.full(sx.shape, f32(f32(s.focusDistance) / scale_z), f32)
    ox, oy = (tx + p[:, 0]).astype(f32), (ty + p[:, 1]).astype(f32)
    diff = np.stack([(p[:, 0] - ox).astype(f32), (p[:, 1] - oy).astype(f32), (fz - zero).astype(f32)], -1)
    return _affine(W, ox, oy, zero), _normalize(_vec(W, diff[:, 0], diff[:, 1], diff[:, 2])), mint, maxt


def pinhole_twin(sc):
    """The scene as the oracle reads it: the perspective sensor of the same fov and transform."""
    from mitsuba_amd.scene import Sensor
    s = sc.sensor
    twin = copy.copy(sc)
    twin.sensor = Sensor(fov=s.fov, fovAxis=s.fovAxis, nearClip=s.nearClip, farClip=s.farClip, toWorld=s.toWorld,
                         width=s.width, height=s.height)
    return twin


def sensor_first_hits(sc, twin, ob, sx, sy, ax=None, ay=None):
    """delta_ref.first_hits for sc.sensor's rays: the same dict, from the restated rays."""
    from mitsuba_amd.scene import BSDF
    o, d, mint, maxt = sensor_rays(sc, ob, sx, sy, ax, ay)
    geo = copy.copy(twin)
    geo.bsdfs = [BSDF('diffuse') for _ in twin.bsdfs]
    h = fr.oracle_intersect(geo, ob, o, d)
    uv = fr.hit_uv(geo, ob.trace_rays(geo, o, d, mint, maxt))
    n, s = h[:, 8:11].copy(), h[:, 11:14].copy()
    t = dr.cross(n, s)
    nd = -d
    wi = np.stack([dr.dot(nd, s), dr.dot(nd, t), dr.dot(nd, n)], -1)
    return dict(rd=d, valid=h[:, 0] != 0, p=h[:, 2:5].copy(), geoN=h[:, 5:8].copy(), n=n, s=s, t=t, wi=wi,
                shape=h[:, 14].astype(np.int64), uv=uv, o=o, its=h, mint=mint, maxt=maxt)
