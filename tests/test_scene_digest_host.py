"""The configured scene as a whole, on the host (no GPU needed): one FNV-1a hash per
HostScene member (mtsgpu_scene_digest_host) of scenes that between them reach every branch
of mtsg_configure_scene, against tests/golden/scene_digest.json.

The golden file pins what configure computes, so that moving its code cannot change a bit
of it unnoticed.  It is rewritten by `python tests/test_scene_digest_host.py` -- only when
a change of configure's output is the purpose of the work."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, reference_microfacet_dir   # (first: it makes mitsuba_amd importable)
import delta_ref as dr
from mitsuba_amd import abi, integrator, scenes
from mitsuba_amd.scene import BSDF, Checkerboard, Emitter, Mesh, Scene, Sensor, look_at
from mitsuba_amd.transform import Transform

GOLDEN_FILE = os.path.join(GOLDEN, 'scene_digest.json')
# HostScene's members in declaration order, as mtsgpu_scene_digest_host hashes them (include/mtsgpu.h)
MEMBERS = ('nodes hnodes tris prim_vtx dpdu positions normals face_n shapes bsdfs emitters deltas area_cdf em_cdf '
           'em_norm aabb_min aabb_max cam cam_lens film_w film_h bvh_depth env env_texels env_cdf_rows env_cdf_cols '
           'env_row_weights env_guide_rows env_guide_cols rtrans texcoords ext analytic').split()
TINY = dict(width=8, height=6, spp=1)


def _c1(materials='diffuse'):
    return scenes.build('C1', materials=materials, **TINY)[0]


def _with_sensor(sc, kind, **kw):
    s = sc.sensor
    args = dict(nearClip=s.nearClip, farClip=s.farClip, toWorld=s.toWorld, width=s.width, height=s.height)
    if kind == 'thinlens':
        args.update(fov=s.fov, fovAxis=s.fovAxis, apertureRadius=0.3, focusDistance=5.0)
    args.update(kw)
    sc.sensor = Sensor(type=kind, **args)
    return sc


def _mesh_variants():
    """Every way a triangle mesh gets its normals and tangents: supplied normals flipped, face
    normals flipped, computed normals flipped, texture coordinates with a singular UV map, a
    degenerate triangle (TriAccel k == 3), an emitting mesh on the default BSDF."""
    base = _c1()
    quad = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)], np.float32)
    idx = np.array([(0, 1, 2), (0, 2, 3)], np.uint32)
    nrm = np.array([(0, 0.6, 0.8), (0.6, 0, 0.8), (0, 0, 1), (0.8, 0, 0.6)], np.float32)
    tc = np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.float32)
    line = np.array([(0, 0, 2), (1, 0, 2), (2, 0, 2), (1, 1, 2)], np.float32)     # 0, 1, 2 are collinear
    flat_uv = np.array([(0.5, 0.5)] * 4, np.float32)
    meshes = [
        Mesh(quad + np.float32(3), idx, normals=nrm, bsdf=0, flipNormals=True),
        Mesh(quad + np.float32(5), idx, bsdf=1, faceNormals=True, flipNormals=True),
        Mesh(quad + np.float32(7), idx, texcoords=tc, bsdf=2, flipNormals=True),
        Mesh(line, np.array([(0, 1, 2), (0, 1, 3)], np.uint32), texcoords=flat_uv, bsdf=0),
        Mesh(quad + np.float32(9), idx, bsdf=-1),
        Mesh(quad + np.float32(11), idx, bsdf=-1, emitter=0),
    ]
    return Scene(base.sensor, meshes, base.bsdfs, [Emitter('area', radiance=(1.0, 2.0, 3.0), samplingWeight=2.0)])


def _furnace():
    """A constant emitter over analytic shapes, one behind a twosided BSDF (tests/test_oracle_shapes.py)."""
    sensor = Sensor(fov=30.0, fovAxis='x', toWorld=look_at(np.array([0, 0, -6.0]), np.array([0, 0, 0.0]), (0, 1, 0)),
                    width=8, height=6)
    white = BSDF('diffuse', reflectance=Checkerboard(color0=0.9, color1=1.3, uscale=3.0, vscale=2.0))
    meshes = [Mesh(shape='sphere', center=(0, 0, 0), radius=1.0, bsdf=0),
              Mesh(shape='disk', toWorld=Transform().scale(1.2).translate(0.5, 0.3, -1.5), bsdf=1)]
    return Scene(sensor, meshes, [white, BSDF('twosided', nested=[BSDF('diffuse', reflectance=1.0)])],
                 [Emitter('constant', radiance=(0.5, 0.25, 0.125))])


def _deltas():
    """Point, spot and directional emitters next to the area light (tests/delta_ref.py)."""
    t = Transform().rotate((1, 0, 0), 80.0).translate(2.5, 5.0, 2.5)
    ems = [Emitter('point', intensity=(30.0, 24.0, 12.0), position=(2.1, 4.4, 2.4)),
           Emitter('spot', intensity=(50.0, 60.0, 70.0), cutoffAngle=30.0, beamWidth=20.0, toWorld=t),
           Emitter('directional', irradiance=(3.0, 2.0, 1.0), direction=(0.2, -1.0, 0.1), samplingWeight=0.5)]
    return dr.delta_scene(ems, keep_area=True, **TINY)[0]


def _one_leaf():
    """Two triangles: the whole scene fits one leaf (the root node made by hand)."""
    base = _c1()
    return Scene(base.sensor, [copy.copy(base.meshes[-1])], base.bsdfs, base.emitters)


def _skewed():
    """Triangles at geometrically growing distances: the SAH peels them off one by one, the
    tree gets as deep as the builder lets it, and the forced median splits take over."""
    pos, idx = [], []
    for i in range(64):
        x = np.float32(2.0) ** i
        s = x * np.float32(0.01)
        pos += [(x, 0, 0), (x + s, 0, 0), (x, s, s)]
        idx.append((3 * i, 3 * i + 1, 3 * i + 2))
    base = _c1()
    return Scene(base.sensor, [Mesh(np.asarray(pos, np.float32), np.asarray(idx, np.uint32), bsdf=0, emitter=0,
                                    faceNormals=True)], base.bsdfs, base.emitters)


def _env(config):
    return scenes.build(config, env_size=(16, 8), blob=(8, 5), **TINY)[0]


SCENES = {
    'C1': _c1,
    'C3': lambda: _env('C3'),
    'C3_area_light': lambda: scenes.build('C3', env_size=(16, 8), blob=(8, 5), area_light=True, env_weight=0.5, **TINY)[0],
    'C4': lambda: scenes.build('C4', columns=(1, 2), seg=8, rings=2, **TINY)[0],
    'C5': lambda: _env('C5'),
    'cornell_rough': lambda: _c1('rough'),
    'cornell_plastic': lambda: _c1('plastic'),
    'cornell_smooth': lambda: _c1('smooth'),
    'cornell_shapes': lambda: _c1('shapes'),
    'mesh_variants': _mesh_variants,
    'furnace': _furnace,
    'deltas': _deltas,
    'thinlens': lambda: _with_sensor(_c1(), 'thinlens'),
    'orthographic': lambda: _with_sensor(_c1(), 'orthographic'),
    'telecentric': lambda: _with_sensor(_c1(), 'telecentric', apertureRadius=0.25, focusDistance=7.5),
    # the environment's bounding sphere grows by the sensor's own box (envmap_bsphere)
    'C3_thinlens': lambda: _with_sensor(_env('C3'), 'thinlens'),
    'C3_orthographic': lambda: _with_sensor(_env('C3'), 'orthographic'),
    'C3_telecentric': lambda: _with_sensor(_env('C3'), 'telecentric', apertureRadius=0.25, focusDistance=7.5),
    'one_leaf': _one_leaf,
    'skewed': _skewed,
}


def digest(sc):
    L = integrator.load_library()
    L.mtsgpu_scene_digest_host.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(C.c_uint64), C.c_size_t,
                                           C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]
    d = sc.desc()
    out, n, buf = (C.c_uint64 * 64)(), C.c_uint32(0), C.create_string_buffer(1024)
    rc = L.mtsgpu_scene_digest_host(C.byref(d), out, 64, C.byref(n), buf, 1024)
    assert rc == abi.OK, buf.value.decode()
    assert n.value == len(MEMBERS)
    return {m: '%016x' % out[i] for i, m in enumerate(MEMBERS)}


@pytest.fixture(autouse=True)
def _tables(monkeypatch):
    # roughplastic reads the reference's own rough-transmittance tables (tests/golden/microfacet),
    # not the ones a build generated, and configure's knobs are at their defaults
    monkeypatch.setenv('MTSGPU_MICROFACET_DIR', reference_microfacet_dir())
    for k in ('MITSUBA_DIR', 'MTSGPU_SAH_BINS', 'MTSGPU_SAH_CI', 'MTSGPU_LEAF_MAX', 'MTSGPU_NO_ENV_GUIDE'):
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


def test_golden_lists_the_scenes(golden):
    assert sorted(golden) == sorted(SCENES)
    assert all(list(v) == MEMBERS for v in golden.values())


@pytest.mark.parametrize('name', sorted(SCENES))
def test_scene_digest(golden, name):
    sc = SCENES[name]()
    got = digest(sc)
    assert got == digest(sc), 'two configure calls of one scene differ'
    differ = [m for m in MEMBERS if got[m] != golden[name][m]]
    assert not differ, '%s: members %s differ from the golden digest' % (name, differ)


def test_skewed_scene_reaches_the_forced_median():
    """The builder's own condition for a forced median split (bvh_build.cpp Builder::build:
    depth + lg + 2 >= kMaxDepth = 28, lg ~ log2(count / 2)) holds at some inner node of `skewed`."""
    refs = integrator.bvh_host(_skewed())[0][:, 12:14].view(np.int32)
    forced = []

    def walk(ref, depth):
        if ref < 0:
            return ~ref & 15
        count = sum(walk(int(c), depth + 1) for c in refs[ref])
        lg = 0
        while (2 << lg) * 2 < count:
            lg += 1
        forced.append(depth + lg + 2 >= 28)
        return count
    assert walk(0, 0) == 64 and any(forced)


if __name__ == '__main__':
    os.environ['MTSGPU_MICROFACET_DIR'] = reference_microfacet_dir()
    for k in ('MITSUBA_DIR', 'MTSGPU_SAH_BINS', 'MTSGPU_SAH_CI', 'MTSGPU_LEAF_MAX', 'MTSGPU_NO_ENV_GUIDE'):
        os.environ.pop(k, None)
    with open(GOLDEN_FILE, 'w') as f:
        json.dump({k: digest(SCENES[k]()) for k in sorted(SCENES)}, f, indent=1)
        f.write('\n')
