"""Host-side scene model mirroring the reference's plugin properties.

A `Scene` holds what Mitsuba 0.6 has after parsing and plugin construction
(SceneHandler -> PluginManager::createObject, src/librender/scenehandler.cpp):
world-space triangle meshes (the TriMesh that the obj/ply/serialized/cube shape
plugins produce, with their `toWorld` already applied), BSDF and emitter
parameters under the reference's property names, the perspective sensor, the
film and the sampler.  `Scene.desc()` packs it into the C-ABI structs of
include/mtsgpu.h; everything the reference derives in configure() is derived
behind the ABI by libmtsgpu.so.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import abi
from .transform import Transform, _normalize, coordinate_system, deg_to_rad, transform_has_scale

# IOR table entries used by the configs (src/bsdfs/ior.h:40-67)
IOR = {'vacuum': 1.0, 'air': 1.000277, 'water': 1.3330, 'bk7': 1.5046, 'glass': 1.5046,
       'diamond': 2.419, 'polypropylene': 1.49, 'acrylic glass': 1.49, 'fused quartz': 1.458}


def lookup_ior(v):
    if isinstance(v, str):
        return IOR[v.lower()]
    return float(v)


# sampler plugin names -> MTSGPU_SAMPLER_* (include/mtsgpu.h)
SAMPLERS = {'sobol': abi.SAMPLER_SOBOL, 'independent': abi.SAMPLER_INDEPENDENT,
            'independent-sfmt': abi.SAMPLER_SFMT_REPLAY, 'independent-sfmt-blocks': abi.SAMPLER_SFMT_BLOCKS}

@dataclass
class Checkerboard:
    """`checkerboard` texture (src/textures/checkerboard.cpp) with Texture2D's
    uv transform (src/librender/texture.cpp:81-121): uv' = uv * scale + offset,
    color0 where (2 (floor-mod of int(2u')) - 1) (2 (.. v') - 1) == 1."""
    color0: tuple = (0.4, 0.4, 0.4)
    color1: tuple = (0.2, 0.2, 0.2)
    uoffset: float = 0.0
    voffset: float = 0.0
    uscale: float = 1.0
    vscale: float = 1.0

    def fill(self, t):
        t.type = abi.TEX_CHECKERBOARD
        t.color0[:] = _spec(self.color0)
        t.color1[:] = _spec(self.color1)
        t.uoffset, t.voffset, t.uscale, t.vscale = self.uoffset, self.voffset, self.uscale, self.vscale

    def average(self):
        c0, c1 = np.asarray(_spec(self.color0), np.float32), np.asarray(_spec(self.color1), np.float32)
        return tuple(float(x) for x in ((c0 + c1) * np.float32(0.5)))


def _spec(v):
    """A Spectrum property: a float is Spectrum(value), a 3-tuple RGB."""
    if isinstance(v, (int, float, np.floating)):
        return (float(v),) * 3
    return tuple(float(x) for x in v)


BSDF_TYPES = {'diffuse': abi.BSDF_DIFFUSE, 'roughconductor': abi.BSDF_ROUGHCONDUCTOR,
              'roughdielectric': abi.BSDF_ROUGHDIELECTRIC, 'roughplastic': abi.BSDF_ROUGHPLASTIC,
              'conductor': abi.BSDF_CONDUCTOR, 'dielectric': abi.BSDF_DIELECTRIC,
              'plastic': abi.BSDF_PLASTIC, 'twosided': abi.BSDF_TWOSIDED,
              'mixturebsdf': abi.BSDF_MIXTURE, 'blendbsdf': abi.BSDF_BLEND, 'mask': abi.BSDF_MASK,
              'difftrans': abi.BSDF_DIFFTRANS, 'roughdiffuse': abi.BSDF_ROUGHDIFFUSE, 'phong': abi.BSDF_PHONG}

# the BSDFs that hold other BSDFs in `nested`
WRAPPERS = ('twosided', 'mixturebsdf', 'blendbsdf', 'mask')


@dataclass
class BSDF:
    """One of diffuse / roughconductor / roughdielectric / roughplastic /
    conductor / dielectric / plastic / twosided with Mitsuba property names.
    `reflectance` (diffuse), `diffuseReflectance` ((rough)plastic) and `alpha`
    (rough BSDFs, isotropic) may be a Checkerboard.  A twosided BSDF holds its
    one or two nested BSDFs in `nested` (twosided.cpp:63-103).

    The combinators hold theirs there too: `mixturebsdf` (weights=[...], one per nested
    BSDF, up to 8), `blendbsdf` (weight: a float or a Checkerboard; two nested) and `mask`
    (opacity: a spectrum or a Checkerboard; one nested).  One chain is supported,
    [mask] -> [twosided] -> [mixturebsdf | blendbsdf] -> leaf; the library refuses the
    rest when the scene is checked or uploaded.

    Three more leaves: `difftrans` (transmittance: a spectrum or a Checkerboard, default
    0.5), `roughdiffuse` (reflectance and alpha, default 0.2, each possibly a Checkerboard;
    useFastApprox) and `phong` (exponent, default 30; diffuseReflectance, possibly a
    Checkerboard, default 0.5; specularReflectance, default 0.2).  phong and roughdiffuse may
    be nested in twosided and the combinators; difftrans may not."""
    type: str = 'diffuse'
    reflectance: object = (0.5, 0.5, 0.5)
    distribution: str = 'beckmann'
    alpha: object = None
    alphaU: Optional[float] = None
    alphaV: Optional[float] = None
    sampleVisible: bool = True
    specularReflectance: Optional[tuple] = None   # None: the plugin's default, Spectrum(1); phong's is 0.2 (phong.cpp:63)
    specularTransmittance: tuple = (1.0, 1.0, 1.0)
    eta: Optional[tuple] = None        # roughconductor: explicit RGB eta/k override `material`
    k: Optional[tuple] = None
    material: Optional[str] = 'Cu'     # roughconductor.cpp:174 default
    extEta: object = 'air'
    intIOR: object = None              # roughdielectric: bk7 (roughdielectric.cpp:186); roughplastic: polypropylene
    extIOR: object = 'air'
    diffuseReflectance: object = (0.5, 0.5, 0.5)   # roughplastic.cpp:201
    nonlinear: bool = False
    rtransDir: Optional[str] = None    # where data/microfacet/<distribution>.dat is looked up first (rtrans.py)
    ensureEnergyConservation: bool = True
    nested: list = field(default_factory=list)   # twosided: [front] or [front, back]; the combinators' children
    weights: Optional[list] = None     # mixturebsdf 'weights'
    weight: object = 0.5               # blendbsdf 'weight' (blendbsdf.cpp:63)
    opacity: object = 0.5              # mask 'opacity' (mask.cpp:76-77)
    exponent: float = 30.0             # phong 'exponent' (phong.cpp:65)
    transmittance: object = (0.5, 0.5, 0.5)   # difftrans 'transmittance' (difftrans.cpp:54-56)
    useFastApprox: bool = False        # roughdiffuse 'useFastApprox' (roughdiffuse.cpp:96)

    def __post_init__(self):
        if self.specularReflectance is None:
            self.specularReflectance = (0.2, 0.2, 0.2) if self.type == 'phong' else (1.0, 1.0, 1.0)

    def int_ior(self):
        if self.intIOR is not None:
            return self.intIOR
        return 'polypropylene' if self.type in ('roughplastic', 'plastic') else 'bk7'

    def to_desc(self):
        d = abi.BsdfDesc()
        if self.type not in BSDF_TYPES:
            raise NotImplementedError('BSDF plugin "%s" is not on the GPU path' % self.type)
        d.type = BSDF_TYPES[self.type]
        d.nested[0] = d.nested[1] = -1
        d.distribution = {'beckmann': abi.DISTR_BECKMANN, 'ggx': abi.DISTR_GGX,
                          'phong': abi.DISTR_PHONG, 'as': abi.DISTR_PHONG}[self.distribution.lower()]
        d.sample_visible = int(self.sampleVisible)
        d.ensure_energy_conservation = int(self.ensureEnergyConservation)
        if self.type == 'mixturebsdf':
            w = [] if self.weights is None else [float(x) for x in self.weights]
            if len(w) > abi.MIXTURE_MAX or len(self.nested) > abi.MIXTURE_MAX:
                raise NotImplementedError('mixturebsdf: more than %d nested BSDFs are not supported' % abi.MIXTURE_MAX)
            d.num_weights = len(w)
            d.weights[:len(w)] = w
        if self.type == 'blendbsdf':
            if isinstance(self.weight, Checkerboard):
                self.weight.fill(d.weight_tex)
            else:
                d.weight = float(self.weight)
        if self.type == 'mask':
            if isinstance(self.opacity, Checkerboard):
                self.opacity.fill(d.opacity_tex)
            else:
                d.opacity[:] = _spec(self.opacity)
        # MicrofacetDistribution(props) defaults alphaU = alphaV = 0.1 (microfacet.h:99-101,117-130)
        if isinstance(self.alpha, Checkerboard):
            if self.alphaU is not None or self.alphaV is not None:
                raise ValueError("Microfacet model: please specify either 'alpha' or 'alphaU'/'alphaV'.")
            au = av = 0.1
            self.alpha.fill(d.alpha_tex)
        elif self.alpha is not None:
            au = av = float(self.alpha)
        elif self.alphaU is not None or self.alphaV is not None:
            if self.alphaU is None or self.alphaV is None:
                raise ValueError("Microfacet model: both 'alphaU' and 'alphaV' must be specified.")
            au, av = float(self.alphaU), float(self.alphaV)
        else:
            au = av = 0.2 if self.type == 'roughdiffuse' else 0.1   # (roughdiffuse.cpp:97)
        d.alpha_u, d.alpha_v = au, av
        if self.type == 'phong':
            if isinstance(self.exponent, Checkerboard):
                raise NotImplementedError("phong: a textured 'exponent' is not on the GPU path")
            d.exponent = float(self.exponent)
        if self.type == 'phong' and isinstance(self.specularReflectance, Checkerboard):
            raise NotImplementedError("phong: a textured 'specularReflectance' is not on the GPU path")
        if self.type == 'difftrans':
            if isinstance(self.transmittance, Checkerboard):
                self.transmittance.fill(d.transmittance_tex)
            else:
                d.transmittance[:] = _spec(self.transmittance)
        d.use_fast_approx = int(self.useFastApprox)
        if isinstance(self.reflectance, Checkerboard):
            if self.type in ('diffuse', 'roughdiffuse'):
                self.reflectance.fill(d.reflectance_tex)
        else:
            d.reflectance[:] = _spec(self.reflectance)
        d.specular_reflectance[:] = _spec(self.specularReflectance)
        d.specular_transmittance[:] = _spec(self.specularTransmittance)
        if self.type in ('roughconductor', 'conductor'):
            # intEta/intK from the material, overridden by explicit 'eta'/'k' (roughconductor.cpp:172-190)
            from .conductors import conductor_rgb
            eta, k = conductor_rgb(self.material or 'Cu')
            d.eta[:] = self.eta if self.eta is not None else eta
            d.k[:] = self.k if self.k is not None else k
        if self.type in ('roughplastic', 'plastic', 'phong'):
            if isinstance(self.diffuseReflectance, Checkerboard):
                self.diffuseReflectance.fill(d.reflectance_tex)
            else:
                d.diffuse_reflectance[:] = _spec(self.diffuseReflectance)
            d.nonlinear = int(self.nonlinear)
        if self.type == 'roughplastic':
            from .rtrans import table_bytes
            data = table_bytes(self.distribution, [self.rtransDir])
            buf = C.create_string_buffer(data, len(data))
            d.rtrans_data = C.cast(buf, C.c_void_p)
            d.rtrans_bytes = len(data)
            d._keep = buf                  # the buffer lives as long as the descriptor
        d.ext_eta = lookup_ior(self.extEta)
        d.int_ior = lookup_ior(self.int_ior())
        d.ext_ior = lookup_ior(self.extIOR)
        return d


@dataclass
class Emitter:
    """`area` (src/emitters/area.cpp), `envmap` (src/emitters/envmap.cpp) or
    `constant` (src/emitters/constant.cpp: a uniform `radiance` environment).

    envmap: `bitmap` is the decoded lat-long image, (H, W, 3) linear RGB float32
    (what Bitmap(EAuto, stream) yields for an RGB EXR/PFM/HDR file), `scale` and
    `toWorld` (a transform.Transform) as in the XML.

    The delta emitters `point` (src/emitters/point.cpp: `intensity`, `position` xor
    `toWorld`), `spot` (spot.cpp: `intensity`, `toWorld`, `cutoffAngle` and `beamWidth`
    in degrees; no projection texture) and `directional` (directional.cpp: `irradiance`,
    `direction` xor `toWorld`, which must not scale).  `position` and `direction` become
    the transform the plugins build, in float32: Transform::translate, and
    Transform::lookAt(0, d, u) with u from coordinateSystem(normalize(direction)).
    Spectrum::getD65() is 1 in the RGB build, so every default intensity is 1."""
    type: str = 'area'
    radiance: tuple = (1.0, 1.0, 1.0)
    samplingWeight: float = 1.0
    bitmap: Optional[np.ndarray] = None
    scale: float = 1.0
    toWorld: object = None
    intensity: Optional[tuple] = None      # point, spot
    irradiance: Optional[tuple] = None     # directional
    position: Optional[tuple] = None       # point
    direction: Optional[tuple] = None      # directional
    cutoffAngle: float = 20.0              # spot (spot.cpp:70-71)
    beamWidth: Optional[float] = None      # spot: 3/4 cutoffAngle

    TYPES = {'area': abi.EMITTER_AREA, 'envmap': abi.EMITTER_ENVMAP, 'constant': abi.EMITTER_CONSTANT,
             'point': abi.EMITTER_POINT, 'spot': abi.EMITTER_SPOT, 'directional': abi.EMITTER_DIRECTIONAL}
    DELTA = ('point', 'spot', 'directional')

    def __post_init__(self):
        if self.type not in self.TYPES:
            raise ValueError('emitter type "%s"' % self.type)
        f32 = np.float32
        if self.type == 'point' and self.position is not None:          # point.cpp:60-66
            if self.toWorld is not None:
                raise ValueError("Only one of the parameters 'position' and 'toWorld' can be used!'")
            self.toWorld = Transform.translate_(*[f32(x) for x in self.position])
        if self.type == 'directional':                                   # directional.cpp:59-72
            if self.direction is not None:
                if self.toWorld is not None:
                    raise ValueError("Only one of the parameters 'direction' and 'toWorld'can be used at a time!")
                d = _normalize(np.asarray(self.direction, f32))
                u = coordinate_system(d)[0]
                self.toWorld = Transform.look_at_((0.0, 0.0, 0.0), d, u)
            elif self.toWorld is not None and transform_has_scale(self.toWorld):
                raise ValueError('Scale factors in the emitter-to-world transformation are not allowed!')
        if self.type == 'spot':                                          # spot.cpp:70-74
            if self.beamWidth is None:
                self.beamWidth = float(f32(f32(self.cutoffAngle) * f32(f32(3.0) / f32(4.0))))
            if not (deg_to_rad(self.cutoffAngle) >= deg_to_rad(self.beamWidth)):
                raise ValueError("Assertion 'm_cutoffAngle >= m_beamWidth' failed")
        if self.type in self.DELTA:
            v = self.irradiance if self.type == 'directional' else self.intensity
            if v is not None:
                self.radiance = tuple(float(x) for x in v)
            if self.type == 'directional':
                self.irradiance = tuple(self.radiance)
            else:
                self.intensity = tuple(self.radiance)

    def to_desc(self):
        d = abi.EmitterDesc()
        d.type = self.TYPES[self.type]
        d.radiance[:] = self.radiance
        d.sampling_weight = self.samplingWeight
        d.env_scale = self.scale
        if self.type == 'spot':
            d.cutoff_angle, d.beam_width = self.cutoffAngle, self.beamWidth
        if self.toWorld is not None:
            d.env_to_world[:] = [float(x) for x in np.asarray(self.toWorld.m, np.float32).reshape(-1)]
            d.env_to_world_inv[:] = [float(x) for x in np.asarray(self.toWorld.inv, np.float32).reshape(-1)]
        else:
            d.env_to_world[:] = [float(x) for x in np.eye(4, dtype=np.float32).reshape(-1)]
            d.env_to_world_inv[:] = [float(x) for x in np.eye(4, dtype=np.float32).reshape(-1)]
        return d


@dataclass
class Mesh:
    """A shape: a world-space triangle mesh (obj/ply/serialized/cube) or, with
    `shape` = 'rectangle' / 'disk' / 'sphere', an analytic shape intersected
    exactly (src/shapes/{rectangle,disk,sphere}.cpp) -- then positions/indices
    are None and toWorld (+ its carried inverse), center and radius apply."""
    positions: Optional[np.ndarray] = None   # (n,3) float32, world space
    indices: Optional[np.ndarray] = None     # (m,3) uint32
    normals: Optional[np.ndarray] = None
    texcoords: Optional[np.ndarray] = None
    bsdf: int = -1
    emitter: int = -1
    faceNormals: bool = False
    flipNormals: bool = False
    name: str = ''
    shape: str = 'trimesh'
    toWorld: object = None                   # 'toWorld': transform.Transform or 4x4 (rectangle / disk / sphere)
    toWorldInv: Optional[np.ndarray] = None  # its inverse as the reference's Transform carries it
    center: tuple = (0.0, 0.0, 0.0)          # sphere
    radius: float = 1.0                      # sphere

    @property
    def analytic(self):
        return self.shape != 'trimesh'


@dataclass
class Sensor:
    fov: float = 39.3077
    fovAxis: str = 'x'
    nearClip: float = 1e-2
    farClip: float = 1e4
    toWorld: np.ndarray = field(default_factory=lambda: np.eye(4, dtype=np.float32))
    width: int = 768
    height: int = 576
    # 'perspective' | 'thinlens' | 'orthographic' | 'telecentric' (src/sensors); fov and
    # fovAxis belong to the first two.  shutterOpen == shutterClose: no time sample
    type: str = 'perspective'
    apertureRadius: Optional[float] = None   # thinlens: required (0 becomes Epsilon); telecentric: 0
    focusDistance: Optional[float] = None    # thinlens, telecentric: farClip (sensor.cpp:162)

    TYPES = ('perspective', 'thinlens', 'orthographic', 'telecentric')

    def __post_init__(self):
        if self.type not in self.TYPES:
            raise ValueError('sensor type "%s" (%s)' % (self.type, ', '.join(self.TYPES)))
        lens = self.type in ('thinlens', 'telecentric')
        if not lens and (self.apertureRadius is not None or self.focusDistance is not None):
            raise ValueError("sensor '%s' has no 'apertureRadius' / 'focusDistance'" % self.type)
        if self.type == 'thinlens':                                      # thinlens.cpp:131-142
            if self.apertureRadius is None:
                raise ValueError('Property "apertureRadius" has not been specified!')
            if self.apertureRadius == 0:
                self.apertureRadius = 1e-4                               # Epsilon
            if transform_has_scale(Transform(np.asarray(self.toWorld, np.float32).reshape(4, 4))):
                raise ValueError('Scale factors in the camera-to-world transformation are not allowed!')
        if self.type == 'telecentric' and self.apertureRadius is None:   # telecentric.cpp:81
            self.apertureRadius = 0.0
        if lens and self.focusDistance is None:
            self.focusDistance = self.farClip


def look_at(origin, target, up):
    """Transform::lookAt (src/libcore/transform.cpp:191-214), float32."""
    p = np.asarray(origin, np.float32)
    t = np.asarray(target, np.float32)
    up = np.asarray(up, np.float32)

    def normalize(v):
        ln = np.float32(np.sqrt(np.float32(v[0] * v[0] + v[1] * v[1]) + np.float32(v[2] * v[2])))
        r = np.float32(1.0) / ln
        return (v * r).astype(np.float32)

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2],
                         a[0] * b[1] - a[1] * b[0]], np.float32)
    d = normalize((t - p).astype(np.float32))
    left = normalize(cross(up, d))
    new_up = cross(d, left)
    m = np.zeros((4, 4), np.float32)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = left, new_up, d, p
    m[3, 3] = 1
    return m


class Scene:
    """Scene after plugin construction (the C-ABI scene description)."""

    def __init__(self, sensor: Sensor, meshes: List[Mesh], bsdfs: List[BSDF], emitters: List[Emitter], name=''):
        self.sensor, self.meshes, self.bsdfs, self.emitters, self.name = sensor, meshes, bsdfs, emitters, name

    @property
    def num_triangles(self):
        """Primitives of the acceleration structure (an analytic shape counts one)."""
        return sum(1 if m.analytic else int(m.indices.shape[0]) for m in self.meshes)

    def flat_bsdfs(self):
        """The BSDF list as desc() packs it: the nested BSDFs of twosided, mixturebsdf, blendbsdf
        and mask go after the scene's own (mesh indices stay valid), a nested wrapper's own
        children after those; (list, {wrapper index: [nested indices]})."""
        flat = list(self.bsdfs)
        nested_idx = {}
        i = 0
        while i < len(flat):
            b = flat[i]
            if b.type in WRAPPERS:
                if b.type == 'twosided' and not 1 <= len(b.nested) <= 2:
                    raise ValueError('twosided: one or two nested BSDFs (twosided.cpp:82-87, 161-170)')
                if b.type == 'blendbsdf' and len(b.nested) != 2:
                    raise ValueError('blendbsdf: BSDF count mismatch: expected two nested BSDF instances!')
                if b.type == 'mask' and len(b.nested) != 1:
                    raise ValueError('mask: A child BSDF is required' if not b.nested
                                     else 'mask: only a single nested BSDF can be added')
                nested_idx[i] = []
                for nb in b.nested:
                    nested_idx[i].append(len(flat))
                    flat.append(nb)
            i += 1
        return flat, nested_idx

    def desc(self):
        """Pack into abi.SceneDesc; the returned object keeps every buffer alive."""
        keep = []
        md = (abi.MeshDesc * len(self.meshes))()
        for i, m in enumerate(self.meshes):
            if m.analytic:
                md[i].shape_type = {'rectangle': abi.SHAPE_RECTANGLE, 'disk': abi.SHAPE_DISK,
                                    'sphere': abi.SHAPE_SPHERE}[m.shape]
                md[i].bsdf, md[i].emitter = m.bsdf, m.emitter
                md[i].flip_normals = int(m.flipNormals)
                md[i].has_to_world = int(m.toWorld is not None)
                tw, twi = m.toWorld, m.toWorldInv
                if hasattr(tw, 'inv'):           # a transform.Transform: matrix + carried inverse
                    tw, twi = tw.m, tw.inv
                T = np.eye(4, dtype=np.float32) if tw is None else np.asarray(tw, np.float32)
                md[i].to_world[:] = [float(x) for x in T.reshape(-1)]
                if twi is not None:
                    md[i].to_world_inv[:] = [float(x) for x in np.asarray(twi, np.float32).reshape(-1)]
                elif tw is None:
                    md[i].to_world_inv[:] = [float(x) for x in T.reshape(-1)]
                md[i].center[:] = [float(x) for x in m.center]
                md[i].radius = float(m.radius)
                continue
            pos = np.ascontiguousarray(m.positions, np.float32)
            idx = np.ascontiguousarray(m.indices, np.uint32)
            nrm = None if m.normals is None else np.ascontiguousarray(m.normals, np.float32)
            uv = None if m.texcoords is None else np.ascontiguousarray(m.texcoords, np.float32)
            keep += [pos, idx, nrm, uv]
            md[i].positions = abi.fptr(pos)
            md[i].normals = abi.fptr(nrm)
            md[i].texcoords = abi.fptr(uv)
            md[i].indices = abi.uptr(idx)
            md[i].num_vertices = pos.shape[0]
            md[i].num_triangles = idx.shape[0]
            md[i].bsdf, md[i].emitter = m.bsdf, m.emitter
            md[i].face_normals, md[i].flip_normals = int(m.faceNormals), int(m.flipNormals)
        flat, nested_idx = self.flat_bsdfs()
        bd = (abi.BsdfDesc * max(1, len(flat)))()
        for i, b in enumerate(flat):
            bdi = b.to_desc()
            keep.append(getattr(bdi, '_keep', None))
            if i in nested_idx and b.type == 'mixturebsdf':
                bdi.num_children = len(nested_idx[i])
                for k, j in enumerate(nested_idx[i][:abi.MIXTURE_MAX]):
                    bdi.children[k] = j
            elif i in nested_idx:
                for k, j in enumerate(nested_idx[i]):
                    bdi.nested[k] = j
            bd[i] = bdi
        ed = (abi.EmitterDesc * max(1, len(self.emitters)))()
        for i, e in enumerate(self.emitters):
            ed[i] = e.to_desc()
            if e.type == 'envmap':
                if e.bitmap is None:
                    raise ValueError('envmap emitter needs a bitmap')
                img = np.ascontiguousarray(e.bitmap, np.float32)
                keep.append(img)
                ed[i].env_rgb = abi.fptr(img)
                ed[i].env_height, ed[i].env_width = img.shape[0], img.shape[1]
        d = abi.SceneDesc()
        d.meshes, d.num_meshes = md, len(self.meshes)
        d.bsdfs, d.num_bsdfs = bd, len(flat)
        d.emitters, d.num_emitters = ed, len(self.emitters)
        s = self.sensor
        d.sensor.fov = s.fov
        d.sensor.fov_axis = {'x': abi.FOV_X, 'y': abi.FOV_Y, 'diagonal': abi.FOV_DIAGONAL,
                             'smaller': abi.FOV_SMALLER, 'larger': abi.FOV_LARGER}[s.fovAxis]
        d.sensor.near_clip, d.sensor.far_clip = s.nearClip, s.farClip
        d.sensor.to_world[:] = [float(x) for x in np.asarray(s.toWorld, np.float32).reshape(-1)]
        d.sensor.film_width, d.sensor.film_height = s.width, s.height
        d.sensor.type = {'perspective': abi.SENSOR_PERSPECTIVE, 'thinlens': abi.SENSOR_THINLENS,
                         'orthographic': abi.SENSOR_ORTHOGRAPHIC, 'telecentric': abi.SENSOR_TELECENTRIC}[s.type]
        d.sensor.aperture_radius = s.apertureRadius or 0.0
        d.sensor.focus_distance = s.focusDistance or 0.0
        d._keep = (keep, md, bd, ed)
        return d


@dataclass
class PathIntegrator:
    """Properties of the reference `path` plugin (MonteCarloIntegrator ctor,
    src/librender/integrator.cpp:190-225) plus sampler/film settings."""
    maxDepth: int = -1
    rrDepth: int = 5
    strictNormals: bool = False
    hideEmitters: bool = False
    sampleCount: int = 4           # sobol 'sampleCount' (sobol.cpp:87)
    scramble: int = 0
    rfilter: str = 'gaussian'      # film default (film.cpp:93)
    rfilterParam: float = 0.5      # box radius / gaussian stddev
    hasAlpha: bool = False         # hdrfilm pixelFormat default "rgb" (hdrfilm.cpp:216)
    crop: Optional[tuple] = None   # hdrfilm crop window (x0, y0, w, h) (film.cpp:35-43); None = whole film
    film: Optional['HDRFilm'] = None   # hdrfilm output format (film.py); None = the hdrfilm defaults
    # 'sobol', 'independent' (counter-based streams), 'independent-sfmt' (the reference's
    # SFMT19937 stream of a one-worker render, replayed) or 'independent-sfmt-blocks' (one
    # SFMT clone per 32x32 block): include/mtsgpu.h MTSGPU_SAMPLER_*
    sampler: str = 'sobol'

    def __post_init__(self):
        if self.sampler not in SAMPLERS:
            raise ValueError('sampler "%s" (%s)' % (self.sampler, ', '.join(SAMPLERS)))
        if self.rrDepth <= 0:
            raise ValueError("'rrDepth' must be set to a value greater than zero!")
        if self.maxDepth <= 0 and self.maxDepth != -1:
            raise ValueError("'maxDepth' must be set to -1 (infinite) or a value greater than zero!")
        if self.film is None:
            from .film import HDRFilm
            self.film = HDRFilm()

    def params(self, width, height, x0=0, y0=0, w=None, h=None, row_block=0, row_stride=1, row_phase=0):
        p = abi.RenderParams()
        p.spp = self.sampleCount
        p.scramble = self.scramble
        p.max_depth, p.rr_depth = self.maxDepth, self.rrDepth
        p.strict_normals, p.hide_emitters = int(self.strictNormals), int(self.hideEmitters)
        p.has_alpha = int(self.hasAlpha)
        p.rfilter = {'box': abi.RFILTER_BOX, 'gaussian': abi.RFILTER_GAUSSIAN}[self.rfilter]
        p.rfilter_param = self.rfilterParam
        p.x0, p.y0 = x0, y0
        p.width = width - x0 if w is None else w
        p.height = height - y0 if h is None else h
        p.row_block, p.row_stride, p.row_phase = row_block, row_stride, row_phase
        p.integrator = abi.INTEGRATOR_PATH
        p.sampler = SAMPLERS[self.sampler]
        return p


@dataclass
class VolpathIntegrator(PathIntegrator):
    """The reference `volpath` plugin (MIVolumetricPathTracer,
    src/integrators/path/volpath.cpp) on scenes without participating media:
    path's properties; shadow rays are Scene::evalTransmittance segments to the
    sampled emitter point, the strictNormals test and the path-length count
    follow volpath.cpp.  Media are out of scope."""

    def params(self, *a, **kw):
        p = super().params(*a, **kw)
        p.integrator = abi.INTEGRATOR_VOLPATH
        return p


@dataclass
class DirectIntegrator(PathIntegrator):
    """Properties of the reference `direct` plugin (MIDirectIntegrator,
    src/integrators/direct/direct.cpp:90-135): `shadingSamples` sets both
    `emitterSamples` and `bsdfSamples` unless given; strictNormals/hideEmitters
    as in `path`.  Sampler and film settings as PathIntegrator (maxDepth and
    rrDepth are unused)."""
    shadingSamples: int = 1
    emitterSamples: Optional[int] = None
    bsdfSamples: Optional[int] = None

    def __post_init__(self):
        super().__post_init__()
        if self.emitterSamples is None:
            self.emitterSamples = self.shadingSamples
        if self.bsdfSamples is None:
            self.bsdfSamples = self.shadingSamples
        if self.emitterSamples + self.bsdfSamples <= 0 or min(self.emitterSamples, self.bsdfSamples) < 0:
            raise ValueError('direct: emitterSamples + bsdfSamples must be positive (direct.cpp:106)')

    def params(self, *a, **kw):
        p = super().params(*a, **kw)
        p.integrator = abi.INTEGRATOR_DIRECT
        p.emitter_samples, p.bsdf_samples = self.emitterSamples, self.bsdfSamples
        return p


# FieldIntegrator::EField (field.cpp:57-67) = MTSGPU_FIELD_*
FIELDS = ('position', 'relPosition', 'distance', 'geoNormal', 'shNormal', 'uv', 'albedo', 'shapeIndex',
          'primIndex')


@dataclass
class FieldIntegrator:
    """The reference `field` plugin (FieldIntegrator, src/integrators/misc/field.cpp:
    55-187): one field of the camera ray's intersection record per sample;
    `undefined` (a float or three) is the value where the ray hits nothing."""
    field: str
    undefined: object = 0.0

    def __post_init__(self):
        if self.field not in FIELDS:       # field.cpp:91-93
            raise ValueError("Invalid 'field' parameter. Must be one of 'position', 'relPosition', 'distance', "
                             "'geoNormal', 'shNormal', 'primIndex', 'shapeIndex', or 'uv'!")
        u = np.asarray(self.undefined, np.float32).reshape(-1)
        if u.size not in (1, 3):
            raise ValueError("'undefined' must be a float or a spectrum of three values")
        self.undefined = tuple(float(x) for x in (u if u.size == 3 else np.repeat(u, 3)))

    def to_desc(self):
        d = abi.FieldDesc()
        d.field = FIELDS.index(self.field)
        d.undefined[:] = self.undefined
        return d


# the sampler / film settings every integrator here carries (the reference keeps them on the sensor)
_SETTINGS = ('sampleCount', 'scramble', 'rfilter', 'rfilterParam', 'crop', 'film', 'sampler')


class MultiChannelIntegrator:
    """The reference `multichannel` plugin (MultiChannelIntegrator, src/integrators/
    misc/multichannel.cpp:87-262): several nested integrators run per sample, each
    into its own channels of the film.  `children` are FieldIntegrators and at most
    one radiance integrator (path / volpath / direct), at any position.  The sampler
    and film settings (sampleCount, scramble, sampler, rfilter, rfilterParam, crop,
    film) are those of the radiance integrator unless given here; alpha is always
    opacity (renderBlock never strips EOpacity, multichannel.cpp:181-215)."""

    def __init__(self, children, **settings):
        self.children = list(children)
        if not self.children:              # multichannel.cpp:131-132
            raise ValueError('No sub-integrators were supplied to the multi-channel integrator!')
        for c in self.children:
            if not isinstance(c, (FieldIntegrator, PathIntegrator)):
                raise ValueError('multichannel: nested integrators must be field, path, volpath or direct')
        radiance = [c for c in self.children if isinstance(c, PathIntegrator)]
        if len(radiance) > 1:
            # renderBlock hands every nested Li the one sampler (multichannel.cpp:208-214): the
            # second radiance integrator continues the first one's sampler dimensions, which a
            # separate render of it cannot reproduce
            raise NotImplementedError('multichannel: more than one radiance integrator (path / volpath / direct): '
                                      'in the reference the second one continues the first one\'s sampler '
                                      'dimensions, which a separate render cannot reproduce')
        if len(self.children) - len(radiance) > abi.MAX_FIELDS:
            raise ValueError('multichannel: at most %d field integrators' % abi.MAX_FIELDS)
        bad = set(settings) - set(_SETTINGS)
        if bad:
            raise TypeError('multichannel: unknown settings %s' % sorted(bad))
        base = radiance[0] if radiance else PathIntegrator()
        for k in _SETTINGS:
            setattr(self, k, settings.get(k, getattr(base, k)))
        self.hasAlpha = True
        if self.sampler not in SAMPLERS:
            raise ValueError('sampler "%s" (%s)' % (self.sampler, ', '.join(SAMPLERS)))

    @property
    def fields(self):
        return [c for c in self.children if isinstance(c, FieldIntegrator)]

    @property
    def radiance(self):
        """The nested radiance integrator with this integrator's sampler and film
        settings and an alpha channel, or None."""
        import dataclasses
        for c in self.children:
            if isinstance(c, PathIntegrator):
                return dataclasses.replace(c, hasAlpha=True, **{k: getattr(self, k) for k in _SETTINGS})
        return None

    def params(self, *a, **kw):
        """Render parameters of the field pass (its integrator fields are ignored)."""
        p = PathIntegrator(hasAlpha=True, **{k: getattr(self, k) for k in _SETTINGS}).params(*a, **kw)
        return p


def film_border(rfilter, param):
    """ReconstructionFilter border size (rfilter.cpp:50)."""
    import math
    radius = np.float32(param) + np.float32(1e-5) if rfilter == 'box' else np.float32(4) * np.float32(param)
    return int(math.ceil(np.float32(radius - np.float32(0.5))))
