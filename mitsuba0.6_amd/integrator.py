"""`PathTracer`: the host-side mirror of the reference's `path` Integrator plugin.

Mirrors MIPathTracer / MonteCarloIntegrator (src/integrators/path/path.cpp:110-
117, src/librender/integrator.cpp:190-225): same property names and the same
errors (raised as ValueError where the reference calls Log(EError)).  Rendering
goes through libmtsgpu.so's C-ABI; there is no CPU fallback -- without the HIP
library or a gfx950 device every call raises `NativeUnavailable`.
"""
import ctypes as C
import os

import numpy as np

from . import LIB_PATH, abi
from .scene import FieldIntegrator, MultiChannelIntegrator, PathIntegrator, film_border


class NativeUnavailable(RuntimeError):
    pass


class MtsgpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('%s (%d): %s' % (abi.STATUS_NAMES.get(code, '?'), code, msg))
        self.code = code


EXPORTS = ['mtsgpu_create', 'mtsgpu_upload_scene', 'mtsgpu_film_border', 'mtsgpu_render',
           'mtsgpu_render_device', 'mtsgpu_last_error', 'mtsgpu_destroy', 'mtsgpu_abi_version',
           'mtsgpu_debug_arith', 'mtsgpu_debug_scene_info', 'mtsgpu_debug_counters', 'mtsgpu_debug_sfmt', 'mtsgpu_develop', 'mtsgpu_develop_device', 'mtsgpu_check_scene',
           'mtsgpu_trace_rays', 'mtsgpu_group_create', 'mtsgpu_group_size', 'mtsgpu_group_upload_scene',
           'mtsgpu_group_render', 'mtsgpu_group_render_device', 'mtsgpu_group_member', 'mtsgpu_group_last_error',
           'mtsgpu_group_destroy', 'mtsgpu_trace_rays_ex', 'mtsgpu_debug_kdtree', 'mtsgpu_kdtree_host', 'mtsgpu_debug_libm',
           'mtsgpu_bvh_host', 'mtsgpu_group_member_params', 'mtsgpu_render_pixels',
           'mtsgpu_xml_bsdf', 'mtsgpu_xml_bsdf_ex', 'mtsgpu_scan_host', 'mtsgpu_index_host', 'mtsgpu_lookup_host',
           'mtsgpu_face_normals_host', 'mtsgpu_render_fields', 'mtsgpu_render_fields_device', 'mtsgpu_develop_multi',
           'mtsgpu_develop_multi_device', 'mtsgpu_albedo_factors_host', 'mtsgpu_combo_host', 'mtsgpu_leaf_host',
           'mtsgpu_develop_ldr',
           'mtsgpu_develop_ldr_device', 'mtsgpu_plan_host']

_lib = None


def load_library(path=None):
    """Load libmtsgpu.so (the in-tree build).  Raises NativeUnavailable if absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise NativeUnavailable('libmtsgpu.so not built: %s (run __graft_entry__.build())' % p)
    # PyTorch ships its own libamdhip64: load it first, so that libmtsgpu binds
    # to the same HIP runtime and device pointers / streams from torch are valid
    # in both (two runtimes in one process hide the GPU from the second one).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(p)
    P = C.POINTER
    L.mtsgpu_create.argtypes = [C.c_int, P(C.c_void_p)]
    L.mtsgpu_upload_scene.argtypes = [C.c_void_p, P(abi.SceneDesc)]
    L.mtsgpu_film_border.argtypes = [C.c_int32, C.c_float]
    L.mtsgpu_group_member_params.argtypes = [P(abi.RenderParams), C.c_int, C.c_int, P(abi.RenderParams)]
    L.mtsgpu_render_pixels.argtypes = [P(abi.RenderParams)]
    L.mtsgpu_render_pixels.restype = C.c_uint64
    L.mtsgpu_xml_bsdf.argtypes = [C.c_char_p, C.c_char_p, P(abi.XmlNode), C.c_int, P(abi.XmlProp), C.c_int,
                                  P(C.c_int), P(C.c_int), C.c_char_p, C.c_size_t]
    L.mtsgpu_xml_bsdf_ex.argtypes = [C.c_char_p, C.c_char_p, C.c_int32, P(C.c_char_p), P(C.c_char_p), C.c_int32,
                                     P(abi.XmlNode), C.c_int, P(abi.XmlProp), C.c_int, P(C.c_int), P(C.c_int),
                                     C.c_char_p, C.c_size_t]
    L.mtsgpu_render.argtypes = [C.c_void_p, P(abi.RenderParams), P(C.c_float), P(C.c_float), P(abi.Stats)]
    L.mtsgpu_render_device.argtypes = [C.c_void_p, P(abi.RenderParams), C.c_void_p, C.c_void_p, P(abi.Stats)]
    L.mtsgpu_last_error.argtypes = [C.c_void_p]
    L.mtsgpu_last_error.restype = C.c_char_p
    L.mtsgpu_destroy.argtypes = [C.c_void_p]
    L.mtsgpu_debug_arith.argtypes = [C.c_void_p, P(C.c_float), P(C.c_float), P(C.c_float), C.c_int]
    L.mtsgpu_debug_scene_info.argtypes = [C.c_void_p, P(C.c_uint32)]
    L.mtsgpu_debug_counters.argtypes = [C.c_void_p, P(C.c_uint64)]
    L.mtsgpu_debug_sfmt.argtypes = [C.c_void_p, C.c_uint64, C.c_int, P(C.c_uint64), C.c_int]
    L.mtsgpu_debug_libm.argtypes = [C.c_void_p, C.c_int, P(C.c_float), P(C.c_float), P(C.c_float), C.c_size_t,
                                    C.c_uint32]
    L.mtsgpu_trace_rays.argtypes = [C.c_void_p, P(C.c_float), C.c_uint32, C.c_int, P(C.c_float), P(C.c_double)]
    L.mtsgpu_check_scene.argtypes = [P(abi.SceneDesc), C.c_char_p, C.c_size_t]
    L.mtsgpu_develop.argtypes = [C.c_void_p, P(abi.DevelopParams), P(C.c_float), C.c_void_p]
    L.mtsgpu_develop_device.argtypes = [C.c_void_p, P(abi.DevelopParams), C.c_void_p, C.c_void_p, C.c_void_p]
    L.mtsgpu_trace_rays_ex.argtypes = [C.c_void_p, P(C.c_float), C.c_uint32, C.c_uint32, P(C.c_float), P(C.c_double)]
    L.mtsgpu_debug_kdtree.argtypes = [C.c_void_p, P(C.c_uint32), C.c_size_t, P(C.c_uint32), C.c_size_t, P(C.c_uint32)]
    L.mtsgpu_kdtree_host.argtypes = [P(abi.SceneDesc), P(C.c_uint32), C.c_size_t, P(C.c_uint32), C.c_size_t,
                                     P(C.c_uint32), C.c_char_p, C.c_size_t]
    L.mtsgpu_bvh_host.argtypes = [P(abi.SceneDesc), P(C.c_uint32), C.c_size_t, P(C.c_uint32), C.c_size_t,
                                  P(C.c_uint32), C.c_size_t, P(C.c_uint32), C.c_char_p, C.c_size_t]
    if hasattr(L, 'mtsgpu_scan_host'):   # added within ABI 8: an A/B library of an earlier build has none
        L.mtsgpu_scan_host.argtypes = [P(abi.SceneDesc), P(C.c_float), C.c_size_t, P(C.c_uint32)]
    if hasattr(L, 'mtsgpu_index_host'):   # added within ABI 8 as well
        L.mtsgpu_index_host.argtypes = [P(C.c_uint32), P(C.c_uint32), C.c_size_t, P(C.c_uint32), P(C.c_uint32)]
        L.mtsgpu_lookup_host.argtypes = [C.c_uint32, C.c_uint64, P(C.c_uint32), C.c_size_t, P(C.c_uint64)]
    if hasattr(L, 'mtsgpu_face_normals_host'):
        L.mtsgpu_face_normals_host.argtypes = [P(abi.SceneDesc), P(C.c_float), P(C.c_float), C.c_size_t, P(C.c_uint32)]
    if hasattr(L, 'mtsgpu_render_fields'):   # added within ABI 8 as well (field / multichannel integrators)
        L.mtsgpu_render_fields.argtypes = [C.c_void_p, P(abi.RenderParams), P(abi.FieldDesc), C.c_uint32, P(C.c_float),
                                           P(C.c_float), P(abi.Stats)]
        L.mtsgpu_render_fields_device.argtypes = [C.c_void_p, P(abi.RenderParams), P(abi.FieldDesc), C.c_uint32,
                                                  C.c_void_p, C.c_void_p, P(abi.Stats)]
        L.mtsgpu_develop_multi.argtypes = [C.c_void_p, P(abi.DevelopMultiParams), P(C.c_void_p), C.c_void_p]
        L.mtsgpu_develop_multi_device.argtypes = [C.c_void_p, P(abi.DevelopMultiParams), P(C.c_void_p), C.c_void_p,
                                                  C.c_void_p]
        L.mtsgpu_albedo_factors_host.argtypes = [P(abi.SceneDesc), P(C.c_float), C.c_char_p, C.c_size_t]
    if hasattr(L, 'mtsgpu_develop_ldr'):   # added within ABI 8 as well (ldrfilm)
        L.mtsgpu_develop_ldr.argtypes = [C.c_void_p, P(abi.DevelopLdrParams), P(C.c_float), C.c_void_p, P(C.c_float)]
        L.mtsgpu_develop_ldr_device.argtypes = [C.c_void_p, P(abi.DevelopLdrParams), C.c_void_p, C.c_void_p,
                                                C.c_void_p, P(C.c_float)]
    if hasattr(L, 'mtsgpu_plan_host'):   # added within ABI 8 as well (the render plan without a device)
        L.mtsgpu_plan_host.argtypes = [P(abi.SceneDesc), P(abi.RenderParams), C.c_uint32, C.c_int, P(C.c_uint64),
                                       P(C.c_uint64), C.c_size_t, C.c_char_p, C.c_size_t]
    L.mtsgpu_group_create.argtypes = [P(C.c_int), C.c_int, P(C.c_void_p)]
    L.mtsgpu_group_size.argtypes = [C.c_void_p]
    L.mtsgpu_group_upload_scene.argtypes = [C.c_void_p, P(abi.SceneDesc)]
    L.mtsgpu_group_render.argtypes = [C.c_void_p, P(abi.RenderParams), P(C.c_float), P(abi.Stats)]
    L.mtsgpu_group_render_device.argtypes = [C.c_void_p, P(abi.RenderParams), C.c_void_p, P(abi.Stats)]
    L.mtsgpu_group_member.argtypes = [C.c_void_p, C.c_int]
    L.mtsgpu_group_member.restype = C.c_void_p
    L.mtsgpu_group_last_error.argtypes = [C.c_void_p]
    L.mtsgpu_group_last_error.restype = C.c_char_p
    L.mtsgpu_group_destroy.argtypes = [C.c_void_p]
    if L.mtsgpu_abi_version() != abi.ABI_VERSION:
        raise NativeUnavailable('ABI version mismatch')
    if path is None:
        _lib = L
    return L


def check_scene(scene):
    """Host-only configure of `scene` (mtsgpu_check_scene): raises MtsgpuError with
    the reference's configure() error message, or returns None."""
    L = load_library()
    d = scene.desc()
    buf = C.create_string_buffer(1024)
    rc = L.mtsgpu_check_scene(C.byref(d), buf, 1024)
    if rc != 0:
        raise MtsgpuError(rc, buf.value.decode())


def albedo_factors_host(scene):
    """Per BSDF the scalar factor of its getDiffuseReflectance, configured on the host
    without a device (mtsgpu_albedo_factors_host): plastic 1 - fdrExt, roughplastic with
    a constant alpha the external table's evalDiffuse(alpha) (-1 for a textured alpha),
    1 for diffuse, 0 otherwise; in the order of scene.flat_bsdfs()."""
    L = load_library()
    d = scene.desc()
    out = np.zeros(max(1, d.num_bsdfs), np.float32)     # one per BSDF of scene.flat_bsdfs()
    buf = C.create_string_buffer(512)
    rc = L.mtsgpu_albedo_factors_host(C.byref(d), abi.fptr(out), buf, 512)
    if rc != 0:
        raise MtsgpuError(rc, buf.value.decode())
    return out[:d.num_bsdfs]


def combo_host(scene, index):
    """What configure() derives for the mixturebsdf / blendbsdf / mask at `index` of
    scene.flat_bsdfs(), on the host without a device (mtsgpu_combo_host): {'n', 'weights' (the
    mixture's m_weights after the rescale), 'cdf' (m_pdf's, n + 1 entries), 'pdf' (m_pdf[i]),
    'value' (blend weight x3 / mask opacity), 'flags'}."""
    L = load_library()
    L.mtsgpu_combo_host.argtypes = [C.POINTER(abi.SceneDesc), C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_int32),
                                    C.c_char_p, C.c_size_t]
    d = scene.desc()
    out = np.zeros(21, np.float32)
    flags = C.c_int32(0)
    buf = C.create_string_buffer(512)
    rc = L.mtsgpu_combo_host(C.byref(d), index, abi.fptr(out), C.byref(flags), buf, 512)
    if rc != 0:
        raise MtsgpuError(rc, buf.value.decode())
    n = int(out[0])
    cdf = out[9:10 + n].copy()
    return {'n': n, 'weights': out[1:1 + n].copy(), 'cdf': cdf, 'pdf': cdf[1:] - cdf[:-1], 'value': out[18:21].copy(),
            'flags': flags.value}


def leaf_host(scene, index):
    """What configure() derives for the difftrans / roughdiffuse / phong at `index` of
    scene.flat_bsdfs(), on the host without a device (mtsgpu_leaf_host): {'reflectance' (after
    ensureEnergyConservation; roughdiffuse reflectance, phong diffuseReflectance, difftrans
    transmittance; a checkerboard's color0), 'reflectance1' (its color1, or the same),
    'specularReflectance' and 'specularSamplingWeight' (phong), 'alpha' (roughdiffuse's alpha or
    phong's exponent), 'useFastApprox', 'flags'}."""
    L = load_library()
    L.mtsgpu_leaf_host.argtypes = [C.POINTER(abi.SceneDesc), C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_int32),
                                   C.c_char_p, C.c_size_t]
    d = scene.desc()
    out = np.zeros(16, np.float32)
    flags = C.c_int32(0)
    buf = C.create_string_buffer(512)
    rc = L.mtsgpu_leaf_host(C.byref(d), index, abi.fptr(out), C.byref(flags), buf, 512)
    if rc != 0:
        raise MtsgpuError(rc, buf.value.decode())
    return {'reflectance': out[0:3].copy(), 'reflectance1': out[3:6].copy(), 'specularReflectance': out[6:9].copy(),
            'specularSamplingWeight': out[12], 'alpha': out[14], 'useFastApprox': bool(out[15]), 'flags': flags.value}


KD_KEYS = ('nodes', 'indices', 'inner', 'leaves', 'nonempty_leaves', 'retracted', 'pruned', 'max_depth')


def bvh_host(scene):
    """The BVH the kernels traverse, built on the host without a device
    (mtsgpu_bvh_host): (nodes (N, 16) uint32 MtsgNode words, hnodes (N, 8) MtsgHNode
    words, qnodes (M, 16) MtsgQNode words, 4-wide inner-node levels)."""
    L = load_library()
    d = scene.desc()
    info = (C.c_uint32 * 4)()
    buf = C.create_string_buffer(512)
    rc = L.mtsgpu_bvh_host(C.byref(d), None, 0, None, 0, None, 0, info, buf, 512)
    if rc != 0:
        raise MtsgpuError(rc, buf.value.decode())
    n = np.zeros((info[0], 16), np.uint32)
    h = np.zeros((info[1], 8), np.uint32)
    q = np.zeros((info[2], 16), np.uint32)
    up = C.POINTER(C.c_uint32)
    rc = L.mtsgpu_bvh_host(C.byref(d), n.ctypes.data_as(up), n.size, h.ctypes.data_as(up), h.size,
                           q.ctypes.data_as(up), q.size, info, buf, 512)
    if rc != 0:
        raise MtsgpuError(rc, buf.value.decode())
    return n, h, q, int(info[3])


def scan_host(scene):
    """The tiny-scene scan's record layout, formed on the host without a device
    (mtsgpu_scan_host): (records (N, 12) uint32 MtsgTri words, the six group sizes,
    the six groups' pair counts).  N = 0 for a scene the kernels do not scan."""
    L = load_library()
    d = scene.desc()
    counts = (C.c_uint32 * 12)()
    rc = L.mtsgpu_scan_host(C.byref(d), None, 0, counts)
    if rc != 0:
        raise MtsgpuError(rc, 'mtsgpu_scan_host')
    rec = np.zeros((sum(counts[:6]), 12), np.uint32)
    rc = L.mtsgpu_scan_host(C.byref(d), rec.ctypes.data_as(C.POINTER(C.c_float)), rec.size, counts)
    if rc != 0:
        raise MtsgpuError(rc, 'mtsgpu_scan_host')
    return rec, list(counts[:6]), list(counts[6:])


def index_host(window, lane_round, row=(1, 1, 0), tile_shard=False, spp=1, run_shift=0, lanes=256):
    """The megakernel's item -> pixel arithmetic on the host (mtsgpu_index_host), by the
    functions the kernels compile: for each (lane, round) row of `lane_round` a row
    (has_item, jj, pix, px, py, rendered) of uint32, and (compact pixels, tiles across).
    window = (x0, y0, width, height); row = (block, stride, phase)."""
    L = load_library()
    geom = (C.c_uint32 * 11)(*window, *row, 1 if tile_shard else 0, spp, run_shift, lanes)
    lr = np.ascontiguousarray(lane_round, np.uint32).reshape(-1, 2)
    out = np.zeros((lr.shape[0], 6), np.uint32)
    info = (C.c_uint32 * 2)()
    up = C.POINTER(C.c_uint32)
    rc = L.mtsgpu_index_host(geom, lr.ctypes.data_as(up), lr.shape[0], out.ctypes.data_as(up), info)
    if rc != 0:
        raise MtsgpuError(rc, 'mtsgpu_index_host')
    return out, (int(info[0]), int(info[1]))


def face_normals_host(scene):
    """The per-primitive unit face normals staged with an LDS scene, formed on the host
    without a device (mtsgpu_face_normals_host): (normals (N, 3), corners (N, 3, 3)) float32."""
    L = load_library()
    d = scene.desc()
    n = C.c_uint32()
    rc = L.mtsgpu_face_normals_host(C.byref(d), None, None, 0, C.byref(n))
    if rc != 0:
        raise MtsgpuError(rc, 'mtsgpu_face_normals_host')
    nrm = np.zeros((n.value, 3), np.float32)
    cor = np.zeros((n.value, 3, 3), np.float32)
    fp = C.POINTER(C.c_float)
    rc = L.mtsgpu_face_normals_host(C.byref(d), nrm.ctypes.data_as(fp), cor.ctypes.data_as(fp), n.value, C.byref(n))
    if rc != 0:
        raise MtsgpuError(rc, 'mtsgpu_face_normals_host')
    return nrm, cor


def lookup_host(m, scramble, px_py_j):
    """sobol::look_up at film resolution 2^m through the kernels' folded tables
    (mtsgpu_lookup_host): the uint64 sequence index of each (px, py, j) row."""
    L = load_library()
    q = np.ascontiguousarray(px_py_j, np.uint32).reshape(-1, 3)
    out = np.zeros(q.shape[0], np.uint64)
    rc = L.mtsgpu_lookup_host(m, scramble, q.ctypes.data_as(C.POINTER(C.c_uint32)), q.shape[0],
                              out.ctypes.data_as(C.POINTER(C.c_uint64)))
    if rc != 0:
        raise MtsgpuError(rc, 'mtsgpu_lookup_host')
    return out


PLAN_ENGINES = ('megakernel', 'wavefront', 'fields')
# debug counter 15: the delta-emitter instantiations ran (MTSG_FEAT_DELTA; megakernel, direct or wavefront)
VARIANT_DELTA = 1 << 18
# ... and the instantiations of scenes whose sensor is not `perspective` (MTSG_FEAT_SET_LENS, the field pass's too)
VARIANT_LENS = 1 << 19
# ... and the instantiations of scenes with a mixturebsdf, blendbsdf or mask (MTSG_FEAT_SET_COMBO = 7175; they hold the
# lens and delta code too, bits 18 and 19 then say what the scene has)
VARIANT_COMBO = 1 << 20
# ... and the instantiations of scenes with a difftrans, roughdiffuse or phong (MTSG_FEAT_SET_LEAF2 =
# 15367; they hold the combinators' code too, bit 20 then says whether the scene has one)
VARIANT_LEAF2 = 1 << 21


def kernel_variant_of(word):
    """Debug counter 15 (render_plan.cpp plan_variant_word) decoded: {'instr', 'scene_lds',
    'feat', 'waves', 'name'}, name being the megakernel's template as rocprofv3 reports it,
    e.g. 'path_kernel<false, false, 336, 4>'; None for the wavefront engine and a field pass."""
    c = int(word)
    if c & (3 << 16):   # the wavefront engine, or a field pass (field_kernel)
        return None
    feat = ((c & 0xff) | (256 if c & (1 << 14) else 0) | (512 if c & (1 << 15) else 0) |
            (1024 if c & (VARIANT_DELTA | VARIANT_LENS | VARIANT_COMBO | VARIANT_LEAF2) else 0) |
            (2048 if c & (VARIANT_LENS | VARIANT_COMBO | VARIANT_LEAF2) else 0) |
            (4096 if c & (VARIANT_COMBO | VARIANT_LEAF2) else 0) | (8192 if c & VARIANT_LEAF2 else 0))
    instr, lds, waves = bool(c & (1 << 13)), bool(c & (1 << 12)), (c >> 8) & 0xf
    b = lambda v: 'true' if v else 'false'
    return {'instr': instr, 'scene_lds': lds, 'feat': feat, 'waves': waves, 'delta': bool(c & VARIANT_DELTA),
            'lens': bool(c & VARIANT_LENS), 'combo': bool(c & VARIANT_COMBO), 'leaf2': bool(c & VARIANT_LEAF2),
            'name': 'path_kernel<%s, %s, %d, %d>' % (b(instr), b(lds), feat, waves)}


def plan_host(scene, integ, fields=None, window=None, samples=False, row=(0, 1, 0), tile_shard=False, engine=None,
              cus=256, blocks_per_cu=0, free_bytes=0, params=None, max_launches=64):
    """What a render of `scene` with `integ` would launch, planned on the host without a
    device (mtsgpu_plan_host) by the functions the renders run, under the MTSGPU_*
    environment of the call.  The arguments are Context.render's (fields: a list of
    FieldIntegrators or names, as Context.render_fields); cus, blocks_per_cu (0: the plan's
    waves per SIMD) and free_bytes (0: unknown) describe the device; params: a ready
    abi.RenderParams instead of integ's.  Returns a dict: 'engine', 'variant_word' (what debug
    counter 15 would read), 'variant' (kernel_variant_of it), 'pixels' (compact), 'chunk',
    'launches', 'waves', 'lds_dims', 'nibbles', 'scene_lds', 'scan', 'start_queue', 'gather',
    'replay', 'gather_h', 'lds_bytes', 'wf_slots' and 'launch': the first max_launches
    launches as (chunk_spp, grid, round_shift).  Raises MtsgpuError as the render would."""
    L = load_library()
    d = scene.desc()
    if params is None:
        W, H = scene.sensor.width, scene.sensor.height
        x0, y0, w, h = window if window else (integ.crop or (0, 0, W, H))
        params = integ.params(W, H, x0, y0, w, h, row[0], row[1], row[2])
        if tile_shard:
            params.flags |= abi.FLAG_TILE_SHARD
        params.flags |= Context._engine_flags(engine)
    cap = 16 + 3 * max_launches
    out = (C.c_uint64 * cap)()
    dev = (C.c_uint64 * 3)(cus, blocks_per_cu, free_bytes)
    buf = C.create_string_buffer(1024)
    rc = L.mtsgpu_plan_host(C.byref(d), C.byref(params), len(fields) if fields else 0, 1 if samples else 0, dev, out,
                            cap, buf, 1024)
    if rc != 0:
        raise MtsgpuError(rc, buf.value.decode())
    n = min(int(out[4]), max_launches)
    bits = int(out[8])
    return {'engine': PLAN_ENGINES[out[0]], 'variant_word': int(out[1]), 'variant': kernel_variant_of(out[1]),
            'pixels': int(out[2]), 'chunk': int(out[3]), 'launches': int(out[4]), 'waves': int(out[5]),
            'lds_dims': int(out[6]), 'nibbles': int(out[7]), 'scene_lds': bool(bits & 1), 'scan': bool(bits & 2),
            'start_queue': bool(bits & 4), 'gather': bool(bits & 8), 'replay': bool(bits & 16),
            'gather_h': int(out[9]), 'lds_bytes': int(out[10]), 'wf_slots': int(out[11]),
            'launch': [(int(out[16 + 3 * i]), int(out[17 + 3 * i]), int(out[18 + 3 * i])) for i in range(n)]}


def kdtree_host(scene):
    """The reference's SAH kd-tree of `scene`, built on the host without a device
    (mtsgpu_kdtree_host): (nodes (N, 2) uint32 KDNode words, indices, info dict)."""
    L = load_library()
    d = scene.desc()
    info = (C.c_uint32 * 8)()
    buf = C.create_string_buffer(512)
    rc = L.mtsgpu_kdtree_host(C.byref(d), None, 0, None, 0, info, buf, 512)
    if rc != 0:
        raise MtsgpuError(rc, buf.value.decode())
    nodes = np.zeros((info[0], 2), np.uint32)
    idx = np.zeros(max(1, info[1]), np.uint32)
    up = C.POINTER(C.c_uint32)
    rc = L.mtsgpu_kdtree_host(C.byref(d), nodes.ctypes.data_as(up), nodes.size, idx.ctypes.data_as(up), idx.size,
                              info, buf, 512)
    if rc != 0:
        raise MtsgpuError(rc, buf.value.decode())
    return nodes, idx[:info[1]], dict(zip(KD_KEYS, list(info)))


class Context:
    """One libmtsgpu context (one HIP device)."""

    def __init__(self, device=-1, lib_path=None):
        self.L = load_library(lib_path)
        h = C.c_void_p()
        rc = self.L.mtsgpu_create(device, C.byref(h))
        if rc != 0:
            raise NativeUnavailable('mtsgpu_create failed: %s' % self.L.mtsgpu_last_error(None).decode())
        self.h = h
        self.scene = None

    def _check(self, rc):
        if rc != 0:
            raise MtsgpuError(rc, self.L.mtsgpu_last_error(self.h).decode())

    def upload(self, scene):
        d = scene.desc()
        self._check(self.L.mtsgpu_upload_scene(self.h, C.byref(d)))
        self.scene = scene

    def debug_counters(self):
        """The 16 raw device counters of the last render (include/mtsgpu.h)."""
        out = (C.c_uint64 * 16)()
        self._check(self.L.mtsgpu_debug_counters(self.h, out))
        return list(out)

    def launch_chunks(self):
        """The launches the last render's sample count was split into (debug counter 8)."""
        return self.debug_counters()[8]

    def kernel_variant(self):
        """The megakernel instantiation the last render launched, decoded from debug
        counter 15 (kernel_variant_of); None after a wavefront-engine render or a field pass."""
        return kernel_variant_of(self.debug_counters()[15])

    def debug_sfmt(self, seed, n, clone=0):
        """n nextULong draws of the device's SFMT19937 from Random(seed) (or its clone-th clone)."""
        out = np.zeros(n, np.uint64)
        self._check(self.L.mtsgpu_debug_sfmt(self.h, C.c_uint64(seed), clone, out.ctypes.data_as(C.POINTER(C.c_uint64)), n))
        return out

    def scene_info(self):
        info = (C.c_uint32 * 4)()
        self._check(self.L.mtsgpu_debug_scene_info(self.h, info))
        return {'nodes': info[0], 'prims': info[1], 'depth': info[2], 'cus': info[3]}

    @staticmethod
    def _engine_flags(engine):
        if engine is None:
            return 0
        if engine == 'wavefront':
            return abi.FLAG_WAVEFRONT
        if engine == 'megakernel':
            return abi.FLAG_MEGAKERNEL
        if engine == 'kdtree':       # the wavefront engine over the reference's kd-tree
            return abi.FLAG_KDTREE
        raise ValueError('engine must be None, "wavefront", "megakernel" or "kdtree"')

    def render(self, integ, window=None, samples=False, row=(0, 1, 0), traversal_stats=False, engine=None,
               tile_shard=False, cancel=None):
        """Returns (film (H+2b, W+2b, 5) float32, per-sample records or None, stats dict).
        engine: None (the library's default), 'wavefront', 'megakernel' or 'kdtree'
        (the wavefront engine tracing through the reference's kd-tree).
        row = (row_block, row_stride, row_phase); tile_shard: row_stride/row_phase
        select 8x8 tiles (MTSGPU_FLAG_TILE_SHARD) instead of row blocks.
        cancel: a ctypes.c_int32 the library polls between launches (a non-zero word
        ends the render with MTSGPU_ECANCEL); not passed on to a MultiChannelIntegrator."""
        if isinstance(integ, MultiChannelIntegrator):
            return self._render_multichannel(integ, window, samples, row, traversal_stats, engine, tile_shard)
        sc = self.scene
        W, H = sc.sensor.width, sc.sensor.height
        x0, y0, w, h = window if window else (integ.crop or (0, 0, W, H))
        p = integ.params(W, H, x0, y0, w, h, row[0], row[1], row[2])
        if traversal_stats:
            p.flags |= abi.FLAG_TRAVERSAL_STATS
        if tile_shard:
            p.flags |= abi.FLAG_TILE_SHARD
        p.flags |= self._engine_flags(engine)
        if cancel is not None:
            p.cancel = C.pointer(cancel)
        b = film_border(integ.rfilter, integ.rfilterParam)
        film = np.zeros((H + 2 * b, W + 2 * b, 5), np.float32)
        smp = np.zeros((w * h * integ.sampleCount, abi.SAMPLE_RECORD_FLOATS), np.float32) if samples else None
        st = abi.Stats()
        self._check(self.L.mtsgpu_render(self.h, C.byref(p), film.ctypes.data_as(C.POINTER(C.c_float)),
                                          smp.ctypes.data_as(C.POINTER(C.c_float)) if samples else None,
                                          C.byref(st)))
        return film, smp, st.as_dict()

    def render_fields(self, integ, fields, window=None, samples=False, row=(0, 1, 0), tile_shard=False):
        """The field pass (mtsgpu_render_fields): `fields` is a list of FieldIntegrators (or
        field names), `integ` supplies the sampler, filter and crop settings (any integrator
        here; its integrator properties are ignored).  The primary ray of every sample is
        traced once for all fields.  Returns (films (N, H+2b, W+2b, 5) float32, one
        {f.r, f.g, f.b, alpha, w} film per field; per-sample records (w*h*spp, 4 + 3N)
        {samplePos.x, samplePos.y, alpha, hit, f0.rgb, ...} or None; stats dict)."""
        fields = [f if isinstance(f, FieldIntegrator) else FieldIntegrator(f) for f in fields]
        sc = self.scene
        if any(f.field == 'albedo' for f in fields) and any(b.type in ('mixturebsdf', 'blendbsdf', 'mask')
                                                            for b in sc.flat_bsdfs()[0]):
            raise NotImplementedError("the 'albedo' field is not supported in a scene with a mixturebsdf, blendbsdf "
                                      "or mask BSDF")
        W, H = sc.sensor.width, sc.sensor.height
        x0, y0, w, h = window if window else (integ.crop or (0, 0, W, H))
        p = integ.params(W, H, x0, y0, w, h, row[0], row[1], row[2])
        if tile_shard:
            p.flags |= abi.FLAG_TILE_SHARD
        n = len(fields)
        descs = (abi.FieldDesc * max(1, n))(*[f.to_desc() for f in fields])
        b = film_border(integ.rfilter, integ.rfilterParam)
        films = np.zeros((max(1, n), H + 2 * b, W + 2 * b, 5), np.float32)
        smp = np.zeros((w * h * integ.sampleCount, 4 + 3 * n), np.float32) if samples else None
        st = abi.Stats()
        self._check(self.L.mtsgpu_render_fields(self.h, C.byref(p), descs, n, abi.fptr(films),
                                                 abi.fptr(smp) if samples else None, C.byref(st)))
        return films[:n], smp, st.as_dict()

    def _render_multichannel(self, integ, window, samples, row, traversal_stats, engine, tile_shard):
        """MultiChannelIntegrator: the radiance integrator's normal render with an alpha
        channel, then the field pass at the same sample positions.  Returns (films
        (N, H+2b, W+2b, 5) in child order, (colour records or None, field records) or
        None, stats of the colour render plus 'field_kernel_ms' -- or of the field pass
        when there is no radiance integrator)."""
        rad = integ.radiance
        film_c = smp_c = st = None
        if rad is not None:
            film_c, smp_c, st = self.render(rad, window, samples, row, traversal_stats, engine, tile_shard)
        flds = integ.fields
        films_f = smp_f = None
        if flds:
            films_f, smp_f, st_f = self.render_fields(integ, flds, window, samples, row, tile_shard)
            if st is None:
                st = st_f
            st['field_kernel_ms'] = st_f['kernel_ms']
        out, k = [], 0
        for c in integ.children:
            if isinstance(c, FieldIntegrator):
                out.append(films_f[k])
                k += 1
            else:
                out.append(film_c)
        return np.stack(out), ((smp_c, smp_f) if samples else None), st

    def develop_multi(self, films, border, hdrfilm):
        """hdrfilm develop with several pixel formats (mtsgpu_develop_multi): `films`
        (N, H+2b, W+2b, 5) float32, one per pixel format of `hdrfilm`; film 0 supplies
        alpha and weight.  Returns (H, W, C) in hdrfilm's component dtype, channels in
        format order (hdrfilm.channel_names)."""
        films = np.ascontiguousarray(films, np.float32)
        if films.ndim != 4 or films.shape[3] != 5 or films.shape[0] != len(hdrfilm.pixel_formats):
            raise ValueError('develop_multi: films must be (N, H+2b, W+2b, 5) float32, one per pixel format')
        p = hdrfilm.develop_multi_params(films.shape[1:], border)
        out = hdrfilm.output_array(films.shape[1:], border)
        ptrs = (C.c_void_p * films.shape[0])(*[films[i].ctypes.data for i in range(films.shape[0])])
        self._check(self.L.mtsgpu_develop_multi(self.h, C.byref(p), ptrs, out.ctypes.data_as(C.c_void_p)))
        return out

    def render_device(self, integ, film_ptr, stream_ptr=None, window=None, row=(0, 1, 0), engine=None,
                      tile_shard=False):
        sc = self.scene
        W, H = sc.sensor.width, sc.sensor.height
        x0, y0, w, h = window if window else (integ.crop or (0, 0, W, H))
        p = integ.params(W, H, x0, y0, w, h, row[0], row[1], row[2])
        if tile_shard:
            p.flags |= abi.FLAG_TILE_SHARD
        p.flags |= self._engine_flags(engine)
        st = abi.Stats()
        self._check(self.L.mtsgpu_render_device(self.h, C.byref(p), C.c_void_p(film_ptr),
                                                 C.c_void_p(stream_ptr) if stream_ptr else None, C.byref(st)))
        return st.as_dict()

    def develop(self, film, border, hdrfilm):
        """hdrfilm develop on the device (mtsgpu_develop): `film` (H+2b, W+2b, 5)
        float32 host array -> (H, W, C) in hdrfilm's component dtype."""
        film = np.ascontiguousarray(film, np.float32)
        if film.ndim != 3 or film.shape[2] != 5:
            raise ValueError('develop: film must be (H+2b, W+2b, 5) float32')
        p = hdrfilm.develop_params(film.shape, border)
        out = hdrfilm.output_array(film.shape, border)
        self._check(self.L.mtsgpu_develop(self.h, C.byref(p), abi.fptr(film), out.ctypes.data_as(C.c_void_p)))
        return out

    def develop_device(self, film_ptr, film_shape, border, hdrfilm, out_ptr, stream_ptr=None):
        """Same on device buffers (e.g. torch tensors' data_ptr()); the output
        holds hdrfilm.output_array(film_shape, border).nbytes bytes."""
        p = hdrfilm.develop_params(film_shape, border)
        self._check(self.L.mtsgpu_develop_device(self.h, C.byref(p), C.c_void_p(film_ptr), C.c_void_p(out_ptr),
                                                  C.c_void_p(stream_ptr) if stream_ptr else None))

    def develop_ldr(self, film, border, ldrfilm, info=False):
        """ldrfilm develop on the device (mtsgpu_develop_ldr): `film` (H+2b, W+2b, 5)
        float32 host array -> (H, W, C) uint8; with info=True also the float32 pair
        {logAvgLuminance, maxLuminance} of the reinhard method (zeros for gamma)."""
        film = np.ascontiguousarray(film, np.float32)
        if film.ndim != 3 or film.shape[2] != 5:
            raise ValueError('develop_ldr: film must be (H+2b, W+2b, 5) float32')
        p = ldrfilm.develop_params(film.shape, border)
        out = ldrfilm.output_array(film.shape, border)
        info2 = np.zeros(2, np.float32)
        self._check(self.L.mtsgpu_develop_ldr(self.h, C.byref(p), abi.fptr(film), out.ctypes.data_as(C.c_void_p),
                                              abi.fptr(info2)))
        return (out, info2) if info else out

    def develop_ldr_device(self, film_ptr, film_shape, border, ldrfilm, out_ptr, stream_ptr=None):
        """Same on device buffers (e.g. torch tensors' data_ptr()); the output holds
        ldrfilm.output_array(film_shape, border).nbytes bytes and is aligned to its pixel
        size.  Returns the float32 pair {logAvgLuminance, maxLuminance}."""
        p = ldrfilm.develop_params(film_shape, border)
        info2 = np.zeros(2, np.float32)
        self._check(self.L.mtsgpu_develop_ldr_device(self.h, C.byref(p), C.c_void_p(film_ptr), C.c_void_p(out_ptr),
                                                     C.c_void_p(stream_ptr) if stream_ptr else None,
                                                     abi.fptr(info2)))
        return info2

    def kdtree(self):
        """The reference's SAH kd-tree of the uploaded scene (mtsgpu_debug_kdtree):
        (nodes (N, 2) uint32 KDNode words, indices uint32, info dict)."""
        info = (C.c_uint32 * 8)()
        self._check(self.L.mtsgpu_debug_kdtree(self.h, None, 0, None, 0, info))
        nodes = np.zeros((info[0], 2), np.uint32)
        idx = np.zeros(max(1, info[1]), np.uint32)
        up = C.POINTER(C.c_uint32)
        self._check(self.L.mtsgpu_debug_kdtree(self.h, nodes.ctypes.data_as(up), nodes.size, idx.ctypes.data_as(up),
                                               idx.size, info))
        return nodes, idx[:info[1]], dict(zip(KD_KEYS, list(info)))

    def trace_rays(self, o, d, mint=1e-4, maxt=np.inf, shadow=False, kdtree=False):
        """Scene::rayIntersect (shadow=False) / occlusion (shadow=True) for a batch of
        rays: o, d (n, 3); mint, maxt scalars or (n,).  kdtree=True traverses the
        reference's own kd-tree (MTSGPU_TRACE_KDTREE).  Returns (hits (n, 4) float32
        {t, u, v, prim bits}, kernel ms)."""
        o = np.asarray(o, np.float32).reshape(-1, 3)
        d = np.asarray(d, np.float32).reshape(-1, 3)
        n = o.shape[0]
        rays = np.empty((n, 8), np.float32)
        rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, mint, d, maxt
        hits = np.empty((n, 4), np.float32)
        ms = C.c_double()
        flags = (abi.TRACE_SHADOW if shadow else 0) | (abi.TRACE_KDTREE if kdtree else 0)
        self._check(self.L.mtsgpu_trace_rays_ex(self.h, abi.fptr(rays), n, flags, abi.fptr(hits), C.byref(ms)))
        return hits, ms.value

    LIBM_FNS = ('sin', 'cos', 'expf', 'acosf', 'atanf', 'tanf', 'atan2f', 'powf', 'fastexp', 'fastlog')

    def debug_libm(self, fn, a=None, b=None, first=0, n=None):
        """The device's transcendental `fn` (LIBM_FNS name or id) over a (and b),
        or over the n floats whose bits are first, first+1, ..."""
        fid = self.LIBM_FNS.index(fn) if isinstance(fn, str) else int(fn)
        P = C.POINTER(C.c_float)
        if a is not None:
            a = np.ascontiguousarray(a, np.float32)
            n = a.size
        if b is not None:
            b = np.ascontiguousarray(b, np.float32)
        out = np.empty(n, np.float32)
        self._check(self.L.mtsgpu_debug_libm(self.h, fid, abi.fptr(a) if a is not None else P(),
                                             abi.fptr(b) if b is not None else P(), abi.fptr(out), n,
                                             C.c_uint32(first)))
        return out

    def debug_arith(self, a, b):
        a = np.ascontiguousarray(a, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        out = np.zeros((a.size, 8), np.float32)
        self._check(self.L.mtsgpu_debug_arith(self.h, abi.fptr(a), abi.fptr(b), abi.fptr(out), a.size))
        return out

    def close(self):
        if self.h:
            self.L.mtsgpu_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceGroup:
    """One render over several GPUs of this node (mtsgpu_group_*): the library
    shards the 8x8 tiles over the devices, one host thread each, and merges the films
    on the first device over xGMI (include/mtsgpu.h).  A device may be listed
    twice (two contexts on one GPU)."""

    def __init__(self, devices, lib_path=None):
        self.L = load_library(lib_path)
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        rc = self.L.mtsgpu_group_create(devs, len(devices), C.byref(h))
        if rc != 0:
            raise NativeUnavailable('mtsgpu_group_create failed: %s' % self.L.mtsgpu_group_last_error(None).decode())
        self.h = h
        self.devices = list(devices)
        self.scene = None

    def _check(self, rc):
        if rc != 0:
            raise MtsgpuError(rc, self.L.mtsgpu_group_last_error(self.h).decode())

    def __len__(self):
        return self.L.mtsgpu_group_size(self.h)

    def upload(self, scene):
        d = scene.desc()
        self._check(self.L.mtsgpu_group_upload_scene(self.h, C.byref(d)))
        self.scene = scene

    def render(self, integ, window=None, engine=None, row_block=8):
        """Returns (film (H+2b, W+2b, 5) float32, stats dict) of the whole window."""
        sc = self.scene
        W, H = sc.sensor.width, sc.sensor.height
        x0, y0, w, h = window if window else (integ.crop or (0, 0, W, H))
        p = integ.params(W, H, x0, y0, w, h, row_block, 1, 0)
        p.flags |= Context._engine_flags(engine)
        b = film_border(integ.rfilter, integ.rfilterParam)
        film = np.zeros((H + 2 * b, W + 2 * b, 5), np.float32)
        st = abi.Stats()
        self._check(self.L.mtsgpu_group_render(self.h, C.byref(p), film.ctypes.data_as(C.POINTER(C.c_float)),
                                                C.byref(st)))
        return film, st.as_dict()

    def close(self):
        if self.h:
            self.L.mtsgpu_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PathTracer(PathIntegrator):
    """The `path` integrator (MIPathTracer) running on MI355X."""

    def render(self, scene, ctx=None, integrator=None):
        """Renders with this integrator, or with `integrator` (e.g. a
        MultiChannelIntegrator: the films then come in child order, (N, H+2b, W+2b, 5))."""
        ctx = ctx or Context()
        if ctx.scene is not scene:
            ctx.upload(scene)
        film, _, stats = ctx.render(integrator if integrator is not None else self)
        return film, stats
