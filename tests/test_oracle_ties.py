"""The oracle's closest hit resolves exact-t ties by the larger primitive index
whatever the traversal order -- which needs node tests that never cull a box
holding a candidate at t <= the current best.

C4's hall and floor meshes are coplanar at y = 0 (prims 693 and 3644 below are
both hit at t = 0x1.31a142p-3).  The floor's BVH leaf boxes have zero extent in
y at coordinate 0, so a purely relative inflation leaves them flat, and their
slab t rounded one ulp beyond the TriAccel t: the oracle culled the leaf holding
3644 once 693 was found and returned 693, while every GPU engine returned 3644
(tests/test_gpu_bench_kernels.py found the one sample whose path this changed;
tools/diag_c4_ray.py).  The boxes now carry the same absolute inflation as the
product's builder (1e-7 of the scene diagonal, bvh_build.cpp Builder::absEps).
"""
import ctypes as C

import numpy as np

from mitsuba_amd import scenes

F = float.fromhex
O = np.array([F('-0x1.10507p+1'), F('0x1.99dafep-5'), F('0x1.66d228p+3')], np.float32)
D = np.array([F('-0x1.c16b56p-1'), F('-0x1.574dp-2'), F('-0x1.5e7144p-2')], np.float32)
EPS = np.float32(F('0x1.a36e2ep-14'))   # Epsilon: the ray's own mint (path.cpp Ray(its.p, wo, ray.time))


def _triaccel_hit(oracle, sc, mesh, tri):
    L = oracle.lib()
    fp = C.POINTER(C.c_float)
    m = sc.meshes[mesh]
    A, B, Cc = (np.ascontiguousarray(m.positions[m.indices[tri, k]], np.float32) for k in range(3))
    t10 = np.zeros(10, np.float32)
    uvt = np.zeros(3, np.float32)
    L.oracle_triaccel_load(A.ctypes.data_as(fp), B.ctypes.data_as(fp), Cc.ctypes.data_as(fp), t10.ctypes.data_as(fp))
    o, d = np.ascontiguousarray(O), np.ascontiguousarray(D)
    ok = L.oracle_triaccel_intersect(t10.ctypes.data_as(fp), o.ctypes.data_as(fp), d.ctypes.data_as(fp),
                                     C.c_float(EPS), C.c_float(np.inf), uvt.ctypes.data_as(fp))
    return ok, uvt[2]


def test_coplanar_tie_takes_the_larger_primitive(oracle):
    sc, it = scenes.build('C4', rfilter='box')
    n0 = len(sc.meshes[0].indices)
    ok0, t0 = _triaccel_hit(oracle, sc, 0, 693)
    ok1, t1 = _triaccel_hit(oracle, sc, 1, 3644 - n0)
    assert ok0 and ok1 and t0 == t1, (t0, t1)           # an exact-t tie
    h = oracle.trace_rays(sc, O[None], D[None], mint=EPS)
    assert h[0, 3].view(np.uint32) == 3644 and h[0, 0] == t0
