// dhit.h -- the hit record: fillIntersectionRecord<true> (include/mitsuba/render/skdtree.h:
// 343-429) and computeShadingFrame (src/librender/util.cpp:603-608) from the vertex data in
// HBM or its LDS copy (HitSrc), the wavefront engine's stored form of the record,
// and the closest-hit query of the one-lane-per-sample kernels (direct_kernel, field_kernel).
// Included by dpath.h after danalytic.h (ana_fill), dtraverse.h and dscan.h.
#pragma once

struct Hit {
    int valid;
    float t;
    f3 p, geoN, wi;
    ShFrame sh;
    int shape;
    float u, v;       // its.uv (textured scenes only; dead otherwise)
};

// computeShadingFrame (util.cpp:603-608); t = cross(n, s) is ShFrame::t()
__device__ __forceinline__ ShFrame shading_frame(f3 n, f3 dpdu) {
    ShFrame f;
    f.n = n;
    f.s = normalize(sub(dpdu, mul(f.n, dot(f.n, dpdu))));
    return f;
}

// Where a vertex's triangle data comes from: HBM, or (small scenes, SCENE_LDS)
// the LDS copy every workgroup stages next to the BVH
typedef __attribute__((address_space(3))) const float lds_f32;
typedef __attribute__((address_space(1))) const MtsgShape glb_shape;
typedef __attribute__((address_space(3))) const MtsgShape lds_shape;
template <bool INLDS> struct HitSrc;
template <> struct HitSrc<false> { glb_u32 *pv; glb_f32 *pos, *nrm, *dpdu; glb_shape *shapes; };
// (LDS scenes also stage the primitives' unit face normals, fn: a constant of the triangle
// that fill_hit and the area-light sample would otherwise re-form, ~45 VALU each)
template <> struct HitSrc<true> { lds_u32 *pv; lds_f32 *pos, *nrm, *dpdu, *fn; lds_shape *shapes; };
template <typename P> __device__ __forceinline__ f3 ldp3(P p) { return mk(p[0], p[1], p[2]); }

// fillIntersectionRecord<true> (skdtree.h:343-429); UV = TEX
template <bool TEX, bool ANA, typename HS>
__device__ __forceinline__ void fill_hit(const MtsgDeviceScene &S, const HS &hs, uint32_t slot, uint32_t prim, float u,
                                         float v, float t, f3 o, f3 d, Hit &h) {
    if constexpr (ANA) {
        const MtsgTri &tr = S.tris[slot];
        if (tr.k == MTSG_K_ANALYTIC) {   // Shape::fillIntersectionRecord + skdtree.h:425-427
            const AnaHit a = ana_fill(((GAna *)S.analytic)[__float_as_uint(tr.n_u)], o, d, t, u, v);
            h.valid = 1;
            h.t = t;
            h.shape = (int)tr.shape;
            h.p = a.p;
            h.geoN = a.geoN;
            h.sh = shading_frame(a.shN, a.dpdu);
            h.wi = to_local(h.sh, neg(d));
            if constexpr (TEX) { h.u = a.u; h.v = a.v; }
            return;
        }
    }
    const uint4 pv = make_uint4(hs.pv[4 * prim], hs.pv[4 * prim + 1], hs.pv[4 * prim + 2], hs.pv[4 * prim + 3]);
    h.valid = 1;
    h.t = t;
    h.shape = (int)pv.w;
    const float bx = 1 - u - v, by = u, bz = v;
    const f3 p0 = ldp3(hs.pos + 3 * (size_t)pv.x), p1 = ldp3(hs.pos + 3 * (size_t)pv.y),
             p2 = ldp3(hs.pos + 3 * (size_t)pv.z);
    h.p = add(add(mul(p0, bx), mul(p1, by)), mul(p2, bz));
    f3 faceNormal;
    if constexpr (std::is_same<HS, HitSrc<true>>::value) {
        faceNormal = ldp3(hs.fn + 3 * (size_t)prim);   // the same operations, done by the host (mtsg_face_normal)
    } else {
        const f3 side1 = sub(p1, p0), side2 = sub(p2, p0);
        faceNormal = cross(side1, side2);
        const float length = len(faceNormal);
        if (!is_zero(faceNormal)) faceNormal = divs(faceNormal, length);
    }
    const f3 dpdu = ldp3(hs.dpdu + 3 * (size_t)prim);
    f3 shN;
    if (hs.shapes[h.shape].has_normals) {
        const f3 n0 = ldp3(hs.nrm + 3 * (size_t)pv.x), n1 = ldp3(hs.nrm + 3 * (size_t)pv.y),
                 n2 = ldp3(hs.nrm + 3 * (size_t)pv.z);
        shN = normalize(add(add(mul(n0, bx), mul(n1, by)), mul(n2, bz)));
        if (dot(faceNormal, shN) < 0) faceNormal = neg(faceNormal);
    } else {
        shN = faceNormal;
    }
    h.geoN = faceNormal;
    h.sh = shading_frame(shN, dpdu);
    h.wi = to_local(h.sh, neg(d));
    if constexpr (TEX) {   // skdtree.h:398-405: t0*b.x + t1*b.y + t2*b.z, else (b.y, b.z)
        if (hs.shapes[h.shape].has_uv) {
            const float *tc = S.texcoords;
            h.u = tc[2 * (size_t)pv.x] * bx + tc[2 * (size_t)pv.y] * by + tc[2 * (size_t)pv.z] * bz;
            h.v = tc[2 * (size_t)pv.x + 1] * bx + tc[2 * (size_t)pv.y + 1] * by + tc[2 * (size_t)pv.z + 1] * bz;
        } else {
            h.u = by;
            h.v = bz;
        }
    }
}

// The wavefront engine's hit record formed by the trace kernel (MtsgWave::hitrec,
// MTSG_WF_HIT_VECS float4 per slot): fill_hit's result, bit for bit, so a shade
// kernel starts from one contiguous record instead of the slot -> prim -> vertex
// chain of dependent loads.  The 6th vector (UVs) is written for textured scenes only.
__device__ __forceinline__ void hit_store(float4 *r, const Hit &h, bool uv) {
    r[0] = make_float4(h.t, h.p.x, h.p.y, h.p.z);
    r[1] = make_float4(h.geoN.x, h.geoN.y, h.geoN.z, h.wi.x);
    const f3 t = h.sh.t();
    r[2] = make_float4(h.wi.y, h.wi.z, h.sh.s.x, h.sh.s.y);
    r[3] = make_float4(h.sh.s.z, t.x, t.y, t.z);
    r[4] = make_float4(h.sh.n.x, h.sh.n.y, h.sh.n.z, __int_as_float(h.shape));
    if (uv) r[5] = make_float4(h.u, h.v, 0.0f, 0.0f);
}
template <bool UV> __device__ __forceinline__ void hit_load(const float4 *r, Hit &h) {
    const float4 a = r[0], b = r[1], c = r[2], d = r[3], e = r[4];
    h.valid = 1;
    h.t = a.x;
    h.p = mk(a.y, a.z, a.w);
    h.geoN = mk(b.x, b.y, b.z);
    h.wi = mk(b.w, c.x, c.y);
    h.sh.s = mk(c.z, c.w, d.x);
    h.sh.n = mk(e.x, e.y, e.z);   // (d.yzw: t, re-formed as cross(n, s))
    h.shape = __float_as_int(e.w);
    if constexpr (UV) { const float4 f = r[5]; h.u = f.x; h.v = f.y; }
}

// Scene::rayIntersect through the launch's structure (the tiny-scene scan, the BVH in LDS or
// in HBM): the clipped interval and the closest hit (slot, hu, hv, ht: fill_hit's arguments).
// stkN / stkD: the lane's traversal stack; cN / cT: node and test counts (dead without STATS)
// (fill_hit stays with the callers: with it in here their one if / else on the hit became two,
// and direct_kernel and field_kernel compiled to other code)
template <bool SCENE_LDS, bool ANA>
__device__ __forceinline__ bool closest_hit(const MtsgLaunch &L, lds_node *ldsNodes, lds_tri *ldsTris, lds_stk_n *stkN,
                                            lds_stk_d *stkD, f3 o, f3 d, float rmint, float rmaxt, uint32_t &slot,
                                            float &hu, float &hv, float &ht, unsigned long long &cN,
                                            unsigned long long &cT) {
    const MtsgDeviceScene &S = L.scene;
    float mint, maxt;
    bool hit = false;
    if (ray_interval(S, o, d, rmint, rmaxt, false, mint, maxt)) {
        if (SCENE_LDS && L.scan)
            hit = scan_tris<false, false>(L, o, d, mint, maxt, slot, hu, hv, ht, cT);
        else if (SCENE_LDS)
            hit = traverse<false, false, ANA>(ldsNodes, ldsTris, o, d, mint, maxt, stkN, stkD, slot, hu, hv, ht, cN, cT,
                                              S.analytic);
        else
            hit = traverse<false, false, ANA>((glb_node *)S.nodes, (glb_tri *)S.tris, o, d, mint, maxt, stkN, stkD, slot,
                                              hu, hv, ht, cN, cT, S.analytic);
    }
    return hit;
}
// the primitive of a hit's slot (the scan returns the primitive itself)
template <bool SCENE_LDS>
__device__ __forceinline__ uint32_t hit_prim(const MtsgLaunch &L, lds_tri *ldsTris, uint32_t slot) {
    return (SCENE_LDS && L.scan) ? slot : SCENE_LDS ? ldsTris[slot].prim : L.scene.tris[slot].prim;
}
