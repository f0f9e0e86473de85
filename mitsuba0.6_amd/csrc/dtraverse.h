// dtraverse.h -- a ray against the scene's acceleration structures: the BVH2 node load and the
// speculative while-while traversal with TriAccel leaves (include/mitsuba/render/triaccel.h:92-160),
// the reference's own kd-tree as SAHKDTree3D::rayIntersectHavran (include/mitsuba/render/
// sahkdtree3.h:178-308, skdtree.h:248-338), and the ray's clipped interval: AABB::rayIntersect
// (include/mitsuba/core/aabb.h:308-338) and ShapeKDTree::rayIntersect's epsilon rule
// (src/librender/skdtree.cpp:112-142, 207-226).  Included by dpath.h after dsampler.h.
#pragma once

// one BVH2 node's two child boxes and child references: the 64 B MtsgNode
// (LDS or HBM) in four 16 B loads, or the 32 B MtsgHNode in two, its half
// bounds widened exactly to float (the conversions fold into the slab FMAs)
__device__ __forceinline__ float half_lo(uint32_t w) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xffffu)); }
__device__ __forceinline__ float half_hi(uint32_t w) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16)); }
template <typename NodeT>
__device__ __forceinline__ void load_node(NodeT *n, vf4 &a, vf4 &b, vf4 &c, int &c0, int &c1) {
    if constexpr (std::is_same<NodeT, glb_hnode>::value) {
        const vu4 p = *reinterpret_cast<glb_u4 *>(&n->box[0]);
        const vu4 q = *reinterpret_cast<glb_u4 *>(&n->box[4]);
        a = vf4{half_lo(p.x), half_hi(p.x), half_lo(p.y), half_hi(p.y)};
        b = vf4{half_lo(p.z), half_hi(p.z), half_lo(p.w), half_hi(p.w)};
        c = vf4{half_lo(q.x), half_hi(q.x), half_lo(q.y), half_hi(q.y)};
        c0 = (int)q.z;
        c1 = (int)q.w;
    } else {
        typedef typename std::conditional<std::is_same<NodeT, lds_node>::value, lds_f4, glb_f4>::type F4;
        typedef typename std::conditional<std::is_same<NodeT, lds_node>::value, lds_i4, glb_i4>::type I4;
        a = *reinterpret_cast<F4 *>(&n->c0lox);
        b = *reinterpret_cast<F4 *>(&n->c1lox);
        c = *reinterpret_cast<F4 *>(&n->c0loz);
        const vi4 e = *reinterpret_cast<I4 *>(&n->c0);
        c0 = e.x;
        c1 = e.y;
    }
}

// ---------------------------------------------------------------------------
// BVH2 traversal
// ---------------------------------------------------------------------------
// LDS traversal stack, lane-strided: node index (4 B) + entry distance as the
// top 16 bits of the (non-negative) float, i.e. bfloat16 rounded toward zero:
// a lower bound of the true entry distance, so culling on pop stays
// conservative (6 B/entry keeps 3 blocks per CU on large scenes)
typedef __attribute__((address_space(3))) int lds_stk_n;
typedef __attribute__((address_space(3))) uint16_t lds_stk_d;
__device__ __forceinline__ uint16_t dist_down16(float t) { return (uint16_t)(__float_as_uint(fmaxf(t, 0.0f)) >> 16); }
__device__ __forceinline__ float dist_up16(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
// Speculative while-while traversal (Aila & Laine 2009): a lane that reaches a
// leaf parks it and keeps descending until every lane of the wave holds a
// leaf; then all lanes test their parked leaves together.  Same closest hit
// (tie rule included) as a plain depth-first traversal.
// LDSK > 0: the first LDSK stack entries live in LDS, deeper ones in a per-lane
// global array `ovf` ({node, distance} pairs): a short LDS stack keeps the
// traversal kernel's LDS per lane small (wf_trace occupancy); 0: all in LDS
// (Round 4 measured the stack's top entry cached in two registers: bit-identical,
// but C2 -0.9%, C3 -4.2%, C4 -5.2%, C5 -3.9%, profiles/r04_ab_reg_top.log; removed.)
template <bool ANY, bool STATS, bool ANA = false, int LDSK = 0, typename NodeT, typename TriT>
__device__ __forceinline__ bool traverse(NodeT *nodesArr, TriT *trisArr, f3 o, f3 d, float mint, float maxt,
                                         lds_stk_n *stkN, lds_stk_d *stkD, uint32_t &bestSlot, float &bu, float &bv,
                                         float &bt, unsigned long long &nodes, unsigned long long &tests,
                                         const MtsgAnalytic *anaArr = nullptr, uint2 *ovf = nullptr) {
    typedef typename std::conditional<std::is_same<NodeT, lds_node>::value, lds_f4, glb_f4>::type F4;
    const float ix = (d.x == 0.0f) ? copysignf(1e30f, d.x) : 1.0f / d.x;
    const float iy = (d.y == 0.0f) ? copysignf(1e30f, d.y) : 1.0f / d.y;
    const float iz = (d.z == 0.0f) ? copysignf(1e30f, d.z) : 1.0f / d.z;
    const float ox = o.x * ix, oy = o.y * iy, oz = o.z * iz;
    constexpr int DONE = 0x7fffffff;
    bool found = false;
    uint32_t bestPrim = 0;
    bt = maxt;
    int sp = 0;
    int node = 0, leaf = 0;
    auto pop = [&]() -> int {
        while (sp > 0) {
            --sp;
            if (LDSK == 0 || sp < LDSK) {
                // the entry's node read ahead of the cull test (the empty asm pins it
                // there) instead of inside the taken branch: C3 +2.0%, C4 +1.6%, C5
                // +1.2% (round 5, profiles/r05_ab_pop_both.log).  Both reads issued
                // before one wait lost 1.1-1.6% against this (r05_ab_pop_onewait.log),
                // so the gain is in the shape of the compiled pop loop, not in LDS
                // round trips
                int n = stkN[sp * BLOCK];
                asm volatile("" : "+v"(n));
                if (ANY || dist_up16(stkD[sp * BLOCK]) <= bt) return n;
            } else {
                const uint2 e = ovf[sp - LDSK];
                if (ANY || dist_up16((uint16_t)e.y) <= bt) return (int)e.x;
            }
        }
        return DONE;
    };
    while (node != DONE) {
        // inner nodes
        while ((uint32_t)node < (uint32_t)DONE) {
            if (STATS) nodes++;
            vf4 a, b, c;
            int ec0, ec1;
            load_node(nodesArr + node, a, b, c, ec0, ec1);
            // slab tests; node boxes are conservatively inflated on the host
            const float t0x = __builtin_fmaf(a.x, ix, -ox), t1x = __builtin_fmaf(a.y, ix, -ox);
            const float t0y = __builtin_fmaf(a.z, iy, -oy), t1y = __builtin_fmaf(a.w, iy, -oy);
            const float t0z = __builtin_fmaf(c.x, iz, -oz), t1z = __builtin_fmaf(c.y, iz, -oz);
            const float n0 = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fmaxf(fminf(t0z, t1z), mint));
            const float f0 = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fminf(fmaxf(t0z, t1z), bt));
            const float u0x = __builtin_fmaf(b.x, ix, -ox), u1x = __builtin_fmaf(b.y, ix, -ox);
            const float u0y = __builtin_fmaf(b.z, iy, -oy), u1y = __builtin_fmaf(b.w, iy, -oy);
            const float u0z = __builtin_fmaf(c.z, iz, -oz), u1z = __builtin_fmaf(c.w, iz, -oz);
            const float n1 = fmaxf(fmaxf(fminf(u0x, u1x), fminf(u0y, u1y)), fmaxf(fminf(u0z, u1z), mint));
            const float f1 = fminf(fminf(fmaxf(u0x, u1x), fmaxf(u0y, u1y)), fminf(fmaxf(u0z, u1z), bt));
            const bool h0 = n0 <= f0, h1 = n1 <= f1;
            if (h0 && h1) {
                int nearC = ec0, farC = ec1;
                float farT = n1;
                if (n1 < n0) { nearC = ec1; farC = ec0; farT = n0; }
                if (LDSK == 0 || sp < LDSK) {
                    stkN[sp * BLOCK] = farC;
                    stkD[sp * BLOCK] = dist_down16(farT);
                } else {
                    ovf[sp - LDSK] = make_uint2((uint32_t)farC, dist_down16(farT));
                }
                ++sp;
                node = nearC;
            } else if (h0) {
                node = ec0;
            } else if (h1) {
                node = ec1;
            } else {
                node = pop();
            }
            // park the first leaf reached and keep descending
            if (node < 0 && leaf == 0) {
                leaf = node;
                node = pop();
            }
            if (!__any(leaf == 0)) break;
        }
        // leaves
        while (leaf < 0) {
            const uint32_t ref = (uint32_t)(~leaf);
            const uint32_t first = ref >> 4, count = ref & 15u, end = first + count;
            // the next record's loads are in flight during a record's test (round 5:
            // C4 +1.7%, C3 +1.3%, C5 +0.4%, profiles/r05_ab_leaf_prefetch.log)
            vf4 p0 = *reinterpret_cast<F4 *>(&trisArr[first].k);
            vf4 p1 = *reinterpret_cast<F4 *>(&trisArr[first].a_u);
            vf4 p2 = *reinterpret_cast<F4 *>(&trisArr[first].c_nu);
            for (uint32_t i = first; i < end; ++i) {
                if (STATS) tests++;
                const vf4 q0 = p0, q1 = p1, q2 = p2;
                if (i + 1 < end) {
                    TriT *tn = trisArr + i + 1;
                    p0 = *reinterpret_cast<F4 *>(&tn->k);
                    p1 = *reinterpret_cast<F4 *>(&tn->a_u);
                    p2 = *reinterpret_cast<F4 *>(&tn->c_nu);
                }
                const uint32_t k = __float_as_uint(q0.x);
                // TriAccel::rayIntersect (triaccel.h:92-160)
                float o_u, o_v, o_k, d_u, d_v, d_k;
                if (k == 0) { o_u = o.y; o_v = o.z; o_k = o.x; d_u = d.y; d_v = d.z; d_k = d.x; }
                else if (k == 1) { o_u = o.z; o_v = o.x; o_k = o.y; d_u = d.z; d_v = d.x; d_k = d.y; }
                else if (k == 2) { o_u = o.x; o_v = o.y; o_k = o.z; d_u = d.x; d_v = d.y; d_k = d.z; }
                else {
                    if constexpr (ANA) {
                        // analytic primitive (skdtree.h:280-290: Shape::rayIntersect on [mint, maxt])
                        float at, alx, aly;
                        if (k == MTSG_K_ANALYTIC &&
                            ana_intersect<ANY>(((GAna *)anaArr)[__float_as_uint(q0.y)], o, d, mint, bt, at, alx, aly)) {
                            if (ANY) return true;
                            const uint32_t prim = __float_as_uint(q2.z);
                            if (!found || at < bt || prim > bestPrim) {
                                found = true; bestPrim = prim; bestSlot = i; bt = at; bu = alx; bv = aly;
                            }
                        }
                    }
                    continue;
                }
                const float n_u = q0.y, n_v = q0.z, n_d = q0.w;
                const float a_u = q1.x, a_v = q1.y, b_nu = q1.z, b_nv = q1.w;
                const float c_nu = q2.x, c_nv = q2.y;
                const float t = (n_d - o_u * n_u - o_v * n_v - o_k) / (d_u * n_u + d_v * n_v + d_k);
                if (t < mint || t > bt) continue;
                const float hu = o_u + t * d_u - a_u;
                const float hv = o_v + t * d_v - a_v;
                const float u = hv * b_nu + hu * b_nv;
                const float v = hu * c_nu + hv * c_nv;
                if (u >= 0 && v >= 0 && u + v <= 1.0f) {
                    if (ANY) return true;
                    const uint32_t prim = __float_as_uint(q2.z);
                    // ties (t == bt): the larger primitive index wins
                    if (!found || t < bt || prim > bestPrim) {
                        found = true; bestPrim = prim; bestSlot = i; bt = t; bu = u; bv = v;
                    }
                }
            }
            leaf = 0;
            if (node < 0) {   // the next stack entry is a leaf too: take it now
                leaf = node;
                node = pop();
            }
        }
    }
    return found;
}

// AABB::rayIntersect (core/aabb.h:308-338) against the scene bounds.  dRcp: the
// reciprocals 1 / d_i it formed (0 for an axis it did not reach or with d_i = 0);
// after `true` every axis with d_i != 0 has its own
__device__ __forceinline__ bool aabb_clip(const MtsgDeviceScene &S, f3 o, f3 d, float &nearT, float &farT, f3 &dRcp) {
    nearT = -INFINITY; farT = INFINITY;
    dRcp = mk(0, 0, 0);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float origin = comp(o, i), di = comp(d, i);
        const float minVal = S.aabb_min[i], maxVal = S.aabb_max[i];
        if (di == 0) {
            if (origin < minVal || origin > maxVal) return false;
        } else {
            const float rcp = (float)1 / di;                 // ray.dRcp (ray.h:86-93)
            if (i == 0) dRcp.x = rcp; else if (i == 1) dRcp.y = rcp; else dRcp.z = rcp;
            float t1 = (minVal - origin) * rcp;
            float t2 = (maxVal - origin) * rcp;
            if (t1 > t2) { float t = t1; t1 = t2; t2 = t; }
            nearT = smax(t1, nearT);
            farT = smin(t2, farT);
            if (!(nearT <= farT)) return false;
        }
    }
    return true;
}

// The reference's own kd-tree (kdtree_build.cpp) traversed as
// SAHKDTree3D::rayIntersectHavran (sahkdtree3.h:178-308): entry/exit points on
// a stack of MTS_KD_MAXDEPTH entries, leaves tested over the global [mint,
// maxt] with the 8-entry hashed mailbox (:138-152, MTS_KD_MAILBOX_ENABLED),
// and ShapeKDTree::intersect's TriAccel test (skdtree.h:248-338), which keeps
// a hit at t == maxt: among exactly tied triangles the last one tested wins,
// as in the reference.  TriAccel records are in leaf-list order (tris[e] is
// the record of primitive indices[e], duplicated where leaves share one).
// The reference's stack (entries indexed by enPt / exPt, each with a prev
// link to the exit point below it) holds the pending far children in push
// order: every pop takes the most recent live push, and a push never
// overwrites a live entry (it lands above exPt, skipping enPt).  So here it is
// a plain LIFO whose entry keeps the far child and, by value, the exit point
// that was current when it was pushed -- what the reference reaches through
// prev -- and a pop is one stack read instead of three dependent ones.  A
// point (t, split, axis) is p = ray(t) with p[axis] = split; p[a] is re-formed
// as split (a == axis) or o[a] + d[a] * t, the same rounded product and sum
// the reference stores, so every comparison sees the same floats.  The entry
// and exit points the descent compares against are held in registers (only a
// push or a pop changes them), so a descent step reads no stack memory.  The
// reference's bottom entries, ray(mint) and ray(maxt) with node NONE, become
// the initial registers and the empty stack.  LDSK = 0: the stack lives in
// scratch; LDSK > 0: its first LDSK entries live in LDS, lane-strided
// (lstk[entry * BLOCK]), deeper entries in scratch; MBL: the mailbox in LDS
// (lmbox[slot * BLOCK]), else in scratch.
struct KdEnt { uint32_t node; float t; float split; uint32_t axis; };
typedef __attribute__((address_space(3))) vu4 lds_kdent;
typedef __attribute__((address_space(3))) uint32_t lds_w32;
template <bool ANY, int LDSK = 0, bool MBL = (LDSK > 0)>
__device__ bool kd_traverse(const uint2 *__restrict__ nodes, const uint32_t *__restrict__ indices,
                            const MtsgTri *__restrict__ tris, f3 o, f3 d, float mint, float maxt, float &bt,
                            float &bu, float &bv, uint32_t &bprim, lds_kdent *lstk = nullptr,
                            lds_w32 *lmbox = nullptr) {
    typedef KdEnt Ent;
    constexpr uint32_t NOAXIS = 3u, DEPTH = 46;   // MTS_KD_MAXDEPTH = 48 entries, two of them the bottom
    Ent stackS[DEPTH - LDSK];
    uint32_t mboxS[MBL ? 1 : 8];
    // entry i: LDS below LDSK, scratch above
    auto ld = [&](uint32_t i) -> Ent {
        if (LDSK && i < (uint32_t)LDSK) {
            const vu4 v = lstk[i * BLOCK];
            return Ent{v.x, __uint_as_float(v.y), __uint_as_float(v.z), v.w};
        }
        return stackS[i - LDSK];
    };
    auto st = [&](uint32_t i, const Ent &e) {
        if (LDSK && i < (uint32_t)LDSK) lstk[i * BLOCK] = vu4{e.node, __float_as_uint(e.t), __float_as_uint(e.split), e.axis};
        else stackS[i - LDSK] = e;
    };
    auto mb = [&](uint32_t k) -> uint32_t { if constexpr (MBL) return lmbox[k * BLOCK]; else return mboxS[k]; };
    auto mbset = [&](uint32_t k, uint32_t v) { if constexpr (MBL) lmbox[k * BLOCK] = v; else mboxS[k] = v; };
#pragma unroll
    for (int i = 0; i < 8; ++i) mbset(i, 0xffffffffu);
    const float rcp[3] = {1.0f / d.x, 1.0f / d.y, 1.0f / d.z};   // Ray::setDirection (ray.h:86-93)
    // p[a] of a point (t, split, eaxis): the stored point of sahkdtree3.h:239-244
    auto pt = [&](float t, float split, uint32_t eaxis, int a) -> float {
        if ((uint32_t)a == eaxis) return split;
        const float oa = a == 0 ? o.x : (a == 1 ? o.y : o.z);
        const float da = a == 0 ? d.x : (a == 1 ? d.y : d.z);
        return oa + da * t;
    };
    uint32_t sp = 0;
    // the two newest stack entries held in registers (entries sp - 1 and sp - 2
    // when nr = 2), the rest in memory; a cached entry packs its axis into the
    // node word's top bits (kd node indices stay below 2^30, capi.cpp)
    uint32_t nr = 0, c0n = 0, c1n = 0;
    float c0t = 0, c0s = 0, c1t = 0, c1s = 0;
    float en_t = mint, en_split = 0, ex_t = maxt, ex_split = 0;   // ray(mint), ray(maxt)
    uint32_t en_axis = NOAXIS, ex_axis = NOAXIS;
    bool found = false;
    uint32_t node = 0;
    while (true) {
        uint2 n = nodes[node];
        while (!(n.x & 0x80000000u)) {
            const float split = __uint_as_float(n.y);
            const int axis = (int)(n.x & 3u);
            const uint32_t left = node + ((n.x & ~(3u | 0x40000000u)) >> 2);
            const float enP = pt(en_t, en_split, en_axis, axis);
            const float exP = pt(ex_t, ex_split, ex_axis, axis);
            uint32_t farChild;
            if (enP <= split) {
                if (exP <= split) { node = left; n = nodes[node]; continue; }
                if (enP == split) { node = left + 1; n = nodes[node]; continue; }
                node = left;
                farChild = left + 1;
            } else {
                if (split < exP) { node = left + 1; n = nodes[node]; continue; }
                farChild = left;
                node = left + 1;
            }
            const float oa = axis == 0 ? o.x : (axis == 1 ? o.y : o.z);
            const float distToSplit = (split - oa) * rcp[axis];
            if (sp >= DEPTH) return found;   // MTS_KD_MAXDEPTH bounds the tree depth; never taken
            if (nr == 2) st(sp - 2, Ent{c1n & 0x3fffffffu, c1t, c1s, c1n >> 30});
            c1n = c0n; c1t = c0t; c1s = c0s;
            c0n = farChild | (ex_axis << 30); c0t = ex_t; c0s = ex_split;
            nr = nr < 2 ? nr + 1 : 2;
            ++sp;
            ex_t = distToSplit;
            ex_split = split;
            ex_axis = (uint32_t)axis;
            n = nodes[node];
        }
        for (uint32_t e = n.x & 0x7fffffffu; e != n.y; ++e) {
            // the record of list entry e (tris in leaf-list order): its loads do
            // not wait on indices[e], and the test is formed before the mailbox
            // decides whether it counts, so no load sits behind that branch
            const MtsgTri &tr = tris[e];
            const uint32_t prim = tr.prim;
            const uint32_t k = tr.k;
            float o_u, o_v, o_k, d_u, d_v, d_k;
            if (k == 0) { o_u = o.y; o_v = o.z; o_k = o.x; d_u = d.y; d_v = d.z; d_k = d.x; }
            else if (k == 1) { o_u = o.z; o_v = o.x; o_k = o.y; d_u = d.z; d_v = d.x; d_k = d.y; }
            else { o_u = o.x; o_v = o.y; o_k = o.z; d_u = d.x; d_v = d.y; d_k = d.z; }
            // TriAccel::rayIntersect (triaccel.h:92-160) on [mint, maxt]
            const float t = (tr.n_d - o_u * tr.n_u - o_v * tr.n_v - o_k) / (d_u * tr.n_u + d_v * tr.n_v + d_k);
            const float hu = o_u + t * d_u - tr.a_u;
            const float hv = o_v + t * d_v - tr.a_v;
            const float u = hv * tr.b_nu + hu * tr.b_nv;
            const float v = hu * tr.c_nu + hv * tr.c_nv;
            if (mb(prim & 7u) == prim) continue;   // the hashed mailbox (sahkdtree3.h:138-152)
            if (!(t < mint || t > maxt) && u >= 0 && v >= 0 && u + v <= 1.0f) {
                if (ANY) return true;
                maxt = t;
                found = true;
                bt = t; bu = u; bv = v; bprim = prim;
            }
            mbset(prim & 7u, prim);
        }
        if (ex_t > maxt) break;
        if (sp == 0) break;   // the exit point was ray(maxt), whose node is NONE
        en_t = ex_t;
        en_split = ex_split;
        en_axis = ex_axis;
        Ent e;
        if (nr) {
            e = Ent{c0n & 0x3fffffffu, c0t, c0s, c0n >> 30};
            c0n = c1n; c0t = c1t; c0s = c1s;
            --nr;
        } else {
            e = ld(sp - 1);
        }
        --sp;
        node = e.node;
        ex_t = e.t;
        ex_split = e.split;
        ex_axis = e.axis;
    }
    return found;
}

// ShapeKDTree::rayIntersect (skdtree.cpp:112-142 closest, :207-226 shadow):
// scene-AABB clip + adaptive ray epsilon -> [mint, maxt] for the traversal
// (dRcp: aabb_clip's reciprocals, which scan_pair divides by)
__device__ __forceinline__ bool ray_interval(const MtsgDeviceScene &S, f3 o, f3 d, float rmint, float rmaxt,
                                             bool shadow, float &mint, float &maxt, f3 &dRcp) {
    if (!aabb_clip(S, o, d, mint, maxt, dRcp)) return false;
    float rayMinT = rmint;
    if (rayMinT == D_EPSILON) {
        if (shadow) rayMinT *= smax(smax(fabsf(o.x), fabsf(o.y)), fabsf(o.z));
        else rayMinT *= smax(smax(smax(fabsf(o.x), fabsf(o.y)), fabsf(o.z)), D_EPSILON);
    }
    if (rayMinT > mint) mint = rayMinT;
    if (rmaxt < maxt) maxt = rmaxt;
    return maxt > mint;
}
__device__ __forceinline__ bool ray_interval(const MtsgDeviceScene &S, f3 o, f3 d, float rmint, float rmaxt,
                                             bool shadow, float &mint, float &maxt) {
    f3 dRcp;
    return ray_interval(S, o, d, rmint, rmaxt, shadow, mint, maxt, dRcp);
}
