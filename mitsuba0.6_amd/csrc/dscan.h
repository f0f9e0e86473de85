// dscan.h -- the tiny-scene scan: every lane tests every TriAccel record
// (include/mitsuba/render/triaccel.h:92-160), read with uniform indices from the constant
// address space, one ray at a time (scan_tris) or a bounce's shadow and closest-hit rays
// together (scan_pair).  Included by dpath.h.
#pragma once

typedef __attribute__((address_space(4))) const MtsgTri cst_tri;
// one projection axis' records: the coordinate permutation is a compile-time
// constant, so the loop is straight-line code around the correctly rounded
// division; each record is read whole (two scalar loads) at the loop head
// AL: the group whose plane normal lies along axis K (n_u and n_v both +-0,
// L.scan_n): then the numerator is n_d - o_k and the denominator d_k,
// exactly (a +-0 product added to a nonzero value leaves it unchanged).  Where
// the sum is zero the two forms may differ in the sign of that zero only: a
// zero numerator gives t = +-0 either way, and +0 and -0 pass every comparison
// alike; a zero d_k gives +-inf (rejected by the finite clipped [mint, maxt])
// or NaN (rejected by the barycentric test).  C2 +1.75%
// (profiles/r05_ab_aligned_scan.log)
template <int K, bool AL, bool ANY, bool STATS>
__device__ __forceinline__ bool scan_k(cst_tri *tris, uint32_t n, f3 o, f3 d, float mint, bool &found,
                                       uint32_t &bestPrim, float &bu, float &bv, float &bt,
                                       unsigned long long &tests) {
    const float o_u = K == 0 ? o.y : K == 1 ? o.z : o.x, o_v = K == 0 ? o.z : K == 1 ? o.x : o.y,
                o_k = K == 0 ? o.x : K == 1 ? o.y : o.z;
    const float d_u = K == 0 ? d.y : K == 1 ? d.z : d.x, d_v = K == 0 ? d.z : K == 1 ? d.x : d.y,
                d_k = K == 0 ? d.x : K == 1 ? d.y : d.z;
    for (uint32_t i = 0; i < n; ++i) {
        if (STATS) tests++;
        cst_tri &tr = tris[i];
        const float n_u = tr.n_u, n_v = tr.n_v, n_d = tr.n_d, a_u = tr.a_u, a_v = tr.a_v, b_nu = tr.b_nu,
                    b_nv = tr.b_nv, c_nu = tr.c_nu, c_nv = tr.c_nv;
        const uint32_t prim = tr.prim;
        // TriAccel::rayIntersect (triaccel.h:92-160)
        const float t = AL ? (n_d - o_k) / d_k : (n_d - o_u * n_u - o_v * n_v - o_k) / (d_u * n_u + d_v * n_v + d_k);
        if (t < mint || t > bt) continue;
        const float hu = o_u + t * d_u - a_u;
        const float hv = o_v + t * d_v - a_v;
        const float u = hv * b_nu + hu * b_nv;
        const float v = hu * c_nu + hv * c_nv;
        if (u >= 0 && v >= 0 && u + v <= 1.0f) {
            if (ANY) return true;
            if (!found || t < bt || prim > bestPrim) {
                found = true; bestPrim = prim; bt = t; bu = u; bv = v;
            }
        }
    }
    return false;
}

// Tiny scenes (<= MTSG_SCAN_MAX triangles, no analytic shapes): every lane
// tests every TriAccel record, read from the constant address space with a
// uniform index (scalar loads into SGPRs): no traversal stack, no divergent
// node loop.  The records come grouped by projection axis (L.scan_tris, each
// axis' records with an axis-aligned plane last); the
// result -- the closest t, ties to the larger primitive index as in
// traverse() -- does not depend on the test order.  Returns the
// primitive index (not a slot) in bestPrim.
template <bool ANY, bool STATS>
__device__ __forceinline__ bool scan_tris(const MtsgLaunch &L, f3 o, f3 d, float mint, float maxt,
                                          uint32_t &bestPrim, float &bu, float &bv, float &bt,
                                          unsigned long long &tests) {
    cst_tri *tris = (cst_tri *)L.scan_tris;
    bool found = false;
    bestPrim = 0;
    bt = maxt;
#define MTSG_SCAN_GROUP(K, AL)                                                                                   \
    if (scan_k<K, AL, ANY, STATS>(tris, L.scan_n[2 * K + AL] & 0xffffu, o, d, mint, found, bestPrim, bu, bv, bt, \
                                  tests))                                                                        \
        return true;                                                                                             \
    tris += L.scan_n[2 * K + AL] & 0xffffu;
    MTSG_SCAN_GROUP(0, false) MTSG_SCAN_GROUP(0, true) MTSG_SCAN_GROUP(1, false) MTSG_SCAN_GROUP(1, true)
    MTSG_SCAN_GROUP(2, false) MTSG_SCAN_GROUP(2, true)
#undef MTSG_SCAN_GROUP
    return found;
}

// The megakernel's two rays of one bounce leave the same vertex (the NEE
// shadow ray and the next closest-hit ray, both from its.p), so a tiny scene
// tests them in one pass over the records: the TriAccel numerator is shared,
// the records are loaded once, and the pairs of products pack into
// v_pk_mul/v_pk_add.  Each ray's result is exactly that of its own scan_tris
// (an empty interval, mint = +inf and maxt = -inf, disables a ray).
// a / b from y = RN(1/b) (correctly rounded, computed once per ray): the
// quotient a * y with two residual corrections, r = a - b q exact by FMA and
// q' = RN(q + r y) (Markstein's theorem: with y = RN(1/b) and q within an ulp
// of a/b, q' = RN(a/b)).  It equals IEEE a / b wherever nothing underflows;
// scan_pair takes it only for rays with |b| >= 2^-60 and mint >= 2^-30, where
// a quotient small enough to underflow is rejected by mint either way.  Host
// check: 1.6e9 random and edge-mantissa pairs over that range, bit-equal to
// IEEE division (tools/gpu_runs/r05/fast_div_check.c).
__device__ __forceinline__ float div_by_rcp(float a, float b, float y) {
    float q = a * y;
    float r = __builtin_fmaf(-b, q, a);
    q = __builtin_fmaf(r, y, q);
    r = __builtin_fmaf(-b, q, a);
    return __builtin_fmaf(r, y, q);
}

// FAST (axis-aligned groups only): the two quotients through div_by_rcp with
// the rays' reciprocals yS = RN(1/s_k), yC = RN(1/c_k)
// The group's first np pairs of records (tris[2i], tris[2i + 1]) share their
// plane and vertex A bit for bit (render_plan.cpp mtsg_scan_layout: the two triangles
// of a quad), so num, both quotients and each ray's hu, hv are formed once for
// the two; only the barycentrics and the acceptance run per partner.  Every
// lane ends with what two successive single iterations give it: partner 1's
// interval test would read tC against bt after partner 0, which is either
// unchanged or tC itself, so it passes whenever partner 0's did and is not
// repeated; on that tie the prim > bestPrim rule decides as before.
template <int K, bool AL, bool FAST, bool STATS>
__device__ __forceinline__ void scan_pair_k(cst_tri *tris, uint32_t n, uint32_t np, f3 o, f3 ds, f3 dc, float minS,
                                            float maxS, float minC, bool &occ, bool &found, uint32_t &bestPrim,
                                            float &bu, float &bv, float &bt, unsigned long long &tests, float yS = 0,
                                            float yC = 0) {
    const float o_u = K == 0 ? o.y : K == 1 ? o.z : o.x, o_v = K == 0 ? o.z : K == 1 ? o.x : o.y,
                o_k = K == 0 ? o.x : K == 1 ? o.y : o.z;
    const float s_u = K == 0 ? ds.y : K == 1 ? ds.z : ds.x, s_v = K == 0 ? ds.z : K == 1 ? ds.x : ds.y,
                s_k = K == 0 ? ds.x : K == 1 ? ds.y : ds.z;
    const float c_u = K == 0 ? dc.y : K == 1 ? dc.z : dc.x, c_v = K == 0 ? dc.z : K == 1 ? dc.x : dc.y,
                c_k = K == 0 ? dc.x : K == 1 ? dc.y : dc.z;
    for (uint32_t i = 0; i < np; ++i) {
        if (STATS) tests += 4;
        cst_tri &tr = tris[2 * i], &tq = tris[2 * i + 1];
        const float n_u = tr.n_u, n_v = tr.n_v, n_d = tr.n_d, a_u = tr.a_u, a_v = tr.a_v;
        const float b_nu0 = tr.b_nu, b_nv0 = tr.b_nv, c_nu0 = tr.c_nu, c_nv0 = tr.c_nv;
        const float b_nu1 = tq.b_nu, b_nv1 = tq.b_nv, c_nu1 = tq.c_nu, c_nv1 = tq.c_nv;
        const uint32_t prim0 = tr.prim, prim1 = tq.prim;
        const float num = AL ? n_d - o_k : n_d - o_u * n_u - o_v * n_v - o_k;
        const float tS = (AL && FAST) ? div_by_rcp(num, s_k, yS) : num / (AL ? s_k : s_u * n_u + s_v * n_v + s_k);
        const float tC = (AL && FAST) ? div_by_rcp(num, c_k, yC) : num / (AL ? c_k : c_u * n_u + c_v * n_v + c_k);
        if (!(tS < minS || tS > maxS)) {
            const float hu = o_u + tS * s_u - a_u;
            const float hv = o_v + tS * s_v - a_v;
            const float u0 = hv * b_nu0 + hu * b_nv0;
            const float v0 = hu * c_nu0 + hv * c_nv0;
            if (u0 >= 0 && v0 >= 0 && u0 + v0 <= 1.0f) occ = true;
            const float u1 = hv * b_nu1 + hu * b_nv1;
            const float v1 = hu * c_nu1 + hv * c_nv1;
            if (u1 >= 0 && v1 >= 0 && u1 + v1 <= 1.0f) occ = true;
        }
        if (!(tC < minC || tC > bt)) {
            const float hu = o_u + tC * c_u - a_u;
            const float hv = o_v + tC * c_v - a_v;
            const float u0 = hv * b_nu0 + hu * b_nv0;
            const float v0 = hu * c_nu0 + hv * c_nv0;
            if (u0 >= 0 && v0 >= 0 && u0 + v0 <= 1.0f) {
                if (!found || tC < bt || prim0 > bestPrim) {
                    found = true; bestPrim = prim0; bt = tC; bu = u0; bv = v0;
                }
            }
            const float u1 = hv * b_nu1 + hu * b_nv1;
            const float v1 = hu * c_nu1 + hv * c_nv1;
            if (u1 >= 0 && v1 >= 0 && u1 + v1 <= 1.0f) {
                if (!found || tC < bt || prim1 > bestPrim) {
                    found = true; bestPrim = prim1; bt = tC; bu = u1; bv = v1;
                }
            }
        }
    }
    for (uint32_t i = 2 * np; i < n; ++i) {
        if (STATS) tests += 2;
        cst_tri &tr = tris[i];
        const float n_u = tr.n_u, n_v = tr.n_v, n_d = tr.n_d, a_u = tr.a_u, a_v = tr.a_v, b_nu = tr.b_nu,
                    b_nv = tr.b_nv, c_nu = tr.c_nu, c_nv = tr.c_nv;
        const uint32_t prim = tr.prim;
        // TriAccel::rayIntersect (triaccel.h:92-160) for both rays
        // (AL: as in scan_k)
        const float num = AL ? n_d - o_k : n_d - o_u * n_u - o_v * n_v - o_k;
        const float tS = (AL && FAST) ? div_by_rcp(num, s_k, yS) : num / (AL ? s_k : s_u * n_u + s_v * n_v + s_k);
        const float tC = (AL && FAST) ? div_by_rcp(num, c_k, yC) : num / (AL ? c_k : c_u * n_u + c_v * n_v + c_k);
        if (!(tS < minS || tS > maxS)) {
            const float hu = o_u + tS * s_u - a_u;
            const float hv = o_v + tS * s_v - a_v;
            const float u = hv * b_nu + hu * b_nv;
            const float v = hu * c_nu + hv * c_nv;
            if (u >= 0 && v >= 0 && u + v <= 1.0f) occ = true;
        }
        if (!(tC < minC || tC > bt)) {
            const float hu = o_u + tC * c_u - a_u;
            const float hv = o_v + tC * c_v - a_v;
            const float u = hv * b_nu + hu * b_nv;
            const float v = hu * c_nu + hv * c_nv;
            if (u >= 0 && v >= 0 && u + v <= 1.0f) {
                if (!found || tC < bt || prim > bestPrim) {
                    found = true; bestPrim = prim; bt = tC; bu = u; bv = v;
                }
            }
        }
    }
}

// rS, rC: the rays' reciprocal directions as ray_interval's clip formed them.  A ray
// that is on passed the clip's three axes, so each r_k with d_k != 0 is RN(1 / d_k), and
// `fast` admits only such axes; a ray that is off (no ray, an early exit of the clip, an
// empty interval) may carry anything there: its interval rejects every finite or
// infinite quotient and its barycentric test a NaN one.
// (-DMTSG_CLIP_RCP=0: scan_pair divides again, for A/B builds)
#ifndef MTSG_CLIP_RCP
#define MTSG_CLIP_RCP 1
#endif
template <bool STATS>
__device__ __forceinline__ void scan_pair(const MtsgLaunch &L, f3 o, f3 ds, f3 dc, f3 rS, f3 rC, float minS, float maxS,
                                          float minC, float maxC, bool &occ, bool &found, uint32_t &bestPrim,
                                          float &bu, float &bv, float &bt, unsigned long long &tests) {
    cst_tri *tris = (cst_tri *)L.scan_tris;
    occ = false;
    found = false;
    bestPrim = 0;
    bt = maxC;
    // a disabled ray (empty interval) may take the fast quotient whatever its direction
    const bool offS = !(minS <= maxS), offC = !(minC <= maxC);
    // scan_n: records | leading pairs << 16 per group (the rare slow aligned
    // pass tests its pairs as singles: the same result, less code)
#define MTSG_SCAN_GROUP(K)                                                                                         \
    {                                                                                                              \
        const uint32_t ng = L.scan_n[2 * K] & 0xffffu, na = L.scan_n[2 * K + 1] & 0xffffu;                         \
        scan_pair_k<K, false, false, STATS>(tris, ng, L.scan_n[2 * K] >> 16, o, ds, dc, minS, maxS, minC, occ,     \
                                            found, bestPrim, bu, bv, bt, tests);                                   \
        tris += ng;                                                                                                \
        if (na) {                                                                                                  \
            const float s_k = K == 0 ? ds.x : K == 1 ? ds.y : ds.z, c_k = K == 0 ? dc.x : K == 1 ? dc.y : dc.z;    \
            const float yS = MTSG_CLIP_RCP ? (K == 0 ? rS.x : K == 1 ? rS.y : rS.z) : 1.0f / s_k;                  \
            const float yC = MTSG_CLIP_RCP ? (K == 0 ? rC.x : K == 1 ? rC.y : rC.z) : 1.0f / c_k;                  \
            const bool fast = (offS || (minS >= 0x1p-30f && fabsf(s_k) >= 0x1p-60f)) &&                            \
                              (offC || (minC >= 0x1p-30f && fabsf(c_k) >= 0x1p-60f));                              \
            if (__all(fast))                                                                                       \
                scan_pair_k<K, true, true, STATS>(tris, na, L.scan_n[2 * K + 1] >> 16, o, ds, dc, minS, maxS,      \
                                                  minC, occ, found, bestPrim, bu, bv, bt, tests, yS, yC);          \
            else                                                                                                   \
                scan_pair_k<K, true, false, STATS>(tris, na, 0, o, ds, dc, minS, maxS, minC, occ, found,           \
                                                   bestPrim, bu, bv, bt, tests);                                   \
            tris += na;                                                                                            \
        }                                                                                                          \
    }
    MTSG_SCAN_GROUP(0) MTSG_SCAN_GROUP(1) MTSG_SCAN_GROUP(2)
#undef MTSG_SCAN_GROUP
}
