// dcombo.h -- the combinator BSDFs on the device: mixturebsdf, blendbsdf, mask, and twosided
// over them (the MTSG_FEAT_SET_COMBO kernels only).
//
//   src/bsdfs/mixturebsdf.cpp:174-277   src/bsdfs/blendbsdf.cpp:135-270
//   src/bsdfs/mask.cpp:113-219          src/bsdfs/twosided.cpp:108-185
//   include/mitsuba/core/pmf.h:124-169  (m_pdf.sampleReuse: dpath.h dd_sample_reuse)
//
// The reference nests BSDF objects and recurses through their virtual eval / pdf / sample.
// The device has no recursion: the one chain configure accepts (configure_bsdf.cpp),
//     [mask] -> [twosided] -> [mixturebsdf | blendbsdf] -> leaf
// is walked level by level, every level optional; the leaves are dbsdf.h's out-of-line
// bsdf_eval / bsdf_pdf / bsdf_sample.  Only component == -1, typeMask == EAll queries exist
// (path.cpp, volpath.cpp, direct.cpp make no other), eval / pdf only in the solid-angle measure.
#pragma once
#include "dbsdf.h"

typedef const __attribute__((address_space(1))) MtsgCombo GCombo;

// Spectrum::getLuminance (spectrum.h, the sRGB build): (r * 0.212671f + g * 0.715160f) + b * 0.072169f
__device__ __forceinline__ float combo_luminance(f3 s) { return (s.x * 0.212671f + s.y * 0.715160f) + s.z * 0.072169f; }
// the combinator's texture or constant at the hit: blend 'weight', mask 'opacity'
__device__ __forceinline__ f3 combo_tex(GCombo &c, float u, float v) {
    if (c.tex.type) return tex_eval(c.tex, u, v);
    return ld3(c.value);
}
// BlendBSDF's weight (blendbsdf.cpp:136-137): min(1, max(0, m_weight->eval(its).average()))
__device__ __forceinline__ float blend_weight(GCombo &c, float u, float v) {
    return smin(1.0f, smax(0.0f, avg3(combo_tex(c, u, v))));
}
// child i's weight and selection probability: mixture m_weights[i] / m_pdf[i], blend weights[i] twice
__device__ __forceinline__ void combo_child_w(GCombo &c, int i, float bw, float &w, float &p) {
    if (c.type == BSDF_BLEND) { w = p = i == 0 ? 1 - bw : bw; }
    else { w = c.w[i]; p = c.cdf[i + 1] - c.cdf[i]; }
}

// The sum over the children of a mixture / blend, in index order, on top of `acc`:
//   acc.pdf += child.pdf * p[i];  acc.val += child.eval * w[i]      (every i but `skip`)
// pdf() and eval() start from zero with skip = -1 (mixturebsdf.cpp:178-179, 195-196;
// blendbsdf.cpp:141-142, 162-163); sample() starts from the chosen child's scaled sample and
// skips it (mixturebsdf.cpp:258-263, blendbsdf.cpp:247-252): one function, so the path's NEE
// (eval, pdf) and its BSDF sample form the sibling terms by the same code.  The children's
// eval and pdf are separate calls: bsdf_eval_pdf would zero a pdf whose value is zero
template <int BS>
__device__ __forceinline__ EvalPdf combo_sum(GBsdf *bsdfs, glb_f32 *rt, GCombo &c, float bw, int skip, EvalPdf acc, f3 wi,
                                             f3 wo, float u, float v) {
    for (int i = 0; i < c.n; ++i) {
        if (i == skip) continue;
        GBsdf &cb = bsdfs[c.child[i]];
        float w, p;
        combo_child_w(c, i, bw, w, p);
        acc.pdf += bsdf_pdf<BS>(cb, rt, wi, wo, u, v) * p;
        acc.val = add(acc.val, mul(bsdf_eval<BS>(cb, rt, wi, wo, u, v), w));
    }
    return acc;
}

// eval(bRec, ESolidAngle) and pdf(bRec, ESolidAngle) of the BSDF `top` through the chain
template <int BS>
__device__ __noinline__ EvalPdf combo_eval_pdf(GBsdf *bsdfs, GCombo *combos, glb_f32 *rt, GBsdf *top, f3 wi, f3 wo,
                                               float u, float v) {
    GBsdf *b = top;
    bool masked = false;
    f3 opacity = mk(1.0f, 1.0f, 1.0f);
    if (b->type == BSDF_MASK) {          // mask.cpp:113-147
        GCombo &m = combos[b->nested[0]];
        opacity = combo_tex(m, u, v);
        masked = true;
        b = &bsdfs[m.child[0]];
    }
    if (b->type == BSDF_TWOSIDED) {      // twosided.cpp:108-134
        const bool flip = !(wi.z > 0);
        b = &bsdfs[b->nested[flip ? 1 : 0]];
        if (flip) { wi.z = -wi.z; wo.z = -wo.z; }
    }
    EvalPdf r;
    if (b->type == BSDF_MIXTURE || b->type == BSDF_BLEND) {
        GCombo &c = combos[b->nested[0]];
        const float bw = b->type == BSDF_BLEND ? blend_weight(c, u, v) : 0.0f;
        const EvalPdf zero = {mk(0, 0, 0), 0.0f};
        r = combo_sum<BS>(bsdfs, rt, c, bw, -1, zero, wi, wo, u, v);
    } else {
        r.val = bsdf_eval<BS>(*b, rt, wi, wo, u, v);
        r.pdf = bsdf_pdf<BS>(*b, rt, wi, wo, u, v);
    }
    if (masked) {
        r.val = mulv(r.val, opacity);
        r.pdf *= combo_luminance(opacity);
    }
    return r;
}

// sample(bRec, pdf, sample) of the BSDF `top` through the chain
template <int BS>
__device__ __noinline__ BSample combo_sample(GBsdf *bsdfs, GCombo *combos, glb_f32 *rt, GBsdf *top, f3 wi, float sx,
                                             float sy, float u, float v) {
    GBsdf *b = top;
    bool masked = false;
    f3 opacity = mk(1.0f, 1.0f, 1.0f);
    float prob = 1.0f;
    if (b->type == BSDF_MASK) {          // mask.cpp:183-219
        GCombo &m = combos[b->nested[0]];
        opacity = combo_tex(m, u, v);
        prob = combo_luminance(opacity);
        if (sx < prob) {
            sx /= prob;
            masked = true;
            b = &bsdfs[m.child[0]];
        } else {                         // the null lobe: straight through
            BSample r;
            r.wo = neg(wi);
            r.eta = 1.0f;
            r.sampledType = MTSG_F_NULL;
            r.pdf = 1 - prob;
            r.weight = divs(sub(mk(1.0f, 1.0f, 1.0f), opacity), r.pdf);
            return r;
        }
    }
    bool flip = false;
    if (b->type == BSDF_TWOSIDED) {      // twosided.cpp:161-185
        flip = wi.z < 0;
        if (flip) wi.z = -wi.z;
        b = &bsdfs[b->nested[flip ? 1 : 0]];
    }
    BSample bs;
    if (b->type == BSDF_MIXTURE || b->type == BSDF_BLEND) {
        GCombo &c = combos[b->nested[0]];
        float bw = 0.0f, w, p;
        int entry;
        if (b->type == BSDF_BLEND) {     // blendbsdf.cpp:224-236
            bw = blend_weight(c, u, v);
            const float w0 = 1 - bw;
            if (sx < w0) { entry = 0; sx /= w0; }
            else { entry = 1; sx = (sx - w0) / bw; }
        } else {                         // mixturebsdf.cpp:248
            entry = (int)dd_sample_reuse((const float *)c.cdf, (uint32_t)c.n, sx, nullptr);
        }
        combo_child_w(c, entry, bw, w, p);
        GBsdf &cb = bsdfs[c.child[entry]];
        bs = bsdf_sample<BS>(cb, rt, wi, sx, sy, 0.0f, u, v, rp_pre_for<BS>(cb, rt, wi, u, v));
        // sampling failed: the weight is zero and stays zero through twosided's flip test and the
        // mask's `* opacity / prob`, which are skipped here; the callers read nothing else of a
        // failed sample (its pdf would lack the mask's `*= prob`)
        if (is_zero(bs.weight)) return bs;
        EvalPdf acc;
        acc.val = mul(bs.weight, w * bs.pdf);
        acc.pdf = bs.pdf * p;
        // a delta sample: the siblings are queried in the discrete measure, where every smooth
        // lobe evaluates to exactly 0 in value and in pdf (configure allows one delta-lobed child)
        if (!(bs.sampledType & MTSG_F_DELTA)) acc = combo_sum<BS>(bsdfs, rt, c, bw, entry, acc, wi, bs.wo, u, v);
        bs.weight = divs(acc.val, acc.pdf);
        bs.pdf = acc.pdf;
    } else {
        bs = bsdf_sample<BS>(*b, rt, wi, sx, sy, 0.0f, u, v, rp_pre_for<BS>(*b, rt, wi, u, v));
    }
    if (flip && !is_zero(bs.weight) && bs.pdf != 0) bs.wo.z = -bs.wo.z;
    if (masked) {
        bs.weight = divs(mulv(bs.weight, opacity), prob);
        bs.pdf *= prob;
    }
    return bs;
}
