// dleaf2.h -- three more leaf BSDFs on the device: difftrans, roughdiffuse and phong (the
// MTSG_FEAT_SET_LEAF2 kernels only; included by dbsdf.h in front of its dispatchers).
//
//   src/bsdfs/difftrans.cpp:76-116   src/bsdfs/roughdiffuse.cpp:128-251   src/bsdfs/phong.cpp:127-250
//
// Float32 in the reference's expression order; powf, sincosf and acosf are glibc's
// (glibc_f32.h).  Only component == -1, typeMask == EAll queries exist, eval / pdf only in the
// solid-angle measure.  The records reuse MtsgBsdf's fields (layout.h names which).
#pragma once

enum { BSDF_DIFFTRANS = 12, BSDF_ROUGHDIFFUSE = 13, BSDF_PHONG = 14 };   // = MTSGPU_BSDF_*

__device__ __forceinline__ BSample leaf2_zero() {
    BSample r;
    r.weight = mk(0, 0, 0); r.pdf = 0; r.eta = 1.0f; r.sampledType = 0; r.wo = mk(0, 0, 1);
    return r;
}
__device__ __forceinline__ float l2_clamp(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float l2_sin_theta(f3 v) {           // frame.h:113-118
    const float temp = sin_theta2(v);
    if (temp <= 0.0f) return 0.0f;
    return dsqrt(temp);
}
__device__ __forceinline__ float l2_sin_phi(f3 v) {             // frame.h:140-145
    const float st = l2_sin_theta(v);
    if (st == 0.0f) return 1.0f;
    return l2_clamp(v.y / st, -1.0f, 1.0f);
}
__device__ __forceinline__ float l2_cos_phi(f3 v) {             // frame.h:149-154
    const float st = l2_sin_theta(v);
    if (st == 0.0f) return 1.0f;
    return l2_clamp(v.x / st, -1.0f, 1.0f);
}
__device__ __forceinline__ float l2_safe_acos(float v) { return d_acos(smin(1.0f, smax(-1.0f, v))); }   // math.h:250

// ---- difftrans -----------------------------------------------------------------------------
template <int BS>
__device__ __forceinline__ f3 dt_eval(GBsdf &b, f3 wi, f3 wo, float u, float v) {     // :76-83
    if (wi.z * wo.z >= 0) return mk(0, 0, 0);
    return mul(bsdf_refl<BS>(b, u, v), D_INV_PI * fabsf(wo.z));
}
__device__ __forceinline__ float dt_pdf(f3 wi, f3 wo) {                               // :85-91
    if (wi.z * wo.z >= 0) return 0.0f;
    return fabsf(wo.z) * D_INV_PI;
}
template <int BS>
__device__ __forceinline__ BSample dt_sample(GBsdf &b, f3 wi, float sx, float sy, float u, float v) {   // :105-116
    BSample r = leaf2_zero();
    r.wo = square_to_cosine_hemisphere(sx, sy);
    if (wi.z > 0) r.wo.z *= -1;
    r.eta = 1.0f;
    r.sampledType = MTSG_F_DIFF_TRANS;
    r.pdf = fabsf(r.wo.z) * D_INV_PI;
    r.weight = bsdf_refl<BS>(b, u, v);
    return r;
}

// ---- roughdiffuse --------------------------------------------------------------------------
template <int BS>
__device__ __forceinline__ f3 rdiff_eval(GBsdf &b, f3 wi, f3 wo, float u, float v) {   // :128-218
    if (wi.z <= 0 || wo.z <= 0) return mk(0, 0, 0);
    const float conversionFactor = 1 / dsqrt(2.0f);
    float alpha = b.alpha_u;   // m_alpha->eval(its).average()
    if (b.alpha_tex.type) alpha = avg3(tex_eval(b.alpha_tex, u, v));
    else alpha = avg3(mk(alpha, alpha, alpha));
    const float sigma = alpha * conversionFactor;
    const float sigma2 = sigma * sigma;
    const float sinThetaI = l2_sin_theta(wi), sinThetaO = l2_sin_theta(wo);
    float cosPhiDiff = 0;
    if (sinThetaI > D_EPSILON && sinThetaO > D_EPSILON) {
        const float sinPhiI = l2_sin_phi(wi), cosPhiI = l2_cos_phi(wi), sinPhiO = l2_sin_phi(wo), cosPhiO = l2_cos_phi(wo);
        cosPhiDiff = cosPhiI * cosPhiO + sinPhiI * sinPhiO;
    }
    const f3 rho = bsdf_refl<BS>(b, u, v);
    if (b.nonlinear) {   // useFastApprox (:159-174)
        const float A = 1.0f - 0.5f * sigma2 / (sigma2 + 0.33f), B = 0.45f * sigma2 / (sigma2 + 0.09f);
        float sinAlpha, tanBeta;
        if (wi.z > wo.z) {
            sinAlpha = sinThetaO;
            tanBeta = sinThetaI / wi.z;
        } else {
            sinAlpha = sinThetaI;
            tanBeta = sinThetaO / wo.z;
        }
        return mul(rho, D_INV_PI * wo.z * (A + B * smax(cosPhiDiff, 0.0f) * sinAlpha * tanBeta));
    }
    // the full model (:175-217)
    const float thetaI = l2_safe_acos(wi.z), thetaO = l2_safe_acos(wo.z);
    const float alphaA = smax(thetaI, thetaO), beta = smin(thetaI, thetaO);
    float sinAlpha, sinBeta, tanBeta;
    if (wi.z > wo.z) {
        sinAlpha = sinThetaO; sinBeta = sinThetaI;
        tanBeta = sinThetaI / wi.z;
    } else {
        sinAlpha = sinThetaI; sinBeta = sinThetaO;
        tanBeta = sinThetaO / wo.z;
    }
    const float tmp = sigma2 / (sigma2 + 0.09f), tmp2 = (4 * D_INV_PI * D_INV_PI) * alphaA * beta,
                tmp3 = 2 * beta * D_INV_PI;
    const float C1 = 1.0f - 0.5f * sigma2 / (sigma2 + 0.33f);
    float C2 = 0.45f * tmp;
    const float C3 = 0.125f * tmp * tmp2 * tmp2, C4 = 0.17f * sigma2 / (sigma2 + 0.13f);
    if (cosPhiDiff > 0) C2 *= sinAlpha;
    else C2 *= sinAlpha - tmp3 * tmp3 * tmp3;
    const float tanHalf = (sinAlpha + sinBeta) / (safe_sqrt(1.0f - sinAlpha * sinAlpha) + safe_sqrt(1.0f - sinBeta * sinBeta));
    const f3 snglScat = mul(rho, C1 + cosPhiDiff * C2 * tanBeta + (1.0f - fabsf(cosPhiDiff)) * C3 * tanHalf);
    const f3 dblScat = mul(mulv(rho, rho), C4 * (1.0f - cosPhiDiff * tmp3 * tmp3));
    return mul(add(snglScat, dblScat), D_INV_PI * wo.z);
}
__device__ __forceinline__ float rdiff_pdf(f3 wi, f3 wo) {                               // :220-227
    if (wi.z <= 0 || wo.z <= 0) return 0.0f;
    return D_INV_PI * wo.z;
}
template <int BS>
__device__ __forceinline__ BSample rdiff_sample(GBsdf &b, f3 wi, float sx, float sy, float u, float v) {   // :241-251
    BSample r = leaf2_zero();
    if (wi.z <= 0) return r;
    r.wo = square_to_cosine_hemisphere(sx, sy);
    r.eta = 1.0f;
    r.sampledType = MTSG_F_GLOSSY_REFL;
    r.pdf = D_INV_PI * r.wo.z;
    r.weight = divs(rdiff_eval<BS>(b, wi, r.wo, u, v), r.pdf);
    return r;
}

// ---- phong ---------------------------------------------------------------------------------
__device__ __forceinline__ float phong_exponent(GBsdf &b) { return avg3(mk(b.alpha_u, b.alpha_u, b.alpha_u)); }
template <int BS>
__device__ __forceinline__ f3 phong_eval(GBsdf &b, f3 wi, f3 wo, float u, float v) {   // :127-151
    if (wi.z <= 0 || wo.z <= 0) return mk(0, 0, 0);
    f3 result = mk(0, 0, 0);
    const float alpha = dot(wo, mk(-wi.x, -wi.y, wi.z)), exponent = phong_exponent(b);
    if (alpha > 0.0f) result = add(result, mul(ld3(b.spec_r), (exponent + 2) * D_INV_TWOPI * d_powf(alpha, exponent)));
    result = add(result, mul(bsdf_refl<BS>(b, u, v), D_INV_PI));
    return mul(result, wo.z);
}
__device__ __forceinline__ float phong_pdf(GBsdf &b, f3 wi, f3 wo) {                    // :153-183
    if (wi.z <= 0 || wo.z <= 0) return 0.0f;
    float specProb = 0.0f;
    const float diffuseProb = D_INV_PI * wo.z;
    const float alpha = dot(wo, mk(-wi.x, -wi.y, wi.z)), exponent = phong_exponent(b);
    if (alpha > 0) specProb = d_powf(alpha, exponent) * (exponent + 1.0f) / (2.0f * D_PI);
    return b.spec_weight * specProb + (1 - b.spec_weight) * diffuseProb;
}
template <int BS>
__device__ __forceinline__ BSample phong_sample(GBsdf &b, f3 wi, float sx, float sy, float u, float v) {   // :185-245
    BSample r = leaf2_zero();
    bool choseSpecular = true;
    if (sx <= b.spec_weight) {
        sx /= b.spec_weight;
    } else {
        sx = (sx - b.spec_weight) / (1 - b.spec_weight);
        choseSpecular = false;
    }
    if (choseSpecular) {
        const f3 R = mk(-wi.x, -wi.y, wi.z);
        const float exponent = phong_exponent(b);
        // a Phong lobe around (0, 0, 1) ...
        const float sinAlpha = dsqrt(1 - d_powf(sy, 2 / (exponent + 1)));
        const float cosAlpha = d_powf(sy, 1 / (exponent + 1));
        const float phi = (2.0f * D_PI) * sx;
        float s, c;
        d_sincos(phi, &s, &c);
        const f3 localDir = mk(sinAlpha * c, sinAlpha * s, cosAlpha);
        // ... rotated about R: Frame(R).toWorld, coordinateSystem (util.cpp:592-601)
        f3 fs, ft;
        if (fabsf(R.x) > fabsf(R.y)) {
            const float invLen = 1.0f / dsqrt(R.x * R.x + R.z * R.z);
            ft = mk(R.z * invLen, 0.0f, -R.x * invLen);
        } else {
            const float invLen = 1.0f / dsqrt(R.y * R.y + R.z * R.z);
            ft = mk(0.0f, R.z * invLen, -R.y * invLen);
        }
        fs = cross(ft, R);
        r.wo = add(add(mul(fs, localDir.x), mul(ft, localDir.y)), mul(R, localDir.z));
        r.sampledType = MTSG_F_GLOSSY_REFL;
        if (r.wo.z <= 0) return r;
    } else {
        r.wo = square_to_cosine_hemisphere(sx, sy);
        r.sampledType = MTSG_F_DIFF_REFL;
    }
    r.eta = 1.0f;
    r.pdf = phong_pdf(b, wi, r.wo);
    if (r.pdf == 0) return r;
    r.weight = divs(phong_eval<BS>(b, wi, r.wo, u, v), r.pdf);
    return r;
}

// ---- the three behind one out-of-line call each (dbsdf.h's dispatchers, BSet<BS>::LEAF2) -----
template <int BS>
__device__ __noinline__ f3 leaf2_eval(GBsdf &b, f3 wi, f3 wo, float u, float v) {
    if (b.type == BSDF_PHONG) return phong_eval<BS>(b, wi, wo, u, v);
    if (b.type == BSDF_ROUGHDIFFUSE) return rdiff_eval<BS>(b, wi, wo, u, v);
    return dt_eval<BS>(b, wi, wo, u, v);
}
template <int BS>
__device__ __noinline__ float leaf2_pdf(GBsdf &b, f3 wi, f3 wo) {
    if (b.type == BSDF_PHONG) return phong_pdf(b, wi, wo);
    if (b.type == BSDF_ROUGHDIFFUSE) return rdiff_pdf(wi, wo);
    return dt_pdf(wi, wo);
}
template <int BS>
__device__ __noinline__ BSample leaf2_sample(GBsdf &b, f3 wi, float sx, float sy, float u, float v) {
    if (b.type == BSDF_PHONG) return phong_sample<BS>(b, wi, sx, sy, u, v);
    if (b.type == BSDF_ROUGHDIFFUSE) return rdiff_sample<BS>(b, wi, sx, sy, u, v);
    return dt_sample<BS>(b, wi, sx, sy, u, v);
}
