// configure_bsdf.cpp -- the BSDF plugins' constructors and configure():
//   diffuse, roughconductor, roughdielectric   bsdfs/diffuse.cpp:75-101, roughconductor.cpp:168-240,
//                                              roughdielectric.cpp:183-256, librender/bsdf.cpp:88-113
//   conductor, dielectric, plastic             conductor.cpp:164-212, dielectric.cpp:146-201, plastic.cpp:144-216
//   roughplastic                               roughplastic.cpp:197-300
//   twosided                                   twosided.cpp:82-103
//   difftrans, roughdiffuse, phong             difftrans.cpp:52-74, roughdiffuse.cpp:89-122, phong.cpp:60-107
//   default BSDFs                              Shape::configure (librender/shape.cpp:48-75)
#include "scene_build_impl.h"

namespace mtsg_host {
namespace {

float energy_scale(const float *s, int ensure) {   // BSDF::ensureEnergyConservation (bsdf.cpp:88-113)
    if (!ensure) return 1.0f;
    float mx = s[0];
    mx = fmax_std(mx, s[1]);
    mx = fmax_std(mx, s[2]);
    if (mx > 1.0f) return 0.99f * (1.0f / mx);
    return 1.0f;
}

// Texture getMaximum/getMinimum/getAverage (checkerboard.cpp, texture.cpp ConstantSpectrumTexture)
void tex_max(const mtsgpu_texture_desc &t, const float *c, float out[3]) {
    for (int i = 0; i < 3; ++i) out[i] = t.type ? fmax_std(t.color0[i], t.color1[i]) : c[i];
}
void tex_min(const mtsgpu_texture_desc &t, const float *c, float out[3]) {
    for (int i = 0; i < 3; ++i) out[i] = t.type ? fmin_std(t.color0[i], t.color1[i]) : c[i];
}
void tex_avg(const mtsgpu_texture_desc &t, const float *c, float out[3]) {
    for (int i = 0; i < 3; ++i) out[i] = t.type ? (t.color0[i] + t.color1[i]) * 0.5f : c[i];
}
float avg_spec(const float s[3]) { float r = 0.0f; r += s[0]; r += s[1]; r += s[2]; return r * (1.0f / 3); }

// a textured parameter into the device record; `scale` = ensureEnergyConservation's
// ScaleTexture factor (eval = nested eval * scale, scale.cpp:85-87)
int set_tex(const mtsgpu_texture_desc &t, float scale, MtsgTex &o, std::string &err) {
    std::memset(&o, 0, sizeof o);
    if (t.type == MTSGPU_TEX_NONE) return MTSGPU_OK;
    if (t.type != MTSGPU_TEX_CHECKERBOARD) { err = "unsupported texture type"; return MTSGPU_EINVAL; }
    o.type = t.type;
    for (int i = 0; i < 3; ++i) {
        o.c0[i] = scale != 1.0f ? t.color0[i] * scale : t.color0[i];
        o.c1[i] = scale != 1.0f ? t.color1[i] * scale : t.color1[i];
    }
    o.uoff = t.uoffset; o.voff = t.voffset; o.uscale = t.uscale; o.vscale = t.vscale;
    return MTSGPU_OK;
}

// m_specularSamplingWeight = sAvg / (dAvg + sAvg) of the (scaled) textures' averages
// (plastic.cpp:204-210, roughplastic.cpp:281-287); sd: the diffuse reflectance's energy scale
float specular_weight(const mtsgpu_bsdf_desc &d, float sd, const MtsgBsdf &b) {
    float davg[3], savg[3];
    tex_avg(d.reflectance_tex, d.diffuse_reflectance, davg);
    for (int i = 0; i < 3; ++i) {
        if (sd != 1.0f) davg[i] = davg[i] * sd;
        savg[i] = b.spec_r[i];
    }
    const float dAvg = luminance(davg), sAvg = luminance(savg);
    return sAvg / (dAvg + sAvg);
}

// RoughPlastic ctor + configure (roughplastic.cpp:197-300)
int configure_roughplastic(const mtsgpu_bsdf_desc &d, MtsgBsdf &b, std::vector<float> &rt, std::string &err) {
    if (d.int_ior < 0 || d.ext_ior < 0 || d.int_ior == d.ext_ior) {
        err = "The interior and exterior indices of refraction must be positive and differ!";
        return MTSGPU_EINVAL;
    }
    b.eta = d.int_ior / d.ext_ior;
    b.nonlinear = d.nonlinear ? 1 : 0;
    if (d.distribution < 0 || d.distribution > 2) {
        err = "Specified an invalid distribution, must be \"beckmann\", \"ggx\", or \"phong\"/\"as\"!";
        return MTSGPU_EINVAL;
    }
    b.distr = d.distribution;
    b.sample_visible = d.distribution == MTSGPU_DISTR_PHONG ? 0 : d.sample_visible;
    const float au = fmax_std(d.alpha_u, 1e-4f), av = fmax_std(d.alpha_v, 1e-4f);
    if (d.alpha_tex.type == MTSGPU_TEX_NONE && au != av) {
        err = "The 'roughplastic' plugin currently does not support anisotropic microfacet distributions!";
        return MTSGPU_EINVAL;
    }
    // m_alpha = ConstantFloatTexture(distr.getAlpha()) unless a texture was added
    float alpha3[3] = {au, au, au};
    b.alpha_u = b.alpha_v = avg3(au);
    int rc;
    // ensureEnergyConservation of both reflectances (bsdf.cpp:88-113)
    float mx[3];
    tex_max(d.reflectance_tex, d.diffuse_reflectance, mx);
    const float sd = energy_scale(mx, d.ensure_energy_conservation);
    const float ss = energy_scale(d.specular_reflectance, d.ensure_energy_conservation);
    for (int i = 0; i < 3; ++i) {
        b.refl[i] = sd != 1.0f ? d.diffuse_reflectance[i] * sd : d.diffuse_reflectance[i];
        b.spec_r[i] = ss != 1.0f ? d.specular_reflectance[i] * ss : d.specular_reflectance[i];
    }
    if ((rc = set_tex(d.reflectance_tex, sd, b.refl_tex, err))) return rc;
    if ((rc = set_tex(d.alpha_tex, 1.0f, b.alpha_tex, err))) return rc;
    b.spec_weight = specular_weight(d, sd, b);
    b.inv_eta2 = 1.0f / (b.eta * b.eta);
    b.flags = MTSG_F_GLOSSY_REFL | MTSG_F_DIFF_REFL | MTSG_F_FRONT;
    // RoughTransmittance(m_type): the distribution's table, checked and reduced
    MtsgRTrans ext;
    if ((rc = mtsg_rtrans_load(d.rtrans_data, (size_t)d.rtrans_bytes, ext, err))) {
        if (!d.rtrans_data) err = "roughplastic: no rough transmittance table (data/microfacet/<distribution>.dat)";
        return rc;
    }
    float amin[3], amax[3];
    tex_min(d.alpha_tex, alpha3, amin);
    tex_max(d.alpha_tex, alpha3, amax);
    if ((rc = mtsg_rtrans_check(ext, b.eta, avg_spec(amin), avg_spec(amax), err))) return rc;
    MtsgRTrans in = ext;
    mtsg_rtrans_set_eta(ext, b.eta);
    mtsg_rtrans_set_eta(in, 1 / b.eta);
    if (d.alpha_tex.type == MTSGPU_TEX_NONE) mtsg_rtrans_set_alpha(ext, b.alpha_u);
    b.rt_theta = (int32_t)ext.theta;
    b.rt_alpha = (int32_t)ext.alpha;
    b.rt_alpha_fixed = ext.alphaFixed ? 1 : 0;
    b.rt_alpha_min = ext.alphaMin;
    b.rt_alpha_max = ext.alphaMax;
    b.rt_ext = (int32_t)rt.size();
    rt.insert(rt.end(), ext.trans.begin(), ext.trans.end());
    b.rt_int = (int32_t)rt.size();
    rt.insert(rt.end(), in.diff.begin(), in.diff.end());
    // getDiffuseReflectance's m_externalRoughTransmittance->evalDiffuse(alpha) (roughplastic.cpp:
    // 309-315): the value for a constant alpha, the table's diffuse slice for a textured one
    if (d.alpha_tex.type == MTSGPU_TEX_NONE) b.ftr_ext = mtsg_rtrans_eval_diffuse(ext, b.alpha_u);
    else rt.insert(rt.end(), ext.diff.begin(), ext.diff.end());
    return MTSGPU_OK;
}

// fresnelDielectricExt(cosThetaI, eta) (util.cpp:651-677)
float fresnel_dielectric_ext_h(float cosThetaI_, float eta) {
    if (eta == 1) return 0.0f;
    const float scale = (cosThetaI_ > 0) ? 1 / eta : eta,
                cosThetaTSqr = 1 - (1 - cosThetaI_ * cosThetaI_) * (scale * scale);
    if (cosThetaTSqr <= 0.0f) return 1.0f;
    const float cosThetaI = std::fabs(cosThetaI_), cosThetaT = std::sqrt(cosThetaTSqr);
    const float Rs = (cosThetaI - eta * cosThetaT) / (cosThetaI + eta * cosThetaT);
    const float Rp = (eta * cosThetaI - cosThetaT) / (eta * cosThetaI + cosThetaT);
    return 0.5f * (Rs * Rs + Rp * Rp);
}

// GaussLobattoIntegrator(1024, 0, 1e-5f) with the convergence estimate
// (quad.cpp:287-409) over fresnelDiffuseIntegrand (util.cpp:808-811): the
// accurate branch of fresnelDiffuseReflectance(eta, false) (util.cpp:814-860).
// The six sub-steps are summed (and their evaluations counted) left to right.
struct FdrQuad {
    float eta;
    size_t evals = 0;
    static constexpr size_t kMaxEvals = 1024;
    static constexpr float kRelError = 1e-5f;
    const float alpha = (float)std::sqrt(2.0 / 3.0), beta = (float)(1.0 / std::sqrt(5.0));
    const float x1 = (float)0.94288241569547971906, x2 = (float)0.64185334234578130578,
                x3 = (float)0.23638319966214988028;
    float f(float xi) const { return fresnel_dielectric_ext_h(std::sqrt(xi), eta); }
    float abs_tolerance(float a, float b) {
        const float m = (a + b) / 2, h = (b - a) / 2;
        const float y1 = f(a), y3 = f(m - alpha * h), y5 = f(m - beta * h), y7 = f(m), y9 = f(m + beta * h),
                    y11 = f(m + alpha * h), y13 = f(b);
        const float acc = h * ((float)0.0158271919734801831 * (y1 + y13)
                             + (float)0.0942738402188500455 * (f(m - x1 * h) + f(m + x1 * h))
                             + (float)0.1550719873365853963 * (y3 + y11)
                             + (float)0.1888215739601824544 * (f(m - x2 * h) + f(m + x2 * h))
                             + (float)0.1997734052268585268 * (y5 + y9)
                             + (float)0.2249264653333395270 * (f(m - x3 * h) + f(m + x3 * h))
                             + (float)0.2426110719014077338 * y7);
        evals += 13;
        float r = 1.0f;
        const float integral2 = (h / 6) * (y1 + y13 + 5 * (y5 + y9));
        const float integral1 = (h / 1470) * (77 * (y1 + y13) + 432 * (y3 + y11) + 625 * (y5 + y9) + 672 * y7);
        if (std::fabs(integral2 - acc) != 0.0f) r = std::fabs(integral1 - acc) / std::fabs(integral2 - acc);
        if (r == 0.0f || r > 1.0f) r = 1.0f;
        float result = INFINITY;
        if (acc != 0) result = acc * fmax_std(kRelError, FLT_EPSILON) / (r * FLT_EPSILON);
        return result;
    }
    float step(float a, float b, float fa, float fb, float acc) {
        const float h = (b - a) / 2, m = (a + b) / 2;
        const float mll = m - alpha * h, ml = m - beta * h, mr = m + beta * h, mrr = m + alpha * h;
        const float fmll = f(mll), fml = f(ml), fm = f(m), fmr = f(mr), fmrr = f(mrr);
        const float integral2 = (h / 6) * (fa + fb + 5 * (fml + fmr));
        const float integral1 = (h / 1470) * (77 * (fa + fb) + 432 * (fmll + fmrr) + 625 * (fml + fmr) + 672 * fm);
        evals += 5;
        if (evals >= kMaxEvals) return integral1;
        const float dist = acc + (integral1 - integral2);
        if (dist == acc || mll <= a || b <= mrr) return integral1;
        float r = step(a, mll, fa, fmll, acc);
        r = r + step(mll, ml, fmll, fml, acc);
        r = r + step(ml, m, fml, fm, acc);
        r = r + step(m, mr, fm, fmr, acc);
        r = r + step(mr, mrr, fmr, fmrr, acc);
        r = r + step(mrr, b, fmrr, fb, acc);
        return r;
    }
    float integrate() {   // over [0, 1]
        const float tol = abs_tolerance(0.0f, 1.0f);
        evals += 2;
        return step(0.0f, 1.0f, f(0.0f), f(1.0f), tol);
    }
};

float fresnel_diffuse_reflectance(float eta) {
    FdrQuad q;
    q.eta = eta;
    return q.integrate();
}

// SmoothConductor / SmoothDielectric / SmoothPlastic ctor + configure
// (conductor.cpp:164-212, dielectric.cpp:146-201, plastic.cpp:144-216)
int configure_smooth(const mtsgpu_bsdf_desc &d, MtsgBsdf &b, std::string &err) {
    const float ss = energy_scale(d.specular_reflectance, d.ensure_energy_conservation);
    for (int i = 0; i < 3; ++i) b.spec_r[i] = ss != 1.0f ? d.specular_reflectance[i] * ss : d.specular_reflectance[i];
    if (d.type == MTSGPU_BSDF_CONDUCTOR) {
        const float r = 1.0f / d.ext_eta;   // m_eta = eta / extEta (Spectrum / Float: reciprocal multiply)
        for (int i = 0; i < 3; ++i) { b.eta3[i] = d.eta[i] * r; b.k3[i] = d.k[i] * r; }
        b.flags = MTSG_F_DELTA_REFL | MTSG_F_FRONT;
        return MTSGPU_OK;
    }
    if (d.int_ior < 0 || d.ext_ior < 0) {
        err = "The interior and exterior indices of refraction must be positive!";
        return MTSGPU_EINVAL;
    }
    b.eta = d.int_ior / d.ext_ior;
    if (d.type == MTSGPU_BSDF_DIELECTRIC) {
        b.inv_eta = 1 / b.eta;
        const float st = energy_scale(d.specular_transmittance, d.ensure_energy_conservation);
        for (int i = 0; i < 3; ++i)
            b.spec_t[i] = st != 1.0f ? d.specular_transmittance[i] * st : d.specular_transmittance[i];
        b.flags = MTSG_F_DELTA_REFL | MTSG_F_DELTA_TRANS | MTSG_F_FRONT | MTSG_F_BACK;
        return MTSGPU_OK;
    }
    // plastic
    b.nonlinear = d.nonlinear ? 1 : 0;
    float mx[3];
    tex_max(d.reflectance_tex, d.diffuse_reflectance, mx);
    const float sd = energy_scale(mx, d.ensure_energy_conservation);
    for (int i = 0; i < 3; ++i) b.refl[i] = sd != 1.0f ? d.diffuse_reflectance[i] * sd : d.diffuse_reflectance[i];
    int rc;
    if ((rc = set_tex(d.reflectance_tex, sd, b.refl_tex, err))) return rc;
    b.fdr_int = fresnel_diffuse_reflectance(1 / b.eta);
    b.fdr_ext = fresnel_diffuse_reflectance(b.eta);
    b.spec_weight = specular_weight(d, sd, b);
    b.inv_eta2 = 1 / (b.eta * b.eta);
    b.flags = MTSG_F_DELTA_REFL | MTSG_F_DIFF_REFL | MTSG_F_FRONT;
    return MTSGPU_OK;
}

// DiffuseTransmitter, RoughDiffuse and Phong: ctor + configure into the fields
// MtsgBsdf already has (layout.h names which)
int configure_leaf2(const mtsgpu_bsdf_desc &d, MtsgBsdf &b, std::string &err) {
    int rc;
    const int ens = d.ensure_energy_conservation;
    if (d.type == MTSGPU_BSDF_DIFFTRANS || d.type == MTSGPU_BSDF_ROUGHDIFFUSE) {
        const bool dt = d.type == MTSGPU_BSDF_DIFFTRANS;
        const mtsgpu_texture_desc &t = dt ? d.transmittance_tex : d.reflectance_tex;
        const float *c = dt ? d.transmittance : d.reflectance;
        float mx[3];
        tex_max(t, c, mx);
        const float sc = energy_scale(mx, ens);
        for (int i = 0; i < 3; ++i) b.refl[i] = sc != 1.0f ? c[i] * sc : c[i];
        if ((rc = set_tex(t, sc, b.refl_tex, err))) return rc;
        if (dt) {
            b.flags = MTSG_F_DIFF_TRANS | MTSG_F_FRONT | MTSG_F_BACK;
            return MTSGPU_OK;
        }
        // m_alpha = ConstantFloatTexture(alpha) as given: no clamp (roughdiffuse.cpp:97)
        b.alpha_u = b.alpha_v = d.alpha_u;
        if ((rc = set_tex(d.alpha_tex, 1.0f, b.alpha_tex, err))) return rc;
        b.nonlinear = d.use_fast_approx ? 1 : 0;
        b.flags = MTSG_F_GLOSSY_REFL | MTSG_F_FRONT;
        return MTSGPU_OK;
    }
    // phong: ensureEnergyConservation(specular, diffuse, .., 1.0f), the pair form (bsdf.cpp:115-146):
    // one scale from the component-wise maximum of the two maxima's sum, on both
    float dmx[3], sum[3];
    tex_max(d.reflectance_tex, d.diffuse_reflectance, dmx);
    for (int i = 0; i < 3; ++i) sum[i] = d.specular_reflectance[i] + dmx[i];
    const float sc = energy_scale(sum, ens);
    for (int i = 0; i < 3; ++i) {
        b.spec_r[i] = sc != 1.0f ? d.specular_reflectance[i] * sc : d.specular_reflectance[i];
        b.refl[i] = sc != 1.0f ? d.diffuse_reflectance[i] * sc : d.diffuse_reflectance[i];
    }
    if ((rc = set_tex(d.reflectance_tex, sc, b.refl_tex, err))) return rc;
    b.spec_weight = specular_weight(d, sc, b);   // phong.cpp:97-99
    b.alpha_u = b.alpha_v = d.exponent;
    b.flags = MTSG_F_GLOSSY_REFL | MTSG_F_DIFF_REFL | MTSG_F_FRONT;
    return MTSGPU_OK;
}

int configure_bsdf(const mtsgpu_bsdf_desc &d, MtsgBsdf &b, std::vector<float> &rt, std::string &err) {
    std::memset(&b, 0, sizeof b);
    b.type = d.type;
    b.nested[0] = b.nested[1] = -1;
    if (d.type == MTSGPU_BSDF_TWOSIDED) return MTSGPU_OK;   // resolved by configure_twosided
    if (d.type == MTSGPU_BSDF_MIXTURE || d.type == MTSGPU_BSDF_BLEND || d.type == MTSGPU_BSDF_MASK)
        return MTSGPU_OK;                                   // resolved by configure_combo / configure_mask
    if (d.type >= MTSGPU_BSDF_DIFFTRANS && d.type <= MTSGPU_BSDF_PHONG) return configure_leaf2(d, b, err);
    if (d.type == MTSGPU_BSDF_CONDUCTOR || d.type == MTSGPU_BSDF_DIELECTRIC || d.type == MTSGPU_BSDF_PLASTIC)
        return configure_smooth(d, b, err);
    if (d.type == MTSGPU_BSDF_DIFFUSE) {
        float mx[3];
        tex_max(d.reflectance_tex, d.reflectance, mx);
        float sc = energy_scale(mx, d.ensure_energy_conservation);
        for (int i = 0; i < 3; ++i) b.refl[i] = sc != 1.0f ? d.reflectance[i] * sc : d.reflectance[i];
        int rc = set_tex(d.reflectance_tex, sc, b.refl_tex, err);
        if (rc) return rc;
        float m2[3];
        tex_max(d.reflectance_tex, b.refl, m2);
        if (d.reflectance_tex.type) for (int i = 0; i < 3; ++i) m2[i] = fmax_std(b.refl_tex.c0[i], b.refl_tex.c1[i]);
        float mxs = fmax_std(fmax_std(m2[0], m2[1]), m2[2]);
        b.flags = mxs > 0 ? (MTSG_F_DIFF_REFL | MTSG_F_FRONT) : 0;
        return MTSGPU_OK;
    }
    if (d.type == MTSGPU_BSDF_ROUGHPLASTIC) return configure_roughplastic(d, b, rt, err);
    if (d.type != MTSGPU_BSDF_ROUGHCONDUCTOR && d.type != MTSGPU_BSDF_ROUGHDIELECTRIC) {
        err = "unsupported BSDF type"; return MTSGPU_EINVAL;
    }
    if (d.alpha_tex.type != MTSGPU_TEX_NONE) {
        int rc = set_tex(d.alpha_tex, 1.0f, b.alpha_tex, err);
        if (rc) return rc;
    }
    if (d.distribution < 0 || d.distribution > 2) {
        err = "Specified an invalid distribution, must be \"beckmann\", \"ggx\", or \"phong\"/\"as\"!";
        return MTSGPU_EINVAL;
    }
    b.distr = d.distribution;
    b.sample_visible = d.distribution == MTSGPU_DISTR_PHONG ? 0 : d.sample_visible;
    const float au = fmax_std(d.alpha_u, 1e-4f), av = fmax_std(d.alpha_v, 1e-4f);
    b.alpha_u = avg3(au);
    b.alpha_v = avg3(av);
    float sc = energy_scale(d.specular_reflectance, d.ensure_energy_conservation);
    for (int i = 0; i < 3; ++i) b.spec_r[i] = sc != 1.0f ? d.specular_reflectance[i] * sc : d.specular_reflectance[i];
    if (d.type == MTSGPU_BSDF_ROUGHCONDUCTOR) {
        const float r = 1.0f / d.ext_eta;
        for (int i = 0; i < 3; ++i) { b.eta3[i] = d.eta[i] * r; b.k3[i] = d.k[i] * r; }
        b.flags = MTSG_F_GLOSSY_REFL | MTSG_F_FRONT;
    } else {
        if (d.int_ior < 0 || d.ext_ior < 0 || d.int_ior == d.ext_ior) {
            err = "The interior and exterior indices of refraction must be positive and differ!";
            return MTSGPU_EINVAL;
        }
        b.eta = d.int_ior / d.ext_ior;
        b.inv_eta = 1 / b.eta;
        float st = energy_scale(d.specular_transmittance, d.ensure_energy_conservation);
        for (int i = 0; i < 3; ++i) b.spec_t[i] = st != 1.0f ? d.specular_transmittance[i] * st : d.specular_transmittance[i];
        b.flags = MTSG_F_GLOSSY_REFL | MTSG_F_GLOSSY_TRANS | MTSG_F_FRONT | MTSG_F_BACK;
    }
    return MTSGPU_OK;
}

// TwoSidedBRDF::configure (twosided.cpp:82-103): nested[1] defaults to
// nested[0]; components = front ones | back ones; no transmission allowed
int configure_twosided(const mtsgpu_bsdf_desc &d, int nb, const std::vector<MtsgBsdf> &bsdfs, MtsgBsdf &b,
                       std::string &err) {
    if (d.nested[0] < 0 || d.nested[0] >= nb) { err = "A nested one-sided material is required!"; return MTSGPU_EINVAL; }
    const int n1 = d.nested[1] < 0 ? d.nested[0] : d.nested[1];
    if (n1 >= nb) { err = "twosided: nested BSDF index out of range"; return MTSGPU_EINVAL; }
    const int n[2] = {d.nested[0], n1};
    uint32_t flags = 0;
    for (int k = 0; k < 2; ++k) {
        const MtsgBsdf &c = bsdfs[n[k]];
        if (c.type == MTSGPU_BSDF_TWOSIDED) { err = "twosided: nesting a twosided BSDF is not supported"; return MTSGPU_EINVAL; }
        if (c.type == MTSGPU_BSDF_MASK) { err = "twosided: nesting a mask BSDF is not supported (mask wraps the chain)"; return MTSGPU_EINVAL; }
        const uint32_t lobes = (uint32_t)c.flags & ~(uint32_t)(MTSG_F_FRONT | MTSG_F_BACK);
        if (lobes) flags |= lobes | (k == 0 ? MTSG_F_FRONT : MTSG_F_BACK);
    }
    if (flags & MTSG_F_TRANSMISSION) { err = "Only materials without a transmission component can be nested!"; return MTSGPU_EINVAL; }
    b.flags = (int32_t)flags;
    b.nested[0] = n[0];
    b.nested[1] = n[1];
    return MTSGPU_OK;
}

const char *plugin_name(int type) {
    static const char *names[] = {"diffuse", "roughconductor", "roughdielectric", "roughplastic", "conductor", "dielectric",
                                  "plastic", "twosided", "mixturebsdf", "blendbsdf", "mask", "?",
                                  "difftrans", "roughdiffuse", "phong"};
    return type >= 0 && type <= MTSGPU_BSDF_PHONG ? names[type] : "?";
}

int refuse(std::string &err, const char *plugin, const std::string &what) {
    err = std::string(plugin) + ": " + what;
    return MTSGPU_EINVAL;
}

// MixtureBSDF::configure (mixturebsdf.cpp:115-172) and BlendBSDF's constructor and configure
// (blendbsdf.cpp:60-75, 101-133) into the side table; the record's flags are its children's.
// The device walks one chain (dcombo.h): children are leaves, none a roughdielectric (its
// sample() draws a 1D number inside the chosen branch only), at most one with a delta lobe
int configure_combo(const mtsgpu_bsdf_desc &d, int nb, const std::vector<MtsgBsdf> &bsdfs, MtsgBsdf &b,
                    std::vector<MtsgCombo> &combos, std::string &err) {
    const char *me = plugin_name(d.type);
    MtsgCombo c;
    std::memset(&c, 0, sizeof c);
    c.type = d.type;
    int rc;
    if (d.type == MTSGPU_BSDF_MIXTURE) {
        if (d.num_children < 0 || d.num_children > MTSGPU_MIXTURE_MAX || d.num_weights > MTSGPU_MIXTURE_MAX)
            return refuse(err, me, "more than 8 nested BSDFs are not supported");
        if (d.num_weights <= 0) return refuse(err, me, "No weights were supplied!");
        if (d.num_children != d.num_weights)
            return refuse(err, me, "BSDF count mismatch: " + std::to_string(d.num_children) + " bsdfs, but specified " +
                                       std::to_string(d.num_weights) + " weights");
        c.n = d.num_children;
        float totalWeight = 0;
        for (int i = 0; i < c.n; ++i) {
            if (d.weights[i] < 0) return refuse(err, me, "Invalid BSDF weight!");
            totalWeight += d.weights[i];
        }
        if (totalWeight <= 0) return refuse(err, me, "The weights must sum to a value greater than zero!");
        for (int i = 0; i < c.n; ++i) c.w[i] = d.weights[i];
        if (d.ensure_energy_conservation && totalWeight > 1) {
            const float scale = 1.0f / totalWeight;
            for (int i = 0; i < c.n; ++i) c.w[i] *= scale;
        }
        // m_pdf: DiscreteDistribution::append per child, then normalize() (pmf.h:52-58, 101-114)
        c.cdf[0] = 0.0f;
        for (int i = 0; i < c.n; ++i) c.cdf[i + 1] = c.cdf[i] + c.w[i];
        const float sum = c.cdf[c.n];
        if (sum > 0) {
            const float normalization = 1.0f / sum;
            for (int i = 1; i <= c.n; ++i) c.cdf[i] *= normalization;
            c.cdf[c.n] = 1.0f;
        }
        for (int i = 0; i < c.n; ++i) c.child[i] = d.children[i];
    } else {
        if (d.nested[0] < 0 || d.nested[1] < 0)
            return refuse(err, me, "BSDF count mismatch: expected two nested BSDF instances!");
        c.n = 2;
        c.child[0] = d.nested[0];
        c.child[1] = d.nested[1];
        c.value[0] = c.value[1] = c.value[2] = d.weight;
        if ((rc = set_tex(d.weight_tex, 1.0f, c.tex, err))) return rc;
    }
    uint32_t flags = 0;
    int deltas = 0;
    for (int i = 0; i < c.n; ++i) {
        if (c.child[i] < 0 || c.child[i] >= nb) return refuse(err, me, "nested BSDF index out of range");
        const MtsgBsdf &cb = bsdfs[c.child[i]];
        if (cb.type >= MTSGPU_BSDF_TWOSIDED && cb.type <= MTSGPU_BSDF_MASK)
            return refuse(err, me, std::string("nesting a '") + plugin_name(cb.type) +
                                       "' BSDF is not supported (the chain is [mask] -> [twosided] -> [mixturebsdf | "
                                       "blendbsdf] -> leaf)");
        // (difftrans: a child on both sides of the surface is not walked by dcombo.h)
        if (cb.type == MTSGPU_BSDF_ROUGHDIELECTRIC || cb.type == MTSGPU_BSDF_DIFFTRANS)
            return refuse(err, me, std::string("a nested '") + plugin_name(cb.type) + "' BSDF is not supported");
        if (cb.flags & (MTSG_F_DELTA_REFL | MTSG_F_DELTA_TRANS)) ++deltas;
        flags |= (uint32_t)cb.flags;
    }
    if (deltas > 1)
        return refuse(err, me, "more than one nested BSDF with a delta lobe (conductor, plastic, dielectric) is not supported");
    // (BlendBSDF::configure pushes the children's types as they are, blendbsdf.cpp:119-131: a
    //  textured weight adds no ESpatiallyVarying there, unlike Mask's opacity)
    b.flags = (int32_t)flags;
    b.nested[0] = (int32_t)combos.size();
    combos.push_back(c);
    return MTSGPU_OK;
}

// Mask's constructor and configure (mask.cpp:74-111): the nested BSDF's lobes plus the null
// lobe, on both sides; opacity through ensureEnergyConservation(opacity, "opacity", 1.0f)
int configure_mask(const mtsgpu_bsdf_desc &d, int nb, const std::vector<MtsgBsdf> &bsdfs, MtsgBsdf &b,
                   std::vector<MtsgCombo> &combos, std::string &err) {
    if (d.nested[0] < 0) return refuse(err, "mask", "A child BSDF is required");
    if (d.nested[0] >= nb) return refuse(err, "mask", "nested BSDF index out of range");
    const MtsgBsdf &cb = bsdfs[d.nested[0]];
    if (cb.type == MTSGPU_BSDF_MASK) return refuse(err, "mask", "nesting a 'mask' BSDF is not supported");
    bool rd = cb.type == MTSGPU_BSDF_ROUGHDIELECTRIC;
    if (cb.type == MTSGPU_BSDF_TWOSIDED)   // (a mixture's or blend's children were checked where it was configured)
        for (int k = 0; k < 2; ++k) rd |= bsdfs[cb.nested[k]].type == MTSGPU_BSDF_ROUGHDIELECTRIC;
    if (rd) return refuse(err, "mask", "a nested 'roughdielectric' BSDF is not supported");
    if (cb.type == MTSGPU_BSDF_DIFFTRANS)
        return refuse(err, "mask", std::string("a nested '") + plugin_name(cb.type) + "' BSDF is not supported");
    MtsgCombo c;
    std::memset(&c, 0, sizeof c);
    c.type = d.type;
    c.n = 1;
    c.child[0] = d.nested[0];
    float mx[3];
    tex_max(d.opacity_tex, d.opacity, mx);
    const float sc = energy_scale(mx, d.ensure_energy_conservation);
    for (int i = 0; i < 3; ++i) c.value[i] = sc != 1.0f ? d.opacity[i] * sc : d.opacity[i];
    int rc;
    if ((rc = set_tex(d.opacity_tex, sc, c.tex, err))) return rc;
    // extraFlags = ESpatiallyVarying on every component when the opacity is not constant (mask.cpp:98-106)
    b.flags = cb.flags | MTSG_F_NULL | MTSG_F_FRONT | MTSG_F_BACK | (c.tex.type ? MTSG_F_SPATIALLY_VARYING : 0);
    b.nested[0] = (int32_t)combos.size();
    combos.push_back(c);
    return MTSGPU_OK;
}

}  // namespace

// The scene's BSDF records, the two default BSDFs behind them (records nb and nb + 1), and
// whether the scene runs the MTSG_FEAT_EXT kernels
int configure_bsdfs(const mtsgpu_scene_desc &D, HostScene &S, std::string &err) {
    const uint32_t nb = D.num_bsdfs;
    int rc;
    S.bsdfs.resize(nb + 2);
    for (uint32_t i = 0; i < nb; ++i)
        if ((rc = configure_bsdf(D.bsdfs[i], S.bsdfs[i], S.rtrans, err))) return rc;
    // the wrappers inside out: mixture / blend over leaves, twosided over those, mask over all
    for (uint32_t i = 0; i < nb; ++i)
        if ((D.bsdfs[i].type == MTSGPU_BSDF_MIXTURE || D.bsdfs[i].type == MTSGPU_BSDF_BLEND) &&
            (rc = configure_combo(D.bsdfs[i], (int)nb, S.bsdfs, S.bsdfs[i], S.combos, err)))
            return rc;
    for (uint32_t i = 0; i < nb; ++i)
        if (D.bsdfs[i].type == MTSGPU_BSDF_TWOSIDED &&
            (rc = configure_twosided(D.bsdfs[i], (int)nb, S.bsdfs, S.bsdfs[i], err)))
            return rc;
    for (uint32_t i = 0; i < nb; ++i)
        if (D.bsdfs[i].type == MTSGPU_BSDF_MASK &&
            (rc = configure_mask(D.bsdfs[i], (int)nb, S.bsdfs, S.bsdfs[i], S.combos, err)))
            return rc;
    for (uint32_t i = 0; i < nb; ++i) {
        const MtsgBsdf &b = S.bsdfs[i];
        if (b.type >= MTSGPU_BSDF_ROUGHPLASTIC || b.refl_tex.type || b.alpha_tex.type) S.ext = true;
        if (b.type >= MTSGPU_BSDF_DIFFTRANS) S.leaf2 = true;
    }
    for (uint32_t i = 0; i < D.num_meshes; ++i)   // analytic shapes run the EXT | ANA variant
        if (D.meshes[i].shape_type != MTSGPU_SHAPE_TRIMESH) S.ext = true;
    // Shape::configure defaults (shape.cpp:48-70): black for emitters, 0.5 otherwise
    mtsgpu_bsdf_desc dd; std::memset(&dd, 0, sizeof dd);
    dd.type = MTSGPU_BSDF_DIFFUSE; dd.ensure_energy_conservation = 1;
    configure_bsdf(dd, S.bsdfs[nb], S.rtrans, err);
    dd.reflectance[0] = dd.reflectance[1] = dd.reflectance[2] = 0.5f;
    configure_bsdf(dd, S.bsdfs[nb + 1], S.rtrans, err);
    return MTSGPU_OK;
}

}  // namespace mtsg_host
