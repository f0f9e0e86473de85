// configure_emitter.cpp -- the emitter plugins' constructors and configure():
//   envmap        emitters/envmap.cpp:105-345, render/mipmap.h:155-301, core/rfilter.h:107-280
//   constant      emitters/constant.cpp:44-96
//   point, spot, directional   emitters/point.cpp, spot.cpp:68-94, directional.cpp:61-94
//   emitter PDF   Scene::initialize (librender/scene.cpp:376-381)
//   scene bounds  gkdtree.h:996-1001,1211-1217 (MTS_KD_AABB_EPSILON)
#include <cstdlib>

#include "scene_build_impl.h"

namespace mtsg_host {
namespace {

// LanczosSincFilter::eval with lobes = 2 (rfilters/lanczos.cpp:43-55)
float lanczos2(float x) {
    x = std::fabs(x);
    if (x < 1e-4f) return 1.0f;
    if (x > 2.0f) return 0.0f;
    const float x1 = kPi * x;   // M_PI is M_PI_FLT in the SINGLE_PRECISION build (constants.h:80-83)
    const float x2 = x1 / 2.0f;
    return (std::sin(x1) * std::sin(x2)) / (x1 * x2);
}

// Resampler<float> in resampling mode (core/rfilter.h:107-198) +
// resampleAndClamp(min 0, max inf) (rfilter.h:232-280); repeat or clamp boundary
struct Resampler1D {
    int src, dst, taps;
    bool repeat;
    std::vector<int> start;
    std::vector<float> w;
    Resampler1D(int sourceRes, int targetRes, bool rep) : src(sourceRes), dst(targetRes), repeat(rep) {
        float filterRadius = 2.0f, scale = 1.0f, invScale = 1.0f;
        if (targetRes < sourceRes) {
            scale = (float)sourceRes / (float)targetRes;
            invScale = 1 / scale;
            filterRadius *= scale;
        }
        taps = (int)std::ceil(filterRadius * 2);
        start.resize(targetRes);
        w.resize((size_t)taps * targetRes);
        for (int i = 0; i < targetRes; i++) {
            const float center = ((float)i + 0.5f) / (float)targetRes * (float)sourceRes;
            start[i] = (int)std::floor(center - filterRadius + 0.5f);
            float sum = 0;
            for (int j = 0; j < taps; j++) {
                const float pos = (float)(start[i] + j) + 0.5f - center;
                const float weight = lanczos2(pos * invScale);
                w[(size_t)i * taps + j] = weight;
                sum += weight;
            }
            const float normalization = 1.0f / sum;
            for (int j = 0; j < taps; j++) w[(size_t)i * taps + j] = w[(size_t)i * taps + j] * normalization;
        }
    }
    // source/target: `channels` interleaved floats per sample, sample stride in samples
    void run(const float *source, size_t sstride, float *target, size_t tstride, int channels) const {
        for (int i = 0; i < dst; ++i) {
            for (int ch = 0; ch < channels; ++ch) {
                float result = 0;
                for (int j = 0; j < taps; ++j) {
                    int pos = start[i] + j;
                    if (pos < 0 || pos >= src) {
                        if (repeat) { pos %= src; if (pos < 0) pos += src; }
                        else pos = std::min(std::max(pos, 0), src - 1);
                    }
                    result += source[sstride * channels * (size_t)pos + ch] * w[(size_t)i * taps + j];
                }
                const float lo = (0.0f < result) ? result : 0.0f;              // std::max(min, result)
                target[tstride * channels * (size_t)i + ch] = (lo < INFINITY) ? lo : INFINITY;
            }
        }
    }
};

// Bitmap::resample with the MIP map's lanczos-2 filter, ERepeat (u) / EClamp (v)
// (libcore/bitmap.cpp:2230-2329): an x pass then a y pass, each only if the size changes
std::vector<float> resample_level(const std::vector<float> &src, int w, int h, int nw, int nh) {
    std::vector<float> cur = src;
    if (w != nw) {
        Resampler1D r(w, nw, true);
        std::vector<float> tmp((size_t)nw * h * 3);
        for (int y = 0; y < h; ++y) r.run(cur.data() + (size_t)y * w * 3, 1, tmp.data() + (size_t)y * nw * 3, 1, 3);
        cur.swap(tmp);
    }
    if (h != nh) {
        Resampler1D r(h, nh, false);
        std::vector<float> tmp((size_t)nw * nh * 3);
        for (int x = 0; x < nw; ++x) r.run(cur.data() + (size_t)x * 3, nw, tmp.data() + (size_t)x * 3, nw, 3);
        cur.swap(tmp);
    }
    return cur;
}

// Guide tables for the envmap's two CDF searches (the cutpoint method): with
// G = 2^bits buckets, guide[k] = lower_bound(cdf, k / G).  For u in [k/G,
// (k+1)/G) the reference's std::lower_bound(cdf, u) (envmap.cpp:687-692) lies
// in [guide[k], guide[k+1]] because the CDF is non-decreasing, so the device
// searches that range only and lands on the same index.  A CDF that is not
// non-decreasing (negative or NaN texels) keeps the full-range search: its
// lower_bound depends on the search path.
uint32_t guide_bits(uint32_t size) {
    uint32_t b = 0;
    while ((1u << b) < size && b < 12) ++b;
    return b;
}
void build_guide(const float *cdf, uint32_t size, uint32_t bits, uint16_t *g) {
    const uint32_t G = 1u << bits;
    bool mono = true;
    for (uint32_t i = 0; i < size; ++i) mono &= cdf[i] <= cdf[i + 1];
    for (uint32_t k = 0; k <= G; ++k) {
        if (!mono) { g[k] = (uint16_t)(k == 0 ? 0 : size + 1); continue; }
        const float u = (float)k * (1.0f / (float)G);   // exact: G is a power of two
        g[k] = (uint16_t)(std::lower_bound(cdf, cdf + size + 1, u) - cdf);
    }
}
void build_env_guides(HostScene &S, int W, int H) {
    S.env_guide_rows.clear();
    S.env_guide_cols.clear();
    MtsgEnv &E = S.env;
    E.guide_rbits = E.guide_cbits = 0;
    if (W + 1 > 65535 || H + 1 > 65535 || std::getenv("MTSGPU_NO_ENV_GUIDE")) return;
    E.guide_rbits = guide_bits((uint32_t)H);
    E.guide_cbits = guide_bits((uint32_t)W);
    const uint32_t gr = (1u << E.guide_rbits) + 1, gc = (1u << E.guide_cbits) + 1;
    S.env_guide_rows.assign(gr, 0);
    S.env_guide_cols.assign((size_t)gc * H, 0);
    build_guide(S.env_cdf_rows.data(), (uint32_t)H, E.guide_rbits, S.env_guide_rows.data());
    for (int y = 0; y < H; ++y)
        build_guide(S.env_cdf_cols.data() + (size_t)y * (W + 1), (uint32_t)W, E.guide_cbits,
                    S.env_guide_cols.data() + (size_t)y * gc);
}

// EnvironmentMap ctor (envmap.cpp:105-185: TMIPMap with EEWA, anisotropy 10,
// mipmap.h:155-301) and configure() (envmap.cpp:261-321)
int build_envmap(const mtsgpu_emitter_desc &e, int index, HostScene &S, std::string &err) {
    const int W = (int)e.env_width, H = (int)e.env_height;
    if (!e.env_rgb || W <= 0 || H <= 0) { err = "envmap: missing image data"; return MTSGPU_EINVAL; }
    if (std::max(W, H) > 0xFFFF) {
        err = "Environment maps images must be smaller than 65536  pixels in width and height";
        return MTSGPU_EINVAL;
    }
    MtsgEnv &E = S.env;
    std::memset(&E, 0, sizeof E);
    E.emitter = index;
    E.w0 = W; E.h0 = H;
    E.scale = e.env_scale;
    E.max_aniso = 10.0f;
    E.inv_ln2 = 1.0f / std::log(2.0f);
    // level 0: BlockedArray::init (barray.h:103-126) -> clampNegative if min < 0 (mipmap.h:226-236)
    std::vector<float> cur(e.env_rgb, e.env_rgb + (size_t)W * H * 3);
    bool negative = false;
    for (float x : cur) negative |= x < 0;
    if (negative)
        for (float &x : cur) x = (0.0f < x) ? x : 0.0f;
    S.env_texels.clear();
    auto quantize = [&](const std::vector<float> &lv, int w, int h, int level) {
        E.lw[level] = w; E.lh[level] = h;
        E.loff[level] = (uint32_t)(S.env_texels.size() / 4);
        E.ratio_x[level] = (float)w / (float)W;
        E.ratio_y[level] = (float)h / (float)H;
        for (size_t t = 0; t < (size_t)w * h; ++t) {
            S.env_texels.push_back(float_to_half(lv[3 * t]));
            S.env_texels.push_back(float_to_half(lv[3 * t + 1]));
            S.env_texels.push_back(float_to_half(lv[3 * t + 2]));
            S.env_texels.push_back(0);
        }
    };
    quantize(cur, W, H, 0);
    int levels = 1, w = W, h = H;
    while (w > 1 || h > 1) {   // mipmap.h:241-263
        const int nw = std::max(1, (w + 1) / 2), nh = std::max(1, (h + 1) / 2);
        cur = resample_level(cur, w, h, nw, nh);
        if (levels >= MTSG_ENV_MAX_LEVELS) { err = "envmap: too many MIP levels"; return MTSGPU_EINVAL; }
        quantize(cur, nw, nh, levels);
        ++levels;
        w = nw; h = nh;
    }
    E.levels = levels;
    for (int i = 0; i < MTSG_EWA_LUT; ++i) {   // mipmap.h:296-301
        const float r2 = (float)i / (float)(MTSG_EWA_LUT - 1);
        E.lut[i] = (float)std::exp((double)(-2.0f * r2)) - (float)std::exp((double)-2.0f);
    }
    // sampling CDFs over sin(theta)-weighted luminance of level 0
    S.env_cdf_cols.assign((size_t)(W + 1) * H, 0.0f);
    S.env_cdf_rows.assign((size_t)H + 1, 0.0f);
    S.env_row_weights.assign((size_t)H, 0.0f);
    size_t colPos = 0, rowPos = 0;
    float rowSum = 0.0f;
    S.env_cdf_rows[rowPos++] = 0;
    for (int y = 0; y < H; ++y) {
        float colSum = 0;
        S.env_cdf_cols[colPos++] = 0;
        for (int x = 0; x < W; ++x) {
            const uint16_t *t = &S.env_texels[((size_t)y * W + x) * 4];
            const float c[3] = {half_to_float(t[0]), half_to_float(t[1]), half_to_float(t[2])};
            colSum += luminance(c);
            S.env_cdf_cols[colPos++] = colSum;
        }
        const float normalization = 1.0f / colSum;
        for (int x = 1; x < W; ++x) S.env_cdf_cols[colPos - x - 1] *= normalization;
        S.env_cdf_cols[colPos - 1] = 1.0f;
        const float weight = std::sin(((float)y + 0.5f) * kPi / (float)H);
        S.env_row_weights[y] = weight;
        rowSum += colSum * weight;
        S.env_cdf_rows[rowPos++] = rowSum;
    }
    const float normalization = 1.0f / rowSum;
    for (int y = 1; y < H; ++y) S.env_cdf_rows[rowPos - y - 1] *= normalization;
    S.env_cdf_rows[rowPos - 1] = 1.0f;
    if (rowSum == 0) { err = "The environment map is completely black -- this is not allowed."; return MTSGPU_EINVAL; }
    if (!std::isfinite(rowSum)) {
        err = "The environment map contains an invalid floating point value (nan/inf) -- giving up.";
        return MTSGPU_EINVAL;
    }
    build_env_guides(S, W, H);
    E.normalization = 1.0f / (rowSum * (2 * kPi / (float)W) * (kPi / (float)H));
    E.pixel_x = 2 * kPi / (float)W;
    E.pixel_y = kPi / (float)H;
    // toWorld and the inverse the reference's Transform carries
    Xf T;
    if (!desc_transform(e.env_to_world, e.env_to_world_inv, T)) { err = "envmap: singular 'toWorld'"; return MTSGPU_EINVAL; }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) { E.to_world[3 * r + c] = T.t.m[r][c]; E.to_local[3 * r + c] = T.inv.m[r][c]; }
    return MTSGPU_OK;
}

// EnvironmentMap::createShape (envmap.cpp:331-345) as called by
// Scene::initializeBidirectional (scene.cpp:385-413): bounding sphere of the
// kd-tree bounds grown by the sensor position, radius x1.5
void envmap_bsphere(HostScene &S, const mtsgpu_sensor_desc &sensor) {
    M4 C;
    for (int i = 0; i < 16; ++i) C.m[i / 4][i % 4] = sensor.to_world[i];
    float mn[3], mx[3];
    for (int a = 0; a < 3; ++a) { mn[a] = S.aabb_min[a]; mx[a] = S.aabb_max[a]; }
    auto grow = [&](V q) {
        const float p[3] = {q.x, q.y, q.z};
        for (int a = 0; a < 3; ++a) {
            mn[a] = fmin_std(mn[a], p[a]);
            mx[a] = fmax_std(mx[a], p[a]);
        }
    };
    if (S.cam_lens.type == MTSGPU_SENSOR_PERSPECTIVE) {
        grow(xf_point(C, v(0.0f, 0.0f, 0.0f)));   // AnimatedTransform::getTranslationBounds (track.cpp:79-83)
    } else {
        // the sensor's own getAABB(): the aperture's box (thinlens.cpp:516-520) or the film rectangle
        // sampleToCamera((0,0,0)) .. sampleToCamera((1,1,0)) (orthographic.cpp:296-302,
        // telecentric.cpp:437-443), its 8 corners through toWorld (getSpatialBounds, track.cpp:123-129)
        float lo[3], hi[3];
        if (S.cam_lens.type == MTSGPU_SENSOR_THINLENS) {
            const float r = S.cam_lens.aperture_radius;
            lo[0] = -r; lo[1] = -r; lo[2] = 0.0f; hi[0] = r; hi[1] = r; hi[2] = 0.0f;
        } else {
            M4 s2c;
            for (int i = 0; i < 16; ++i) s2c.m[i / 4][i % 4] = S.cam.sample_to_camera[i];
            const V a = xf_point(s2c, v(0.0f, 0.0f, 0.0f)), b = xf_point(s2c, v(1.0f, 1.0f, 0.0f));
            lo[0] = fmin_std(a.x, b.x); lo[1] = fmin_std(a.y, b.y); lo[2] = fmin_std(a.z, b.z);
            hi[0] = fmax_std(a.x, b.x); hi[1] = fmax_std(a.y, b.y); hi[2] = fmax_std(a.z, b.z);
        }
        for (int j = 0; j < 8; ++j)   // AABB::getCorner: bit 0 -> x, bit 1 -> y, bit 2 -> z
            grow(xf_point(C, v((j & 1) ? hi[0] : lo[0], (j & 2) ? hi[1] : lo[1], (j & 4) ? hi[2] : lo[2])));
    }
    const V center = v((mx[0] + mn[0]) * 0.5f, (mx[1] + mn[1]) * 0.5f, (mx[2] + mn[2]) * 0.5f);
    const float radius = length(center - v(mx[0], mx[1], mx[2]));
    S.env.center[0] = center.x; S.env.center[1] = center.y; S.env.center[2] = center.z;
    S.env.radius = fmax_std(1e-4f, radius * 1.5f);
}

// ---- delta emitters (emitters/point.cpp, spot.cpp, directional.cpp) ----------
// what the constructors and configure() derive from the emitter's transform; the
// directional emitter's disk waits for the scene bounds (directional_bsphere)
int configure_delta(const mtsgpu_emitter_desc &e, MtsgDelta &o, std::string &err) {
    std::memset(&o, 0, sizeof o);
    Xf X;
    if (!desc_transform(e.env_to_world, e.env_to_world_inv, X)) { err = "Singular matrix in Matrix::invert"; return MTSGPU_EINVAL; }
    const M4 &T = X.t, &Ti = X.inv;
    if (e.type == MTSGPU_EMITTER_DIRECTIONAL) {
        if (has_scale(e.env_to_world)) {   // directional.cpp:69-71
            err = "Scale factors in the emitter-to-world transformation are not allowed!";
            return MTSGPU_EINVAL;
        }
        const V d = xf_vec(T, v(0.0f, 0.0f, 1.0f));
        o.dir[0] = d.x; o.dir[1] = d.y; o.dir[2] = d.z;
        return MTSGPU_OK;
    }
    // trafo.transformAffine(Point(0)) (transform.h:109-121)
    const V p = v(T.m[0][0] * 0.0f + T.m[0][1] * 0.0f + T.m[0][2] * 0.0f + T.m[0][3],
                  T.m[1][0] * 0.0f + T.m[1][1] * 0.0f + T.m[1][2] * 0.0f + T.m[1][3],
                  T.m[2][0] * 0.0f + T.m[2][1] * 0.0f + T.m[2][2] * 0.0f + T.m[2][3]);
    o.pos[0] = p.x; o.pos[1] = p.y; o.pos[2] = p.z;
    if (e.type == MTSGPU_EMITTER_SPOT) {
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) o.to_local[3 * r + c] = Ti.m[r][c];
        // SpotEmitter(props), configure() (spot.cpp:68-94): float cosf
        const float beam = deg2rad(e.beam_width), cutoff = deg2rad(e.cutoff_angle);
        if (!(cutoff >= beam)) { err = "Assertion 'm_cutoffAngle >= m_beamWidth' failed"; return MTSGPU_EINVAL; }
        o.cos_beam = std::cos(beam);
        o.cos_cutoff = std::cos(cutoff);
        o.cutoff = cutoff;
        o.inv_transition = 1.0f / (cutoff - beam);
    }
    return MTSGPU_OK;
}

// DirectionalEmitter::createShape (directional.cpp:88-94): the kd-tree AABB's bounding
// sphere (aabb.cpp:44-47), radius x 1.1; the disk centre of sampleDirect (:162)
void directional_bsphere(const HostScene &S, MtsgDelta &o) {
    const V mx = v(S.aabb_max[0], S.aabb_max[1], S.aabb_max[2]), mn = v(S.aabb_min[0], S.aabb_min[1], S.aabb_min[2]);
    const V center = (mx + mn) * 0.5f;
    float radius = length(center - mx);
    radius *= 1.1f;
    const V d = v(o.dir[0], o.dir[1], o.dir[2]);
    const V disk = center - d * radius;
    o.pos[0] = disk.x; o.pos[1] = disk.y; o.pos[2] = disk.z;
    o.radius = radius;
}

}  // namespace

// One record per emitter, by type: the environment's tables, the delta emitters' records;
// an area emitter waits for its shape (configure_shapes)
int configure_emitters(const mtsgpu_scene_desc &D, HostScene &S, std::string &err) {
    if (D.num_emitters == 0) { err = "scene has no emitters (the sunsky fallback is out of scope)"; return MTSGPU_EINVAL; }
    int rc;
    S.emitters.resize(D.num_emitters);
    for (uint32_t i = 0; i < D.num_emitters; ++i) {
        const mtsgpu_emitter_desc &e = D.emitters[i];
        MtsgEmitter &o = S.emitters[i];
        std::memset(&o, 0, sizeof o);
        o.type = e.type;
        o.shape = -1;
        o.weight = e.sampling_weight;
        for (int k = 0; k < 3; ++k) o.radiance[k] = e.radiance[k];
        if (e.type == MTSGPU_EMITTER_ENVMAP || e.type == MTSGPU_EMITTER_CONSTANT) {
            if (S.env.emitter >= 0) {   // scene.cpp:510-513
                err = "Only one environment emitter can be specified per scene.";
                return MTSGPU_EINVAL;
            }
            if (e.type == MTSGPU_EMITTER_ENVMAP) {
                if ((rc = build_envmap(e, (int)i, S, err))) return rc;
            } else {
                // ConstantBackgroundEmitter (constant.cpp:44-96): a uniform environment on the
                // scene's bounding sphere (createShape, :67-91, as envmap_bsphere)
                S.env.emitter = (int)i;
                S.env.constant = 1;
                for (int k = 0; k < 3; ++k) S.env.radiance[k] = e.radiance[k];
            }
        } else if (e.type == MTSGPU_EMITTER_POINT || e.type == MTSGPU_EMITTER_SPOT ||
                   e.type == MTSGPU_EMITTER_DIRECTIONAL) {
            o.tri_first = (uint32_t)S.deltas.size();
            MtsgDelta dl;
            if ((rc = configure_delta(e, dl, err))) return rc;
            S.deltas.push_back(dl);
        } else if (e.type != MTSGPU_EMITTER_AREA) {
            err = "unsupported emitter type";
            return MTSGPU_EINVAL;
        }
    }
    return MTSGPU_OK;
}

// emitter PDF (scene.cpp:376-381)
void emitter_cdf(HostScene &S) {
    const size_t n = S.emitters.size();
    S.em_cdf.assign(n + 1, 0.0f);
    for (size_t i = 0; i < n; ++i) S.em_cdf[i + 1] = S.em_cdf[i] + S.emitters[i].weight;
    const float sum = S.em_cdf[n];
    if (sum > 0) {
        S.em_norm = 1.0f / sum;
        for (size_t i = 1; i < n + 1; ++i) S.em_cdf[i] *= S.em_norm;
        S.em_cdf[n] = 1.0f;
    } else {
        S.em_norm = 0.0f;
    }
}

// scene bounds, slightly enlarged (gkdtree.h:1211-1217), and the bounding spheres the
// environment and the directional emitters derive from them
void scene_bounds(const mtsgpu_scene_desc &D, SceneBuild &B, HostScene &S) {
    const float eps = 1e-3f;
    for (int a = 0; a < 3; ++a) {
        B.amin[a] -= (B.amax[a] - B.amin[a]) * eps + eps;
        B.amax[a] += (B.amax[a] - B.amin[a]) * eps + eps;
        S.aabb_min[a] = B.amin[a]; S.aabb_max[a] = B.amax[a];
    }
    if (S.env.emitter >= 0) envmap_bsphere(S, D.sensor);
    for (const MtsgEmitter &e : S.emitters)
        if (e.type == MTSGPU_EMITTER_DIRECTIONAL) directional_bsphere(S, S.deltas[e.tri_first]);
}

}  // namespace mtsg_host
