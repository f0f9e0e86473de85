// dpath.h -- the device side of Mitsuba 0.6's `path` integrator shared by both
// execution engines (path_kernel.hip: the persistent megakernel, the `direct`
// integrator and batch ray queries; wf_kernel.hip: the wavefront engine):
// SamplingIntegrator::renderBlock's per-sample loop body
// (src/librender/integrator.cpp:140-188) around MIPathTracer::Li
// (src/integrators/path/path.cpp:119-294) as a per-path state machine
// (PathShader) with the emitter helpers it uses.  It is the one header the kernel
// units include for the device side; its parts by subsystem: dsampler.h (Sobol /
// independent samplers), dtraverse.h (BVH2 and kd-tree traversals), dscan.h (the
// tiny-scene scan), dhit.h (the hit record), dfilm.h (the film splat), dstage.h
// (LDS staging), dsensor.h (camera rays), dcombo.h (combinator BSDFs).
//
// Work items are (sample j, pixel p) pairs, pixels in 8x8 tiles; the megakernel
// hands them out as runs of consecutive samples of one pixel (dmega.h).
// The own-pixel splat of every sample is stored to HBM ([spp][pixels], film_slot)
// and a second kernel sums each pixel in sample order -- the reference's
// ImageBlock accumulation order, bit for bit; splats into other pixels (box
// filter edges) go to a spill film with double atomics, gaussian footprints are
// gathered per pixel in a fixed order (film_gather).  LDS holds the Sobol
// direction numbers of the first dimensions as 4-bit lookup tables (8
// independent reads per 32-bit sample instead of up to 32 dependent ones).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "danalytic.h"
#include "dbsdf.h"
#include "ddelta.h"
#include "denv.h"
#include "layout.h"
#include "sfmt.h"

#define BLOCK MTSG_BLOCK   // layout.h: the host sizes grids, LDS and the wavefront queues by it

#include "dsampler.h"
#include "dtraverse.h"
#include "dscan.h"
#include "dhit.h"
#include "dfilm.h"
#include "dstage.h"

// ---------------------------------------------------------------------------
// per-lane path state
// ---------------------------------------------------------------------------
enum { ST_NEWSAMPLE = 0, ST_PRIMARY = 1, ST_SHADOW = 2, ST_EXT = 3, ST_DONE = 4 };

// DiscreteDistribution::sample/sampleReuse (core/pmf.h:124-169)
__device__ __forceinline__ uint32_t dd_sample_reuse(const float *__restrict__ cdf, uint32_t n, float &value,
                                                   float *pdf) {
    uint32_t lo = 0, hi = n + 1;                          // std::lower_bound
    while (lo < hi) {
        uint32_t mid = (lo + hi) >> 1;
        if (cdf[mid] < value) lo = mid + 1; else hi = mid;
    }
    int idx = (int)lo - 1;
    if (idx < 0) idx = 0;
    uint32_t index = (uint32_t)idx;
    if (index > n - 1) index = n - 1;
    while (cdf[index + 1] - cdf[index] == 0 && index < n - 1) ++index;
    const float c0 = cdf[index], c1 = cdf[index + 1];
    if (pdf) *pdf = c1 - c0;
    value = (value - c0) / (c1 - c0);
    return index;
}

// ---------------------------------------------------------------------------
// the persistent path kernel
// ---------------------------------------------------------------------------
// whether the BSDF sample that spawned the current ray chose a delta lobe
// (BSDFSamplingRecord::sampledType & EDelta, path.cpp:262,280): one bit
#define PV_DELTA(P) ((P).delta != 0)
#define PV_SET_DELTA(P, t) ((P).delta = ((t) & MTSG_F_DELTA) != 0)
struct PathVars {
    f3 L, thr;
    float eta;
    int depth;
    // flags as bits of one word (bools each took a lane-mask SGPR pair across the loop);
    // alpha is the sample's film alpha, 0 or 1 (path.cpp:125-131, records.inl:117-144)
    uint32_t scattered : 1, emitted : 1, delta : 1, alpha : 1;
    Hit its;          // current vertex
    f3 neeC;          // throughput*value*bsdfVal*weight, committed if the shadow ray is unoccluded
    f3 refN;          // DirectSamplingRecord::refN of the current vertex
    float bsdfPdf;
};

#include "dsensor.h"   // the sensors' primary rays and their differentials
#include "dcombo.h"    // mixturebsdf, blendbsdf, mask (the MTSG_FEAT_SET_COMBO kernels)

__device__ __forceinline__ f3 area_Le(const MtsgDeviceScene &S, const Hit &h, f3 d) {   // area.cpp:104-109
    const MtsgEmitter &e = S.emitters[S.shapes[h.shape].emitter];
    if (dot(h.sh.n, d) <= 0) return mk(0, 0, 0);
    return ld3(e.radiance);
}

// Scene::pdfEmitterDirect for a hit h on area light `emitter`, reached along d from `ref`
// (scene.cpp:949-952, area.cpp:175-181, shape.cpp:117-126 / sphere.cpp:357-387); dRec after
// setQuery (records.inl:168-176): d = ray.d, n = its.shFrame.n, dist = its.t.
// (The scene by pointer: a reference parameter is known dereferenceable, and PathShader::shade's
// load of S.em_norm then moved above the branch, where its own code had not had it)
template <bool ANA>
__device__ __forceinline__ float area_hit_pdf(const MtsgDeviceScene *Sp, int emitter, const Hit &h, f3 ref, f3 d, f3 refN) {
    const MtsgDeviceScene &S = *Sp;
    const MtsgEmitter &e = S.emitters[emitter];
    const f3 dn = h.sh.n;
    float pdf = 0.0f;
    if (dot(d, refN) >= 0 && dot(d, dn) < 0) {
        if (ANA && S.shapes[h.shape].analytic >= 0)
            pdf = ana_pdf_direct(((GAna *)S.analytic)[S.shapes[h.shape].analytic], ref, d, dn, h.t);
        else
            pdf = e.inv_area * (h.t * h.t) / absdot(d, dn);
    }
    return pdf * (e.weight * S.em_norm);
}

// ConstantBackgroundEmitter (emitters/constant.cpp): pdfDirect in solid angle
// (:216-231) and sampleDirect (:167-214) on the scene's bounding sphere
#define D_INV_FOURPI 0.07957747154594766788f
__device__ __forceinline__ float const_pdf_direct(f3 d, f3 refN) {
    if (!is_zero(refN)) return D_INV_PI * smax(0.0f, dot(d, refN));
    return D_INV_FOURPI;   // warp::squareToUniformSpherePdf
}
__device__ __noinline__ EnvSample const_sample_direct(glb_env *E, f3 ref, f3 refN, float sx, float sy) {
    EnvSample r;
    r.value = mk(0, 0, 0); r.pdf = 0.0f; r.dist = 0.0f;
    f3 d;
    float pdf;
    if (!is_zero(refN)) {
        d = square_to_cosine_hemisphere(sx, sy);
        pdf = D_INV_PI * d.z;
        Frame F;
        F.n = refN;
        coordinate_system(refN, F.s, F.t);
        d = to_world(F, d);
    } else {
        const float z = 1.0f - 2.0f * sy;   // warp::squareToUniformSphere (warp.cpp:25-31)
        const float rr = safe_sqrt(1.0f - z * z);
        float sinPhi, cosPhi;
        d_sincos(2.0f * D_PI * sx, &sinPhi, &cosPhi);
        d = mk(rr * cosPhi, rr * sinPhi, z);
        pdf = D_INV_FOURPI;
    }
    r.d = d;
    float nearT, farT;
    if (!env_bsphere(E, ref, d, nearT, farT)) return r;
    if (!(nearT < 0 && farT > 0)) return r;
    r.dist = farT;
    r.pdf = pdf;
    if (!is_zero(refN) && dot(d, refN) <= 0) return r;   // roundoff moved the sample to the backside
    r.value = divs(mk(E->radiance[0], E->radiance[1], E->radiance[2]), pdf);
    return r;
}

// (pixel_of, the compact pixel index -> image pixel rule, is shared with the host: layout.h)

#ifndef MTSG_WAVES_PER_EU
#define MTSG_WAVES_PER_EU 3
#endif

// (sobol_lookup_lds, sobol::look_up through the folded tables in LDS, is shared with the host: layout.h)

// ---------------------------------------------------------------------------
// Li() as a per-path state machine, one bounce per step.  One step traces the
// path's pending shadow ray (NEE of the previous vertex) and its closest-hit
// ray (camera or BSDF-sampled), then shades the new vertex: add the NEE
// estimate if unoccluded, the MIS-weighted emission of the hit, Russian
// roulette, then at the new vertex draw the NEE sample and the BSDF sample,
// which produce the next step's two rays.  Sampler dimensions are consumed in
// the reference's order (NEE 2D, BSDF 2D [+1D], RR 1D), and radiance is
// accumulated in the reference's order (NEE term before the BSDF-hit term).
// PathShader holds the three pieces both execution models share: start (the
// renderBlock loop body up to Li's prologue), shade (the rest of one bounce)
// and finish (block->put).  The persistent megakernel (path_kernel) runs them
// with both traversals inline; the wavefront pipeline (wf_shade / wf_trace)
// runs the traversals as separate kernels over compacted ray queues.
// ---------------------------------------------------------------------------
// (the pixel's coordinates and the sample index are not kept: pixel_of(pix)
// and smp.sampleIndex give them where needed, two and one fewer registers
// live across every bounce)
struct PathState {
    uint32_t active : 1, haveRay : 1, primary : 1, haveShadow : 1;   // one word of bits
    uint32_t pix;
    float sx, sy;
    SamplerState smp;
    PathVars P;
    // rays of the next trace step: closest (camera / extension) and shadow (NEE).
    // Both leave P.its.p (the camera position for the primary ray, set by begin()):
    // the closest-hit ray's origin is not held separately
    f3 rd, sd;
    float rmint, rmaxt, smaxt;
};

// What a path needs to begin (PathShader::produce -> load): the sample's sequence
// index (or stream key), film position, camera ray direction and 1 / dl.z (the ray's
// interval is near_clip * invZ .. far_clip * invZ, re-formed by load), its compact
// pixel and its sample of the chunk; dim: the sampler dimensions produce() consumed.
// The MTSG_FEAT_LENS kernels (dsensor.h) carry the ray's own origin and interval instead of
// invZ; no other kernel reads or writes those members
struct StartRec {
    uint64_t sobolIndex;
    float sx, sy;
    f3 rd;
    float invZ;
    uint32_t pix, jj, dim;
    f3 ro;
    float mint, maxt;
};

// The tiny-scene megakernel's start queue (dmega.h): per wave one batch of up to 64
// start records in LDS, structure-of-arrays (word w of slot s at [w * 64 + s]: a wave's
// writes and pops touch 64 consecutive words, no bank conflict).  It lies where the
// traversal stacks would (LdsView::stackBase), which a scanning launch never touches.
// -DMTSG_START_QUEUE=0 (A/B builds): the loop without it
#ifndef MTSG_START_QUEUE
#define MTSG_START_QUEUE 1
#endif
// A production pass finishes the samples whose camera ray misses the scene itself,
// instead of queueing them (dmega.h; kernels without MTSG_FEAT_ENV).
// -DMTSG_EARLY_MISS=0 (A/B builds): every real sample is queued
#ifndef MTSG_EARLY_MISS
#define MTSG_EARLY_MISS 1
#endif
#define MTSG_QUEUE_REC_WORDS 10   // sobolIndex (2), sx, sy, rd (3), invZ, pix, jj
#define MTSG_QUEUE_WORDS ((BLOCK / 64) * MTSG_QUEUE_REC_WORDS * 64)   // per block
// whether a launch of a SCENE_LDS megakernel starts its paths from the queue: scanning
// launches only (the others need the stacks' LDS), and not the SFMT replay (a lane's
// draws follow the order of its own unit)
__host__ __device__ __forceinline__ bool mtsg_start_queue(const MtsgLaunch &L) {
    return MTSG_START_QUEUE && L.scene_lds && L.scan && !L.replay && L.integrator != MTSG_INTEGRATOR_DIRECT;
}

// per-lane counts: 32-bit for the always-on ones (fewer live VGPRs in the
// persistent loop; finish() flushes them long before they could wrap),
// 64-bit for the INSTR-only traversal statistics
struct PathCounters {
    uint32_t rays, shadow, len, samples, err;
    unsigned long long nodes, tests, hits, nee, sobol;
};

// INSTR: traversal statistics + optional per-sample records (tests, roofline
// pass); SCENE_LDS: BVH + TriAccel staged in LDS; FEAT: MTSG_FEAT_ENV (scene
// has an environment emitter) | MTSG_FEAT_EXT (roughplastic, textures, smooth
// BSDFs, twosided) | MTSG_FEAT_ANA (analytic shapes)
// KIND / HITK (the wavefront engine's per-type shade kernels, wf_kernel.hip):
// the BSDF type at the vertex (BSDF_*, -1: any) and whether the step's
// closest-hit ray is known to have hit (1), known to have missed or not to
// exist (2), or unknown (0, the megakernel)
template <bool INSTR, bool SCENE_LDS, int FEAT, int KIND = -1, int HITK = 0>
struct PathShader {
    static constexpr bool STATS = INSTR;
    static constexpr bool ENV = (FEAT & MTSG_FEAT_ENV) != 0, EXT = (FEAT & MTSG_FEAT_EXT) != 0,
                          ANA = (FEAT & MTSG_FEAT_ANA) != 0, DIFF = (FEAT & MTSG_FEAT_DIFF) != 0;
    static constexpr int BSF = FEAT & BSET_BITS;   // the variant's BSDF set (dbsdf.h BSet)
    // the BSDF-set megakernels are built without strictNormals (the geometric normal
    // is then dead once the hit is formed); scenes with it run the generic kernel
    static constexpr bool NOSTRICT = (FEAT & MTSG_FEAT_NOSTRICT) != 0;
    // REFN false (MTSG_FEAT_NOREFN, render_plan.cpp): the scene's only emitter is a non-constant
    // envmap, whose sampleDirect / pdfDirect do not read refN (envmap.cpp:516-556): the area
    // light and constant-emitter code is compiled out and refN (three floats live across the
    // NEE and BSDF calls and the next traversal) is not kept
    static constexpr bool REFN = (FEAT & MTSG_FEAT_NOREFN) == 0;
    // DELTA (MTSG_FEAT_DELTA): the scene has point / spot / directional emitters (ddelta.h).  Its one
    // feature set is compiled with ENV, which such a scene need not have: have_env() asks the scene
    // there and is the constant `true` in every other kernel
    static constexpr bool DELTA = (FEAT & MTSG_FEAT_DELTA) != 0;
    // LENS (MTSG_FEAT_LENS): the sensor is thinlens, orthographic or telecentric (dsensor.h): a
    // primary ray has its own origin and interval (StartRec::ro, mint, maxt), and produce()
    // draws the aperture sample where the sensor takes one
    static constexpr bool LENS = (FEAT & MTSG_FEAT_LENS) != 0;
    // COMBO (MTSG_FEAT_COMBO): the scene holds a mixturebsdf, blendbsdf or mask (dcombo.h).  Its one
    // feature set is the lens set's, which such a scene need not need: lens_ray() asks the sensor
    // there and is the constant `true` in the lens set's own kernels
    static constexpr bool COMBO = (FEAT & MTSG_FEAT_COMBO) != 0;
    __device__ __forceinline__ bool lens_ray() const {
        if constexpr (COMBO) return L.cam_lens.type != MTSG_SENSOR_PERSPECTIVE;
        else return true;
    }
    __device__ __forceinline__ bool have_env() const {
        if constexpr (DELTA) return L.scene.env_emitter >= 0;
        else return true;
    }
    const MtsgLaunch &L;
    const HitSrc<SCENE_LDS> &hs;
    const SobolCtx &SC;
    lds_u32 *ycolTab;
    PathCounters &c;

    // the renderBlock loop body for item `it` up to Li()'s prologue
    // (integrator.cpp:165-186, path.cpp:119-133); false for a padding pixel
    __device__ __forceinline__ bool start(PathState &st, uint64_t it) const {
        const uint32_t jj = (uint32_t)(it / L.num_pixels);
        return start_jp(st, jj, (uint32_t)(it - (uint64_t)jj * L.num_pixels));
    }
    // sample jj of the chunk at compact pixel pix
    __device__ __forceinline__ bool start_jp(PathState &st, uint32_t jj, uint32_t pix) const {
        st.pix = pix;
        int px, py;
        if (!pixel_of(L, st.pix, px, py)) return false;
        begin(st, jj, px, py);
        return true;
    }
    // the SFMT replay's next sample: crop pixel xy (x | y << 16), sample jj of the chunk
    __device__ __forceinline__ void start_xy(PathState &st, uint32_t xy, uint32_t jj) const {
        const uint32_t lx = xy & 0xffffu, ly = xy >> 16;   // row_stride 1: compact row = ly
        st.pix = ((ly >> 3) * L.tiles_x + (lx >> 3)) * 64u + (ly & 7u) * 8u + (lx & 7u);   // pixel_of's inverse
        begin(st, jj, (int)(L.x0 + lx), (int)(L.y0 + ly));
    }

    __device__ __forceinline__ void begin(PathState &st, uint32_t jj, const int px, const int py) const {
        StartRec r;
        produce(r, jj, st.pix, px, py);
        load(st, r);
    }

    // begin()'s producing half: the sample's sequence index, its film position and its
    // camera ray, which depend on (pixel, sample) alone -- any lane may form them (the
    // tiny-scene megakernel: all 64 lanes of a wave at once, dmega.h).  Not for the SFMT
    // replay, whose draws belong to the rendering lane's stream
    __device__ __forceinline__ void produce(StartRec &r, uint32_t jj, uint32_t pix, const int px, const int py) const {
        const MtsgDeviceScene &S = L.scene;
        SamplerState smp;
        float u, v;
        sample_start(SC, L, ycolTab, SC.nibbles, px, py, L.j0 + jj, smp, u, v);
        r.sobolIndex = smp.sobolIndex;
        r.dim = smp.dim;
        r.jj = jj;
        r.pix = pix;
        r.sx = (float)px + u;
        r.sy = (float)py + v;
        if constexpr (LENS) {
            if (lens_ray()) {
            // renderBlock's aperture draw (integrator.cpp:171-172), then the sensor's ray
            float ax = 0.5f, ay = 0.5f;
            if (sensor_needs_aperture(L.cam_lens)) next2d(SC, L.resolution, smp, px, py, ax, ay);
            r.dim = smp.dim;
            r.invZ = 1.0f;
            sensor_ray(S.cam, L.cam_lens, r.sx, r.sy, ax, ay, r.ro, r.rd, r.mint, r.maxt);
            return;
            }
        }
        // the pinhole (dsensor.h): direction and invZ; origin and interval are load()'s
        const MtsgCamera &cam = S.cam;
        const f3 dl = pinhole_dir(cam, r.sx, r.sy, r.invZ);
        r.rd = xf_vector(cam.to_world, dl);
        if constexpr (COMBO) {   // a `perspective` ray in the lens set's record: what load() forms elsewhere
            r.ro = cam_origin();
            r.mint = cam.near_clip * r.invZ;
            r.maxt = cam.far_clip * r.invZ;
        }
    }

    // every camera ray's origin (wave-uniform)
    __device__ __forceinline__ f3 cam_origin() const { return pinhole_origin(L.scene.cam); }

    // begin()'s other half: a start record into the path state, the camera origin and
    // Li()'s prologue
    __device__ __forceinline__ void load(PathState &st, const StartRec &r) const {
        const MtsgCamera &cam = L.scene.cam;
        SamplerState &smp = st.smp;
        PathVars &P = st.P;
        st.pix = r.pix;
        smp.sobolIndex = r.sobolIndex;
        smp.sampleIndex = L.j0 + r.jj;
        smp.dim = r.dim;
        smp.err = false;   // (the first next2d cannot run out of dimensions)
        st.sx = r.sx;
        st.sy = r.sy;
        st.rd = r.rd;
        if constexpr (LENS) {
            st.rmint = r.mint;
            st.rmaxt = r.maxt;
            P.its.p = r.ro;           // the ray's own origin
        } else {
        st.rmint = cam.near_clip * r.invZ;
        st.rmaxt = cam.far_clip * r.invZ;
        P.its.p = cam_origin();   // the ray's origin
        }
        // Li() prologue (path.cpp:119-133)
        P.L = mk(0, 0, 0);
        P.thr = mk(1.0f, 1.0f, 1.0f);
        P.eta = 1.0f;
        P.depth = 1;
        P.scattered = false;
        P.emitted = true;
        st.haveRay = true;
        st.primary = true;
        st.haveShadow = false;
        st.active = true;
    }

    // the rest of one bounce, given the step's trace results: returns true
    // when the path ends (path.cpp:135-292).  usePre: the hit record `pre` is already
    // formed (the wavefront's trace kernel), else fill_hit forms it from (slot, prim, u, v, t)
    __device__ __forceinline__ bool shade(PathState &st, bool occluded, bool hit, uint32_t slot, uint32_t prim,
                                          float hu, float hv, float ht, bool usePre = false, const Hit &pre = Hit{}) const {
        const MtsgDeviceScene &S = L.scene;
        PathVars &P = st.P;
        SamplerState &smp = st.smp;
        // next2d reads the pixel only for dimensions 0-1 (begin() has drawn them)
        const int px = 0, py = 0;
        const float sx = st.sx, sy = st.sy;
        if constexpr (HITK == 1) hit = true;
        if constexpr (HITK == 2) hit = false;
        f3 &rd = st.rd, &sd = st.sd;
        const f3 ro = P.its.p;   // the ray's origin: the previous vertex (or the camera)
        float &rmint = st.rmint, &rmaxt = st.rmaxt, &smaxt = st.smaxt;
        bool endPath = false;
        // NEE of the previous vertex (scene.cpp:838-842, path.cpp:176-199)
        if (st.haveShadow && !occluded) P.L = add(P.L, P.neeC);
        st.haveShadow = false;
        bool vertex = false;
        if (!st.haveRay) {
            endPath = true;   // the BSDF sample at the previous vertex failed
        } else {
            // rRec.rayIntersect / scene->rayIntersect (records.inl:117-144, path.cpp:226)
            // a miss overwrites the whole record: no field of the previous vertex stays
            // live across the next traversal except through an explicit use
            if (hit) {
                if (usePre) P.its = pre;
                else fill_hit<EXT, ANA>(S, hs, slot, prim, hu, hv, ht, ro, rd, P.its);
            } else {
                P.its = Hit{};
            }
            if (STATS && hit) c.hits++;
            if (st.primary) {
                P.alpha = L.has_alpha ? (P.its.valid ? 1u : 0u) : 1u;
                vertex = true;
            } else if (HITK == 2 || !P.its.valid) {
                // missed: the environment emitter, if any (path.cpp:233-247)
                if (ENV && have_env() && !(L.hide_emitters && !P.scattered)) {
                    glb_env *E = (glb_env *)S.env;
                    const bool cst = REFN && E->constant;
                    EnvValPdf vp = {mk(0, 0, 0), 0.0f};
                    if (!cst) vp = env_eval_pdf_at(E, env_uv(E, rd));   // one (u, v) and texel set for both
                    const f3 value = cst ? mk(E->radiance[0], E->radiance[1], E->radiance[2]) : vp.value;
                    float nT, fT;
                    // EnvironmentMap::fillDirectSamplingRecord (envmap.cpp:358-374)
                    if (env_bsphere(E, ro, rd, nT, fT) && !(nT > 0 || fT < 0)) {
                        float lumPdf = 0;
                        if (!PV_DELTA(P))   // pdfDirect (envmap.cpp:545-556) x pdfEmitterDiscrete
                            lumPdf = (cst ? const_pdf_direct(rd, P.refN) : vp.pdf) *
                                     (S.emitters[S.env_emitter].weight * S.em_norm);
                        const float a2 = P.bsdfPdf * P.bsdfPdf, b2 = lumPdf * lumPdf;
                        P.L = add(P.L, mul(mulv(P.thr, value), a2 / (a2 + b2)));
                    }
                }
                // volpath.cpp:326-336: the miss still passes the RR step before the loop ends
                if (L.integrator == MTSG_INTEGRATOR_VOLPATH && P.depth++ >= L.rr_depth) (void)next1d(SC, smp);
                endPath = true;   // !its.isValid(): break after the environment term
            } else if constexpr (HITK != 2) {
                auto &sh = hs.shapes[P.its.shape];
                if (REFN && sh.emitter >= 0) {
                    const f3 value = area_Le(S, P.its, neg(rd));
                    float lumPdf = 0;
                    if (!PV_DELTA(P)) {
                        // Scene::pdfEmitterDirect; dRec.ref = the previous vertex
                        lumPdf = area_hit_pdf<ANA>(&S, sh.emitter, P.its, ro, rd, P.refN);
                    }
                    const float a2 = P.bsdfPdf * P.bsdfPdf, b2 = lumPdf * lumPdf;
                    P.L = add(P.L, mul(mulv(P.thr, value), a2 / (a2 + b2)));
                }
                P.emitted = false;
                if (P.depth++ >= L.rr_depth) {
                    const float q = smin(smaxc(P.thr) * P.eta * P.eta, (float)0.95f);
                    if (next1d(SC, smp) >= q) endPath = true;
                    else P.thr = divs(P.thr, q);
                }
                if (smp.err) endPath = true;
                vertex = !endPath;
            }
        }
        st.haveRay = false;
        st.primary = false;

        if (vertex) {
            // loop head of Li() (path.cpp:135-200); rd is the incoming ray direction
            if (!(P.depth <= L.max_depth || L.max_depth < 0)) {
                endPath = true;
            } else if (HITK == 2 || !P.its.valid) {
                // camera ray missed: scene->evalEnvironment(ray) with the sensor's ray
                // differentials (path.cpp:136-142, perspective.cpp:271-298, integrator.cpp:181)
                if (ENV && have_env() && P.emitted && (!L.hide_emitters || P.scattered)) {
                    const MtsgCamera &cam = S.cam;
                    f3 rxd, ryd;
                    if (LENS && lens_ray()) {
                        // the sensor's own differentials (dsensor.h).  The aperture sample is not
                        // kept across the bounce: dimensions 2, 3 of the sample's index, drawn again
                        // (the same table words as produce()'s next2d: the same bits)
                        float ax = 0.5f, ay = 0.5f;
                        if (sensor_needs_aperture(L.cam_lens)) sobol_sample2(SC, smp.sobolIndex, 2, ax, ay);
                        sensor_ray_diff(cam, L.cam_lens, sx, sy, ax, ay, rd, L.diff_scale, rxd, ryd);
                    } else {
                    const f3 nearP = xf_point(cam.sample_to_camera, mk(sx * cam.inv_res_x, sy * cam.inv_res_y, 0.0f));
                    const f3 rxl = normalize(add(nearP, ld3(cam.dx))), ryl = normalize(add(nearP, ld3(cam.dy)));
                    const float *W = cam.to_world;
                    rxd = mk(W[0] * rxl.x + W[1] * rxl.y + W[2] * rxl.z, W[4] * rxl.x + W[5] * rxl.y + W[6] * rxl.z,
                             W[8] * rxl.x + W[9] * rxl.y + W[10] * rxl.z);
                    ryd = mk(W[0] * ryl.x + W[1] * ryl.y + W[2] * ryl.z, W[4] * ryl.x + W[5] * ryl.y + W[6] * ryl.z,
                             W[8] * ryl.x + W[9] * ryl.y + W[10] * ryl.z);
                    rxd = add(rd, mul(sub(rxd, rd), L.diff_scale));   // RayDifferential::scaleDifferential (ray.h:163-168)
                    ryd = add(rd, mul(sub(ryd, rd), L.diff_scale));
                    }
                    glb_env *E = (glb_env *)S.env;
                    if (REFN && E->constant) {   // ConstantBackgroundEmitter::evalEnvironment (constant.cpp:241-243)
                        P.L = add(P.L, mulv(P.thr, mk(E->radiance[0], E->radiance[1], E->radiance[2])));
                    } else {
                    P.L = add(P.L, mulv(P.thr, env_eval_diff(E, rd, rxd, ryd)));
                    }
                }
                endPath = true;
            } else if constexpr (HITK != 2) {
                auto &sh = hs.shapes[P.its.shape];
                GBsdf &bsdf = ((GBsdf *)S.bsdfs)[sh.bsdf];
                // roughplastic's per-vertex transmittance terms (dbsdf.h rp_pre), formed
                // at the first query of this vertex and reused for the same BSDF and wi
                RpPre rpc = {0.0f, 0.0f, 0.0f};
                GBsdf *rpB = nullptr;
                float rpZ = 0.0f;
                auto rpPre = [&](GBsdf *qb, f3 qwi) -> RpPre {
                    if constexpr (EXT && (KIND < 0 || KIND == BSDF_ROUGHPLASTIC)) {
                        if ((KIND == BSDF_ROUGHPLASTIC || qb->type == BSDF_ROUGHPLASTIC) &&
                            !(rpB == qb && __float_as_uint(rpZ) == __float_as_uint(qwi.z))) {
                            rpc = rp_pre<BSF>(*qb, (glb_f32 *)S.rtrans, qwi, P.its.u, P.its.v);
                            rpB = qb;
                            rpZ = qwi.z;
                        }
                    }
                    return rpc;
                };
                if (REFN && sh.emitter >= 0 && P.emitted && (!L.hide_emitters || P.scattered))
                    P.L = add(P.L, mulv(P.thr, area_Le(S, P.its, neg(rd))));
                // volpath.cpp:214-221 stops only for a strictly negative -dot(geoN, d) * cosTheta(wi)
                const float snp = dot(rd, P.its.geoN) * P.its.wi.z;
                if ((P.depth >= L.max_depth && L.max_depth > 0) ||
                    (!NOSTRICT && L.strict_normals && (L.integrator == MTSG_INTEGRATOR_VOLPATH ? snp > 0 : snp >= 0))) {
                    endPath = true;
                } else {
                    if constexpr (REFN)
                        P.refN = (bsdf.flags & (MTSG_F_TRANSMISSION | MTSG_F_BACK)) == 0 ? P.its.sh.n : mk(0, 0, 0);
                    if (bsdf.flags & MTSG_F_SMOOTH) {
                        // Scene::sampleEmitterDirect (scene.cpp:828-852)
                        float ex, ey;
                        next2d(SC, L.resolution, smp, px, py, ex, ey);
                        // one emitter whose CDF is {0.0f, 1.0f} (L.one_emitter, checked at upload):
                        // sampleReuse returns emitter 0 with pdf 1 - 0 and leaves ex = (ex - 0) / 1
                        float emPdf = 1.0f;
                        uint32_t ei = 0;
                        const bool oneEm = L.one_emitter != 0;
                        if (!oneEm) ei = dd_sample_reuse(S.em_cdf, S.num_emitters, ex, &emPdf);
                        if (STATS) c.nee++;
                        const MtsgEmitter &e = S.emitters[ei];
                        f3 value = mk(0, 0, 0), dd = mk(0, 0, 1);
                        float pdf = 0.0f, dist = 0.0f;
                        f3 vlp = mk(0, 0, 0);   // dRec.p where it does not define dRec.d exactly (volpath)
                        bool vrecomp = false;
                        bool onSurface = true;   // Emitter::isOnSurface(): false for the delta emitters
                        bool isDelta = false;
                        if constexpr (DELTA) isDelta = e.type >= MTSG_EMITTER_POINT;
                        if (DELTA && isDelta) {
                            if constexpr (DELTA) {
                                const DeltaSample ds =
                                    delta_sample_direct(e.type, ((GDelta *)S.delta)[e.tri_first], ld3(e.radiance), P.its.p);
                                value = ds.value; dd = ds.d; dist = ds.dist; pdf = ds.pdf;
                                vlp = ds.p; vrecomp = true;
                                onSurface = false;
                            }
                        } else if (ENV && (!REFN || e.type != MTSG_EMITTER_AREA)) {
                            glb_env *E = (glb_env *)S.env;
                            const EnvSample es = (REFN && E->constant) ? const_sample_direct(E, P.its.p, P.refN, ex, ey)
                                                                       : env_sample_direct(E, P.its.p, ex, ey);
                            value = es.value; dd = es.d; dist = es.dist; pdf = es.pdf;
                            vlp = add(P.its.p, mul(dd, dist));   // dRec.p = ray(farT) (envmap.cpp:536, constant.cpp:254)
                            vrecomp = true;
                        } else if constexpr (!REFN) {
                        } else if (ANA && S.shapes[e.shape].analytic >= 0) {
                            const AnaSample as =
                                ana_sample_direct(((GAna *)S.analytic)[S.shapes[e.shape].analytic], P.its.p, ex, ey);
                            dd = as.d; dist = as.dist; pdf = as.pdf;
                            vlp = as.p; vrecomp = true;
                            // AreaLight::sampleDirect (area.cpp:158-173)
                            if (dot(dd, P.refN) >= 0 && dot(dd, as.n) < 0 && pdf != 0) value = divs(ld3(e.radiance), pdf);
                            else pdf = 0.0f;
                        } else {
                        // TriMesh::samplePosition (trimesh.cpp:412-425), Triangle::sample (triangle.cpp:24-58)
                        float py2 = ey;
                        const uint32_t lt = dd_sample_reuse(S.area_cdf + e.cdf_offset, e.tri_count, py2, nullptr);
                        const uint32_t prim = e.tri_first + lt;
                        const uint4 pv = make_uint4(hs.pv[4 * prim], hs.pv[4 * prim + 1], hs.pv[4 * prim + 2],
                                                    hs.pv[4 * prim + 3]);
                        const float a = safe_sqrt(1.0f - ex);
                        const float bx = 1 - a, by = a * py2;
                        const f3 p0 = ldp3(hs.pos + 3 * (size_t)pv.x), p1 = ldp3(hs.pos + 3 * (size_t)pv.y),
                                 p2 = ldp3(hs.pos + 3 * (size_t)pv.z);
                        const f3 sideA = sub(p1, p0), sideB = sub(p2, p0);
                        const f3 lp = add(add(p0, mul(sideA, bx)), mul(sideB, by));
                        f3 ln;
                        if (hs.shapes[e.shape].has_normals) {
                            const f3 n0 = ldp3(hs.nrm + 3 * (size_t)pv.x), n1 = ldp3(hs.nrm + 3 * (size_t)pv.y),
                                     n2 = ldp3(hs.nrm + 3 * (size_t)pv.z);
                            ln = normalize(add(add(mul(n0, 1.0f - bx - by), mul(n1, bx)), mul(n2, by)));
                        } else {
                            // the staged face normal is normalize(cross(sideA, sideB)) by the same
                            // operations, except that an all-zero cross stays zero there
                            // (fill_hit's guard) where normalize gives NaN: that case keeps this code
                            ln = mk(0, 0, 0);
                            if constexpr (SCENE_LDS) ln = ldp3(hs.fn + 3 * (size_t)prim);
                            if (is_zero(ln)) ln = normalize(cross(sideA, sideB));
                        }
                        pdf = e.inv_area;
                        // Shape::sampleDirect (shape.cpp:102-115)
                        dd = sub(lp, P.its.p);
                        const float distSquared = len2(dd);
                        dist = dsqrt(distSquared);
                        dd = divs(dd, dist);
                        const float dp = absdot(dd, ln);
                        pdf *= dp != 0 ? (distSquared / dp) : 0.0f;
                        // AreaLight::sampleDirect (area.cpp:158-173)
                        if (dot(dd, P.refN) >= 0 && dot(dd, ln) < 0 && pdf != 0) value = divs(ld3(e.radiance), pdf);
                        else pdf = 0.0f;
                        }
                        if (pdf != 0) {
                            // the NEE estimate but for visibility (path.cpp:176-199)
                            float dpdf = pdf;   // pdf * 1 and value / 1 are pdf and value
                            if (!oneEm) {
                                dpdf = pdf * emPdf;
                                value = divs(value, emPdf);
                            }
                            f3 c = mk(0, 0, 0);
                            if (!is_zero(value)) {
                                const f3 wo = to_local(P.its.sh, dd);
                                // twosided (twosided.cpp:105-131): the nested BSDF of the side wi is on
                                f3 qwi = P.its.wi, qwo = wo;
                                GBsdf *qb = &bsdf;
                                EvalPdf ep;
                                bool combo = false;
                                if constexpr (COMBO && KIND < 0) {
                                    // mixturebsdf, blendbsdf, mask and twosided over them: the chain of dcombo.h
                                    if (bsdf.type >= BSDF_TWOSIDED) {
                                        ep = combo_eval_pdf<BSF>((GBsdf *)S.bsdfs, (GCombo *)L.combos, (glb_f32 *)S.rtrans,
                                                                 qb, qwi, qwo, P.its.u, P.its.v);
                                        combo = true;
                                    }
                                }
                                if (!combo) {
                                if constexpr (EXT && KIND < 0) {
                                    if (bsdf.type == BSDF_TWOSIDED) {
                                        const bool flip = !(qwi.z > 0);
                                        qb = &((GBsdf *)S.bsdfs)[bsdf.nested[flip ? 1 : 0]];
                                        if (flip) { qwi.z = -qwi.z; qwo.z = -qwo.z; }
                                    }
                                }
                                ep = bsdf_eval_pdf_k<BSF, KIND>(*qb, (glb_f32 *)S.rtrans, qwi, qwo, P.its.u, P.its.v,
                                                                rpPre(qb, qwi));
                                }
                                const f3 bsdfVal = ep.val;
                                if (!is_zero(bsdfVal) && (NOSTRICT || !L.strict_normals || dot(P.its.geoN, dd) * wo.z > 0)) {
                                    // bsdfPdf = 0 for an emitter that is not on a surface (path.cpp:192-197)
                                    const float bsdfPdf = (DELTA && !onSurface) ? 0.0f : ep.pdf;
                                    const float pa = dpdf * dpdf, pb = bsdfPdf * bsdfPdf;
                                    const float weight = pa / (pa + pb);
                                    c = mul(mulv(mulv(P.thr, value), bsdfVal), weight);
                                }
                            }
                            // Ray(dRec.ref, dRec.d, Epsilon, dRec.dist*(1-ShadowEpsilon)) (scene.cpp:839-840)
                            P.neeC = c;
                            sd = dd;
                            smaxt = dist * (1 - D_SHADOW_EPSILON);
                            if (L.integrator == MTSG_INTEGRATOR_VOLPATH && vrecomp) {
                                // Scene::evalTransmittance (scene.cpp:619-679, 890): the segment to dRec.p,
                                // re-normalised; area lights and the environment are EOnSurface (envmap.cpp:107,
                                // constant.cpp:48) and get the shadow epsilon at the far end, the delta
                                // emitters (p2OnSurface = false) the whole segment: lengthFactor = 1
                                const f3 v = sub(vlp, P.its.p);
                                const float rem = dsqrt(len2(v));
                                sd = divs(v, rem);
                                smaxt = (DELTA && !onSurface) ? rem * 1.0f : rem * (1 - D_SHADOW_EPSILON);
                            }
                            st.haveShadow = true;
                        }
                    }
                    // BSDF sampling (path.cpp:206-226)
                    float bx2, by2;
                    next2d(SC, L.resolution, smp, px, py, bx2, by2);
                    float u1d = 0.0f;
                    if (KIND >= 0 ? KIND == BSDF_ROUGHDIELECTRIC : bsdf.type == BSDF_ROUGHDIELECTRIC)
                        u1d = next1d(SC, smp);   // roughdielectric.cpp:554
                    BSample bs;
                    if (COMBO && KIND < 0 && bsdf.type >= BSDF_TWOSIDED) {
                        if constexpr (COMBO)
                            bs = combo_sample<BSF>((GBsdf *)S.bsdfs, (GCombo *)L.combos, (glb_f32 *)S.rtrans, &bsdf,
                                                   P.its.wi, bx2, by2, P.its.u, P.its.v);
                    } else if (EXT && KIND < 0 && bsdf.type == BSDF_TWOSIDED) {
                        // TwoSidedBRDF::sample(bRec, pdf, sample) (twosided.cpp:151-172)
                        const bool flip = P.its.wi.z < 0;
                        f3 qwi = P.its.wi;
                        if (flip) qwi.z = -qwi.z;
                        GBsdf *nb = &((GBsdf *)S.bsdfs)[bsdf.nested[flip ? 1 : 0]];
                        bs = bsdf_sample_fast<BSF>(*nb, (glb_f32 *)S.rtrans, qwi, bx2, by2, u1d, P.its.u, P.its.v,
                                                   rpPre(nb, qwi));
                        if (flip && !is_zero(bs.weight) && bs.pdf != 0) bs.wo.z = -bs.wo.z;
                    } else {
                        bs = bsdf_sample_k<BSF, KIND>(bsdf, (glb_f32 *)S.rtrans, P.its.wi, bx2, by2, u1d, P.its.u,
                                                      P.its.v, rpPre(&bsdf, P.its.wi));
                    }
                    if (!is_zero(bs.weight) && !smp.err) {
                        P.scattered |= bs.sampledType != MTSG_F_NULL;
                        const f3 wo = to_world(P.its.sh, bs.wo);
                        if (NOSTRICT || !L.strict_normals || dot(P.its.geoN, wo) * bs.wo.z > 0) {
                            // throughput *= bsdfWeight; eta *= bRec.eta (path.cpp:256-257): the same
                            // products as after the hit, formed now so they need not stay live
                            P.thr = mulv(P.thr, bs.weight);
                            P.bsdfPdf = bs.pdf;
                            P.eta *= bs.eta;
                            PV_SET_DELTA(P, bs.sampledType);
                            // Ray(its.p, wo, ray.time): mint = Epsilon, maxt = inf (origin P.its.p)
                            rd = wo;
                            rmint = D_EPSILON;
                            rmaxt = INFINITY;
                            st.haveRay = true;
                        }
                    }
                    // no next ray: the path ends once the pending shadow ray is resolved
                    if (!st.haveRay && !st.haveShadow) endPath = true;
                }
            }
        }
        return endPath;
    }

    // block->put(samplePos, spec, alpha) (integrator.cpp:184) and the sample's records
    // LANE_COUNTS: count the sample into c (the wavefront engine); the megakernel
    // counts finished samples per wave instead (WaveCounters)
    // hold (megakernel, box filter, sample runs of 2 or more): the record of sample 2k is
    // kept in *hold and stored with sample 2k + 1's, which the same lane renders next, as
    // one whole 32 B sector (film_slot)
    template <bool LANE_COUNTS = true>
    __device__ __forceinline__ void finish(PathState &st, float4 *hold = nullptr) const {
        PathVars &P = st.P;
        SamplerState &smp = st.smp;
        const uint32_t j = smp.sampleIndex, pix = st.pix;
        int px = 0, py = 0;
        pixel_of(L, pix, px, py);
        const float sx = st.sx, sy = st.sy;
        // block->put(samplePos, spec, alpha) (integrator.cpp:184): the own-pixel
        // splat is stored as {L.rgb, w} (alpha in {0,1} in the sign bit of w) and
        // film_reduce re-forms weight * value[k] -- the same products
        const float alpha = P.alpha ? 1.0f : 0.0f;
        const float val[5] = {P.L.x, P.L.y, P.L.z, alpha, 1.0f};
        const uint32_t jj = j - L.j0;
        if (hold && !L.gather && L.round_shift != 0 && MTSG_SPLAT_PAIR) {
            float ownW = 0.0f;
            float4 rec4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (film_splat(L, px, py, sx, sy, val, ownW)) rec4 = make_float4(val[0], val[1], val[2], P.alpha ? ownW : -ownW);
            float4 *c4 = reinterpret_cast<float4 *>(L.contrib);
            const size_t slot = film_slot(L, jj, pix);
            if ((jj & 1u) == 0 && jj + 1 < L.chunk_spp) {
                *hold = rec4;
            } else if (jj & 1u) {
                c4[slot - 1] = *hold;
                c4[slot] = rec4;
            } else {
                c4[slot] = rec4;
            }
        } else {
            film_record(L, film_slot(L, jj, pix), px, py, sx, sy, val, P.alpha);
        }
        if (INSTR && L.samples) {
            const uint32_t pixIdx = (uint32_t)(py - (int)L.y0) * L.width + (uint32_t)(px - (int)L.x0);
            float *rec = L.samples + ((size_t)pixIdx * L.spp + j) * 8;
            rec[0] = P.L.x; rec[1] = P.L.y; rec[2] = P.L.z; rec[3] = alpha;
            rec[4] = sx; rec[5] = sy; rec[6] = (float)P.depth; rec[7] = smp.err ? 1.0f : 0.0f;
        }
        if (STATS) c.sobol += (unsigned long long)smp.dim * (smp.dim < L.lds_dims ? 0 : L.nibbles);
        if (!LANE_COUNTS) {
            st.active = false;
            st.haveRay = st.haveShadow = false;
            return;
        }
        c.len += (uint32_t)P.depth;
        c.samples++;
        if (smp.err) c.err++;
        // a lane's rays and shadow rays never exceed its path lengths plus samples:
        // flush the 32-bit counts well before any of them can wrap
        if (__builtin_expect((c.len | c.samples) >= 0x40000000u, 0)) {
            atomicAdd(L.counters + 0, (unsigned long long)c.samples);
            atomicAdd(L.counters + 1, (unsigned long long)c.rays);
            atomicAdd(L.counters + 2, (unsigned long long)c.shadow);
            atomicAdd(L.counters + 3, (unsigned long long)c.len);
            c.samples = c.rays = c.shadow = c.len = 0;
        }
        st.active = false;
        st.haveRay = st.haveShadow = false;
    }

    // The whole path of a sample whose camera ray misses the scene (the start queue's
    // production pass, dmega.h; kernels without ENV only): what load(), one shade() and
    // finish<false>() leave for it -- Li = 0, alpha 0 (1 without has_alpha), depth 1, the
    // two film dimensions drawn.  px, py: the sample's pixel (pixel_of(r.pix))
    __device__ __forceinline__ void retire(const StartRec &r, const int px, const int py) const {
        static_assert(!ENV, "a miss under an environment emitter is not black");
        const bool a = !L.has_alpha;
        const float alpha = a ? 1.0f : 0.0f;
        const float val[5] = {0.0f, 0.0f, 0.0f, alpha, 1.0f};
        // (the per-sample record first: stored after film_record, the instrumented 4-wave
        // kernel spilled 9 VGPRs instead of 6)
        if (INSTR && L.samples) {
            const uint32_t pixIdx = (uint32_t)(py - (int)L.y0) * L.width + (uint32_t)(px - (int)L.x0);
            float *rec = L.samples + ((size_t)pixIdx * L.spp + (L.j0 + r.jj)) * 8;
            rec[0] = 0.0f; rec[1] = 0.0f; rec[2] = 0.0f; rec[3] = alpha;
            rec[4] = r.sx; rec[5] = r.sy; rec[6] = 1.0f; rec[7] = 0.0f;
        }
        film_record(L, film_slot(L, r.jj, r.pix), px, py, r.sx, r.sy, val, a);
        if (STATS) c.sobol += (unsigned long long)r.dim * (r.dim < L.lds_dims ? 0 : L.nibbles);
    }
};

// the megakernel's always-on counts, summed per wave (uniform: SGPRs, not a VGPR
// per lane across the whole bounce loop)
struct WaveCounters {
    uint32_t rays, shadow, len, samples, err;
};
__device__ __forceinline__ uint32_t wave_count(bool b) { return (uint32_t)__popcll(__ballot(b)); }
__device__ __forceinline__ void wave_counters_flush(const MtsgLaunch &L, const WaveCounters &w) {
    if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0) {
        atomicAdd(L.counters + 0, (unsigned long long)w.samples);
        atomicAdd(L.counters + 1, (unsigned long long)w.rays);
        atomicAdd(L.counters + 2, (unsigned long long)w.shadow);
        atomicAdd(L.counters + 3, (unsigned long long)w.len);
        if (w.err) atomicAdd(L.counters + 6, (unsigned long long)w.err);
    }
}

template <bool STATS>
__device__ __forceinline__ void path_counters_flush(const MtsgLaunch &L, const PathCounters &c) {
    atomicAdd(L.counters + 0, (unsigned long long)c.samples);
    atomicAdd(L.counters + 1, (unsigned long long)c.rays);
    atomicAdd(L.counters + 2, (unsigned long long)c.shadow);
    atomicAdd(L.counters + 3, (unsigned long long)c.len);
    if (STATS) {
        atomicAdd(L.counters + 4, c.nodes);
        atomicAdd(L.counters + 5, c.tests);
        atomicAdd(L.counters + 7, c.hits);
        atomicAdd(L.counters + 9, c.nee);
        atomicAdd(L.counters + 10, c.sobol);
    }
    if (c.err) atomicAdd(L.counters + 6, (unsigned long long)c.err);
}

__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
