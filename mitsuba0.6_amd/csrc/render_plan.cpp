// render_plan.cpp -- the launch decisions of a render (render_plan.h): plain host code,
// no HIP call.  capi.cpp render_impl executes the plan; mtsgpu_plan_host reports it.
#include "render_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "launchers.h"   // mtsg_path_features, mtsg_path_variant: host functions of path_kernel.hip

RenderKnobs read_knobs() {
    RenderKnobs K;
    const char *e;
    K.wf_hitrec = (e = std::getenv("MTSGPU_WF_HITREC")) && e[0] == '1';
    K.wf_shade_lds_dims = (e = std::getenv("MTSGPU_WF_SHADE_LDS_DIMS")) ? (uint32_t)std::strtoul(e, nullptr, 10) : ~0u;
    K.wf_generic = std::getenv("MTSGPU_WF_GENERIC") != nullptr;
    K.round_shift = (e = std::getenv("MTSGPU_ROUND_SHIFT")) ? std::min(6, std::max(0, std::atoi(e))) : -1;
    K.no_one_emitter = std::getenv("MTSGPU_NO_ONE_EMITTER") != nullptr;
    K.no_scene_lds = std::getenv("MTSGPU_NO_SCENE_LDS") != nullptr;
    K.no_scan = std::getenv("MTSGPU_NO_SCAN") != nullptr;
    K.no_diff_variant = std::getenv("MTSGPU_NO_DIFF_VARIANT") != nullptr;
    K.no_tiny_set = std::getenv("MTSGPU_NO_TINY_SET") != nullptr;
    K.no_bsdf_sets = std::getenv("MTSGPU_NO_BSDF_SETS") != nullptr;
    K.no_refn_spec = std::getenv("MTSGPU_NO_REFN_SPEC") != nullptr;
    K.waves = (e = std::getenv("MTSGPU_WAVES")) ? (std::atoi(e) == 4 ? 4u : 3u) : 0u;
    K.no_gather = std::getenv("MTSGPU_NO_GATHER") != nullptr;
    K.sobol_lds_dims = (e = std::getenv("MTSGPU_SOBOL_LDS_DIMS"))
                           ? (int)std::min(1024l, std::max(0l, std::strtol(e, nullptr, 10))) : -1;
    K.contrib_bytes = (e = std::getenv("MTSGPU_CONTRIB_BYTES")) ? std::max<size_t>(std::strtoull(e, nullptr, 10), 1 << 20) : 0;
    K.engine_wavefront = (e = std::getenv("MTSGPU_ENGINE")) && std::strcmp(e, "wavefront") == 0;
    K.wf_slots = (e = std::getenv("MTSGPU_WF_SLOTS")) ? std::max<uint64_t>(1, std::strtoull(e, nullptr, 10)) : 0;
    return K;
}

// tiny scenes: the TriAccel records grouped by projection axis and, within
// an axis, planes normal to it (n_u = n_v = 0: the Cornell box's walls)
// last, so the scan runs six branch-free loops, the aligned ones without
// the numerator's and denominator's n_u/n_v terms (the closest hit and its
// tie rule do not depend on the order the records are tested in).
// Within a group, records that share their plane and vertex A -- the two
// triangles of a quad triangulated as a fan -- come first, partners adjacent
// at 2i and 2i+1 (np[group] pairs), the singles after them: a pair's t, hu
// and hv are the same bits for both, so scan_pair forms them once.  Partners
// have a_u and a_v bit-equal and n_u, n_v, n_d bit-equal (an aligned group:
// n_d only, its loops never read n_u / n_v).  Bit-equality is an equivalence,
// so pairing each record with the next unpaired equal one leaves at most one
// single per plane.  MTSGPU_NO_SCAN_PAIRS: no pairs (A/B and tests).
//
// Canonical zero (MTSG_SCAN_ZERO_SIGN, default 1; with and without pairs): the two
// triangles of a quad can come out of the TriAccel construction with n_u (or n_v)
// = +0 in one and -0 in the other, which the bit-equality above keeps apart.  The
// copy in g -- only g, the array the scans read; H.tris, the LDS and BVH records
// and the oracle's keep theirs -- gets +0 for an n_u or n_v that is -0 wherever the
// record's n_d is not +-0.  No reader of g (scan_pair_k; scan_k in the megakernel's
// scan_tris, the wavefront engine, direct_kernel and trace_rays with its arbitrary
// mint and maxt) can tell, for any ray:
//  * numerator ((n_d - o_u n_u) - o_v n_v) - o_k: a finite o_u times +-0 is a zero,
//    and n_d minus a zero of either sign is n_d exactly when n_d != 0 (also an
//    infinite or NaN n_d).  A non-finite o_u makes the product NaN under both signs.
//    (With n_d = -0 the difference is +0 or -0 by that sign, and through t = +-0, a
//    zero origin and a zero a_u it reaches a stored t, u or v: hence the exclusion.)
//  * denominator (d_u n_u + d_v n_v) + d_k: the zero product matters only where
//    d_v n_v is a zero too and d_k = 0; then the denominator is a zero of one sign or
//    the other and t is +-inf, or NaN with a zero numerator, either way.  -inf fails
//    t < mint.  +inf passes t > maxt only against maxt = +inf, and then hu = o_u +
//    t d_u - a_u and hv are each infinite or NaN, so are u and v (inf * 0 = NaN), and
//    u >= 0, v >= 0, u + v <= 1 cannot all hold.  A NaN t passes the interval test
//    and fails u >= 0 the same way.  So a ray that sees the sign is rejected under
//    both, and no accept decision and no stored (t, u, v) changes.
// The same holds with u and v exchanged (n_v = -0).  The aligned groups' records, whose
// partners need not share n_u / n_v and whose loops never read them, are copied as they are.
#ifndef MTSG_SCAN_ZERO_SIGN
#define MTSG_SCAN_ZERO_SIGN 1
#endif
void mtsg_scan_layout(const std::vector<MtsgTri> &tris, std::vector<MtsgTri> &g, uint32_t n[6], uint32_t np[6]) {
    const bool pairs = !std::getenv("MTSGPU_NO_SCAN_PAIRS");
    auto bits = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; };
    g.clear();
    for (uint32_t k = 0; k < 3; ++k)
        for (uint32_t al = 0; al < 2; ++al) {
            std::vector<MtsgTri> m, singles;
            for (const MtsgTri &t : tris)
                if (t.k == k && (uint32_t)(t.n_u == 0.0f && t.n_v == 0.0f) == al) {
                    m.push_back(t);
                    if (MTSG_SCAN_ZERO_SIGN && !al && t.n_d != 0.0f) {   // (t.n_d != 0: neither +0 nor -0)
                        if (bits(t.n_u) == 0x80000000u) m.back().n_u = 0.0f;
                        if (bits(t.n_v) == 0x80000000u) m.back().n_v = 0.0f;
                    }
                }
            std::vector<char> used(m.size(), 0);
            uint32_t &cnt = np[2 * k + al];
            cnt = 0;
            for (size_t i = 0; i < m.size(); ++i) {
                if (used[i]) continue;
                size_t j = m.size();
                if (pairs)
                    for (j = i + 1; j < m.size(); ++j)
                        if (!used[j] && bits(m[i].a_u) == bits(m[j].a_u) && bits(m[i].a_v) == bits(m[j].a_v) &&
                            bits(m[i].n_d) == bits(m[j].n_d) &&
                            (al || (bits(m[i].n_u) == bits(m[j].n_u) && bits(m[i].n_v) == bits(m[j].n_v))))
                            break;
                if (j < m.size()) {
                    used[j] = 1;
                    g.push_back(m[i]);
                    g.push_back(m[j]);
                    cnt++;
                } else
                    singles.push_back(m[i]);
            }
            g.insert(g.end(), singles.begin(), singles.end());
            n[2 * k + al] = (uint32_t)m.size();
        }
}

// tiny scenes: the scan's grouped records (mtsg_scan_layout)
void scene_scan_n(const HostScene &H, std::vector<MtsgTri> &g, uint32_t scan_n[6]) {
    g.clear();
    for (int k = 0; k < 6; ++k) scan_n[k] = 0;
    if (H.tris.size() > MTSG_SCAN_MAX || !H.analytic.empty()) return;
    uint32_t n[6], np[6];
    mtsg_scan_layout(H.tris, g, n, np);
    for (int k = 0; k < 6; ++k) scan_n[k] = n[k] | np[k] << 16;
    if (g.empty()) g.push_back(MtsgTri{});
}

// a launch constant of the scene: sampleReuse over the CDF {0, 1} is the identity (dpath.h shade)
uint32_t scene_one_emitter(const HostScene &H) {
    uint32_t w[2] = {1u, 0u};
    if (H.em_cdf.size() == 2) std::memcpy(w, H.em_cdf.data(), 8);
    return (H.emitters.size() == 1 && w[0] == 0u && w[1] == 0x3f800000u) ? 1u : 0u;
}

void scene_scalars(const HostScene &H, MtsgDeviceScene &D) {
    D.num_emitters = (uint32_t)H.emitters.size();
    D.num_prims = (uint32_t)H.tris.size();
    D.em_norm = H.em_norm;
    D.env_emitter = H.env.emitter;
    for (int a = 0; a < 3; ++a) { D.aabb_min[a] = H.aabb_min[a]; D.aabb_max[a] = H.aabb_max[a]; }
    D.cam = H.cam;
}

// megakernel sample runs (dmega.h): a lane renders 2^s consecutive samples of one pixel, so
// its wave keeps the same 64 pixels for 2^s paths.  Large scenes: the longest runs that leave
// every lane MTSG_MIN_RUNS of them (full frame: C3 s = 4 +13%, C5 s = 5 +14% over s = 0; longer
// runs leave a tail, profiles/r06_rounds/).  Tiny LDS scenes gain nothing: pairs, whose box
// records share a 32 B sector (film_slot).  MTSGPU_ROUND_SHIFT=s overrides (A/B): knob >= 0
uint32_t run_shift(const MtsgLaunch &L, uint64_t lanes, int knob) {
    if (knob >= 0) return (uint32_t)knob;
    uint32_t s = L.scene_lds ? 1u : 6u;
    const uint64_t perLane = L.num_items / std::max<uint64_t>(1, lanes);
    while (s > 0 && ((1u << s) > L.chunk_spp || (perLane >> s) < MTSG_MIN_RUNS)) --s;
    return s;
}

// the window's work decomposition: compact rows (interleave) x columns in 8x8 tiles, or
// (tile shards) every row_stride-th 8x8 tile of the window; with the reciprocals the
// kernels divide by (layout.h pixel_of)
void launch_geometry(MtsgLaunch &L, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, uint32_t row_block,
                     uint32_t row_stride, uint32_t row_phase, bool tile_shard) {
    L.x0 = x0; L.y0 = y0; L.width = width; L.height = height;
    L.row_block = row_block ? row_block : 1;
    L.row_stride = row_stride ? row_stride : 1;
    L.row_phase = row_phase % L.row_stride;
    L.tile_shard = tile_shard ? 1u : 0u;
    L.tiles_x = (width + 7) / 8;
    if (L.tile_shard) {
        const uint64_t tiles = (uint64_t)L.tiles_x * ((height + 7) / 8);
        L.num_pixels = (uint32_t)((tiles + L.row_stride - 1) / L.row_stride * 64);
    } else {
        const uint32_t rowsCompact =
            ((height + L.row_block - 1) / L.row_block + L.row_stride - 1) / L.row_stride * L.row_block;
        const uint32_t tilesY = (rowsCompact + 7) / 8;
        L.num_pixels = L.tiles_x * tilesY * 64;
    }
    mtsg_launch_index(L, 0);   // the reciprocals; the megakernel's grid is known per launch (plan_launch)
}

namespace {

int bad(std::string &err, const char *msg) {
    err = msg;
    return MTSGPU_EINVAL;
}

// the scene's BSDF set, for the specialised megakernel variants (dbsdf.h BSet)
uint32_t plan_bset(const HostScene &H, const mtsgpu_render_params &P, const RenderKnobs &K) {
    bool ggx = true, rc = false, rd = false;
    for (const MtsgBsdf &b : H.bsdfs) {
        const bool rough = b.type == MTSGPU_BSDF_ROUGHCONDUCTOR || b.type == MTSGPU_BSDF_ROUGHDIELECTRIC ||
                           b.type == MTSGPU_BSDF_ROUGHPLASTIC;
        if (rough && b.distr != MTSGPU_DISTR_GGX) ggx = false;
        rc |= b.type == MTSGPU_BSDF_ROUGHCONDUCTOR;
        rd |= b.type == MTSGPU_BSDF_ROUGHDIELECTRIC;
    }
    // the set variants traverse half-float node boxes (layout.h MtsgHNode): a
    // scene beyond half range would get infinite (still exact, but useless) boxes
    float extent = 0.0f;
    for (int a = 0; a < 3; ++a) extent = std::max(extent, std::max(std::fabs(H.aabb_min[a]), std::fabs(H.aabb_max[a])));
    // (the set kernels are built without strictNormals: MTSG_FEAT_NOSTRICT)
    const bool lens = H.cam_lens.type != MTSG_SENSOR_PERSPECTIVE;   // (the lens set, like the delta set: the generic kernel)
    uint32_t bset = (K.no_bsdf_sets || !(extent < 32768.0f) || P.strict_normals || !H.deltas.empty() || lens || !H.combos.empty() || H.leaf2) ? 0u
                    : (ggx ? (uint32_t)MTSG_FEAT_GGX : 0u) | (rc ? 0u : (uint32_t)MTSG_FEAT_NORC) |
                          (rd ? 0u : (uint32_t)MTSG_FEAT_NORD);
    // envmap-only scenes (no area light, no constant emitter): the set kernels without
    // refN (MTSG_FEAT_NOREFN, dpath.h PathShader::REFN)
    bool envOnly = H.env.emitter >= 0 && !H.env.constant && !K.no_refn_spec;
    for (const MtsgEmitter &em : H.emitters) envOnly &= em.type == MTSG_EMITTER_ENVMAP;
    if (bset && envOnly) bset |= (uint32_t)MTSG_FEAT_NOREFN;
    return bset;
}

// which kernel variant runs and what it stages in LDS: scene-in-LDS, scan, waves per SIMD,
// Sobol dims in LDS, the BSDF-set bits (L.nibbles and L.stack_depth are set)
void plan_variant(MtsgLaunch &L, const HostScene &H, const mtsgpu_render_params &P, const RenderKnobs &K) {
    // small scenes: stage the whole BVH + TriAccel array in LDS (<= 32 KiB)
    const size_t sceneBytes = H.nodes.size() * sizeof(MtsgNode) + H.tris.size() * sizeof(MtsgTri) +
                              H.prim_vtx.size() * 4 + H.dpdu.size() * 4 + H.face_n.size() * 4 + H.positions.size() * 4 +
                              H.normals.size() * 4 + H.shapes.size() * sizeof(MtsgShape);
    L.scene_lds = (sceneBytes <= (32u << 10) && !K.no_scene_lds) ? 1u : 0u;
    L.scan = (L.scene_lds && H.tris.size() <= MTSG_SCAN_MAX && H.analytic.empty() && !K.no_scan) ? 1u : 0u;
    L.ext = H.ext ? 1u : 0u;
    L.ana = H.analytic.empty() ? 0u : 1u;
    // point / spot / directional emitters: the MTSG_FEAT_SET_DELTA kernels, the generic BSDF set only
    L.delta = H.deltas.empty() ? 0u : 1u;
    // thinlens / orthographic / telecentric sensors: the MTSG_FEAT_SET_LENS kernels, the generic BSDF set
    // only; no start queue (mtsg_path_start_queue) and, compiled with ENV, no early miss
    L.lens = H.cam_lens.type != MTSG_SENSOR_PERSPECTIVE ? 1u : 0u;
    L.cam_lens = H.cam_lens;
    // mixturebsdf / blendbsdf / mask: the MTSG_FEAT_SET_COMBO kernels, which hold the lens set's code
    // and ask the sensor type at run time; like that set the generic BSDF set, no start queue, no early miss
    L.combo = H.combos.empty() ? 0u : 1u;
    // difftrans / roughdiffuse / phong: the MTSG_FEAT_SET_LEAF2 kernels, the combinator set | LEAF2, on the same terms
    L.leaf2 = H.leaf2 ? 1u : 0u;
    L.all_diffuse = (K.no_diff_variant || L.delta || L.lens || L.combo || L.leaf2) ? 0u : 1u;
    for (const MtsgBsdf &b : H.bsdfs) L.all_diffuse &= b.type == MTSGPU_BSDF_DIFFUSE ? 1u : 0u;
    L.bset = plan_bset(H, P, K);
    // large scenes are latency-bound: run 4 waves/SIMD when 4 blocks' traversal
    // stacks + look_up tables fit the 160 KiB LDS, with as many Sobol dims in
    // LDS as the rest allows (the others are read through L1/L2)
    L.lds_dims = 32;
    L.waves = 3;
    if (!L.scene_lds) {
        const size_t perBlock = (160u << 10) / 4;
        const size_t fixed = ((size_t)L.stack_depth * 3 * MTSG_BLOCK + 1) / 2 * 4 + MTSG_LUT_WORDS * 4;
        if (fixed < perBlock) {
            L.waves = 4;
            L.lds_dims = (uint32_t)std::min<size_t>(32, (perBlock - fixed) / ((size_t)L.nibbles * 16 * 4));
        }
    }
    // the all-diffuse variant makes no calls: 4 waves/SIMD (128 VGPRs) beat 3 (C2 +8.3%)
    // and 5 (-15%) (profiles/r02_ab_c2_waves4.log, r02_ab_c2_waves45.log)
    if (L.scene_lds && L.all_diffuse) L.waves = 4;
    if (K.waves) L.waves = K.waves;
    if (K.sobol_lds_dims >= 0) L.lds_dims = (uint32_t)K.sobol_lds_dims;
}

// The tiny set (dmega.h TINY): the all-diffuse LDS kernel at 4 waves/SIMD holds the Sobol sampler
// with 8-nibble indices alone.  A megakernel launch of such a scene outside that set (layout.h
// mtsg_tiny_set: the independent sampler, an SFMT replay, a sample index of 2^32 or more), or any
// under MTSGPU_NO_TINY_SET, takes the generic LDS kernel path_kernel<*, true, 0, 3>, which renders
// the same samples with every choice at run time.  (direct_kernel, the wavefront engine and the
// field pass do not run the megakernel: their plan is as it was.  MTSGPU_NO_SCAN launches stay:
// the kernel keeps the BVH traversal and the loop without the queue as run-time choices)
void plan_tiny_set(MtsgLaunch &L, bool megakernel, const RenderKnobs &K) {
    if (!megakernel || !L.scene_lds || !L.all_diffuse) return;
    if (mtsg_tiny_set(L) && !K.no_tiny_set) return;
    L.all_diffuse = 0;
    L.waves = K.waves ? K.waves : 3;
}

// MIDirectIntegrator::configure / configureSampler (direct.cpp:128-143)
void plan_direct(MtsgLaunch &L, const mtsgpu_render_params &P) {
    const uint32_t nl = P.emitter_samples, nb = P.bsdf_samples;
    const size_t sum = (size_t)nl + nb;
    L.lum_samples = nl;
    L.bsdf_samples = nb;
    L.weight_bsdf = 1 / (float)nb;
    L.weight_lum = 1 / (float)nl;
    L.frac_bsdf = nb / (float)sum;
    L.frac_lum = nl / (float)sum;
    if (nl > 1) { L.lum_dim = L.array_end; L.array_end += 2; }
    if (nb > 1) { L.bsdf_dim = L.array_end; L.array_end += 2; }
}

// execution engine (same per-sample results): the wavefront pipeline or the megakernel
// (the default; DESIGN.md 4 has the engine A/B), the field pass its own kernel
int plan_engine(const mtsgpu_render_params &P, bool fields, bool pathLike, bool replay, const RenderKnobs &K,
                RenderPlan &plan, std::string &err) {
    bool wave = K.engine_wavefront && pathLike;
    if (P.flags & MTSGPU_FLAG_WAVEFRONT) wave = pathLike;
    if (P.flags & MTSGPU_FLAG_MEGAKERNEL) wave = false;
    if (replay) wave = false;   // one lane per replay unit
    if (fields) wave = false;
    plan.kdtree = false;
    if (!fields && (P.flags & MTSGPU_FLAG_KDTREE)) {
        // the reference's own kd-tree: the wavefront engine with wf_trace_kd
        if (!pathLike || replay)
            return bad(err, "kd-tree traversal: path / volpath with the sobol or independent sampler");
        if (P.flags & MTSGPU_FLAG_MEGAKERNEL) return bad(err, "kd-tree traversal runs in the wavefront engine");
        wave = plan.kdtree = true;
    }
    plan.engine = fields ? MTSG_ENGINE_FIELDS : wave ? MTSG_ENGINE_WAVEFRONT : MTSG_ENGINE_MEGAKERNEL;
    return MTSGPU_OK;
}

}  // namespace

int plan_render(const HostScene &H, const mtsgpu_render_params &Pr, uint32_t num_fields, bool want_samples,
                const DeviceFacts &dev, const RenderKnobs &K, RenderPlan &plan, std::string &err) {
    const mtsgpu_render_params *P = &Pr;
    const bool FJ = num_fields != 0;   // the field pass (the integrator fields of P are ignored)
    if (P->spp == 0) return bad(err, "sampleCount must be positive");
    const uint32_t nFilms = FJ ? num_fields : 1u;
    const bool pathLike = !FJ && (P->integrator == MTSGPU_INTEGRATOR_PATH || P->integrator == MTSGPU_INTEGRATOR_VOLPATH);
    if (pathLike && P->rr_depth <= 0) return bad(err, "'rrDepth' must be set to a value greater than zero!");
    if (pathLike && P->max_depth <= 0 && P->max_depth != -1)
        return bad(err, "'maxDepth' must be set to -1 (infinite) or a value greater than zero!");
    if ((uint64_t)P->x0 + P->width > H.film_w || (uint64_t)P->y0 + P->height > H.film_h)
        return bad(err, "render window exceeds the film");

    MtsgLaunch &L = plan.L;
    std::memset(&L, 0, sizeof L);
    scene_scalars(H, L.scene);
    if (mtsg_configure_filter(P->rfilter, P->rfilter_param, L.filter, err)) return MTSGPU_EINVAL;
    // SobolSampler::setFilmResolution(cropSize, bucketed = true) (sobol.cpp:147-158)
    // the render window is the film's crop window: cropSize drives the sampler
    // (Integrator::configureSampler, integrator.cpp:37-41)
    const uint32_t mx = std::max(P->width, P->height);
    uint32_t r = mx - 1;
    r |= r >> 1; r |= r >> 2; r |= r >> 4; r |= r >> 8; r |= r >> 16; r += 1;
    uint32_t m = 0;
    while ((1u << m) < r) ++m;
    L.resolution = (float)r;
    L.diff_scale = 1.0f / std::sqrt((float)P->spp);   // integrator.cpp:144-145
    mtsg_sobol_lookup_table(m, L.lut);
    uint64_t scr = P->scramble;
    if (scr) scr = mtsg_sample_tea((uint32_t)scr, (uint32_t)(scr >> 32), 4);   // sobol.cpp:93-101
    L.scramble = (uint32_t)scr;
    L.scramble64 = scr;
    L.spp = P->spp;
    L.max_depth = P->max_depth;
    L.rr_depth = P->rr_depth;
    L.strict_normals = P->strict_normals;
    L.hide_emitters = P->hide_emitters;
    L.has_alpha = FJ ? 1 : P->has_alpha;
    L.film_w = (int)H.film_w;
    L.film_h = (int)H.film_h;
    L.fw = (int)H.film_w + 2 * L.filter.border;
    L.fh = (int)H.film_h + 2 * L.filter.border;
    launch_geometry(L, P->x0, P->y0, P->width, P->height, P->row_block, P->row_stride, P->row_phase,
                    (P->flags & MTSGPU_FLAG_TILE_SHARD) != 0);
    L.one_emitter = K.no_one_emitter ? 0u : H.launch.one_emitter;
    // Sobol index width: frame << 2m | 2m bits (sobolseq.h:93-125); 52 columns per dimension
    // the direct integrator's 2D sample arrays index the Sobol sequence at spp x count
    const bool direct = !FJ && P->integrator == MTSGPU_INTEGRATOR_DIRECT;
    if (!pathLike && !direct && !FJ) return bad(err, "unknown integrator");
    if (direct && P->emitter_samples + P->bsdf_samples == 0)
        return bad(err, "direct: emitterSamples + bsdfSamples must be positive");
    if (P->sampler < MTSGPU_SAMPLER_SOBOL || P->sampler > MTSGPU_SAMPLER_SFMT_BLOCKS) return bad(err, "unknown sampler");
    const bool replay = P->sampler == MTSGPU_SAMPLER_SFMT_REPLAY || P->sampler == MTSGPU_SAMPLER_SFMT_BLOCKS;
    if (replay && FJ)
        return bad(err, "field pass: the SFMT replay samplers' draw positions depend on how many numbers the "
                        "radiance integrator consumed; a separate pass cannot reproduce the sample positions");
    if (replay && H.cam_lens.type != MTSG_SENSOR_PERSPECTIVE)
        return bad(err, "SFMT replay: the perspective sensor only (nothing could check a replayed aperture stream of "
                        "a thinlens, orthographic or telecentric sensor)");
    if (replay && (!pathLike || L.row_stride > 1 || P->width > 65535 || P->height > 65535))
        return bad(err, "SFMT replay: path/volpath over a whole crop window (no row shards)");
    L.sampler = (uint32_t)P->sampler;
    const uint64_t perSampleIdx = direct ? std::max<uint64_t>(1, std::max(P->emitter_samples, P->bsdf_samples)) : 1;
    uint32_t sppBits = 0;
    while ((1ull << sppBits) < (uint64_t)P->spp * perSampleIdx) ++sppBits;
    const uint32_t indexBits = (m > 1 ? 2 * m : 0) + sppBits;
    if (L.sampler == MTSGPU_SAMPLER_SOBOL && indexBits > 52)
        return bad(err, "sample index exceeds the 52-bit Sobol direction numbers");
    // independent streams are keyed by (x, y, sample): 16 + 16 + 32 bits
    if (L.sampler == MTSGPU_SAMPLER_INDEPENDENT && (H.film_w > 65536 || H.film_h > 65536 ||
                                                   (uint64_t)P->spp * perSampleIdx > 0xFFFFFFFFull))
        return bad(err, "independent sampler: film or sample count too large for the stream key");
    L.nibbles = sobol_nibbles(indexBits);
    L.stack_depth = H.bvh_depth + 2;
    L.num_nodes = (uint32_t)H.nodes.size();
    L.num_verts = (uint32_t)(H.positions.size() / 3);
    L.num_shapes = (uint32_t)H.shapes.size();
    plan_variant(L, H, *P, K);
    for (int k = 0; k < 6; ++k) L.scan_n[k] = H.launch.scan_n[k];
    // gfx950 has 32 CUs per XCD; the hardware deals workgroups round-robin over
    // the XCDs of the device (a CPX partition is one XCD: no remap).  A CU count
    // that is not a multiple of 32 is not a whole-XCD partition: no remap either.
    L.xcds = (dev.num_cus % 32 == 0) ? (uint32_t)std::max(1, dev.num_cus / 32) : 1u;
    L.integrator = FJ ? (int32_t)MTSGPU_INTEGRATOR_PATH : P->integrator;
    L.array_end = 5;
    if (direct) plan_direct(L, *P);
    L.round_shift = 0;   // set per launch (run_shift)
    // gather mode (film_gather, path_kernel.hip): filters whose footprint covers the
    // neighbours (gaussian) -- every film pixel sums its neighbourhood's sample records in
    // a fixed order instead of taking atomic splats.  H = the largest footprint offset from a
    // sample's pixel: |x - px| <= floor(radius + 1/2) (film_splat's ceil/floor bounds)
    if (P->rfilter != MTSGPU_RFILTER_BOX) {
        const int h = std::max(L.filter.border, (int)std::floor(L.filter.radius + 0.5f));
        if (h >= 1 && h <= MTSG_GATHER_HMAX && !K.no_gather) {
            L.gather = 1;
            L.gather_h = (uint32_t)h;
        }
    }
    // own-pixel splat buffer [chunk][pixels] of float4; spp processed in chunks
    // that fit the budget: a quarter of the device's free HBM, at most 32 GiB
    // (C5's 1280x720x1024 splats, 15 GB, then run as one launch, one tail)
    size_t budget = (size_t)8 << 30;
    if (dev.free_bytes / 4 > budget) budget = std::min<size_t>(dev.free_bytes / 4 + dev.contrib_held, (size_t)32 << 30);
    if (K.contrib_bytes) budget = K.contrib_bytes;
    const size_t perSample = (size_t)L.num_pixels * (L.gather ? 32 : 16);   // one (gather mode: two) float4 per sample
    // (the field pass keeps one record array per field under the same budget)
    plan.chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(P->spp, budget / (perSample * nFilms)));
    plan.films = nFilms;
    plan.filmFloats = (size_t)L.fw * L.fh * 5;
    plan.fieldBytes = perSample * (plan.chunk + (plan.chunk & 1));   // one field's record array
    plan.recFloats = FJ ? 4 + 3 * (size_t)nFilms : (size_t)MTSGPU_SAMPLE_RECORD_FLOATS;
    plan.nsamp = want_samples ? (size_t)P->width * P->height * P->spp * plan.recFloats : 0;
    plan.stats_mode = (P->flags & MTSGPU_FLAG_TRAVERSAL_STATS) != 0;
    plan.instr = plan.nsamp != 0 || plan.stats_mode;
    plan.num_cus = dev.num_cus;
    plan.round_shift_knob = K.round_shift;
    // sensor->getWorldTransform()->eval(its.t).inverse() (field.cpp:137-139)
    if (FJ && !mtsg_invert4(H.cam.to_world, plan.world_to_cam)) return bad(err, "Singular matrix in Matrix::invert");
    plan.replay = replay;
    if (replay) {
        // IndependentSampler's Random() = seed(5489); RenderJob clones it per worker in
        // order (renderjob.cpp:58-66).  Units: one worker over all blocks, or one per block
        if (plan.chunk < P->spp) return bad(err, "SFMT replay: sampleCount exceeds one chunk");
        L.replay = 1;
        L.units = P->sampler == MTSGPU_SAMPLER_SFMT_BLOCKS
                      ? (P->width + MTSG_BLOCK_SIZE - 1) / MTSG_BLOCK_SIZE * ((P->height + MTSG_BLOCK_SIZE - 1) / MTSG_BLOCK_SIZE)
                      : 1u;
    }
    if (int rc = plan_engine(*P, FJ, pathLike, replay, K, plan, err)) return rc;
    plan_tiny_set(L, plan.engine == MTSG_ENGINE_MEGAKERNEL && pathLike, K);
    return MTSGPU_OK;
}

LaunchPlan plan_launch(const RenderPlan &plan, uint32_t j0, int blocks_per_cu) {
    MtsgLaunch L = plan.L;   // (run_shift reads the launch's items)
    LaunchPlan lp = {};
    lp.chunk_spp = L.chunk_spp = std::min(plan.chunk, L.spp - j0);
    lp.num_items = L.num_items = (uint64_t)L.chunk_spp * L.num_pixels;
    if (plan.engine == MTSG_ENGINE_WAVEFRONT) return lp;
    const uint64_t blocksNeeded = plan.replay ? (L.units + 255) / 256 : (L.num_items + 255) / 256;
    lp.grid = (int)std::min<uint64_t>((uint64_t)plan.num_cus * std::max(1, blocks_per_cu), std::max<uint64_t>(1, blocksNeeded));
    // the replay renders one unit per lane (its own SFMT stream): every unit needs a resident lane
    if (plan.replay && (uint64_t)lp.grid * 256 < L.units)
        lp.err = "SFMT replay: more 32x32 blocks than resident lanes (crop too large)";
    lp.round_shift = run_shift(L, (uint64_t)lp.grid * MTSG_BLOCK, plan.round_shift_knob);
    return lp;
}

// Entries per region of the wavefront queues.  A kernel's block b appends to
// region b % R, at most BLOCK entries per block.  Ray queues are filled by the
// shade kernels, one per kind over n_k <= slots entries in all: a region gets at
// most sum_k ceil(ceil(n_k / BLOCK) / R) <= ceil((slots / BLOCK + K) / R) + K
// blocks.  A kind queue gets the trace kernel's closest-hit entries (its first
// nc <= slots entries: ceil((slots / BLOCK + 1) / R) + 1 blocks per region), and
// the miss queue the shade kernels' appends as well.  Round 4 sized every
// region for all slots: 8x the ray-queue bytes that can be live.
static void wf_caps(size_t slots, size_t &capRay, size_t &capCls) {
    const size_t B = MTSG_BLOCK, R = MTSG_WF_REGIONS, K = MTSG_WK_KINDS, nb = (slots + B - 1) / B;
    const size_t shade = (nb + K + R - 1) / R + K, trace = (nb + 1 + R - 1) / R + 1;
    capRay = std::min(slots, B * shade);
    capCls = std::min(slots, B * (shade + trace));
}

// shape -> shade kind (wf_kernel.hip) from the shape's BSDF type; per kind,
// whether every BSDF of that kind uses the GGX distribution
static void wf_kinds(const HostScene &H, bool generic, WfPlan &plan) {
    bool any[MTSG_WK_KINDS] = {}, nonGgx[MTSG_WK_KINDS] = {};
    plan.shapeKind.assign(std::max<size_t>(1, H.shapes.size()), (uint32_t)MTSG_WK_GEN);
    for (size_t i = 0; i < H.shapes.size(); ++i) {
        const MtsgBsdf &b = H.bsdfs[H.shapes[i].bsdf];
        int k = MTSG_WK_GEN;
        switch (b.type) {
            case MTSGPU_BSDF_DIFFUSE: k = MTSG_WK_DIFF; break;
            case MTSGPU_BSDF_ROUGHCONDUCTOR: k = MTSG_WK_RC; break;
            case MTSGPU_BSDF_ROUGHDIELECTRIC: k = MTSG_WK_RD; break;
            case MTSGPU_BSDF_ROUGHPLASTIC: k = MTSG_WK_RP; break;
            default: break;
        }
        if (generic) k = MTSG_WK_GEN;   // A/B: every hit through the generic kernel
        plan.shapeKind[i] = (uint32_t)k;
        any[k] = true;
        if (b.distr != MTSGPU_DISTR_GGX) nonGgx[k] = true;
    }
    for (int k = 0; k < MTSG_WK_KINDS; ++k) {
        plan.kinds[k] = any[k] || k == MTSG_WK_MISS;
        plan.ggx[k] = any[k] && !nonGgx[k];
    }
}

WfPlan plan_wavefront(const RenderPlan &plan, const HostScene &H, const RenderKnobs &K) {
    const MtsgLaunch &L = plan.L;
    WfPlan wf;
    wf_kinds(H, K.wf_generic, wf);
    // path slots: about 2M (MTSGPU_WF_SLOTS), whole blocks; the kernels run one queue
    // entry per thread, so each grid covers the largest its queues can be (slots;
    // 2 x slots for the trace kernel's two ray queues) and surplus blocks exit at once
    uint64_t target = K.wf_slots ? K.wf_slots : (uint64_t)1 << 21;
    const uint64_t items = (uint64_t)std::min(plan.chunk, L.spp) * L.num_pixels;
    target = std::min(target, items);
    wf.slots = (uint32_t)((std::max<uint64_t>(1, target) + MTSG_BLOCK - 1) / MTSG_BLOCK * MTSG_BLOCK);
    for (int k = 0; k < MTSG_WK_KINDS; ++k)
        if (wf.kinds[k]) wf.shadeGrid[k] = (int)(wf.slots / MTSG_BLOCK);
    wf.traceGrid = (int)(2 * (uint64_t)wf.slots / MTSG_BLOCK);
    wf.hitrec = K.wf_hitrec;
    wf.hitrecUv = (mtsg_path_features(L) & MTSG_FEAT_EXT) != 0;
    wf_caps(wf.slots, wf.cap, wf.capCls);
    wf.ovfDepth = L.stack_depth > MTSG_WF_LDS_STACK ? L.stack_depth - MTSG_WF_LDS_STACK : 0;
    wf.partBlocks = wf.traceGrid;
    for (int k = 0; k < MTSG_WK_KINDS; ++k) wf.partBlocks = std::max(wf.partBlocks, wf.shadeGrid[k]);
    // the shade kernels' launch record: their blocks are short-lived (one queue entry
    // per thread), so the Sobol dimensions they stage in LDS are a per-block cost;
    // MTSGPU_WF_SHADE_LDS_DIMS caps them (0: every dimension from HBM/L2)
    wf.shadeLdsDims = std::min(L.lds_dims, K.wf_shade_lds_dims);
    return wf;
}

// counter 15: which kernel ran -- for the megakernel path_kernel<INSTR, SCENE_LDS, FEAT, WAVES>:
// FEAT's low 8 bits | WAVES << 8 | SCENE_LDS << 12 | INSTR << 13 | (FEAT & NOSTRICT) << 14 (the
// set kernels' strictNormals-free build) | (FEAT & NOREFN) << 15; 1 << 16 for the wavefront engine;
// 1 << 18 (MTSGPU_VARIANT_DELTA) on top of any of these: the MTSG_FEAT_SET_DELTA instantiations of
// scenes with delta emitters -- the megakernel, direct_kernel or the wavefront shade kernels;
// 1 << 19 (MTSGPU_VARIANT_LENS): the MTSG_FEAT_SET_LENS instantiations of scenes whose sensor is
// not `perspective` (those kernels hold the delta emitters too: bit 18 is then set only with
// such emitters in the scene), the field pass's included;
// 1 << 20 (MTSGPU_VARIANT_COMBO): the MTSG_FEAT_SET_COMBO instantiations of scenes with a mixturebsdf,
// blendbsdf or mask (they hold the lens and delta code too: bits 19 and 18 say what the scene has)
// 1 << 21 (MTSGPU_VARIANT_LEAF2): the MTSG_FEAT_SET_LEAF2 instantiations of scenes with a difftrans,
// roughdiffuse or phong (they hold the combinators' code too: bit 20 says whether the scene has one)
// (tests and A/B logs read it)
uint64_t plan_variant_word(const RenderPlan &plan) {
    const MtsgLaunch &L = plan.L;
    const uint64_t lbit = L.lens ? 1ull << 19 : 0;
    const uint64_t dbit = (L.delta ? 1ull << 18 : 0) | lbit | (L.combo ? 1ull << 20 : 0) | (L.leaf2 ? 1ull << 21 : 0);
    if (plan.engine == MTSG_ENGINE_WAVEFRONT) return (1ull << 16) | dbit;
    if (plan.engine == MTSG_ENGINE_FIELDS)   // field_kernel<SCENE_LDS, ..>: 1 << 17 | SCENE_LDS << 12
        return (1ull << 17) | ((uint64_t)L.scene_lds << 12) | lbit | (L.leaf2 ? 1ull << 21 : 0);   // (| its LEAF2 instantiation)
    const int v = mtsg_path_variant(L);
    return dbit | (uint64_t)((v & 0xff) | (int)(L.waves << 8) | (int)(L.scene_lds << 12) | (plan.instr ? 1 << 13 : 0) |
                      ((v & MTSG_FEAT_NOSTRICT) ? 1 << 14 : 0) | ((v & MTSG_FEAT_NOREFN) ? 1 << 15 : 0));
}
