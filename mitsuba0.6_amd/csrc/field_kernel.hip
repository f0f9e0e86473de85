// field_kernel.hip -- the `field` integrator (integrators/misc/field.cpp:55-187) as the
// multichannel integrator runs it (integrators/misc/multichannel.cpp:164-221): one lane per
// (pixel, sample) item; per item the sampler's first 2D draw, the camera ray, ONE closest-hit
// query through the scene's own structure (tiny-scene scan, LDS BVH or HBM BVH; analytic
// shapes included) and the intersection record with its uv -- then every requested field is
// read off that one record.  The prologue is direct_kernel's (path_kernel.hip), so a field
// sample sits at the position, and sees the hit, of the colour render's sample.
//
// Each field is recorded as {f.r, f.g, f.b, alpha, 1} through film_record (dfilm.h) into its
// own record array and summed by film_reduce / film_gather into its own ordinary 5-float
// film.  multichannel's blocks are built with warnInvalid off (multichannel.cpp:143-145):
// negative values (normals, positions) are kept, film_record<false>.
//
// Built with path_kernel.hip's flags (Makefile PK_FLAGS): it inlines the same traversal.
#include "dpath.h"
#include "launchers.h"

// BSDF::getDiffuseReflectance(its) of the hit shape's BSDF
// L2 (the MTSG_FEAT_LEAF2 instantiations): phong's diffuseReflectance (phong.cpp:109-111) and
// roughdiffuse's reflectance (roughdiffuse.cpp:124-126); difftrans has BSDF's default, whose
// eval(typeMask = EDiffuseReflection) it rejects
template <bool L2>
__device__ __forceinline__ f3 field_albedo(const MtsgDeviceScene &S, GBsdf &top, const Hit &h) {
    constexpr int BS = (int)MTSG_FEAT_EXT;
    GBsdf *b = &top;
    if (b->type == BSDF_TWOSIDED)   // twosided.cpp:198-203: its is handed on as it is
        b = &((GBsdf *)S.bsdfs)[top.nested[h.wi.z > 0 ? 0 : 1]];
    if constexpr (L2) {
        if (b->type == BSDF_PHONG || b->type == BSDF_ROUGHDIFFUSE) return bsdf_refl<BS>(*b, h.u, h.v);
    }
    switch (b->type) {
        case BSDF_DIFFUSE:   // diffuse.cpp:106-108
            return bsdf_refl<BS>(*b, h.u, h.v);
        case BSDF_PLASTIC:   // plastic.cpp:219-221
            return mul(bsdf_refl<BS>(*b, h.u, h.v), 1 - b->fdr_ext);
        case BSDF_ROUGHPLASTIC: {   // roughplastic.cpp:309-315
            float ftr = b->ftr_ext;
            if (b->alpha_tex.type) {   // RoughTransmittance::evalDiffuse, eta fixed (rtrans.h:254-259, 283)
                const float alpha = avg3(tex_eval(b->alpha_tex, h.u, h.v));
                const float r = cubic1d(rt_warp_alpha(*b, alpha), (glb_f32 *)S.rtrans + b->rt_int + b->rt_alpha,
                                        (uint32_t)b->rt_alpha);
                ftr = smin(1.0f, smax(0.0f, r));
            }
            return mul(bsdf_refl<BS>(*b, h.u, h.v), ftr);
        }
        default:   // BSDF::getDiffuseReflectance (bsdf.cpp:82-86): eval with typeMask = EDiffuseReflection,
            return mk(0, 0, 0);   // which the conductors and dielectrics reject
    }
}

template <bool SCENE_LDS, int FEAT>
__global__ __launch_bounds__(BLOCK, MTSG_WAVES_PER_EU) void field_kernel(MtsgLaunch L, MtsgFieldArgs FA) {
    constexpr bool ANA = (FEAT & MTSG_FEAT_ANA) != 0;
    extern __shared__ __attribute__((aligned(64))) uint32_t lds[];   // (dsampler.h sobol_row)
    const MtsgDeviceScene &S = L.scene;
    const LdsView<SCENE_LDS> V = stage_lds<SCENE_LDS>(L, lds);   // ends with a barrier
    lds_u32 *ycolTab = V.ycolTab;
    lds_node *ldsNodes = V.nodes;
    lds_tri *ldsTris = V.tris;
    const HitSrc<SCENE_LDS> &hs = V.hs;
    const SobolCtx &SC = V.SC;   // (no SFMT replay: render_plan.cpp refuses it)
    lds_stk_n *stkN = (lds_stk_n *)(lds + V.stackBase) + threadIdx.x;
    lds_stk_d *stkD = (lds_stk_d *)(lds + V.stackBase + L.stack_depth * BLOCK) + threadIdx.x;
    unsigned long long cSamples = 0, cErr = 0, cN = 0, cT = 0;

    const uint64_t lanes = (uint64_t)gridDim.x * BLOCK;
    for (uint64_t it = (uint64_t)xcd_block(L.xcds) * BLOCK + threadIdx.x; it < L.num_items; it += lanes) {
        uint32_t jj, pix;
        int px, py;
        if (!item_pixel(L, it, jj, pix, px, py)) continue;
        const uint32_t j = L.j0 + jj;
        SamplerState smp;
        float u, v;
        sample_start(SC, L, ycolTab, L.nibbles, px, py, j, smp, u, v);
        const float sx = (float)px + u, sy = (float)py + v;
        f3 ro, rd;
        float rmint, rmaxt;
        if constexpr ((FEAT & MTSG_FEAT_LENS) != 0) {
            // the other sensors (dsensor.h): the aperture draw of renderBlock, then the sensor's ray
            float ax = 0.5f, ay = 0.5f;
            if (sensor_needs_aperture(L.cam_lens)) next2d(SC, L.resolution, smp, px, py, ax, ay);
            sensor_ray(S.cam, L.cam_lens, sx, sy, ax, ay, ro, rd, rmint, rmaxt);
        } else {
            camera_ray(S.cam, sx, sy, ro, rd, rmint, rmaxt);
        }

        // rRec.rayIntersect(sensorRay): the one closest-hit query of the sample
        uint32_t slot = 0, prim = 0;
        float hu = 0, hv = 0, ht = 0;
        const bool hit = closest_hit<SCENE_LDS, ANA>(L, ldsNodes, ldsTris, stkN, stkD, ro, rd, rmint, rmaxt, slot, hu, hv,
                                                     ht, cN, cT);
        Hit its = Hit{};
        bool analytic = false;
        if (hit) {
            prim = hit_prim<SCENE_LDS>(L, ldsTris, slot);
            fill_hit<true, ANA>(S, hs, slot, prim, hu, hv, ht, ro, rd, its);
            if constexpr (ANA) analytic = hs.shapes[its.shape].analytic >= 0;
        }
        const float alpha = hit ? 1.0f : 0.0f;   // rRec.alpha: always opacity (multichannel.cpp:181-215)

        const uint32_t nf = FA.num_fields;
        float *rec = nullptr;
        if (L.samples) {
            const uint32_t pixIdx = (uint32_t)(py - (int)L.y0) * L.width + (uint32_t)(px - (int)L.x0);
            rec = L.samples + ((size_t)pixIdx * L.spp + j) * FA.record_floats;
            rec[0] = sx; rec[1] = sy; rec[2] = alpha; rec[3] = hit ? 1.0f : 0.0f;
        }
        const size_t slot0 = film_slot(L, jj, pix);
        const size_t fieldSlots = (size_t)(FA.contrib_stride / (L.gather ? 8u : 4u));
        for (uint32_t f = 0; f < nf; ++f) {
            f3 r = mk(FA.undefined[f][0], FA.undefined[f][1], FA.undefined[f][2]);
            if (hit) {
                switch (FA.field[f]) {   // FieldIntegrator::Li (field.cpp:132-174)
                    case MTSG_FIELD_POSITION: r = its.p; break;
                    case MTSG_FIELD_REL_POSITION: r = xf_point(FA.world_to_cam, its.p); break;
                    case MTSG_FIELD_DISTANCE: r = mk(its.t, its.t, its.t); break;
                    case MTSG_FIELD_GEO_NORMAL: r = its.geoN; break;
                    case MTSG_FIELD_SH_NORMAL: r = its.sh.n; break;
                    case MTSG_FIELD_UV: r = mk(its.u, its.v, 0.0f); break;
                    case MTSG_FIELD_ALBEDO: r = field_albedo<(FEAT & MTSG_FEAT_LEAF2) != 0>(S, ((GBsdf *)S.bsdfs)[hs.shapes[its.shape].bsdf], its); break;
                    case MTSG_FIELD_SHAPE_INDEX: { const float s = (float)its.shape; r = mk(s, s, s); break; }
                    default: {   // MTSG_FIELD_PRIM_INDEX: the triangle within its mesh; KNoTriangleFlag otherwise
                        const float p = analytic ? (float)0xffffffffu : (float)(prim - FA.shape_first[its.shape]);
                        r = mk(p, p, p);
                    }
                }
            }
            // block->put(samplePos, temp) with temp = {.., alpha, 1} (multichannel.cpp:207-217)
            const float val[5] = {r.x, r.y, r.z, alpha, 1.0f};
            film_record<false>(L, slot0 + f * fieldSlots, px, py, sx, sy, val, alpha != 0.0f, FA.spill[f]);
            if (rec) { rec[4 + 3 * f] = r.x; rec[5 + 3 * f] = r.y; rec[6 + 3 * f] = r.z; }
        }
        cSamples++;
        if (smp.err) cErr++;
    }
    atomicAdd(L.counters + 0, cSamples);
    atomicAdd(L.counters + 1, cSamples);   // one closest-hit ray per sample
    if (cErr) atomicAdd(L.counters + 6, cErr);
}

// this object's view of the launch record (capi.cpp launch_layout_error)
extern "C" uint32_t mtsg_launch_bytes_field_kernel() { return (uint32_t)sizeof(MtsgLaunch); }

// the instantiation of a launch; its dynamic LDS is the megakernel's (mtsg_path_lds_bytes: the same layout)
typedef void (*FieldKernelFn)(MtsgLaunch, MtsgFieldArgs);
static FieldKernelFn field_pick(const MtsgLaunch &L) {
    constexpr int EXT = MTSG_FEAT_EXT, ANA = MTSG_FEAT_EXT | MTSG_FEAT_ANA;
    // thinlens / orthographic / telecentric: one instantiation that holds the analytic shapes too
    if (L.leaf2) {   // a difftrans / roughdiffuse / phong in the scene: field_albedo knows them
        constexpr int L2 = MTSG_FEAT_LEAF2;
        if (L.lens) return L.scene_lds ? field_kernel<true, ANA | MTSG_FEAT_LENS | L2> : field_kernel<false, ANA | MTSG_FEAT_LENS | L2>;
        if (L.ana) return L.scene_lds ? field_kernel<true, ANA | L2> : field_kernel<false, ANA | L2>;
        return L.scene_lds ? field_kernel<true, EXT | L2> : field_kernel<false, EXT | L2>;
    }
    if (L.lens) return L.scene_lds ? field_kernel<true, ANA | MTSG_FEAT_LENS> : field_kernel<false, ANA | MTSG_FEAT_LENS>;
    if (L.ana) return L.scene_lds ? field_kernel<true, ANA> : field_kernel<false, ANA>;
    return L.scene_lds ? field_kernel<true, EXT> : field_kernel<false, EXT>;
}

hipError_t mtsg_launch_field(const MtsgLaunch &L, const MtsgFieldArgs &FA, int grid, hipStream_t stream) {
    hipLaunchKernelGGL(field_pick(L), dim3(grid), dim3(BLOCK), mtsg_path_lds_bytes(L), stream, L, FA);
    return hipGetLastError();
}

int mtsg_field_occupancy(const MtsgLaunch &L, int *bpc) {
    return (int)hipOccupancyMaxActiveBlocksPerMultiprocessor(bpc, field_pick(L), BLOCK, mtsg_path_lds_bytes(L));
}
