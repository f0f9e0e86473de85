// path_f.hip -- the megakernel variants (dmega.h) of one scene feature set
// PATH_FEAT (MTSG_FEAT_ENV | EXT | ANA bits), built once per set by the
// Makefile (-DPATH_FEAT=n -> path_f<n>.o), so the sets compile in parallel.
//
// Per set: the generic kernel (every BSDF, virtual-dispatch order of
// path.cpp:171-211), for all-diffuse small scenes (PATH_FEAT 0) the DIFF
// kernel, and the 7 BSDF-set specialisations of large scenes (dbsdf.h BSet):
// bits = {every rough BSDF is GGX, no roughdielectric, no roughconductor};
// with an environment emitter also the 7 sets of envmap-only scenes (bit 3,
// MTSG_FEAT_NOREFN: no area light, no constant emitter).
// The set kernels are compiled without strictNormals (MTSG_FEAT_NOSTRICT).
// PATH_FEAT 1031 (MTSG_FEAT_SET_DELTA) is the set of scenes with point / spot /
// directional emitters: the generic kernel alone, with and without SCENE_LDS.
// PATH_FEAT 3079 (MTSG_FEAT_SET_LENS) is the set of scenes whose sensor is thinlens,
// orthographic or telecentric (dsensor.h): the generic kernel alone as well.
#include "dmega.h"

static_assert(mtsg_is_feat_set(PATH_FEAT), "-DPATH_FEAT names a set of layout.h's MTSG_FEAT_SETS");
#define PF_NAME2(a, N) a##N
#define PF_NAME(a, N) PF_NAME2(a, N)

// this object's view of the launch record (capi.cpp launch_layout_error)
extern "C" uint32_t PF_NAME(mtsg_launch_bytes_path_f, PATH_FEAT)() { return (uint32_t)sizeof(MtsgLaunch); }

namespace {
constexpr int spec_feat(int bits) {
    return PATH_FEAT | (int)MTSG_FEAT_NOSTRICT | ((bits & 1) ? (int)MTSG_FEAT_GGX : 0) |
           ((bits & 2) ? (int)MTSG_FEAT_NORD : 0) | ((bits & 4) ? (int)MTSG_FEAT_NORC : 0) |
           ((bits & 8) ? (int)MTSG_FEAT_NOREFN : 0);
}

// variants: small scenes (BVH in LDS) run 3 waves/SIMD with 32 Sobol dims in
// LDS (all-diffuse ones 4: no calls in their bounce loop); large scenes run 4
// waves/SIMD (128 VGPRs) when the traversal stacks fit 4 blocks per CU, else 3
// (render_plan.cpp plan_render picks L.waves and L.lds_dims)
template <int FEAT>
PathKernelFn pick_v(const MtsgLaunch &L, bool instr) {
    if constexpr ((FEAT & (MTSG_FEAT_GGX | MTSG_FEAT_NORD | MTSG_FEAT_NORC)) != 0) {   // large scenes only
        return L.waves == 4 ? path_kernel_w<false, FEAT, 4>(instr) : path_kernel_w<false, FEAT, MTSG_WAVES_PER_EU>(instr);
    } else {
        if (L.scene_lds) {
            if constexpr ((FEAT & MTSG_FEAT_DIFF) != 0) {
                if (L.waves == 4) return path_kernel_w<true, FEAT, 4>(instr);
            }
            return path_kernel_w<true, FEAT, MTSG_WAVES_PER_EU>(instr);
        }
        return L.waves == 4 ? path_kernel_w<false, FEAT, 4>(instr) : path_kernel_w<false, FEAT, MTSG_WAVES_PER_EU>(instr);
    }
}
}  // namespace

// the instantiation mtsg_launch_path launches and mtsg_path_kernel_occupancy sizes the grid by
// (path_kernel.hip path_pick); bits: spec_bits
PathKernelFn PF_NAME(mtsg_path_pick_f, PATH_FEAT)(const MtsgLaunch &L, int bits, bool instr) {
    switch (bits) {
#if !(PATH_FEAT & 1024)   // MTSG_FEAT_DELTA (the delta-emitter and the lens set): the generic kernel only (spec_bits gives 0)
        case 1: return pick_v<spec_feat(1)>(L, instr);
        case 2: return pick_v<spec_feat(2)>(L, instr);
        case 3: return pick_v<spec_feat(3)>(L, instr);
        case 4: return pick_v<spec_feat(4)>(L, instr);
        case 5: return pick_v<spec_feat(5)>(L, instr);
        case 6: return pick_v<spec_feat(6)>(L, instr);
        case 7: return pick_v<spec_feat(7)>(L, instr);
#if PATH_FEAT & 1   // envmap-only scenes (MTSG_FEAT_NOREFN): feature sets with an environment emitter
        case 9: return pick_v<spec_feat(9)>(L, instr);
        case 10: return pick_v<spec_feat(10)>(L, instr);
        case 11: return pick_v<spec_feat(11)>(L, instr);
        case 12: return pick_v<spec_feat(12)>(L, instr);
        case 13: return pick_v<spec_feat(13)>(L, instr);
        case 14: return pick_v<spec_feat(14)>(L, instr);
        case 15: return pick_v<spec_feat(15)>(L, instr);
#endif
#endif
        default:
#if PATH_FEAT == 0
            if (L.all_diffuse) return pick_v<MTSG_FEAT_DIFF>(L, instr);
#endif
            return pick_v<PATH_FEAT>(L, instr);
    }
}
