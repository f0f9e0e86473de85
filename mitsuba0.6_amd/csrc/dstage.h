// dstage.h -- what a kernel sets up before its first item: the workgroup renumbering over
// the XCDs, the launch record re-read from the kernarg segment, and the LDS staging of the
// Sobol tables (sobolseq.h:43-57), sobol::look_up's tables and, for small scenes, the BVH,
// TriAccel records and vertex data, with the view (LdsView) of that layout.
// Included by dpath.h after dsampler.h and dhit.h.
#pragma once

// Workgroups are dispatched round-robin over the 8 XCDs, each with its own L2.
// Renumber them so that XCD x runs the x-th contiguous eighth of the grid: the
// items (pixels in 8x8 tiles) the lanes of one XCD hold at a time are then
// neighbours, and their rays share BVH nodes and triangles in that XCD's L2.
// `xcds` comes from the host (MtsgLaunch::xcds: CUs / 32 on gfx950, 1 on a
// CPX partition); no remap when it is 1 or does not divide the grid.
__device__ __forceinline__ uint32_t xcd_remap(uint32_t b, uint32_t nb, uint32_t xcds) {
    return (xcds > 1u && nb % xcds == 0) ? (b % xcds) * (nb / xcds) + b / xcds : b;
}
__device__ __forceinline__ uint32_t xcd_block(uint32_t xcds) { return xcd_remap(blockIdx.x, gridDim.x, xcds); }

// item `it` of a launch: sample jj of the chunk at compact pixel pix, image pixel (px, py)
// (layout.h pixel_of); false for a padding pixel
__device__ __forceinline__ bool item_pixel(const MtsgLaunch &L, uint64_t it, uint32_t &jj, uint32_t &pix, int &px,
                                           int &py) {
    jj = (uint32_t)(it / L.num_pixels);
    pix = (uint32_t)(it - (uint64_t)jj * L.num_pixels);
    return pixel_of(L, pix, px, py);
}

// The kernel's launch record (its first argument), re-read through a pointer
// the compiler cannot follow.  A persistent loop otherwise has LICM hoist every
// launch field and every product of them it finds invariant (camera rows,
// scene pointers, sampler constants) out of the loop; they then stay live
// across the whole bounce, as SGPRs spilled into VGPR lanes or as VGPR copies,
// and push the shading state into scratch.  Re-read per iteration they are
// s_loads from the kernarg segment (scalar cache) at their point of use.
// Requires MtsgLaunch to be the kernel's first argument (kernarg offset 0).
__device__ __forceinline__ const MtsgLaunch &launch_fresh() {
    typedef __attribute__((address_space(4))) const MtsgLaunch KernargLaunch;
    KernargLaunch *kp = (KernargLaunch *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp));
    return *(const MtsgLaunch *)kp;
}

// LDS of path_kernel / wf_shade: [Sobol nibble tables][look_up tables (MTSG_LUT_WORDS, layout.h)]
// [BVH + TriAccel + hit data (SCENE_LDS)][traversal stacks]
template <bool SCENE_LDS>
struct LdsView {
    lds_u32 *ycolTab;
    lds_node *nodes;
    lds_tri *tris;
    HitSrc<SCENE_LDS> hs;
    SobolCtx SC;
    uint32_t stackBase;   // word offset of the traversal stacks
};

template <bool SCENE_LDS>
__device__ __forceinline__ LdsView<SCENE_LDS> lds_view(const MtsgLaunch &L, uint32_t *lds);

// the look_up tables (layout.h sobol_lookup_lds), formed once per block: the inverse is
// applied here, not per look-up
__device__ __forceinline__ void stage_lut(const MtsgLaunch &L, uint32_t *tab) {
    for (uint32_t i = threadIdx.x; i < MTSG_LUT_WORDS; i += BLOCK) tab[i] = mtsg_lut_word(L.lut, i);
}

template <bool SCENE_LDS>
__device__ __forceinline__ LdsView<SCENE_LDS> stage_lds(const MtsgLaunch &L, uint32_t *lds) {
    const MtsgDeviceScene &S = L.scene;
    const uint32_t tabWords = L.lds_dims * L.nibbles * 16;
    for (uint32_t i = threadIdx.x; i < tabWords; i += BLOCK) {
        const uint32_t d = i / (L.nibbles * 16), r = i % (L.nibbles * 16);
        lds[i] = L.sobol_nib[(size_t)d * MTSG_NIBBLES * 16 + r];
    }
    stage_lut(L, lds + tabWords);
    const uint32_t base2 = tabWords + MTSG_LUT_WORDS;
    uint32_t sceneWords = 0;
    if (SCENE_LDS) {
        const uint32_t nodeWords = L.num_nodes * 16, triWords = S.num_prims * 12;
        const uint32_t *gn = reinterpret_cast<const uint32_t *>(S.nodes);
        const uint32_t *gt = reinterpret_cast<const uint32_t *>(S.tris);
        for (uint32_t i = threadIdx.x; i < nodeWords; i += BLOCK) lds[base2 + i] = gn[i];
        for (uint32_t i = threadIdx.x; i < triWords; i += BLOCK) lds[base2 + nodeWords + i] = gt[i];
        sceneWords = nodeWords + triWords;
        // the vertices' triangle data: prim_vtx, dpdu, face normals, positions, normals, shape records
        const uint32_t np = S.num_prims, nv = L.num_verts, ns = L.num_shapes * (sizeof(MtsgShape) / 4);
        const uint32_t *srcs[6] = {S.prim_vtx, reinterpret_cast<const uint32_t *>(S.dpdu),
                                   reinterpret_cast<const uint32_t *>(L.face_n),
                                   reinterpret_cast<const uint32_t *>(S.positions),
                                   reinterpret_cast<const uint32_t *>(S.normals),
                                   reinterpret_cast<const uint32_t *>(S.shapes)};
        const uint32_t lens[6] = {4 * np, 3 * np, 3 * np, 3 * nv, 3 * nv, ns};
        for (int a = 0; a < 6; ++a) {
            for (uint32_t i = threadIdx.x; i < lens[a]; i += BLOCK) lds[base2 + sceneWords + i] = srcs[a][i];
            sceneWords += lens[a];
        }
    }
    __syncthreads();
    return lds_view<SCENE_LDS>(L, lds);
}

// the pointers into the staged LDS (and the scene buffers it mirrors), derived
// from the launch record alone: the persistent megakernel re-derives them per
// bounce from launch_fresh() instead of holding them live across it
template <bool SCENE_LDS>
__device__ __forceinline__ LdsView<SCENE_LDS> lds_view(const MtsgLaunch &L, uint32_t *lds) {
    const MtsgDeviceScene &S = L.scene;
    const uint32_t tabWords = L.lds_dims * L.nibbles * 16;
    const uint32_t base2 = tabWords + MTSG_LUT_WORDS;
    uint32_t sceneWords = 0;
    if (SCENE_LDS) {
        sceneWords = L.num_nodes * 16 + S.num_prims * 12 + 4 * S.num_prims + 6 * S.num_prims + 3 * L.num_verts +
                     3 * L.num_verts + L.num_shapes * (uint32_t)(sizeof(MtsgShape) / 4);
    }
    LdsView<SCENE_LDS> v;
    v.ycolTab = (lds_u32 *)(lds + tabWords);
    // base2 and the node array size are multiples of 4 words: 16-byte aligned (ds_read_b128)
    v.nodes = (lds_node *)__builtin_assume_aligned((const void *)(lds + base2), 16);
    v.tris = (lds_tri *)__builtin_assume_aligned((const void *)(lds + base2 + L.num_nodes * 16), 16);
    // triangle data of hit records and emitter samples (HitSrc)
    if constexpr (SCENE_LDS) {
        const uint32_t np = S.num_prims, nv = L.num_verts;
        lds_u32 *b = (lds_u32 *)(lds + base2 + L.num_nodes * 16 + np * 12);
        v.hs.pv = b;
        v.hs.dpdu = (lds_f32 *)(b + 4 * np);
        v.hs.fn = (lds_f32 *)(b + 7 * np);
        v.hs.pos = (lds_f32 *)(b + 10 * np);
        v.hs.nrm = (lds_f32 *)(b + 10 * np + 3 * nv);
        v.hs.shapes = (lds_shape *)(b + 10 * np + 6 * nv);
    } else {
        v.hs.pv = (glb_u32 *)S.prim_vtx;
        v.hs.dpdu = (glb_f32 *)S.dpdu;
        v.hs.pos = (glb_f32 *)S.positions;
        v.hs.nrm = (glb_f32 *)S.normals;
        v.hs.shapes = (glb_shape *)S.shapes;
    }
    v.SC.lds = (lds_u32 *)lds;
    v.SC.glob = (glb_u32 *)L.sobol_nib;
    v.SC.lds_dims = L.lds_dims;
    v.SC.nibbles = L.nibbles;
    v.SC.scramble = L.scramble;
    v.SC.indep = L.sampler != MTSG_SAMPLER_SOBOL;
    v.SC.replay = L.replay != 0;
#ifndef MTSG_NO_SOBOL_PAIRS   // (A/B builds: the draws as they were)
    v.SC.tight = SCENE_LDS;
#else
    v.SC.tight = false;
#endif
    v.SC.sfmt = L.sfmt;
    v.stackBase = base2 + sceneWords;
    return v;
}
