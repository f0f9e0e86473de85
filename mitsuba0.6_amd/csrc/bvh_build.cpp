// bvh_build.cpp -- the acceleration structure: a binned-SAH BVH2 instead of the reference's
// SAH kd-tree (traversal returns the same closest hit), its half-float nodes,
// the triangles in leaf order, and the 4-wide collapse of the host export.
#include <cstdlib>

#include "scene_build_impl.h"

namespace mtsg_host {
namespace {

const uint32_t kMaxDepth = 28;   // traversal stack (LDS) holds < 32 entries

// SAH knobs (A/B only; results never depend on them): MTSGPU_SAH_BINS (128: C3 +3.4%,
// C4 +0.7% over 32, profiles/r03_ab_sah_C*.log),
// MTSGPU_SAH_CI (cost of a triangle test per node visit, 1), MTSGPU_LEAF_MAX (8, <= 15)
int env_int(const char *k, int def, int lo, int hi) {
    const char *v = std::getenv(k);
    return v ? std::max(lo, std::min(hi, std::atoi(v))) : def;
}
float env_float(const char *k, float def) {
    const char *v = std::getenv(k);
    return v ? (float)std::atof(v) : def;
}

struct Builder {
    std::vector<BuildPrim> &prims;
    std::vector<MtsgNode> &nodes;
    std::vector<uint32_t> order;
    float absEps;
    uint32_t maxDepth = 0;
    const int nbins = env_int("MTSGPU_SAH_BINS", 128, 4, 1024);
    const float ci = env_float("MTSGPU_SAH_CI", 1.0f);
    const uint32_t leafMax = (uint32_t)env_int("MTSGPU_LEAF_MAX", MTSG_LEAF_MAX, 1, 15);
    // the binned SAH's scratch, sized once and reused by every build() call
    std::vector<BBox> bb, lb;
    std::vector<uint32_t> bc, lc;
    explicit Builder(std::vector<BuildPrim> &p, std::vector<MtsgNode> &n)
        : prims(p), nodes(n), bb(nbins), lb(nbins), bc(nbins), lc(nbins) {}

    void inflate(BBox &b) const {
        for (int a = 0; a < 3; ++a) {
            float e = (b.hi[a] - b.lo[a]) * 1e-4f + 1e-6f * (std::fabs(b.lo[a]) + std::fabs(b.hi[a])) + absEps;
            b.lo[a] -= e; b.hi[a] += e;
        }
    }
    BBox bounds(uint32_t first, uint32_t count) const {
        BBox b; b.reset();
        for (uint32_t i = first; i < first + count; ++i) b.grow(prims[order[i]].box);
        return b;
    }
    // returns child reference for the range
    int32_t build(uint32_t first, uint32_t count, uint32_t depth) {
        maxDepth = std::max(maxDepth, depth);
        if (count <= 2 || (count <= leafMax && depth >= kMaxDepth - 1))
            return mtsg_leaf_ref(first, count);
        // switch to median splits early enough that depth stays <= kMaxDepth
        uint32_t lg = 0;
        while ((2u << lg) * 2 < count) ++lg;   // ~log2(count / 2)
        const bool forceMedian = depth + lg + 2 >= kMaxDepth;
        BBox cb; cb.reset();
        for (uint32_t i = first; i < first + count; ++i) cb.growp(prims[order[i]].c);
        const int NB = nbins;
        float bestCost = FLT_MAX; int bestAxis = -1, bestSplit = -1;
        const BBox nb = bounds(first, count);
        const float leafCost = ci * (float)count;
        for (int axis = 0; axis < 3; ++axis) {
            const float ext = cb.hi[axis] - cb.lo[axis];
            if (!(ext > 0)) continue;
            std::fill(bc.begin(), bc.end(), 0u);
            for (int i = 0; i < NB; ++i) bb[i].reset();
            const float k = NB / ext;
            for (uint32_t i = first; i < first + count; ++i) {
                const BuildPrim &p = prims[order[i]];
                int bi = std::min(NB - 1, (int)((p.c[axis] - cb.lo[axis]) * k));
                bb[bi].grow(p.box); bc[bi]++;
            }
            BBox acc; acc.reset(); uint32_t n = 0;
            for (int i = 0; i < NB; ++i) { acc.grow(bb[i]); n += bc[i]; lb[i] = acc; lc[i] = n; }
            acc.reset(); n = 0;
            for (int i = NB - 1; i > 0; --i) {
                acc.grow(bb[i]); n += bc[i];
                if (lc[i - 1] == 0 || n == 0) continue;
                const float cost = 1.0f + ci * (lb[i - 1].area() * lc[i - 1] + acc.area() * n) / std::max(nb.area(), 1e-30f);
                if (cost < bestCost) { bestCost = cost; bestAxis = axis; bestSplit = i; }
            }
        }
        uint32_t mid;
        if (bestAxis < 0 || (count <= leafMax && bestCost >= leafCost)) {
            if (count <= leafMax) return mtsg_leaf_ref(first, count);
            // degenerate centroids: median split on index order
            mid = first + count / 2;
        } else {
            const float ext = cb.hi[bestAxis] - cb.lo[bestAxis];
            const float k = NB / ext;
            auto it = std::partition(order.begin() + first, order.begin() + first + count, [&](uint32_t id) {
                int bi = std::min(NB - 1, (int)((prims[id].c[bestAxis] - cb.lo[bestAxis]) * k));
                return bi < bestSplit;
            });
            mid = (uint32_t)(it - order.begin());
            if (mid == first || mid == first + count) mid = first + count / 2;
        }
        if (forceMedian) {
            // keep the tree shallow: median split on the widest centroid axis
            int axis = 0;
            for (int a = 1; a < 3; ++a) if (cb.hi[a] - cb.lo[a] > cb.hi[axis] - cb.lo[axis]) axis = a;
            mid = first + count / 2;
            std::nth_element(order.begin() + first, order.begin() + mid, order.begin() + first + count,
                             [&](uint32_t x, uint32_t y) { return prims[x].c[axis] < prims[y].c[axis]; });
        }
        const uint32_t id = (uint32_t)nodes.size();
        nodes.push_back(MtsgNode());
        BBox b0 = bounds(first, mid - first), b1 = bounds(mid, first + count - mid);
        inflate(b0); inflate(b1);
        const int32_t c0 = build(first, mid - first, depth + 1);
        const int32_t c1 = build(mid, first + count - mid, depth + 1);
        MtsgNode &n = nodes[id];
        n.c0lox = b0.lo[0]; n.c0hix = b0.hi[0]; n.c0loy = b0.lo[1]; n.c0hiy = b0.hi[1];
        n.c1lox = b1.lo[0]; n.c1hix = b1.hi[0]; n.c1loy = b1.lo[1]; n.c1hiy = b1.hi[1];
        n.c0loz = b0.lo[2]; n.c0hiz = b0.hi[2]; n.c1loz = b1.lo[2]; n.c1hiz = b1.hi[2];
        n.c0 = c0; n.c1 = c1; n.pad0 = n.pad1 = 0;
        return (int32_t)id;
    }
};

// x as a half rounded toward +inf (up) or -inf (down): BVH box bounds that never shrink
uint16_t half_outward(float x, bool up) {
    const uint16_t h = float_to_half(x);
    const float y = half_to_float(h);
    if (up ? !(y < x) : !(y > x)) return h;
    const bool neg = (h & 0x8000u) != 0;
    if (up) return neg ? (uint16_t)(h - 1) : (uint16_t)(h + 1);   // toward +inf (0x7bff + 1 = +inf)
    if ((h & 0x7fffu) == 0) return 0x8001u;                        // +0 -> the negative subnormal
    return neg ? (uint16_t)(h + 1) : (uint16_t)(h - 1);
}

// MtsgNode -> MtsgHNode (layout.h): same children, half boxes rounded outward
MtsgHNode half_node(const MtsgNode &n) {
    const float lo[6] = {n.c0lox, n.c0loy, n.c1lox, n.c1loy, n.c0loz, n.c1loz};
    const float hi[6] = {n.c0hix, n.c0hiy, n.c1hix, n.c1hiy, n.c0hiz, n.c1hiz};
    MtsgHNode h;
    for (int k = 0; k < 6; ++k)
        h.box[k] = (uint32_t)half_outward(lo[k], false) | ((uint32_t)half_outward(hi[k], true) << 16);
    h.c0 = n.c0;
    h.c1 = n.c1;
    return h;
}

// the BVH2 `n2` collapsed to 4-wide nodes (layout.h MtsgQNode), depth-first
// with the root at 0: an inner BVH2 child is replaced by its two children
struct QCollapse {
    const std::vector<MtsgNode> &n2;
    std::vector<MtsgQNode> &q;
    uint32_t depth = 0;
    int32_t emit(int32_t ref, uint32_t level) {
        if (ref < 0) return ref;
        depth = std::max(depth, level);
        struct Kid { float lo[3], hi[3]; int32_t ref; } kids[4];
        int nk = 0;
        auto box = [](const MtsgNode &n, int c, Kid &k) {
            if (c == 0) {
                k.lo[0] = n.c0lox; k.hi[0] = n.c0hix; k.lo[1] = n.c0loy; k.hi[1] = n.c0hiy; k.lo[2] = n.c0loz; k.hi[2] = n.c0hiz;
                k.ref = n.c0;
            } else {
                k.lo[0] = n.c1lox; k.hi[0] = n.c1hix; k.lo[1] = n.c1loy; k.hi[1] = n.c1hiy; k.lo[2] = n.c1loz; k.hi[2] = n.c1hiz;
                k.ref = n.c1;
            }
        };
        const MtsgNode &n = n2[ref];
        for (int c = 0; c < 2; ++c) {
            Kid k;
            box(n, c, k);
            if (k.ref >= 0) {
                box(n2[k.ref], 0, kids[nk++]);
                box(n2[k.ref], 1, kids[nk++]);
            } else {
                kids[nk++] = k;
            }
        }
        const int32_t id = (int32_t)q.size();
        q.push_back(MtsgQNode());
        int32_t refs[4] = {0, 0, 0, 0};
        for (int j = 0; j < nk; ++j) refs[j] = emit(kids[j].ref, level + 1);
        MtsgQNode &out = q[id];
        for (int j = 0; j < 4; ++j) {
            for (int a = 0; a < 3; ++a)
                out.box[3 * j + a] = j < nk ? (uint32_t)half_outward(kids[j].lo[a], false) |
                                                  ((uint32_t)half_outward(kids[j].hi[a], true) << 16)
                                            : 0u;
            out.child[j] = refs[j];
        }
        return id;
    }
};

}  // namespace

// The BVH2 over B.bp (nodes, hnodes, bvh_depth) and the TriAccel records in its leaf order (tris)
int build_bvh(SceneBuild &B, HostScene &S, std::string &err) {
    const uint32_t prims = B.prims;
    Builder bld(B.bp, S.nodes);
    bld.order.resize(prims);
    for (uint32_t i = 0; i < prims; ++i) bld.order[i] = i;
    float diag = 0;
    for (int a = 0; a < 3; ++a) diag += (S.aabb_max[a] - S.aabb_min[a]) * (S.aabb_max[a] - S.aabb_min[a]);
    bld.absEps = 1e-7f * std::sqrt(diag) + 1e-30f;
    S.nodes.reserve(prims + 2);
    const int32_t rootRef = bld.build(0, prims, 0);   // the first inner node created is node 0
    if (rootRef < 0) {
        // whole scene in one leaf: a root node holding that leaf and an empty one
        BBox b = bld.bounds(0, prims);
        bld.inflate(b);
        MtsgNode n;
        n.c0lox = b.lo[0]; n.c0hix = b.hi[0]; n.c0loy = b.lo[1]; n.c0hiy = b.hi[1]; n.c0loz = b.lo[2]; n.c0hiz = b.hi[2];
        n.c1lox = n.c1hix = n.c1loy = n.c1hiy = n.c1loz = n.c1hiz = 0;
        n.c0 = rootRef; n.c1 = mtsg_leaf_ref(0, 0); n.pad0 = n.pad1 = 0;
        S.nodes.push_back(n);
    }
    S.bvh_depth = bld.maxDepth;
    if (bld.maxDepth + 1 >= 32) { err = "BVH too deep for the traversal stack"; return MTSGPU_EINVAL; }
    S.hnodes.resize(S.nodes.size());
    for (size_t i = 0; i < S.nodes.size(); ++i) S.hnodes[i] = half_node(S.nodes[i]);
    // triangles in leaf order
    S.tris.resize(prims);
    for (uint32_t i = 0; i < prims; ++i) S.tris[i] = B.tacc[bld.order[i]];
    return MTSGPU_OK;
}

}  // namespace mtsg_host

// the 4-wide collapse of the BVH2 for mtsgpu_bvh_host only (the device traverses
// the BVH2: the 4-wide traversal lost 5-6%)
void mtsg_build_qnodes(HostScene &S) {
    S.qnodes.clear();
    S.qnodes.reserve(S.nodes.size() / 2 + 2);
    mtsg_host::QCollapse qc{S.nodes, S.qnodes};
    qc.emit(0, 1);
    S.qnode_depth = qc.depth;
}
