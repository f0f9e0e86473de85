// scene_build_impl.h -- what the host configure units share: the stages mtsg_configure_scene
// (scene_build.cpp) runs in order, and the state they hand on.  Private to
//   configure_sensor.cpp  configure_bsdf.cpp  configure_emitter.cpp  configure_shape.cpp
//   bvh_build.cpp  scene_build.cpp
#pragma once
#include <cfloat>

#include "host_math.h"
#include "scene_build.h"

namespace mtsg_host {

struct BBox {
    float lo[3], hi[3];
    void reset() { for (int a = 0; a < 3; ++a) { lo[a] = FLT_MAX; hi[a] = -FLT_MAX; } }
    void grow(const BBox &b) { for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], b.lo[a]); hi[a] = std::max(hi[a], b.hi[a]); } }
    void growp(const float *p) { for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], p[a]); hi[a] = std::max(hi[a], p[a]); } }
    float area() const {
        float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        if (dx < 0) return 0;
        return 2.0f * (dx * dy + dy * dz + dz * dx);
    }
};

struct BuildPrim { BBox box; float c[3]; uint32_t id; };

// What crosses the stages of one mtsg_configure_scene call, next to the HostScene itself.
struct SceneBuild {
    // primitives (a triangle, or one analytic shape) and mesh vertices of the whole scene.
    // configure_shapes counts them first; its per-shape functions and build_bvh read them
    uint32_t prims = 0, verts = 0;
    // first free vertex / primitive: the shape being configured starts there.
    // Written and read by configure_shapes alone, one shape after the other
    uint32_t voff = 0, poff = 0;
    // per global primitive its box and centroid.  configure_shapes (add_prim) writes, build_bvh reads
    std::vector<BuildPrim> bp;
    // per global primitive its TriAccel record.  configure_shapes writes; build_bvh copies them
    // into HostScene::tris in leaf order
    std::vector<MtsgTri> tacc;
    // bounds of every primitive box.  configure_shapes (add_prim) grows them; scene_bounds
    // enlarges them into HostScene::aabb_min / aabb_max
    float amin[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, amax[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
};

// The stages, in the order mtsg_configure_scene runs them.  Those that can refuse a scene
// return MTSGPU_OK or an error code with its message in `err`.
int configure_sensor(const mtsgpu_sensor_desc &s, HostScene &S, std::string &err);    // configure_sensor.cpp
int configure_bsdfs(const mtsgpu_scene_desc &D, HostScene &S, std::string &err);      // configure_bsdf.cpp
int configure_emitters(const mtsgpu_scene_desc &D, HostScene &S, std::string &err);   // configure_emitter.cpp
int configure_shapes(const mtsgpu_scene_desc &D, HostScene &S, SceneBuild &B, std::string &err);   // configure_shape.cpp
void emitter_cdf(HostScene &S);                                                       // configure_emitter.cpp
void scene_bounds(const mtsgpu_scene_desc &D, SceneBuild &B, HostScene &S);           // configure_emitter.cpp
int build_bvh(SceneBuild &B, HostScene &S, std::string &err);                         // bvh_build.cpp

}  // namespace mtsg_host
