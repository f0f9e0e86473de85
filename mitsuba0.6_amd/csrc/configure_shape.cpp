// configure_shape.cpp -- the shapes' constructors and configure():
//   meshes        TriMesh::configure / computeNormals / computeUVTangents /
//                 prepareSamplingTable (librender/trimesh.cpp:361-739)
//   TriAccel      skdtree.cpp:74-109, render/triaccel.h:58-90
//   rectangle, disk, sphere   shapes/rectangle.cpp:80-119, disk.cpp:83-130, sphere.cpp:108-133
//   default BSDFs Shape::configure (librender/shape.cpp:48-75)
#include "scene_build_impl.h"

// Matrix4x4::invert (matrix.inl:138-193) of a row-major 4x4: the inverse a Transform built
// from a matrix carries (transform.h:54-60); false for a singular matrix
bool mtsg_invert4(const float *m16, float *inv16) {
    mtsg_host::M4 a, r;
    std::memcpy(&a.m[0][0], m16, sizeof a.m);
    if (!mtsg_host::invert(a, r)) return false;
    std::memcpy(inv16, &r.m[0][0], sizeof r.m);
    return true;
}

// fill_hit's face normal (dhit.h; skdtree.h:355-360): cross(p1 - p0, p2 - p0) as dmath.h
// forms it, its length by a correctly rounded sqrt, 1 / length, three products; left
// as it is when it is all zero.  (This unit is built with -ffp-contract=off.)
void mtsg_face_normal(const float *p0, const float *p1, const float *p2, float *n) {
    const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
    const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
    float x = (ay * bz) - (az * by), y = (az * bx) - (ax * bz), z = (ax * by) - (ay * bx);
    const float length = std::sqrt(x * x + y * y + z * z);
    if (!(x == 0 && y == 0 && z == 0)) {
        const float r = 1.0f / length;
        x *= r; y *= r; z *= r;
    }
    n[0] = x; n[1] = y; n[2] = z;
}

namespace mtsg_host {
namespace {

// Rectangle / Disk / Sphere constructors + configure() (rectangle.cpp:80-119,
// disk.cpp:83-130, sphere.cpp:108-133) and getAABB()
int configure_analytic(const mtsgpu_mesh_desc &m, MtsgAnalytic &a, BBox &box, std::string &err) {
    std::memset(&a, 0, sizeof a);
    a.type = m.shape_type;
    Xf o2w;
    auto grow = [&](V p) {
        const float q[3] = {p.x, p.y, p.z};
        box.growp(q);
    };
    auto to_world = [&](Xf &out) {   // 'toWorld' as the reference's Transform
        if (desc_transform(m.to_world, m.to_world_inv, out)) return MTSGPU_OK;
        err = "Singular matrix in Matrix::invert";
        return MTSGPU_EINVAL;
    };
    box.reset();
    if (m.shape_type == MTSGPU_SHAPE_RECTANGLE || m.shape_type == MTSGPU_SHAPE_DISK) {
        if (to_world(o2w)) return MTSGPU_EINVAL;
        if (m.flip_normals) o2w = compose(o2w, scale(1, 1, -1));   // (prependScale: m_transform * scale)
        if (m.shape_type == MTSGPU_SHAPE_RECTANGLE) {
            const V dpdu = xf_vec(o2w.t, v(2, 0, 0)), dpdv = xf_vec(o2w.t, v(0, 2, 0));
            const V n = normalize(xf_normal(o2w.inv, v(0, 0, 1)));
            put3(a.dpdu, dpdu); put3(a.dpdv, dpdv); put3(a.n, n);
            put3(a.fs, normalize(dpdu)); put3(a.ft, normalize(dpdv));
            a.inv_area = 1.0f / (length(dpdu) * length(dpdv));
            if (std::fabs(dot(normalize(dpdu), normalize(dpdv))) > 1e-4f) {
                err = "Error: 'toWorld' transformation contains shear!"; return MTSGPU_EINVAL;
            }
            grow(xf_point(o2w.t, v(-1, -1, 0))); grow(xf_point(o2w.t, v(1, -1, 0)));
            grow(xf_point(o2w.t, v(1, 1, 0))); grow(xf_point(o2w.t, v(-1, 1, 0)));
        } else {
            const V dpdu = xf_vec(o2w.t, v(1, 0, 0)), dpdv = xf_vec(o2w.t, v(0, 1, 0));
            if (std::fabs(dot(normalize(dpdu), normalize(dpdv))) > 1e-3f) {
                err = "Error: 'toWorld' transformation contains shear!"; return MTSGPU_EINVAL;
            }
            if (std::fabs(length(dpdu) / length(dpdv) - 1) > 1e-3f) {
                err = "Error: 'toWorld' transformation contains a non-uniform scale!"; return MTSGPU_EINVAL;
            }
            a.inv_area = 1.0f / (kPi * length(dpdu) * length(dpdu));
            put3(a.n, normalize(xf_normal(o2w.inv, v(0, 0, 1))));
            grow(xf_point(o2w.t, v(1, 0, 0))); grow(xf_point(o2w.t, v(-1, 0, 0)));
            grow(xf_point(o2w.t, v(0, 1, 0))); grow(xf_point(o2w.t, v(0, -1, 0)));
        }
    } else if (m.shape_type == MTSGPU_SHAPE_SPHERE) {
        o2w = translate(m.center[0], m.center[1], m.center[2]);
        float radius = m.radius;
        if (m.has_to_world) {
            Xf T;
            if (to_world(T)) return MTSGPU_EINVAL;
            const float r = length(xf_vec(T.t, v(1, 0, 0)));
            const float ir = 1 / r;
            o2w = compose(compose(T, scale(ir, ir, ir)), o2w);
            radius *= r;
        }
        a.flip = m.flip_normals ? 1 : 0;
        const V c = xf_point(o2w.t, v(0, 0, 0));
        put3(a.center, c);
        a.radius = radius;
        a.inv_area = 1 / (4 * kPi * radius * radius);
        if (radius <= 0) { err = "Cannot create spheres of radius <= 0"; return MTSGPU_EINVAL; }
        grow(c - v(radius, radius, radius));
        grow(c + v(radius, radius, radius));
    } else {
        err = "unsupported shape type"; return MTSGPU_EINVAL;
    }
    put16(a.to_world, o2w.t);
    put16(a.to_obj, o2w.inv);
    return MTSGPU_OK;
}

// ---- what every shape does, whatever its kind -------------------------------
// the shape's record: its emitter, and its BSDF or the default one of Shape::configure
// (shape.cpp:48-70: record nb, black, for an emitter; nb + 1, 0.5, otherwise)
int shape_record(const mtsgpu_scene_desc &D, uint32_t si, HostScene &S, std::string &err) {
    const mtsgpu_mesh_desc &m = D.meshes[si];
    const int nb = (int)D.num_bsdfs;
    if (m.emitter >= (int)D.num_emitters) { err = "emitter index out of range"; return MTSGPU_EINVAL; }
    if (m.bsdf >= nb) { err = "bsdf index out of range"; return MTSGPU_EINVAL; }
    MtsgShape &sh = S.shapes[si];
    std::memset(&sh, 0, sizeof sh);
    sh.emitter = m.emitter;
    sh.bsdf = m.bsdf >= 0 ? m.bsdf : (m.emitter >= 0 ? nb : nb + 1);
    sh.kind = m.shape_type;
    sh.analytic = -1;
    return MTSGPU_OK;
}

// primitive p's box: its centroid for the BVH builder, and the scene bounds grown by it
void add_prim(SceneBuild &B, uint32_t p, const BBox &box) {
    BuildPrim &q = B.bp[p];
    q.id = p;
    q.box = box;
    for (int a = 0; a < 3; ++a) {
        q.c[a] = 0.5f * (box.lo[a] + box.hi[a]);
        B.amin[a] = std::min(B.amin[a], box.lo[a]);
        B.amax[a] = std::max(B.amax[a], box.hi[a]);
    }
}

// the shape's area emitter takes primitives [first, first + count) (Shape::addChild: one emitter each)
int attach_emitter(const mtsgpu_mesh_desc &m, uint32_t si, uint32_t first, uint32_t count, HostScene &S,
                   std::string &err) {
    MtsgEmitter &e = S.emitters[m.emitter];
    if (e.shape >= 0) { err = "Tried to attach multiple emitters to a shape!"; return MTSGPU_EINVAL; }
    e.shape = (int)si;
    e.tri_first = first;
    e.tri_count = count;
    return MTSGPU_OK;
}

// one analytic primitive (ShapeKDTree: k = KNoTriangleFlag, skdtree.cpp:74-109)
int configure_analytic_shape(const mtsgpu_scene_desc &D, uint32_t si, HostScene &S, SceneBuild &B, std::string &err) {
    const mtsgpu_mesh_desc &m = D.meshes[si];
    int rc;
    if ((rc = shape_record(D, si, S, err))) return rc;
    MtsgShape &sh = S.shapes[si];
    sh.has_uv = 1;
    sh.analytic = (int32_t)S.analytic.size();
    MtsgAnalytic a;
    BBox box;
    if ((rc = configure_analytic(m, a, box, err))) return rc;
    S.analytic.push_back(a);
    const uint32_t p = B.poff;
    S.prim_vtx[4 * p] = S.prim_vtx[4 * p + 1] = S.prim_vtx[4 * p + 2] = 0;
    S.prim_vtx[4 * p + 3] = si;
    S.dpdu[3 * p] = S.dpdu[3 * p + 1] = S.dpdu[3 * p + 2] = 0.0f;
    MtsgTri &ta = B.tacc[p];
    std::memset(&ta, 0, sizeof ta);
    ta.k = MTSG_K_ANALYTIC;
    std::memcpy(&ta.n_u, &sh.analytic, sizeof(float));
    ta.prim = p;
    ta.shape = si;
    add_prim(B, p, box);
    if (m.emitter >= 0) {
        if ((rc = attach_emitter(m, si, p, 1, S, err))) return rc;
        S.emitters[m.emitter].cdf_offset = 0;
        S.emitters[m.emitter].inv_area = a.inv_area;
    }
    B.poff += 1;
    return MTSGPU_OK;
}

// ---- triangle meshes ---------------------------------------------------------
// EAnisotropic (roughconductor.cpp:229-231) without texcoords: computeUVTangents error (trimesh.cpp:685-691)
// (through twosided: its combined type carries the nested EAnisotropic)
// the leaves below BSDF record `i`: through twosided and the combinators' chain (configure_bsdf.cpp)
void leaf_bsdfs(const HostScene &S, int i, std::vector<int> &out) {
    const MtsgBsdf &b = S.bsdfs[i];
    if (b.type == MTSGPU_BSDF_TWOSIDED) {
        leaf_bsdfs(S, b.nested[0], out);
        leaf_bsdfs(S, b.nested[1], out);
    } else if (b.type == MTSGPU_BSDF_MIXTURE || b.type == MTSGPU_BSDF_BLEND || b.type == MTSGPU_BSDF_MASK) {
        const MtsgCombo &c = S.combos[b.nested[0]];
        for (int k = 0; k < c.n; ++k) leaf_bsdfs(S, c.child[k], out);
    } else {
        out.push_back(i);
    }
}

int check_tangents(const mtsgpu_scene_desc &D, const mtsgpu_mesh_desc &m, const HostScene &S, std::string &err) {
    bool aniso = false;
    if (m.bsdf >= 0) {
        std::vector<int> cand;
        leaf_bsdfs(S, m.bsdf, cand);
        for (int c : cand) {
            const mtsgpu_bsdf_desc &cb = D.bsdfs[c];
            if ((cb.type == MTSGPU_BSDF_ROUGHCONDUCTOR || cb.type == MTSGPU_BSDF_ROUGHDIELECTRIC) &&
                fmax_std(cb.alpha_u, 1e-4f) != fmax_std(cb.alpha_v, 1e-4f))
                aniso = true;
        }
    }
    if (!m.texcoords && aniso) {
        err = "computeUVTangents(): texture coordinates are required to generate tangent vectors. If you "
              "want to render with an anisotropic material, please make sure that all associated shapes "
              "have valid texture coordinates.";
        return MTSGPU_EINVAL;
    }
    return MTSGPU_OK;
}

// TriMesh::computeNormals (trimesh.cpp:608-681): face normals (flipped by swapping two
// indices), the supplied normals, or angle-weighted ones; false: the mesh has no vertex normals
bool compute_normals(const mtsgpu_mesh_desc &m, const std::vector<V> &P, std::vector<uint32_t> &idx, std::vector<V> &N) {
    const uint32_t nv = m.num_vertices, nt = m.num_triangles;
    if (m.face_normals) {
        if (m.flip_normals)
            for (uint32_t t = 0; t < nt; ++t) std::swap(idx[3 * t], idx[3 * t + 1]);
        return false;
    }
    if (m.normals) {
        N.resize(nv);
        for (uint32_t k = 0; k < nv; ++k) {
            N[k] = v(m.normals[3 * k], m.normals[3 * k + 1], m.normals[3 * k + 2]);
            if (m.flip_normals) N[k] = N[k] * -1;
        }
        return true;
    }
    N.assign(nv, v(0, 0, 0));
    for (uint32_t t = 0; t < nt; t++) {
        V n = v(0, 0, 0);
        for (int j = 0; j < 3; ++j) {
            const V v0 = P[idx[3 * t + j]], v1 = P[idx[3 * t + (j + 1) % 3]], v2 = P[idx[3 * t + (j + 2) % 3]];
            const V sideA = v1 - v0, sideB = v2 - v0;
            if (j == 0) {
                n = cross(sideA, sideB);
                float len = length(n);
                if (len == 0) break;
                n = vdiv(n, len);
            }
            float angle = unit_angle(normalize(sideA), normalize(sideB));
            N[idx[3 * t + j]] = N[idx[3 * t + j]] + n * angle;
        }
    }
    for (uint32_t k = 0; k < nv; k++) {
        float len = length(N[k]);
        if (m.flip_normals) len *= -1;
        if (len != 0) N[k] = vdiv(N[k], len);
        else N[k] = v(1, 0, 0);
    }
    return true;
}

// TriMesh::computeUVTangents (trimesh.cpp:683-739) of triangle (i0, i1, i2); dpdu = p1 - p0
// without texcoords (skdtree.h:376-382)
V uv_tangent(const float *uv, const std::vector<V> &P, uint32_t i0, uint32_t i1, uint32_t i2) {
    const V v0 = P[i0], v1 = P[i1], v2 = P[i2];
    if (!uv) return v1 - v0;
    V dp = v(0, 0, 0);
    const V dP1 = v1 - v0, dP2 = v2 - v0;
    const float du1 = uv[2 * i1] - uv[2 * i0], dv1 = uv[2 * i1 + 1] - uv[2 * i0 + 1];
    const float du2 = uv[2 * i2] - uv[2 * i0], dv2 = uv[2 * i2 + 1] - uv[2 * i0 + 1];
    const V n = cross(dP1, dP2);
    const float len = length(n);
    if (len != 0) {
        const float det = du1 * dv2 - dv1 * du2;
        if (det == 0) {
            V b, c;
            coordinate_system(vdiv(n, len), b, c);
            dp = b;
        } else {
            const float invDet = 1.0f / det;
            dp = (dP1 * dv2 - dP2 * dv1) * invDet;
        }
    }
    return dp;
}

// TriAccel::load (triaccel.h:58-90) of triangle (A, B, C); k = 3: degenerate
void tri_accel(V A, V B, V C, MtsgTri &ta) {
    std::memset(&ta, 0, sizeof ta);
    static const int waldModulo[4] = {1, 2, 0, 1};
    const V b = C - A, c = B - A, Nn = cross(c, b);
    ta.k = 0;
    for (int j = 0; j < 3; j++)
        if (std::fabs(at(Nn, j)) > std::fabs(at(Nn, (int)ta.k))) ta.k = (uint32_t)j;
    const int u = waldModulo[ta.k], w = waldModulo[ta.k + 1];
    const float n_k = at(Nn, (int)ta.k), denom = at(b, u) * at(c, w) - at(b, w) * at(c, u);
    if (denom == 0) {
        ta.k = 3;
        return;
    }
    ta.n_u = at(Nn, u) / n_k;
    ta.n_v = at(Nn, w) / n_k;
    ta.n_d = dot(A, Nn) / n_k;
    ta.b_nu = at(b, u) / denom;
    ta.b_nv = -at(b, w) / denom;
    ta.a_u = at(A, u);
    ta.a_v = at(A, w);
    ta.c_nu = at(c, w) / denom;
    ta.c_nv = -at(c, u) / denom;
}

// TriMesh::prepareSamplingTable (trimesh.cpp:389-404), DiscreteDistribution (pmf.h): the
// emitting mesh's area CDF, appended to area_cdf, and its inverse surface area
void sampling_table(const std::vector<V> &P, const std::vector<uint32_t> &idx, uint32_t nt, MtsgEmitter &e,
                    std::vector<float> &area_cdf) {
    e.cdf_offset = (uint32_t)area_cdf.size();
    std::vector<float> cdf(nt + 1);
    cdf[0] = 0.0f;
    for (uint32_t t = 0; t < nt; ++t) {
        const V p0 = P[idx[3 * t]], p1 = P[idx[3 * t + 1]], p2 = P[idx[3 * t + 2]];
        cdf[t + 1] = cdf[t] + 0.5f * length(cross(p1 - p0, p2 - p0));   // Triangle::surfaceArea
    }
    const float sum = cdf[nt];
    if (sum > 0) {
        const float norm = 1.0f / sum;
        for (uint32_t t = 1; t < nt + 1; ++t) cdf[t] *= norm;
        cdf[nt] = 1.0f;
    }
    e.inv_area = 1.0f / sum;
    area_cdf.insert(area_cdf.end(), cdf.begin(), cdf.end());
}

// the mesh's vertices into the scene's arrays at B.voff (normals and UVs where it has them)
void store_vertices(const mtsgpu_mesh_desc &m, const std::vector<V> &P, const std::vector<V> &N, bool hasNormals,
                    const SceneBuild &B, HostScene &S) {
    const uint32_t nv = m.num_vertices, voff = B.voff;
    if (m.texcoords) {
        if (S.texcoords.empty()) S.texcoords.assign((size_t)B.verts * 2, 0.0f);
        std::memcpy(&S.texcoords[2 * (size_t)voff], m.texcoords, sizeof(float) * 2 * (size_t)nv);
    }
    for (uint32_t k = 0; k < nv; ++k) {
        S.positions[3 * (voff + k)] = P[k].x; S.positions[3 * (voff + k) + 1] = P[k].y; S.positions[3 * (voff + k) + 2] = P[k].z;
        if (hasNormals) {
            S.normals[3 * (voff + k)] = N[k].x; S.normals[3 * (voff + k) + 1] = N[k].y; S.normals[3 * (voff + k) + 2] = N[k].z;
        }
    }
}

// TriMesh::configure (trimesh.cpp:361-387) of mesh si, and its triangles as kd-tree primitives
int configure_trimesh(const mtsgpu_scene_desc &D, uint32_t si, HostScene &S, SceneBuild &B, std::string &err) {
    const mtsgpu_mesh_desc &m = D.meshes[si];
    const uint32_t nv = m.num_vertices, nt = m.num_triangles, voff = B.voff, poff = B.poff;
    std::vector<V> P(nv), N;
    for (uint32_t k = 0; k < nv; ++k) P[k] = v(m.positions[3 * k], m.positions[3 * k + 1], m.positions[3 * k + 2]);
    std::vector<uint32_t> idx(m.indices, m.indices + 3 * (size_t)nt);
    for (uint32_t k = 0; k < 3 * nt; ++k)
        if (idx[k] >= nv) { err = "triangle index out of range"; return MTSGPU_EINVAL; }
    int rc;
    if ((rc = shape_record(D, si, S, err))) return rc;
    if ((rc = check_tangents(D, m, S, err))) return rc;
    const bool hasNormals = compute_normals(m, P, idx, N);
    MtsgShape &sh = S.shapes[si];
    sh.has_normals = hasNormals ? 1 : 0;
    // (read by the kernels that form its.uv: the EXT variants and the field pass)
    sh.has_uv = m.texcoords ? 1 : 0;
    store_vertices(m, P, N, hasNormals, B, S);
    for (uint32_t t = 0; t < nt; ++t) {
        const uint32_t i0 = idx[3 * t], i1 = idx[3 * t + 1], i2 = idx[3 * t + 2];
        const uint32_t p = poff + t;
        put3(&S.dpdu[3 * p], uv_tangent(m.texcoords, P, i0, i1, i2));
        S.prim_vtx[4 * p] = voff + i0; S.prim_vtx[4 * p + 1] = voff + i1; S.prim_vtx[4 * p + 2] = voff + i2;
        S.prim_vtx[4 * p + 3] = si;
        mtsg_face_normal(&S.positions[3 * (size_t)(voff + i0)], &S.positions[3 * (size_t)(voff + i1)],
                         &S.positions[3 * (size_t)(voff + i2)], &S.face_n[3 * (size_t)p]);
        MtsgTri &ta = B.tacc[p];
        tri_accel(P[i0], P[i1], P[i2], ta);
        ta.prim = p;
        ta.shape = si;
        BBox box;
        box.reset();
        box.growp(&S.positions[3 * (size_t)(voff + i0)]);
        box.growp(&S.positions[3 * (size_t)(voff + i1)]);
        box.growp(&S.positions[3 * (size_t)(voff + i2)]);
        add_prim(B, p, box);
    }
    if (m.emitter >= 0) {
        if ((rc = attach_emitter(m, si, poff, nt, S, err))) return rc;
        sampling_table(P, idx, nt, S.emitters[m.emitter], S.area_cdf);
    }
    B.voff += nv;
    B.poff += nt;
    return MTSGPU_OK;
}

}  // namespace

// Every shape's record, vertices and primitives in shape order; B receives the primitives'
// boxes and TriAccel records for the bounds and the BVH
int configure_shapes(const mtsgpu_scene_desc &D, HostScene &S, SceneBuild &B, std::string &err) {
    for (uint32_t i = 0; i < D.num_meshes; ++i) {
        const mtsgpu_mesh_desc &m = D.meshes[i];
        if (m.shape_type != MTSGPU_SHAPE_TRIMESH) { B.prims += 1; continue; }
        if (m.num_triangles == 0 || !m.positions || !m.indices) { err = "Encountered an empty triangle mesh!"; return MTSGPU_EINVAL; }
        B.prims += m.num_triangles; B.verts += m.num_vertices;
    }
    S.positions.resize((size_t)B.verts * 3);
    S.normals.assign((size_t)B.verts * 3, 0.0f);
    S.prim_vtx.resize((size_t)B.prims * 4);
    S.dpdu.resize((size_t)B.prims * 3);
    S.face_n.assign((size_t)B.prims * 3, 0.0f);
    S.shapes.resize(D.num_meshes);
    B.bp.resize(B.prims);
    B.tacc.resize(B.prims);
    for (uint32_t si = 0; si < D.num_meshes; ++si) {
        const int rc = D.meshes[si].shape_type != MTSGPU_SHAPE_TRIMESH ? configure_analytic_shape(D, si, S, B, err)
                                                                      : configure_trimesh(D, si, S, B, err);
        if (rc) return rc;
    }
    for (const MtsgEmitter &e : S.emitters)
        if (e.type == MTSGPU_EMITTER_AREA && e.shape < 0) { err = "area emitter without a shape"; return MTSGPU_EINVAL; }
    return MTSGPU_OK;
}

}  // namespace mtsg_host
