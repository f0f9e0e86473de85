// configure_sensor.cpp -- the projective sensors' constructors and configure():
//   perspective   librender/sensor.cpp:95-107,239-305, sensors/perspective.cpp:126-163
//   thinlens      sensors/thinlens.cpp:124-193
//   orthographic, telecentric   sensors/orthographic.cpp:73-135, telecentric.cpp:74-153
#include "scene_build_impl.h"

namespace mtsg_host {
namespace {

// the film's sampleToCamera of projection `proj` (perspective.cpp:146-151, orthographic.cpp:
// 109-116; crop = film), the camera's clip planes and pixel size, and the camera-space
// steps dx / dy of one pixel
void film_setup(const mtsgpu_sensor_desc &s, const Xf &proj, MtsgCamera &cam) {
    const float aspect = (float)s.film_width / (float)s.film_height;
    Xf a = scale(1.0f / 1.0f, 1.0f / 1.0f, 1.0f);
    Xf b = translate(-0.0f, -0.0f, 0.0f);
    Xf c = scale(-0.5f, -0.5f * aspect, 1.0f);
    Xf d = translate(-1.0f, -1.0f / aspect, 0.0f);
    Xf camToSample = compose(compose(compose(compose(a, b), c), d), proj);
    const M4 &s2c = camToSample.inv;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            cam.sample_to_camera[i * 4 + j] = s2c.m[i][j];
            cam.to_world[i * 4 + j] = s.to_world[i * 4 + j];
        }
    cam.inv_res_x = (float)1 / (float)s.film_width;
    cam.inv_res_y = (float)1 / (float)s.film_height;
    cam.near_clip = s.near_clip;
    cam.far_clip = s.far_clip;
    V o0 = xf_point(s2c, v(0.0f, 0.0f, 0.0f));
    V dx = xf_point(s2c, v(cam.inv_res_x, 0.0f, 0.0f)) - o0;
    V dy = xf_point(s2c, v(0.0f, cam.inv_res_y, 0.0f)) - o0;
    put3(cam.dx, dx);
    put3(cam.dy, dy);
}

// OrthographicCamera / TelecentricLensCamera ctor + configure() (orthographic.cpp:73-135,
// telecentric.cpp:74-153, sensor.cpp:156-170): the orthographic sampleToCamera and its
// dx / dy, the world direction of an orthographic ray, telecentric's aperture radius and
// focus distance divided by m_scale as sampleRayDifferential uses them
int configure_ortho_camera(const mtsgpu_sensor_desc &s, MtsgCamera &cam, MtsgCameraLens &ln, std::string &err) {
    if (!(s.near_clip > 0)) { err = "The 'nearClip' parameter must be greater than zero!"; return MTSGPU_EINVAL; }
    if (!(s.near_clip < s.far_clip)) { err = "The 'nearClip' parameter must be smaller than 'farClip'."; return MTSGPU_EINVAL; }
    // Transform::orthographic (transform.cpp:154-157), crop = film
    Xf ortho = compose(scale(1.0f, 1.0f, 1.0f / (s.far_clip - s.near_clip)), translate(0.0f, 0.0f, -s.near_clip));
    film_setup(s, ortho, cam);
    M4 W;
    std::memcpy(&W.m[0][0], s.to_world, sizeof W.m);
    put3(ln.ortho_dir, normalize(xf_vec(W, v(0.0f, 0.0f, 1.0f))));
    if (s.type == MTSGPU_SENSOR_TELECENTRIC) {
        const float scaleX = length(xf_vec(W, v(1.0f, 0.0f, 0.0f))), scaleZ = length(xf_vec(W, v(0.0f, 0.0f, 1.0f)));
        ln.aperture_radius = s.aperture_radius / scaleX;
        ln.focus_distance = s.focus_distance / scaleZ;
    }
    return MTSGPU_OK;
}

int configure_camera(const mtsgpu_sensor_desc &s, MtsgCamera &cam, MtsgCameraLens &ln, std::string &err) {
    if (s.film_width == 0 || s.film_height == 0) { err = "film size must be positive"; return MTSGPU_EINVAL; }
    std::memset(&cam, 0, sizeof cam);
    std::memset(&ln, 0, sizeof ln);
    if (s.type < MTSGPU_SENSOR_PERSPECTIVE || s.type > MTSGPU_SENSOR_TELECENTRIC) {
        err = "unknown sensor type (perspective, thinlens, orthographic, telecentric)"; return MTSGPU_EINVAL;
    }
    ln.type = s.type;
    if (s.type == MTSGPU_SENSOR_ORTHOGRAPHIC || s.type == MTSGPU_SENSOR_TELECENTRIC)
        return configure_ortho_camera(s, cam, ln, err);
    if (s.type == MTSGPU_SENSOR_THINLENS) {
        // ThinLens ctor (thinlens.cpp:124-143); sampleToCamera, dx and dy are perspective's (:156-193)
        ln.aperture_radius = s.aperture_radius == 0 ? 1e-4f : s.aperture_radius;   // Epsilon
        ln.focus_distance = s.focus_distance;
        if (has_scale(s.to_world)) {
            err = "Scale factors in the camera-to-world transformation are not allowed!";
            return MTSGPU_EINVAL;
        }
    }
    const float aspect = (float)s.film_width / (float)s.film_height;
    float xfov = s.fov;
    int axis = s.fov_axis;
    if (axis == MTSGPU_FOV_SMALLER) axis = aspect > 1 ? MTSGPU_FOV_Y : MTSGPU_FOV_X;
    else if (axis == MTSGPU_FOV_LARGER) axis = aspect > 1 ? MTSGPU_FOV_X : MTSGPU_FOV_Y;
    if (axis == MTSGPU_FOV_Y) {
        xfov = rad2deg(2 * std::atan(std::tan(0.5f * deg2rad(s.fov)) * aspect));
    } else if (axis == MTSGPU_FOV_DIAGONAL) {
        float diagonal = 2 * std::tan(0.5f * deg2rad(s.fov));
        float width = diagonal / std::sqrt(1.0f + 1.0f / (aspect * aspect));
        xfov = rad2deg(2 * std::atan(width * 0.5f));
    } else if (axis != MTSGPU_FOV_X) {
        err = "The 'fovAxis' parameter must be set to one of 'smaller', 'larger', 'diagonal', 'x', or 'y'!";
        return MTSGPU_EINVAL;
    }
    if (!(xfov > 0 && xfov < 180)) { err = "The horizontal field of view must be in the interval (0, 180)!"; return MTSGPU_EINVAL; }
    if (!(s.near_clip > 0)) { err = "The 'nearClip' parameter must be greater than zero!"; return MTSGPU_EINVAL; }
    if (!(s.near_clip < s.far_clip)) { err = "The 'nearClip' parameter must be less than 'farClip'!"; return MTSGPU_EINVAL; }
    // Transform::perspective (transform.cpp:99-123)
    float recip = 1.0f / (s.far_clip - s.near_clip);
    float cot = 1.0f / std::tan(deg2rad(xfov / 2.0f));
    M4 P; std::memset(&P, 0, sizeof P);
    P.m[0][0] = cot; P.m[1][1] = cot;
    P.m[2][2] = s.far_clip * recip; P.m[2][3] = -s.near_clip * s.far_clip * recip;
    P.m[3][2] = 1;
    Xf persp;
    persp.t = P;
    if (!invert(P, persp.inv)) { err = "Unable to invert singular matrix"; return MTSGPU_EINVAL; }
    film_setup(s, persp, cam);
    return MTSGPU_OK;
}

}  // namespace

int configure_sensor(const mtsgpu_sensor_desc &s, HostScene &S, std::string &err) {
    const int rc = configure_camera(s, S.cam, S.cam_lens, err);
    if (rc) return rc;
    S.film_w = s.film_width;
    S.film_h = s.film_height;
    return MTSGPU_OK;
}

}  // namespace mtsg_host
