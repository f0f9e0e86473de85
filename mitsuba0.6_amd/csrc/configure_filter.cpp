// configure_filter.cpp -- the reconstruction filter's table (libcore/rfilter.cpp:37-55,
// rfilters/box.cpp, gaussian.cpp).  A render's parameter, not the scene's: the render plan
// and the C-ABI call it, mtsg_configure_scene does not.
#include "host_math.h"
#include "scene_build.h"

int mtsg_configure_filter(int32_t type, float param, MtsgFilter &f, std::string &err) {
    float stddev = 0;
    std::memset(&f, 0, sizeof f);
    f.type = type;
    if (type == MTSGPU_RFILTER_BOX) f.radius = param + 1e-5f;
    else if (type == MTSGPU_RFILTER_GAUSSIAN) { stddev = param; f.radius = 4 * stddev; }
    else { err = "unknown reconstruction filter"; return MTSGPU_EINVAL; }
    if (!(f.radius > 0)) { err = "filter radius must be positive"; return MTSGPU_EINVAL; }
    float sum = 0.0f;
    for (int i = 0; i < MTSG_FILTER_RES; ++i) {
        float x = (f.radius * i) / MTSG_FILTER_RES, value;
        if (type == MTSGPU_RFILTER_BOX) {
            value = std::fabs(x) <= f.radius ? 1.0f : 0.0f;
        } else {
            float alpha = -1.0f / (2.0f * stddev * stddev);
            value = mtsg_host::fmax_std(0.0f, (float)std::exp((double)(alpha * x * x)) -
                                                  (float)std::exp((double)(alpha * f.radius * f.radius)));
        }
        f.values[i] = value;
        sum += value;
    }
    f.values[MTSG_FILTER_RES] = 0.0f;
    f.scale = MTSG_FILTER_RES / f.radius;
    f.border = (int)std::ceil(f.radius - 0.5f);
    sum *= 2 * f.radius / MTSG_FILTER_RES;
    float normalization = 1.0f / sum;
    for (int i = 0; i < MTSG_FILTER_RES; ++i) f.values[i] *= normalization;
    return MTSGPU_OK;
}
