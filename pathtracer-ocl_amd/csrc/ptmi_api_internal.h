// ptmi_api_internal.h -- what the two halves of the C ABI (ptmi_api.cpp, ptmi_image_api.cpp) and the image passes'
// argument checks (ptmi_image_args.h) share: the error message, the HIP status check, reads of the packed records
// and the camera record's conversion.  No HIP include: HIP_TRY names the runtime only where it is expanded.
#pragma once
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/ptmi.h"
#include "ptmi_device.h"

#define HIP_TRY(call)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            set_err(err, err_len, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                    __LINE__);                                                                    \
            return PTMI_ERR_HIP;                                                                  \
        }                                                                                         \
    } while (0)

namespace ptmi {

inline void set_err(char* err, size_t n, const char* fmt, ...) {
    if (!err || n == 0) return;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, n, fmt, ap);
    va_end(ap);
}

template <typename T>
T rd(const uint8_t* p) {
    T v;
    std::memcpy(&v, p, sizeof(T));
    return v;
}

// The 256-byte CLCamera record -> DevCamera, origin included: the one conversion behind ptmi_scene_create,
// ptmi_scene_set_camera and the image passes' previous camera, so all give the kernels the same bits.
inline int convert_camera(const uint8_t* camera, DevCamera& cam, char* err, size_t err_len) {
    cam.width = rd<int32_t>(camera + 0);
    cam.height = rd<int32_t>(camera + 4);
    cam.pixel_size = rd<double>(camera + 16);
    cam.half_width = rd<double>(camera + 24);
    cam.half_height = rd<double>(camera + 32);
    cam.aperture = rd<double>(camera + 40);
    cam.focal_length = rd<double>(camera + 48);
    std::memcpy(cam.inv, camera + 56, 128);
    for (int r = 0; r < 4; r++)  // mul (tracer.cl:369-376) of the point (0,0,0,1); no contraction (Makefile)
        cam.origin[r] = ((cam.inv[4 * r] * 0.0 + cam.inv[4 * r + 1] * 0.0) + cam.inv[4 * r + 2] * 0.0) +
                        cam.inv[4 * r + 3] * 1.0;
    if (cam.width <= 0 || cam.height <= 0 || (int64_t)cam.width * cam.height > (int64_t)1 << 30) {
        set_err(err, err_len, "bad camera size %dx%d", cam.width, cam.height);
        return PTMI_ERR_ARG;
    }
    return PTMI_OK;
}

}  // namespace ptmi
