// gf_pixfmt.hpp — colour -> MONO8 as the reference's node does it ahead of trackImage (getImageFromMsg, rosNodeTest.cpp:238-254: cv_bridge::toCvCopy(msg, MONO8) =
// OpenCV 4.2 cvtColor, color_rgb.cpp RGB2Gray<uchar>: CV_DESCALE(b B2Y + g G2Y + r R2Y, 14) with B2Y 1868, G2Y 9617, R2Y 4899; alpha ignored), and where the
// channels of the four colour encodings lie.  One source for the host decoder (host/rosbag_reader.h, plain C++) and the conversion kernels
// (gf_cvt_kernels.hpp): integer arithmetic, so both give the same bits whatever the compiler does.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/groundfusion_hip.h"   // GF_PIX_*

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define GF_PIX_HD __host__ __device__ __forceinline__
#else
#define GF_PIX_HD inline
#endif

namespace gfpix {

GF_PIX_HD bool valid(int format) { return format >= GF_PIX_MONO8 && format <= GF_PIX_BGRA8; }
// bytes per pixel: 1, 3, 3, 4, 4 (0: no such format)
GF_PIX_HD int channels(int format) { return format == GF_PIX_MONO8 ? 1 : (format == GF_PIX_RGB8 || format == GF_PIX_BGR8) ? 3 : (format == GF_PIX_RGBA8 || format == GF_PIX_BGRA8) ? 4 : 0; }
// byte of a colour pixel that holds red / blue (green is byte 1, alpha byte 3): rgb8, rgba8 = (0, 1, 2), bgr8, bgra8 = (2, 1, 0)
GF_PIX_HD int red_at(int format) { return (format == GF_PIX_BGR8 || format == GF_PIX_BGRA8) ? 2 : 0; }
GF_PIX_HD int blue_at(int format) { return 2 - red_at(format); }
GF_PIX_HD uint8_t gray(unsigned r, unsigned g, unsigned b) { return (uint8_t)((b * 1868u + g * 9617u + r * 4899u + (1u << 13)) >> 14); }

// sensor_msgs/Image.encoding -> format, or -1 (8UC1 is relabelled mono8, rosNodeTest.cpp:241-250)
inline int format_of_encoding(const char* e) {
    if (!strcmp(e, "mono8") || !strcmp(e, "8UC1")) return GF_PIX_MONO8;
    if (!strcmp(e, "rgb8")) return GF_PIX_RGB8;
    if (!strcmp(e, "bgr8")) return GF_PIX_BGR8;
    if (!strcmp(e, "rgba8")) return GF_PIX_RGBA8;
    if (!strcmp(e, "bgra8")) return GF_PIX_BGRA8;
    return -1;
}

}  // namespace gfpix
