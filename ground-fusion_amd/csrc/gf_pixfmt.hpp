// gf_pixfmt.hpp — anything -> MONO8 as the reference's node does it ahead of trackImage (getImageFromMsg, rosNodeTest.cpp:238-254: cv_bridge::toCvCopy(msg, MONO8)).
//   colour        OpenCV 4.2 cvtColor, color_rgb.cpp RGB2Gray<uchar>: CV_DESCALE(b B2Y + g G2Y + r R2Y, 14) with B2Y 1868, G2Y 9617, R2Y 4899; alpha ignored; and where
//                 the channels of the four colour encodings lie
//   Bayer         cvtColor(COLOR_Bayer??2GRAY) on uchar as its generic loop computes it (demosaicing.cpp, Bayer2Gray_Invoker): a bilinear demosaic fused with the
//                 luma sum, the same three constants; border pixels take the value of the nearest interior pixel ("Raw frames")
//   YUV 4:2:2     COLOR_YUV2GRAY_UYVY: the luma byte of every pixel pair
//   MONO16        convertTo(CV_8U, 255. / 65535.): (v + 128) / 257 on little-endian pixels
// One source for the host decoder (host/rosbag_reader.h, plain C++) and the conversion kernels (gf_cvt_kernels.hpp): integer arithmetic, so both give the same
// bits whatever the compiler does.
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

GF_PIX_HD bool is_bayer(int format) { return format >= GF_PIX_BAYER_RGGB8 && format <= GF_PIX_BAYER_GRBG8; }
GF_PIX_HD bool valid(int format) { return (format >= GF_PIX_MONO8 && format <= GF_PIX_BGRA8) || (format >= GF_PIX_BAYER_RGGB8 && format <= GF_PIX_MONO16); }
// bytes per pixel: 1, 3, 3, 4, 4; Bayer 1, YUV 4:2:2 and MONO16 2 (0: no such format)
GF_PIX_HD int channels(int format) {
    return (format == GF_PIX_MONO8 || is_bayer(format)) ? 1 : (format == GF_PIX_RGB8 || format == GF_PIX_BGR8) ? 3 : (format == GF_PIX_RGBA8 || format == GF_PIX_BGRA8) ? 4
         : (format == GF_PIX_YUV422_UYVY || format == GF_PIX_YUV422_YUY2 || format == GF_PIX_MONO16) ? 2 : 0;
}
// smallest frame of a format: the Bayer stencil needs an interior pixel
GF_PIX_HD int min_side(int format) { return is_bayer(format) ? 3 : 1; }
// byte of a colour pixel that holds red / blue (green is byte 1, alpha byte 3): rgb8, rgba8 = (0, 1, 2), bgr8, bgra8 = (2, 1, 0)
GF_PIX_HD int red_at(int format) { return (format == GF_PIX_BGR8 || format == GF_PIX_BGRA8) ? 2 : 0; }
GF_PIX_HD int blue_at(int format) { return 2 - red_at(format); }
GF_PIX_HD uint8_t gray(unsigned r, unsigned g, unsigned b) { return (uint8_t)((b * 1868u + g * 9617u + r * 4899u + (1u << 13)) >> 14); }

// ---- Bayer.  The four letters of an encoding are the colours of pixels (0,0), (0,1), (1,0), (1,1); the pattern has period 2 both ways.  Two bits describe it:
// green_first: pixel (0,0) is green (gbrg, grbg); blue_row0: row 0 holds the blue pixels (bggr, gbrg).
GF_PIX_HD int bayer_green_first(int format) { return format == GF_PIX_BAYER_GBRG8 || format == GF_PIX_BAYER_GRBG8; }
GF_PIX_HD int bayer_blue_row0(int format) { return format == GF_PIX_BAYER_BGGR8 || format == GF_PIX_BAYER_GBRG8; }
// a site is green where (x + y) has the parity the first bit names; a row's other colour is blue where y has the parity the second names
GF_PIX_HD bool bayer_is_green(int green_first, int y, int x) { return (((x + y) & 1) ^ green_first) != 0; }
GF_PIX_HD bool bayer_row_is_blue(int blue_row0, int y) { return ((y & 1) ^ blue_row0) != 0; }
// site colour of (format, y, x): 0 red, 1 green, 2 blue
GF_PIX_HD int bayer_colour(int format, int y, int x) { return bayer_is_green(bayer_green_first(format), y, x) ? 1 : bayer_row_is_blue(bayer_blue_row0(format), y) ? 2 : 0; }
GF_PIX_HD unsigned luma_weight(int colour) { return colour == 0 ? 4899u : colour == 1 ? 9617u : 1868u; }
// red or blue site of weight kc, the opposite colour's weight ko: value C, the sum of the four edge neighbours (green), the sum of the four diagonal ones (opposite)
GF_PIX_HD uint8_t bayer_rb(unsigned kc, unsigned ko, unsigned C, unsigned edge4, unsigned diag4) { return (uint8_t)((4u * kc * C + 9617u * edge4 + ko * diag4 + (1u << 15)) >> 16); }
// green site: value C, left + right (colour of weight kh), above + below (weight kv)
GF_PIX_HD uint8_t bayer_g(unsigned kh, unsigned kv, unsigned C, unsigned we, unsigned ns) { return (uint8_t)((2u * 9617u * C + kh * we + kv * ns + (1u << 14)) >> 15); }
// interior pixel (y, x), 1 <= y <= h - 2, 1 <= x <= w - 2, of a mosaic whose rows y - 1, y, y + 1 start at n, c, s
GF_PIX_HD uint8_t bayer_gray(int green_first, int blue_row0, int y, int x, const uint8_t* n, const uint8_t* c, const uint8_t* s) {
    const unsigned k_row = bayer_row_is_blue(blue_row0, y) ? 1868u : 4899u, k_other = 4899u + 1868u - k_row;   // weight of this row's non-green colour, of the other rows'
    const unsigned we = (unsigned)c[x - 1] + c[x + 1], ns = (unsigned)n[x] + s[x];
    if (bayer_is_green(green_first, y, x)) return bayer_g(k_row, k_other, c[x], we, ns);
    return bayer_rb(k_row, k_other, c[x], we + ns, (unsigned)n[x - 1] + n[x + 1] + s[x - 1] + s[x + 1]);
}
// border pixels take the nearest interior pixel's value: the coordinate a border coordinate stands for
GF_PIX_HD int bayer_clamp(int v, int size) { return v < 1 ? 1 : v > size - 2 ? size - 2 : v; }

// ---- YUV 4:2:2: byte of a two-byte pixel that holds its luma (uyvy: U Y V Y, yuy2: Y U Y V)
GF_PIX_HD int luma_at(int format) { return format == GF_PIX_YUV422_UYVY ? 1 : 0; }
// ---- MONO16 (the pixel's value, whatever the byte order it came in): the rounded v * 255 / 65535 for every v
GF_PIX_HD uint8_t mono16_gray(unsigned v) { return (uint8_t)((v + 128u) / 257u); }

// sensor_msgs/Image.encoding of an image topic -> format, or -1 (8UC1 is relabelled mono8, rosNodeTest.cpp:241-250)
#define GF_PIX_ENCODINGS "mono8, 8UC1, rgb8, bgr8, rgba8, bgra8, bayer_rggb8, bayer_bggr8, bayer_gbrg8, bayer_grbg8, yuv422, yuv422_yuy2, mono16"
inline int format_of_encoding(const char* e) {
    if (!strcmp(e, "mono8") || !strcmp(e, "8UC1")) return GF_PIX_MONO8;
    if (!strcmp(e, "rgb8")) return GF_PIX_RGB8;
    if (!strcmp(e, "bgr8")) return GF_PIX_BGR8;
    if (!strcmp(e, "rgba8")) return GF_PIX_RGBA8;
    if (!strcmp(e, "bgra8")) return GF_PIX_BGRA8;
    if (!strcmp(e, "bayer_rggb8")) return GF_PIX_BAYER_RGGB8;
    if (!strcmp(e, "bayer_bggr8")) return GF_PIX_BAYER_BGGR8;
    if (!strcmp(e, "bayer_gbrg8")) return GF_PIX_BAYER_GBRG8;
    if (!strcmp(e, "bayer_grbg8")) return GF_PIX_BAYER_GRBG8;
    if (!strcmp(e, "yuv422")) return GF_PIX_YUV422_UYVY;
    if (!strcmp(e, "yuv422_yuy2")) return GF_PIX_YUV422_YUY2;
    if (!strcmp(e, "mono16")) return GF_PIX_MONO16;
    return -1;
}

}  // namespace gfpix
