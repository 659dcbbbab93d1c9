// gf_cvt_kernels.hpp — colour and raw frames -> MONO8 on batches of u8 frames: cv_bridge::toCvCopy(msg, MONO8) of getImageFromMsg (rosNodeTest.cpp:238-254), the
// arithmetic of gf_pixfmt.hpp.  Included by gf_cvt.hip (and by tests/native/raw_gray_host.hip, which walks the raw kernels' threads on the CPU).
//
// Colour and MONO8, a pure stream: CH bytes in, one byte out per pixel, nothing is read twice.
//   cvt_gray_vec_kernel<CH, NPX>  a lane takes NPX (4 or 16) consecutive pixels of a row: NPX * CH / 4 source dwords in, NPX / 4 dwords out; consecutive lanes take
//                                 consecutive pieces of a row, so a wavefront reads one contiguous span and writes one.  Needs every row base of source and
//                                 destination on a 4-byte boundary (both pointers, the pitch and the width multiples of 4) and NPX | width.
//   cvt_gray_byte_kernel<CH>      one pixel per lane, byte loads and a byte store: any pointer, any pitch, any width.
// YUV 4:2:2 and MONO16, the same stream with two bytes in (cvt_pair_*): NPX = 16 is two 16-byte loads and one 16-byte store per lane.
// Bayer, a 3 x 3 stencil on bytes (cvt_bayer_*): see there.
// blockIdx.y walks the frames (strided, for batches beyond the grid limit).
//
// The raw kernels keep their per-thread work in __host__ __device__ functions of (block, thread) that hold nothing but plain loads and stores, and the choice of
// form and grid in raw_plan(): a host program can run every thread of a launch on heap buffers of exactly the frames' sizes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_pixfmt.hpp"
#include "gf_frame_ref.hpp"

namespace gfcvt {

constexpr int kThreads = 256;

template <int N> struct __attribute__((packed, aligned(4))) Dwords { uint32_t v[N]; };   // N dwords on a 4-byte boundary: one load / store instruction of that width

// pixel j (0 .. NPX-1) of a piece held as little-endian dwords: byte k of the piece is (v[k >> 2] >> 8 (k & 3)) & 255; all indices are compile-time after unrolling
template <int CH, int NPX> GF_PIX_HD unsigned byte_of(const Dwords<NPX * CH / 4>& s, int k) { return (s.v[k >> 2] >> (8 * (k & 3))) & 255u; }

template <int CH, int NPX>
GF_PIX_HD void cvt_gray_vec_thread(unsigned bx, unsigned tx, unsigned by, unsigned gy, const uint8_t* __restrict__ src, size_t src_pitch, uint8_t* __restrict__ dst, int batch, int w, int h, int red_at) {
    const int per_row = w / NPX;
    const unsigned p = bx * kThreads + tx;   // piece of the frame; the host keeps per_row * h below 2^31
    if (p >= (unsigned)per_row * (unsigned)h) return;
    const int y = p / per_row, xp = p - y * per_row;
    for (int b = by; b < batch; b += gy) {
        const Dwords<NPX * CH / 4> s = *reinterpret_cast<const Dwords<NPX * CH / 4>*>(src + ((size_t)b * h + y) * src_pitch + (size_t)xp * (NPX * CH));
        Dwords<NPX / 4> o;
#pragma unroll
        for (int q = 0; q < NPX / 4; q++) {
            unsigned out = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int k = (4 * q + j) * CH;
                unsigned g;
                if (CH == 1) g = byte_of<CH, NPX>(s, k);
                else {
                    const unsigned c0 = byte_of<CH, NPX>(s, k), c1 = byte_of<CH, NPX>(s, k + 1), c2 = byte_of<CH, NPX>(s, k + 2);
                    g = gfpix::gray(red_at ? c2 : c0, c1, red_at ? c0 : c2);
                }
                out |= g << (8 * j);
            }
            o.v[q] = out;
        }
        *reinterpret_cast<Dwords<NPX / 4>*>(dst + ((size_t)b * h + y) * w + (size_t)xp * NPX) = o;
    }
}
template <int CH, int NPX>
__global__ __launch_bounds__(kThreads) void cvt_gray_vec_kernel(const uint8_t* __restrict__ src, size_t src_pitch, uint8_t* __restrict__ dst, int batch, int w, int h, int red_at) {
    cvt_gray_vec_thread<CH, NPX>(blockIdx.x, threadIdx.x, blockIdx.y, gridDim.y, src, src_pitch, dst, batch, w, h, red_at);
}

template <int CH>
GF_PIX_HD void cvt_gray_byte_thread(unsigned bx, unsigned tx, unsigned by, unsigned gy, const uint8_t* __restrict__ src, size_t src_pitch, uint8_t* __restrict__ dst, int batch, int w, int h, int red_at) {
    const unsigned p = bx * kThreads + tx;   // pixel of the frame; the host keeps w * h below 2^31
    if (p >= (unsigned)w * (unsigned)h) return;
    const int y = p / w, x = p - y * w;
    for (int b = by; b < batch; b += gy) {
        const uint8_t* s = src + ((size_t)b * h + y) * src_pitch + (size_t)x * CH;
        dst[((size_t)b * h + y) * w + x] = CH == 1 ? s[0] : gfpix::gray(s[red_at], s[1], s[2 - red_at]);
    }
}
template <int CH>
__global__ __launch_bounds__(kThreads) void cvt_gray_byte_kernel(const uint8_t* __restrict__ src, size_t src_pitch, uint8_t* __restrict__ dst, int batch, int w, int h, int red_at) {
    cvt_gray_byte_thread<CH>(blockIdx.x, threadIdx.x, blockIdx.y, gridDim.y, src, src_pitch, dst, batch, w, h, red_at);
}

// ---------------------------------------------------------------------------------------------------------------- raw formats
// which form a conversion of a raw format takes and the grid it is launched with (blocks of kThreads lanes)
struct RawPlan { int form; unsigned gx, gy; };   // form: pixels a lane takes per row (16, 4 or 1)
constexpr int kBayerBand = 16;   // rows of a Bayer band

// the dispatch rule of cvt_launch_ch: whole dwords where every row base of source and destination lies on a 4-byte boundary
inline bool raw_dwords(const void* src, size_t src_pitch, const void* dst, int w) { return !((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | src_pitch | (size_t)w) & 3); }
inline unsigned raw_blocks(size_t per_row, size_t rows) { return (unsigned)((per_row * rows + kThreads - 1) / kThreads); }
inline RawPlan raw_plan(bool bayer, const void* src, size_t src_pitch, const void* dst, int batch, int w, int h) {
    const unsigned gy = (unsigned)(batch < 65535 ? batch : 65535);
    const bool dwords = raw_dwords(src, src_pitch, dst, w);
    if (bayer) {   // dwords of four columns walking bands of rows; below eight columns the one-pixel form
        if (dwords && w >= 8) return {4, raw_blocks((size_t)w / 4, ((size_t)h + kBayerBand - 1) / kBayerBand), gy};
        return {1, raw_blocks((size_t)w, (size_t)h), gy};
    }
    if (dwords && !(w & 15)) return {16, raw_blocks((size_t)w / 16, (size_t)h), gy};
    if (dwords) return {4, raw_blocks((size_t)w / 4, (size_t)h), gy};
    return {1, raw_blocks((size_t)w, (size_t)h), gy};
}

// ---- two-byte pixels.  M16: the pixel is a little-endian u16 -> gfpix::mono16_gray; else its byte luma_at (0 or 1) is the result.
template <bool M16> GF_PIX_HD unsigned pair_gray(unsigned lo, unsigned hi, int luma_at) { return M16 ? gfpix::mono16_gray(lo | (hi << 8)) : (luma_at ? hi : lo); }

template <bool M16, int NPX>
GF_PIX_HD void cvt_pair_vec_thread(unsigned bx, unsigned tx, unsigned by, unsigned gy, const uint8_t* src, size_t src_pitch, uint8_t* dst, int batch, int w, int h, int luma_at) {
    const int per_row = w / NPX;
    const unsigned p = bx * kThreads + tx;   // piece of the frame; the host keeps w * h below 2^31
    if (p >= (unsigned)per_row * (unsigned)h) return;
    const int y = p / per_row, xp = p - y * per_row;
    for (int b = by; b < batch; b += gy) {
        const Dwords<NPX / 2> s = *reinterpret_cast<const Dwords<NPX / 2>*>(src + ((size_t)b * h + y) * src_pitch + (size_t)xp * (NPX * 2));
        Dwords<NPX / 4> o;
#pragma unroll
        for (int q = 0; q < NPX / 4; q++) {
            unsigned out = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const unsigned px = s.v[2 * q + (j >> 1)] >> (16 * (j & 1));   // pixel 4 q + j in the low 16 bits
                out |= pair_gray<M16>(px & 255u, (px >> 8) & 255u, luma_at) << (8 * j);
            }
            o.v[q] = out;
        }
        *reinterpret_cast<Dwords<NPX / 4>*>(dst + ((size_t)b * h + y) * w + (size_t)xp * NPX) = o;
    }
}

template <bool M16>
GF_PIX_HD void cvt_pair_byte_thread(unsigned bx, unsigned tx, unsigned by, unsigned gy, const uint8_t* src, size_t src_pitch, uint8_t* dst, int batch, int w, int h, int luma_at) {
    const unsigned p = bx * kThreads + tx;   // pixel of the frame
    if (p >= (unsigned)w * (unsigned)h) return;
    const int y = p / w, x = p - y * w;
    for (int b = by; b < batch; b += gy) {
        const uint8_t* s = src + ((size_t)b * h + y) * src_pitch + (size_t)x * 2;
        dst[((size_t)b * h + y) * w + x] = (uint8_t)pair_gray<M16>(s[0], s[1], luma_at);
    }
}

template <bool M16, int NPX>
__global__ __launch_bounds__(kThreads) void cvt_pair_vec_kernel(const uint8_t* __restrict__ src, size_t src_pitch, uint8_t* __restrict__ dst, int batch, int w, int h, int luma_at) {
    cvt_pair_vec_thread<M16, NPX>(blockIdx.x, threadIdx.x, blockIdx.y, gridDim.y, src, src_pitch, dst, batch, w, h, luma_at);
}
template <bool M16>
__global__ __launch_bounds__(kThreads) void cvt_pair_byte_kernel(const uint8_t* __restrict__ src, size_t src_pitch, uint8_t* __restrict__ dst, int batch, int w, int h, int luma_at) {
    cvt_pair_byte_thread<M16>(blockIdx.x, threadIdx.x, blockIdx.y, gridDim.y, src, src_pitch, dst, batch, w, h, luma_at);
}

// ---- Bayer: out(y, x) = f(clamp(y, 1, h - 2), clamp(x, 1, w - 2)), f the bilinear demosaic fused with the luma sum (gfpix::bayer_rb / bayer_g).
//   cvt_bayer_vec_kernel   a lane owns the four output columns of one dword (x0 = a multiple of 4) and walks a band of kBayerBand rows; consecutive lanes own
//                          consecutive dwords, so a wavefront reads and writes contiguous spans.  The three source rows of the stencil stay in registers as a
//                          sliding window: every source row is loaded once per band (its own dword, and the byte to its left and the byte to its right, which
//                          are the neighbouring lanes' bytes and come from the cache), bands overlap by one row above and one below.  The column parities of
//                          the four pixels are compile-time; the walk goes two rows at a time from a row whose even columns are green, so each of the 2 x 2
//                          site kinds is straight-line code, and the pattern enters as two kernel-argument bits that choose the row to start on and the two
//                          weights.  The border clamp is on the output: the lane of column 0 / w - 1 repeats its neighbouring pixel, row 1 / h - 2 is stored
//                          to row 0 / h - 1 as well.  Rows and columns that are loaded for a window position nothing is computed from are clamped into the
//                          frame, so no address outside the frame is ever formed.  Needs what the dword forms above need, and w >= 8.
//   cvt_bayer_byte_kernel  one pixel per lane, nine byte loads: any pointer, pitch and width.
struct BayerRow { unsigned v[6]; };   // columns x0 - 1 .. x0 + 4 of a source row

GF_PIX_HD BayerRow bayer_row_load(const uint8_t* frame, size_t src_pitch, int y, int x0, int w, int h) {
    const uint8_t* row = frame + (size_t)(y < 0 ? 0 : y > h - 1 ? h - 1 : y) * src_pitch;
    const uint32_t d = *reinterpret_cast<const uint32_t*>(row + x0);
    BayerRow r;
    r.v[0] = row[x0 > 0 ? x0 - 1 : 0];
    r.v[1] = d & 255u; r.v[2] = (d >> 8) & 255u; r.v[3] = (d >> 16) & 255u; r.v[4] = d >> 24;
    r.v[5] = row[x0 + 4 < w ? x0 + 4 : w - 1];
    return r;
}

// the four pixels of a row between its neighbours n and s.  EVEN_GREEN: the even columns of this row are green.  k_row: the weight of the row's other colour
// (red or blue), k_other: of the remaining one.
template <bool EVEN_GREEN> GF_PIX_HD uint32_t bayer_row4(const BayerRow& n, const BayerRow& c, const BayerRow& s, unsigned k_row, unsigned k_other) {
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int i = j + 1;
        const unsigned ns = n.v[i] + s.v[i], we = c.v[i - 1] + c.v[i + 1];
        unsigned g;
        if (((j & 1) == 0) == EVEN_GREEN) g = gfpix::bayer_g(k_row, k_other, c.v[i], we, ns);
        else g = gfpix::bayer_rb(k_row, k_other, c.v[i], we + ns, n.v[i - 1] + n.v[i + 1] + s.v[i - 1] + s.v[i + 1]);
        out |= g << (8 * j);
    }
    return out;
}

// stores the computed row yc (1 .. h - 2) of a band [r0, r1) wherever the band holds an output row that takes its value
GF_PIX_HD void bayer_row_store(uint8_t* frame, uint32_t out, int yc, int x0, int w, int h, int r0, int r1) {
    if (x0 == 0) out = (out & 0xffffff00u) | ((out >> 8) & 255u);                   // column 0 takes column 1
    if (x0 + 4 == w) out = (out & 0x00ffffffu) | ((out << 8) & 0xff000000u);        // column w - 1 takes column w - 2
    if (yc >= r0 && yc < r1) *reinterpret_cast<uint32_t*>(frame + (size_t)yc * w + x0) = out;
    if (yc == 1 && r0 == 0) *reinterpret_cast<uint32_t*>(frame + x0) = out;
    if (yc == h - 2 && r1 == h) *reinterpret_cast<uint32_t*>(frame + (size_t)(h - 1) * w + x0) = out;
}

GF_PIX_HD void cvt_bayer_vec_thread(unsigned bx, unsigned tx, unsigned by, unsigned gy, const uint8_t* src, size_t src_pitch, uint8_t* dst, int batch, int w, int h, int green_first, int blue_row0) {
    const int cols = w / 4, bands = (h + kBayerBand - 1) / kBayerBand;
    const unsigned p = bx * kThreads + tx;   // (band, dword column) of the frame
    if (p >= (unsigned)cols * (unsigned)bands) return;
    const int band = p / cols, x0 = 4 * (int)(p - (unsigned)band * cols);
    const int r0 = band * kBayerBand, r1 = r0 + kBayerBand < h ? r0 + kBayerBand : h;
    const int c0 = gfpix::bayer_clamp(r0, h), c1 = gfpix::bayer_clamp(r1 - 1, h);   // the computed rows the band's output rows stand for
    const int e0 = c0 - (((c0 ^ green_first) & 1) ? 0 : 1);                           // the walk starts on a row whose even columns are green (gfpix::bayer_is_green at x = 0): c0 or the row above it
    // weights of the even-green rows' other colour and of the rows between them
    const unsigned k_a = gfpix::bayer_row_is_blue(blue_row0, e0) ? 1868u : 4899u, k_b = 4899u + 1868u - k_a;
    for (int b = by; b < batch; b += gy) {
        const uint8_t* sf = src + (size_t)b * h * src_pitch;
        uint8_t* df = dst + (size_t)b * h * w;
        BayerRow r_m = bayer_row_load(sf, src_pitch, e0 - 1, x0, w, h), r_0 = bayer_row_load(sf, src_pitch, e0, x0, w, h);
        for (int e = e0; e <= c1; e += 2) {
            const BayerRow r_1 = bayer_row_load(sf, src_pitch, e + 1, x0, w, h), r_2 = bayer_row_load(sf, src_pitch, e + 2, x0, w, h);
            if (e >= c0) bayer_row_store(df, bayer_row4<true>(r_m, r_0, r_1, k_a, k_b), e, x0, w, h, r0, r1);
            if (e + 1 <= c1) bayer_row_store(df, bayer_row4<false>(r_0, r_1, r_2, k_b, k_a), e + 1, x0, w, h, r0, r1);
            r_m = r_1; r_0 = r_2;
        }
    }
}

GF_PIX_HD void cvt_bayer_byte_thread(unsigned bx, unsigned tx, unsigned by, unsigned gy, const uint8_t* src, size_t src_pitch, uint8_t* dst, int batch, int w, int h, int green_first, int blue_row0) {
    const unsigned p = bx * kThreads + tx;   // pixel of the frame
    if (p >= (unsigned)w * (unsigned)h) return;
    const int y = p / w, x = p - y * w, yc = gfpix::bayer_clamp(y, h), xc = gfpix::bayer_clamp(x, w);
    for (int b = by; b < batch; b += gy) {
        const uint8_t* c = src + ((size_t)b * h + yc) * src_pitch;
        dst[((size_t)b * h + y) * w + x] = gfpix::bayer_gray(green_first, blue_row0, yc, xc, c - src_pitch, c, c + src_pitch);
    }
}

__global__ __launch_bounds__(kThreads) void cvt_bayer_vec_kernel(const uint8_t* __restrict__ src, size_t src_pitch, uint8_t* __restrict__ dst, int batch, int w, int h, int green_first, int blue_row0) {
    cvt_bayer_vec_thread(blockIdx.x, threadIdx.x, blockIdx.y, gridDim.y, src, src_pitch, dst, batch, w, h, green_first, blue_row0);
}
__global__ __launch_bounds__(kThreads) void cvt_bayer_byte_kernel(const uint8_t* __restrict__ src, size_t src_pitch, uint8_t* __restrict__ dst, int batch, int w, int h, int green_first, int blue_row0) {
    cvt_bayer_byte_thread(blockIdx.x, threadIdx.x, blockIdx.y, gridDim.y, src, src_pitch, dst, batch, w, h, green_first, blue_row0);
}


// ---------------------------------------------------------------------------------------------------------------- frames by reference
// The six kernels above with the source frames where the caller keeps them: frame b is refs[b] (gf_frame_ref: pointer of row 0, bytes from row to row), the
// destination stays `batch` tight h x w frames.  The form is the frame's own, decided block by block from its entry: a launch of a dword form (want_dwords = 1)
// serves the frames whose pointer and pitch are multiples of 4 and skips the others, a launch of a byte form with want_dwords = 0 serves exactly those others,
// with want_dwords < 0 every frame (sizes that have no dword form).  The host launches the forms the call's frames need (cvt_launch_refs): one launch when they
// agree, two when they are mixed.  Each frame runs the thread function of the tight kernel as a batch of one, so the arithmetic and the loads are the same.
__device__ __forceinline__ bool refs_serves(const gfref::Frame& f, int want_dwords) {
    return want_dwords < 0 || (gfref::form(reinterpret_cast<uintptr_t>(f.data), f.pitch) >= 4) == (want_dwords != 0);
}
#define GF_CVT_REFS_LOOP(CALL)                                                       \
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {                            \
        const gfref::Frame f = gfref::entry(refs, b);                                \
        if (!refs_serves(f, want_dwords)) continue;                                  \
        uint8_t* d = dst + (size_t)b * h * w;                                        \
        CALL;                                                                        \
    }
template <int CH, int NPX>
__global__ __launch_bounds__(kThreads) void cvt_gray_vec_refs_kernel(const gf_frame_ref* __restrict__ refs, int want_dwords, uint8_t* __restrict__ dst, int batch, int w, int h, int red_at) {
    GF_CVT_REFS_LOOP((cvt_gray_vec_thread<CH, NPX>(blockIdx.x, threadIdx.x, 0, 1, f.data, f.pitch, d, 1, w, h, red_at)))
}
template <int CH>
__global__ __launch_bounds__(kThreads) void cvt_gray_byte_refs_kernel(const gf_frame_ref* __restrict__ refs, int want_dwords, uint8_t* __restrict__ dst, int batch, int w, int h, int red_at) {
    GF_CVT_REFS_LOOP((cvt_gray_byte_thread<CH>(blockIdx.x, threadIdx.x, 0, 1, f.data, f.pitch, d, 1, w, h, red_at)))
}
template <bool M16, int NPX>
__global__ __launch_bounds__(kThreads) void cvt_pair_vec_refs_kernel(const gf_frame_ref* __restrict__ refs, int want_dwords, uint8_t* __restrict__ dst, int batch, int w, int h, int luma_at) {
    GF_CVT_REFS_LOOP((cvt_pair_vec_thread<M16, NPX>(blockIdx.x, threadIdx.x, 0, 1, f.data, f.pitch, d, 1, w, h, luma_at)))
}
template <bool M16>
__global__ __launch_bounds__(kThreads) void cvt_pair_byte_refs_kernel(const gf_frame_ref* __restrict__ refs, int want_dwords, uint8_t* __restrict__ dst, int batch, int w, int h, int luma_at) {
    GF_CVT_REFS_LOOP((cvt_pair_byte_thread<M16>(blockIdx.x, threadIdx.x, 0, 1, f.data, f.pitch, d, 1, w, h, luma_at)))
}
__global__ __launch_bounds__(kThreads) void cvt_bayer_vec_refs_kernel(const gf_frame_ref* __restrict__ refs, int want_dwords, uint8_t* __restrict__ dst, int batch, int w, int h, int green_first, int blue_row0) {
    GF_CVT_REFS_LOOP((cvt_bayer_vec_thread(blockIdx.x, threadIdx.x, 0, 1, f.data, f.pitch, d, 1, w, h, green_first, blue_row0)))
}
__global__ __launch_bounds__(kThreads) void cvt_bayer_byte_refs_kernel(const gf_frame_ref* __restrict__ refs, int want_dwords, uint8_t* __restrict__ dst, int batch, int w, int h, int green_first, int blue_row0) {
    GF_CVT_REFS_LOOP((cvt_bayer_byte_thread(blockIdx.x, threadIdx.x, 0, 1, f.data, f.pitch, d, 1, w, h, green_first, blue_row0)))
}
#undef GF_CVT_REFS_LOOP

// ---------------------------------------------------------------------------------------------------------------- one format per frame
// cvt_mixed_kernel: frame b is refs[b] in formats[b] (gf_tracker_set_seq_format: a fleet of cameras with different encodings on one handle; the same
// rosNodeTest.cpp:238-254 per camera).  A block reads its entry with wave-uniform loads, takes the form the frame's own pointer and pitch allow, as the _refs
// kernels do, and branches ONCE to the thread function the homogeneous kernel of that format and form runs, on the arguments of a batch of one: same loads, same
// arithmetic, same bytes.  The branch is on scalars, so no wavefront diverges on the format.  An entry whose format is no GF_PIX_* (the tracker writes -1 for a
// frame that needs no conversion) is skipped: nothing is read, nothing is written for it.
// blockIdx.x walks the pieces of a frame with a stride of gridDim.x: the host sizes the grid for the largest need of the frames it knows (cvt_launch_mixed with
// a host copy of the tables), or for the widest form of the size when it cannot read the tables; a frame that needs more blocks than the grid has takes several
// turns, a block beyond its frame's need leaves before it touches memory.
GF_PIX_HD int mixed_form(int format, const void* data, size_t pitch, int dst_dwords, int w) {   // pixels a lane takes per row: 16, 4 or 1
    const bool dwords = dst_dwords && gfref::form(reinterpret_cast<uintptr_t>(data), pitch) >= 4;
    if (gfpix::is_bayer(format)) return dwords && w >= 8 ? 4 : 1;
    return !dwords ? 1 : !(w & 15) ? 16 : 4;
}
GF_PIX_HD unsigned mixed_blocks(int format, int form, int w, int h) {   // blocks of kThreads lanes a frame of that format and form needs
    const size_t rows = gfpix::is_bayer(format) && form == 4 ? ((size_t)h + kBayerBand - 1) / kBayerBand : (size_t)h;
    return (unsigned)(((size_t)(w / form) * rows + kThreads - 1) / kThreads);
}
// PART: 0 every format, 1 all but Bayer, 2 Bayer alone (a launch of a part skips the other part's frames)
template <int PART> GF_PIX_HD bool mixed_serves(int format) { return gfpix::valid(format) && (PART == 0 || (PART == 2) == gfpix::is_bayer(format)); }

// lane tx of (virtual) block bx of a frame
GF_PIX_HD void cvt_mixed_thread(unsigned bx, unsigned tx, const uint8_t* src, size_t pitch, int format, int form, uint8_t* d, int w, int h) {
    const int ch = gfpix::channels(format), red_at = gfpix::red_at(format);
    if (gfpix::is_bayer(format)) {
        const int gf = gfpix::bayer_green_first(format), br = gfpix::bayer_blue_row0(format);
        if (form == 4) cvt_bayer_vec_thread(bx, tx, 0, 1, src, pitch, d, 1, w, h, gf, br);
        else cvt_bayer_byte_thread(bx, tx, 0, 1, src, pitch, d, 1, w, h, gf, br);
    } else if (format == GF_PIX_MONO16) {
        if (form == 16) cvt_pair_vec_thread<true, 16>(bx, tx, 0, 1, src, pitch, d, 1, w, h, 0);
        else if (form == 4) cvt_pair_vec_thread<true, 4>(bx, tx, 0, 1, src, pitch, d, 1, w, h, 0);
        else cvt_pair_byte_thread<true>(bx, tx, 0, 1, src, pitch, d, 1, w, h, 0);
    } else if (ch == 2) {
        const int la = gfpix::luma_at(format);
        if (form == 16) cvt_pair_vec_thread<false, 16>(bx, tx, 0, 1, src, pitch, d, 1, w, h, la);
        else if (form == 4) cvt_pair_vec_thread<false, 4>(bx, tx, 0, 1, src, pitch, d, 1, w, h, la);
        else cvt_pair_byte_thread<false>(bx, tx, 0, 1, src, pitch, d, 1, w, h, la);
    } else if (ch == 1) {
        if (form == 16) cvt_gray_vec_thread<1, 16>(bx, tx, 0, 1, src, pitch, d, 1, w, h, red_at);
        else if (form == 4) cvt_gray_vec_thread<1, 4>(bx, tx, 0, 1, src, pitch, d, 1, w, h, red_at);
        else cvt_gray_byte_thread<1>(bx, tx, 0, 1, src, pitch, d, 1, w, h, red_at);
    } else if (ch == 3) {
        if (form == 16) cvt_gray_vec_thread<3, 16>(bx, tx, 0, 1, src, pitch, d, 1, w, h, red_at);
        else if (form == 4) cvt_gray_vec_thread<3, 4>(bx, tx, 0, 1, src, pitch, d, 1, w, h, red_at);
        else cvt_gray_byte_thread<3>(bx, tx, 0, 1, src, pitch, d, 1, w, h, red_at);
    } else {
        if (form == 16) cvt_gray_vec_thread<4, 16>(bx, tx, 0, 1, src, pitch, d, 1, w, h, red_at);
        else if (form == 4) cvt_gray_vec_thread<4, 4>(bx, tx, 0, 1, src, pitch, d, 1, w, h, red_at);
        else cvt_gray_byte_thread<4>(bx, tx, 0, 1, src, pitch, d, 1, w, h, red_at);
    }
}

// what block (bx, by) of a grid (gx, gy) does for lane tx, given the entries as the block has read them: the walk a host program repeats
template <int PART, class ENTRY>
GF_PIX_HD void cvt_mixed_block(unsigned bx, unsigned gx, unsigned by, unsigned gy, unsigned tx, ENTRY entry, uint8_t* dst, int batch, int w, int h, int dst_dwords) {
    for (int b = by; b < batch; b += gy) {
        const uint8_t* data; size_t pitch; int format;
        entry(b, data, pitch, format);
        if (!mixed_serves<PART>(format)) continue;
        const int form = mixed_form(format, data, pitch, dst_dwords, w);
        const unsigned need = mixed_blocks(format, form, w, h);
        for (unsigned v = bx; v < need; v += gx) cvt_mixed_thread(v, tx, data, pitch, format, form, dst + (size_t)b * h * w, w, h);
    }
}

template <int PART>
__global__ __launch_bounds__(kThreads) void cvt_mixed_kernel(const gf_frame_ref* __restrict__ refs, const int* __restrict__ formats, uint8_t* __restrict__ dst, int batch, int w, int h, int dst_dwords) {
    cvt_mixed_block<PART>(blockIdx.x, gridDim.x, blockIdx.y, gridDim.y, threadIdx.x, [&](int b, const uint8_t*& data, size_t& pitch, int& format) {
        const gfref::Frame f = gfref::entry(refs, b);
        data = f.data; pitch = f.pitch; format = __builtin_amdgcn_readfirstlane(formats[b]);
    }, dst, batch, w, h, dst_dwords);
}

}  // namespace gfcvt
