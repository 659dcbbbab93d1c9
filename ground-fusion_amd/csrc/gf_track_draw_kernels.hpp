// gf_track_draw_kernels.hpp — the raster of the track image (gf_track_draw.hpp) on the device.  A gather: every output pixel is written once, by the block that
// owns its tile, so there is no order between writers and no atomic.  One launch renders all frames of a call; blockIdx.y is the list position.
// A block owns a tile of kTileW x kTileH pixels and
//   1. culls the frame's primitives against the tile by bounding box (gfdraw::touches), 256 at a time across its lanes, and compacts the survivors into LDS by
//      ballot and popcount.  A list of any length is walked in such pieces -- a piece leaves at most 256 survivors, which is the LDS list's size -- so nothing is
//      ever truncated; the per-pixel state (gfdraw::Acc) is carried from piece to piece, and is independent of how the list is cut;
//   2. resolves each of its pixels, four neighbours of a row per lane, against that short list (LDS broadcast reads);
//   3. assembles the rows' bytes in LDS and stores them in the widest pieces the destination allows.
// Store form.  A pixel is 3 bytes, a tile row 192: twelve 16-byte pieces when the row's first byte is 16-byte aligned.  A row is laid into LDS at the phase its
// first byte has in global memory (address & 15), so that piece k of the LDS row is the aligned 16 bytes of global memory it belongs to: a lane stores a piece
// whole when all of it is the tile's, and otherwise -- at the two ragged ends of a row at an odd address or pitch, or of the image's last tile -- the dwords of
// it that are, and single bytes for the rest.  No byte outside the rows' 3 * width bytes is read or written.
#pragma once
#include <hip/hip_runtime.h>

#include "gf_track_draw.hpp"

namespace gfdraw {

constexpr int kTileW = 64, kTileH = 16, kDrawThreads = 256;
constexpr int kPiece = 256;                               // primitives culled per pass = capacity of the LDS list
constexpr int kRowPieces = (15 + 3 * kTileW + 15) / 16;   // 16-byte pieces a tile row can touch at any phase: 13
constexpr int kRowLds = kRowPieces * 16;
static_assert(kTileW * kTileH == 4 * kDrawThreads && kTileH * kRowPieces <= kDrawThreads && kPiece == kDrawThreads, "four pixels, one primitive of a pass and at most one piece per lane");

__global__ void __launch_bounds__(kDrawThreads) draw_track_kernel(const DrawJob* __restrict__ jobs, int w, int h) {
    __shared__ Prim s_list[kPiece];
    __shared__ int s_index[kPiece];
    __shared__ int s_wave[kDrawThreads / 64];
    __shared__ uint4 s_rows[kTileH * kRowPieces];
    const DrawJob J = jobs[blockIdx.y];
    const int tiles_x = (w + kTileW - 1) / kTileW;
    const int x0 = (int)(blockIdx.x % tiles_x) * kTileW, y0 = (int)(blockIdx.x / tiles_x) * kTileH;
    const int x1 = min(x0 + kTileW, w) - 1, y1 = min(y0 + kTileH, h) - 1;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int row = t >> 4, px = x0 + 4 * (t & 15), y = y0 + row;

    Acc acc[4] = {acc_empty(), acc_empty(), acc_empty(), acc_empty()};
    for (int base = 0; base < J.n; base += kPiece) {
        const int i = base + t;
        Prim p{};
        bool keep = false;
        if (i < J.n) { p = J.prims[i]; keep = touches(p, x0, y0, x1, y1); }
        const unsigned long long votes = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(votes);
        __syncthreads();
        int before = 0, total = 0;
        for (int k = 0; k < kDrawThreads / 64; k++) { const int c = s_wave[k]; if (k < wave) before += c; total += c; }
        if (keep) { const int at = before + __popcll(votes & ((1ull << lane) - 1)); s_list[at] = p; s_index[at] = i; }
        __syncthreads();
        if (y <= y1)
            for (int k = 0; k < total; k++) {
                const Prim q = s_list[k];
                const int qi = s_index[k];
#pragma unroll
                for (int j = 0; j < 4; j++) accumulate(acc[j], q, qi, px + j, y);
            }
        __syncthreads();   // the next pass writes s_wave and the list
    }

    // the row's bytes into LDS at the phase of its first byte in global memory
    uint8_t* rows = reinterpret_cast<uint8_t*>(s_rows);
    if (y <= y1 && px <= x1) {
        const uint8_t* g = J.gray + (size_t)y * J.gray_pitch + px;
        uint32_t gray4 = 0;
        if (px + 3 <= x1 && !((reinterpret_cast<uintptr_t>(J.gray) | (uintptr_t)J.gray_pitch) & 3)) gray4 = *reinterpret_cast<const uint32_t*>(g);   // px is a multiple of 4
        else for (int j = 0; j < 4 && px + j <= x1; j++) gray4 |= (uint32_t)g[j] << (8 * j);
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = finish(acc[j], (uint8_t)(gray4 >> (8 * j)));
        const unsigned phase = (unsigned)((reinterpret_cast<uintptr_t>(J.dst) + (size_t)y * J.dst_pitch + 3 * (size_t)x0) & 15);
        uint8_t* o = rows + row * kRowLds + phase + 12 * (t & 15);
        if (!(phase & 3)) {   // twelve bytes as three dwords (pixels past x1 carry bytes nobody stores)
            uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
            o4[0] = v[0] | (v[1] << 24); o4[1] = (v[1] >> 8) | (v[2] << 16); o4[2] = (v[2] >> 16) | (v[3] << 8);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) { o[3 * j] = (uint8_t)v[j]; o[3 * j + 1] = (uint8_t)(v[j] >> 8); o[3 * j + 2] = (uint8_t)(v[j] >> 16); }
        }
    }
    __syncthreads();

    // one 16-byte piece of one row per lane
    if (t < kTileH * kRowPieces) {
        const int r = t / kRowPieces, piece = t % kRowPieces, yy = y0 + r;
        if (yy > y1) return;
        uint8_t* first = J.dst + (size_t)yy * J.dst_pitch + 3 * (size_t)x0;   // the row's first byte of this tile
        const int phase = (int)(reinterpret_cast<uintptr_t>(first) & 15);
        const int lo = max(16 * piece, phase), hi = min(16 * piece + 16, phase + 3 * (x1 - x0 + 1));   // the tile's bytes of this piece, as LDS row offsets
        if (lo >= hi) return;
        const uint8_t* src = rows + r * kRowLds;
        uint8_t* out = first - phase;   // LDS row offset k <-> out + k; only [lo, hi) is touched
        if (hi - lo == 16) { *reinterpret_cast<uint4*>(out + lo) = *reinterpret_cast<const uint4*>(src + lo); return; }
        for (int k = 16 * piece; k < 16 * piece + 16; k += 4) {
            if (k >= lo && k + 4 <= hi) *reinterpret_cast<uint32_t*>(out + k) = *reinterpret_cast<const uint32_t*>(src + k);
            else for (int b = max(k, lo); b < min(k + 4, hi); b++) out[b] = src[b];
        }
    }
}

}  // namespace gfdraw
