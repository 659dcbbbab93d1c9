// The raw-format conversion kernels of csrc/gf_cvt_kernels.hpp (Bayer, YUV 4:2:2, MONO16 -> MONO8) walked on the CPU: for every case the program asks
// gfcvt::raw_plan for the form and the grid the library would launch, runs the per-thread function of that form for every (block, thread) of the grid on heap
// buffers of exactly the frames' sizes, and compares the destination with a plain double loop over the definition ("Raw frames").  The
// source buffer ends with the last pixel of the last row, so a stencil that reads outside the frames reads outside the allocation, which the AddressSanitizer
// build of this program reports; the destination lies between guard bands that must come back untouched.  hipcc compiles it (the header holds __global__
// functions); no HIP call is made, so it runs without a GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ground-fusion_amd/csrc/gf_cvt_kernels.hpp"

namespace {

const int kGuard = 64;
const uint8_t kGuardByte = 0x5A;

uint32_t rng_state = 12345u;
uint8_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return (uint8_t)(rng_state >> 24); }

// ---- the definition, written out: nothing of gf_pixfmt.hpp is used here
int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
char site(int format, int y, int x) {
    static const char* letters[4] = {"RGGB", "BGGR", "GBRG", "GRBG"};
    return letters[format - 8][2 * (y & 1) + (x & 1)];
}
unsigned weight(char c) { return c == 'R' ? 4899u : c == 'G' ? 9617u : 1868u; }
uint8_t bayer_interior(const uint8_t* f, size_t pitch, int format, int y, int x) {
    auto at = [&](int dy, int dx) { return (unsigned)f[(size_t)(y + dy) * pitch + (x + dx)]; };
    const char c = site(format, y, x);
    if (c == 'G') return (uint8_t)((2u * 9617u * at(0, 0) + weight(site(format, y, x - 1)) * (at(0, -1) + at(0, 1)) + weight(site(format, y - 1, x)) * (at(-1, 0) + at(1, 0)) + (1u << 14)) >> 15);
    return (uint8_t)((4u * weight(c) * at(0, 0) + 9617u * (at(-1, 0) + at(1, 0) + at(0, -1) + at(0, 1)) +
                      weight(site(format, y - 1, x - 1)) * (at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1)) + (1u << 15)) >> 16);
}
void reference(const uint8_t* src, size_t pitch, int format, uint8_t* out, int batch, int w, int h) {
    for (int b = 0; b < batch; b++)
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const uint8_t* f = src + (size_t)b * h * pitch;
                uint8_t v;
                if (format <= 11) v = bayer_interior(f, pitch, format, clampi(y, 1, h - 2), clampi(x, 1, w - 2));
                else if (format == 12) v = f[(size_t)y * pitch + 2 * x + 1];
                else if (format == 13) v = f[(size_t)y * pitch + 2 * x];
                else v = (uint8_t)(((unsigned)f[(size_t)y * pitch + 2 * x] + 256u * f[(size_t)y * pitch + 2 * x + 1] + 128u) / 257u);
                out[((size_t)b * h + y) * w + x] = v;
            }
}

// ---- every thread of the launch the library would make
int walk(const uint8_t* src, size_t pitch, int format, uint8_t* dst, int batch, int w, int h) {
    using namespace gfcvt;
    const bool bayer = gfpix::is_bayer(format);
    const RawPlan pl = raw_plan(bayer, src, pitch, dst, batch, w, h);
    const int gf = gfpix::bayer_green_first(format), br = gfpix::bayer_blue_row0(format), la = gfpix::luma_at(format);
    for (unsigned by = 0; by < pl.gy; by++)
        for (unsigned bx = 0; bx < pl.gx; bx++)
            for (unsigned tx = 0; tx < (unsigned)kThreads; tx++) {
                if (bayer) {
                    if (pl.form == 4) cvt_bayer_vec_thread(bx, tx, by, pl.gy, src, pitch, dst, batch, w, h, gf, br);
                    else cvt_bayer_byte_thread(bx, tx, by, pl.gy, src, pitch, dst, batch, w, h, gf, br);
                } else if (format == GF_PIX_MONO16) {
                    if (pl.form == 16) cvt_pair_vec_thread<true, 16>(bx, tx, by, pl.gy, src, pitch, dst, batch, w, h, 0);
                    else if (pl.form == 4) cvt_pair_vec_thread<true, 4>(bx, tx, by, pl.gy, src, pitch, dst, batch, w, h, 0);
                    else cvt_pair_byte_thread<true>(bx, tx, by, pl.gy, src, pitch, dst, batch, w, h, 0);
                } else {
                    if (pl.form == 16) cvt_pair_vec_thread<false, 16>(bx, tx, by, pl.gy, src, pitch, dst, batch, w, h, la);
                    else if (pl.form == 4) cvt_pair_vec_thread<false, 4>(bx, tx, by, pl.gy, src, pitch, dst, batch, w, h, la);
                    else cvt_pair_byte_thread<false>(bx, tx, by, pl.gy, src, pitch, dst, batch, w, h, la);
                }
            }
    return pl.form;
}

}  // namespace

int main() {
    const int widths[] = {3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 33, 64, 65};
    const int heights[] = {3, 4, 5, 6, 7, gfcvt::kBayerBand - 1, gfcvt::kBayerBand, gfcvt::kBayerBand + 1, 2 * gfcvt::kBayerBand + 1};
    const int pads[] = {0, 1, 2, 3, 5};
    long failures = 0;
    for (int format = 8; format <= 14; format++) {
        long cases = 0, forms[17] = {0};
        const int bpp = gfpix::channels(format);
        for (int w : widths) for (int h : heights) for (int pad : pads) for (int off = 0; off < 4; off++) for (int batch : {1, 3}) {
            const size_t pitch = (size_t)w * bpp + pad, n_in = ((size_t)batch * h - 1) * pitch + (size_t)w * bpp, n_out = (size_t)batch * w * h;
            const int doff = off == 3 ? 1 : 0;   // once the destination off its dword too
            uint8_t* sbuf = (uint8_t*)malloc(off + n_in);   // ends with the last pixel of the last row
            uint8_t* dbuf = (uint8_t*)malloc(kGuard + doff + n_out + kGuard);
            for (size_t i = 0; i < off + n_in; i++) sbuf[i] = rnd();
            if ((w + h + pad) % 7 == 0) for (size_t i = 0; i < off + n_in; i++) sbuf[i] = (i & 1) ? 255 : 0;   // extremes now and then
            std::vector<uint8_t> keep(sbuf, sbuf + off + n_in), want(n_out);
            memset(dbuf, kGuardByte, kGuard + doff + n_out + kGuard);
            uint8_t* dst = dbuf + kGuard + doff;
            reference(sbuf + off, pitch, format, want.data(), batch, w, h);
            const int form = walk(sbuf + off, pitch, format, dst, batch, w, h);
            forms[form]++; cases++;
            bool ok = memcmp(dst, want.data(), n_out) == 0 && memcmp(sbuf, keep.data(), off + n_in) == 0;
            for (int i = 0; i < kGuard + doff; i++) ok = ok && dbuf[i] == kGuardByte;
            for (int i = 0; i < kGuard; i++) ok = ok && dst[n_out + i] == kGuardByte;
            if (!ok) {
                size_t bad = 0, first = n_out;
                for (size_t i = 0; i < n_out; i++) if (dst[i] != want[i]) { if (first == n_out) first = i; bad++; }
                if (failures < 20) printf("format %d %dx%d pad %d offset %d batch %d form %d: FAILED (%zu bytes differ, first at %zu; or guard / source touched)\n", format, w, h, pad, off, batch, form, bad, first);
                failures++;
            }
            free(sbuf); free(dbuf);
        }
        printf("format %d: %ld cases (forms: 16-pixel %ld, 4-pixel %ld, 1-pixel %ld): %s\n", format, cases, forms[16], forms[4], forms[1], failures ? "FAILED" : "ok");
        if ((gfpix::is_bayer(format) ? forms[4] : forms[16] && forms[4]) == 0 || forms[1] == 0) { printf("format %d: a form was never taken\n", format); failures++; }
    }
    return failures ? 1 : 0;
}
