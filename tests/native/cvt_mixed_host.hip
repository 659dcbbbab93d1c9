// cvt_mixed_kernel of csrc/gf_cvt_kernels.hpp (one pixel format per frame, gf_tracker_set_seq_format / gf_cvt_gray_mixed*) walked on the CPU: every (block,
// thread) of the launches the library would make -- the part of the streaming formats and the Bayer part, with the grid of a call that can read its tables
// and with the grid of one that cannot -- through gfcvt::cvt_mixed_block, the function the kernel itself calls, on heap buffers of exactly the frames' sizes.
// One launch holds all twelve formats plus skipped entries, each frame with its own source offset (0 .. 3; offset 0 of a heap block is 16-aligned) and its own
// pitch (tight or odd).  Every source is its own allocation that ends with the last pixel of its last row, so a read outside a frame reads outside its
// allocation, which the AddressSanitizer build reports.  The destination is compared whole with a plain double loop over the definitions of gf_pixfmt.hpp:
// the slots of skipped entries and the guard bands on both sides must keep their fill.  hipcc compiles it; no HIP call is made, so it runs without a GPU.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ground-fusion_amd/csrc/gf_cvt_kernels.hpp"

namespace {

const int kGuard = 64;
const uint8_t kFill = 0x5A;

uint32_t rng_state = 2468u;
uint32_t rnd32() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
uint8_t rnd() { return (uint8_t)rnd32(); }

// the definition of one pixel: a double loop calls it, nothing of the kernels is used
uint8_t definition(const uint8_t* f, size_t pitch, int format, int w, int h, int y, int x) {
    const uint8_t* row = f + (size_t)y * pitch;
    if (gfpix::is_bayer(format)) {
        const int yc = gfpix::bayer_clamp(y, h), xc = gfpix::bayer_clamp(x, w);
        const uint8_t* c = f + (size_t)yc * pitch;
        return gfpix::bayer_gray(gfpix::bayer_green_first(format), gfpix::bayer_blue_row0(format), yc, xc, c - pitch, c, c + pitch);
    }
    if (format == GF_PIX_MONO16) return gfpix::mono16_gray((unsigned)row[2 * x] | ((unsigned)row[2 * x + 1] << 8));
    if (format == GF_PIX_YUV422_UYVY || format == GF_PIX_YUV422_YUY2) return row[2 * x + gfpix::luma_at(format)];
    if (format == GF_PIX_MONO8) return row[x];
    const int ch = gfpix::channels(format);
    return gfpix::gray(row[(size_t)x * ch + gfpix::red_at(format)], row[(size_t)x * ch + 1], row[(size_t)x * ch + gfpix::blue_at(format)]);
}

struct Entry { uint8_t* alloc; const uint8_t* data; size_t pitch, bytes; int format, off; std::vector<uint8_t> keep; };

// one launch of a part over a grid
template <int PART> void walk(const std::vector<Entry>& e, unsigned gx, uint8_t* dst, int w, int h, int dst_dwords) {
    const int batch = (int)e.size();
    const unsigned gy = (unsigned)batch > 5 ? (unsigned)batch - 3 : (unsigned)batch;   // fewer rows of blocks than frames: the strided walk over the list
    auto entry = [&](int b, const uint8_t*& data, size_t& pitch, int& format) { data = e[b].data; pitch = e[b].pitch; format = e[b].format; };
    for (unsigned by = 0; by < gy; by++)
        for (unsigned bx = 0; bx < gx; bx++)
            for (unsigned tx = 0; tx < (unsigned)gfcvt::kThreads; tx++) gfcvt::cvt_mixed_block<PART>(bx, gx, by, gy, tx, entry, dst, batch, w, h, dst_dwords);
}

}  // namespace

int main() {
    using namespace gfcvt;
    const int widths[] = {3, 5, 8, 12, 16, 20, 33, 48, 65};
    const int heights[] = {3, 4, kBayerBand - 1, kBayerBand, kBayerBand + 1, 2 * kBayerBand + 1};
    const int formats[] = {0, 1, 2, 3, 4, 8, 9, 10, 11, 12, 13, 14, -1, 5};   // all twelve, and two entries that are skipped: the tracker's -1 and a value that is no format
    long failures = 0, cases = 0, forms[17] = {0}, turns = 0;
    for (int w : widths) for (int h : heights) for (int round = 0; round < 6; round++) {
        std::vector<int> order(formats, formats + 14);
        for (int i = 13; i > 0; i--) std::swap(order[i], order[rnd32() % (i + 1)]);   // permuted: a frame's slot is its list position, whatever its format
        const int batch = 14, doff = round == 5 ? 1 : 0;   // once the destination off its dword: every frame takes the one-pixel form
        const bool known = round & 1;                      // the grid of a call that reads its tables / of one that cannot
        std::vector<Entry> e(batch);
        const size_t px = (size_t)w * h, n_out = (size_t)batch * px;
        for (int b = 0; b < batch; b++) {
            Entry& q = e[b];
            q.format = order[b];
            const int bpp = gfpix::valid(q.format) ? gfpix::channels(q.format) : 1;
            q.off = (int)((b + round) % 4);
            const int pad = (b + round / 2) % 3 == 0 ? 0 : (b % 2 ? 4 * (1 + (int)(rnd32() % 3)) : 1 + 2 * (int)(rnd32() % 3));   // tight, a multiple of 4, odd
            q.pitch = (size_t)w * bpp + pad;
            q.bytes = (size_t)(h - 1) * q.pitch + (size_t)w * bpp;   // ends with the last pixel of the last row
            q.alloc = (uint8_t*)malloc(q.off + q.bytes);
            for (size_t i = 0; i < q.off + q.bytes; i++) q.alloc[i] = (w + h + b) % 11 == 0 ? ((i & 1) ? 255 : 0) : rnd();
            q.data = q.alloc + q.off;
            q.keep.assign(q.alloc, q.alloc + q.off + q.bytes);
        }
        uint8_t* dbuf = (uint8_t*)malloc(kGuard + doff + n_out + kGuard);
        memset(dbuf, kFill, kGuard + doff + n_out + kGuard);
        uint8_t* dst = dbuf + kGuard + doff;
        std::vector<uint8_t> want(n_out, kFill);
        for (int b = 0; b < batch; b++)
            if (gfpix::valid(e[b].format))
                for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) want[(size_t)b * px + (size_t)y * w + x] = definition(e[b].data, e[b].pitch, e[b].format, w, h, y, x);
        // the grids of cvt_launch_mixed (csrc/gf_cvt.hip)
        const int dst_dwords = !((reinterpret_cast<uintptr_t>(dst) | (size_t)w) & 3) ? 1 : 0;
        unsigned gx_stream = 0, gx_bayer = 0, most = 0;
        for (int b = 0; b < batch; b++) {
            if (!gfpix::valid(e[b].format)) continue;
            const int form = mixed_form(e[b].format, e[b].data, e[b].pitch, dst_dwords, w);
            forms[form]++;
            const unsigned need = mixed_blocks(e[b].format, form, w, h);
            most = std::max(most, need);
            if (gfpix::is_bayer(e[b].format)) gx_bayer = std::max(gx_bayer, need); else gx_stream = std::max(gx_stream, need);
        }
        if (!known) {
            gx_stream = mixed_blocks(GF_PIX_MONO8, dst_dwords ? ((w & 15) ? 4 : 16) : 1, w, h);
            gx_bayer = mixed_blocks(GF_PIX_BAYER_RGGB8, dst_dwords && w >= 8 ? 4 : 1, w, h);
            if (most > std::min(gx_stream, gx_bayer)) turns++;   // a frame that needs more blocks than the grid has
        }
        walk<1>(e, gx_stream, dst, w, h, dst_dwords);
        walk<2>(e, gx_bayer, dst, w, h, dst_dwords);
        cases++;
        bool ok = memcmp(dst, want.data(), n_out) == 0;
        for (int i = 0; i < kGuard + doff; i++) ok = ok && dbuf[i] == kFill;
        for (int i = 0; i < kGuard; i++) ok = ok && dst[n_out + i] == kFill;
        for (int b = 0; b < batch; b++) ok = ok && memcmp(e[b].alloc, e[b].keep.data(), e[b].keep.size()) == 0;
        if (!ok) {
            if (failures < 20) {
                size_t first = n_out;
                for (size_t i = 0; i < n_out && first == n_out; i++) if (dst[i] != want[i]) first = i;
                printf("%dx%d round %d: FAILED (first differing byte %zu = entry %zu, format %d; or a guard / source was touched)\n", w, h, round, first, first / px, first < n_out ? e[first / px].format : -9);
            }
            failures++;
        }
        for (int b = 0; b < batch; b++) free(e[b].alloc);
        free(dbuf);
    }
    printf("mixed launches: %ld cases of 12 formats + 2 skipped entries (frames by form: 16-pixel %ld, 4-pixel %ld, 1-pixel %ld; %ld launches with a frame that took several turns): %s\n",
           cases, forms[16], forms[4], forms[1], turns, failures ? "FAILED" : "ok");
    if (!forms[16] || !forms[4] || !forms[1] || !turns) { printf("a form or the strided walk was never taken\n"); failures++; }
    printf(failures ? "all: FAILED\n" : "all: ok\n");
    return failures ? 1 : 0;
}
