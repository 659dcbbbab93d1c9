// gf_seq_format.hpp as a stand-alone host program, built with -fsanitize=address,undefined: the limits gf_tracker_set_seq_format checks and the plan of a call on
// a handle whose sequences have formats of their own (rosNodeTest.cpp:238-261 per camera) -- offsets against a plain double loop, every conversion and
// equalisation slot used once and inside its buffer, the source of each stage, the homogeneous verdict, offsets past 2^32.  No HIP, no GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "../../ground-fusion_amd/csrc/gf_seq_format.hpp"

namespace {

long failures = 0;
#define CHECK(c) do { if (!(c)) { if (failures < 30) printf("line %d: %s\n", __LINE__, #c); failures++; } } while (0)

uint32_t rng_state = 97531u;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

const int kFormats[12] = {0, 1, 2, 3, 4, 8, 9, 10, 11, 12, 13, 14};
const int kBytes[12] = {1, 3, 3, 4, 4, 1, 1, 1, 1, 2, 2, 2};

bool refused(int w, int h, int pf, int eq, int hs, const char* field) {
    char msg[256] = "";
    const gf_tracker_seq_format f{pf, eq, hs};
    return !gfseqfmt::fits(w, h, f, msg, sizeof msg) && strstr(msg, field) != nullptr;
}
bool accepted(int w, int h, int pf, int eq, int hs) {
    char msg[256] = "";
    const gf_tracker_seq_format f{pf, eq, hs};
    return gfseqfmt::fits(w, h, f, msg, sizeof msg);
}

void limits() {
    const long before = failures;
    for (int pf = -3; pf <= 40; pf++) {
        bool known = false;
        for (int k : kFormats) known = known || k == pf;
        if (known) CHECK(accepted(160, 120, pf, 0, 0) && accepted(160, 120, pf, 1, 0));
        else CHECK(refused(160, 120, pf, 0, 0, "pixel_format"));
    }
    CHECK(refused(160, 120, 1 << 20, 0, 0, "pixel_format"));
    for (int i = 0; i < 12; i++) {
        const int pf = kFormats[i], row = 160 * kBytes[i];
        CHECK(gfseqfmt::row_bytes(160, pf) == (size_t)row && gfseqfmt::frame_bytes(160, 120, pf) == (size_t)row * 120);
        CHECK(accepted(160, 120, pf, 0, row) && accepted(160, 120, pf, 1, row + 5) && accepted(160, 120, pf, 0, 1 << 30));
        CHECK(refused(160, 120, pf, 0, row - 1, "host_stride") && refused(160, 120, pf, 0, 1, "host_stride"));
        CHECK(refused(160, 120, pf, 0, -1, "host_stride") && refused(160, 120, pf, 1, -(1 << 30), "host_stride"));
        CHECK(refused(160, 120, pf, -1, 0, "equalize") && refused(160, 120, pf, 2, 0, "equalize") && refused(160, 120, pf, 255, 0, "equalize"));
        CHECK(refused(8, 120, pf, 1, 0, "equalize") && refused(160, 8, pf, 1, 0, "equalize") && accepted(9, 9, pf, 1, 0));   // CLAHE's 8 x 8 grid
        const bool bayer = pf >= 8 && pf <= 11;
        CHECK(bayer ? refused(2, 120, pf, 0, 0, "pixel_format") && refused(160, 2, pf, 0, 0, "pixel_format") : accepted(2, 120, pf, 0, 0) && accepted(160, 1, pf, 0, 0));
        CHECK(accepted(3, 3, pf, 0, 0));
    }
    gf_tracker_cfg cfg{};
    cfg.pixel_format = GF_PIX_BGRA8; cfg.equalize = 1;
    const gf_tracker_seq_format own = gfseqfmt::of_handle(cfg);
    CHECK(own.pixel_format == GF_PIX_BGRA8 && own.equalize == 1 && own.host_stride == 0);
    CHECK(gfseqfmt::host_stride(gf_tracker_seq_format{0, 0, 0}, 640) == 640 && gfseqfmt::host_stride(gf_tracker_seq_format{0, 0, 700}, 640) == 700);
    printf("limits: %s\n", failures == before ? "ok" : "FAILED");
}

// one call: the plan of `seq` against everything written out again
void check_call(const std::vector<gf_tracker_seq_format>& fmt, const gf_tracker_seq_format& own, const std::vector<int>& seq, int w, int h, bool by_refs) {
    const int B = (int)fmt.size(), N = (int)seq.size();
    const size_t px = (size_t)w * h;
    gfseqfmt::Plan p;
    gfseqfmt::plan_list(p, fmt.data(), own, N, seq.data(), w, h);
    // offsets and sizes: a plain double loop over the rows of the frames listed before
    bool homogeneous = true;
    int n_cvt = 0, n_eq = 0;
    for (int i = 0; i < N; i++) {
        size_t off = 0;
        for (int j = 0; j < i; j++) for (int y = 0; y < h; y++) off += (size_t)w * gfpix::channels(fmt[seq[j]].pixel_format);
        CHECK(p.offset[i] == off);
        CHECK(p.bytes[i] == (size_t)w * h * gfpix::channels(fmt[seq[i]].pixel_format));
        CHECK(p.format[i] == fmt[seq[i]].pixel_format && p.equalize[i] == fmt[seq[i]].equalize);
        if (fmt[seq[i]].pixel_format != own.pixel_format || fmt[seq[i]].equalize != own.equalize) homogeneous = false;
        n_cvt += fmt[seq[i]].pixel_format != GF_PIX_MONO8; n_eq += fmt[seq[i]].equalize;
    }
    CHECK(p.count == N && p.homogeneous == homogeneous && p.n_cvt == n_cvt && p.n_eq == n_eq);
    CHECK(p.total_bytes == (N ? p.offset[N - 1] + p.bytes[N - 1] : 0));
    // where the caller's frames lie: a tight block, or anywhere
    const uintptr_t base = 0x7000000000ull, cvt_buf = 0x100000000ull, eq_buf = 0x200000000ull;
    std::vector<gf_frame_ref> frames(N);
    if (by_refs) for (int i = 0; i < N; i++) frames[i] = gf_frame_ref{reinterpret_cast<const void*>(base + (uintptr_t)(rnd() % 1000) * 4099u + i), gfseqfmt::row_bytes(w, p.format[i]) + rnd() % 9};
    else {
        gfseqfmt::tight_frames(p, reinterpret_cast<const void*>(base), w, frames.data());
        for (int i = 0; i < N; i++) CHECK(reinterpret_cast<uintptr_t>(frames[i].data) == base + p.offset[i] && frames[i].pitch == (size_t)w * gfpix::channels(p.format[i]));
    }
    gfseqfmt::plan_sources(p, frames.data(), reinterpret_cast<const void*>(cvt_buf), reinterpret_cast<const void*>(eq_buf), w, h);
    CHECK((int)p.cvt_src.size() == N && (int)p.pyr_src.size() == N && (int)p.eq_src.size() == n_eq);
    std::set<uintptr_t> cvt_slots, eq_slots;
    auto same = [](const gf_frame_ref& a, const gf_frame_ref& b) { return a.data == b.data && a.pitch == b.pitch; };
    for (int i = 0; i < N; i++) {
        const bool cvt = p.format[i] != GF_PIX_MONO8, eq = p.equalize[i] != 0;
        const gf_frame_ref cslot{reinterpret_cast<const void*>(cvt_buf + (size_t)i * px), (size_t)w};
        CHECK(p.cvt_format[i] == (cvt ? p.format[i] : -1));
        if (cvt) {
            CHECK(same(p.cvt_src[i], frames[i]));
            CHECK(cvt_slots.insert((uintptr_t)i).second && (size_t)i * px + px <= (size_t)B * px);   // the slot is the list position: used once, inside [B] frames
        } else CHECK(p.cvt_src[i].data == nullptr);
        gf_frame_ref last = cvt ? cslot : frames[i];
        if (eq) {
            const int j = p.eq_index[i];
            CHECK(j >= 0 && j < n_eq && j < B && eq_slots.insert((uintptr_t)j).second);
            if (j >= 0 && j < n_eq) CHECK(same(p.eq_src[j], last));
            last = gf_frame_ref{reinterpret_cast<const void*>(eq_buf + (size_t)j * px), (size_t)w};
        } else CHECK(p.eq_index[i] == -1);
        CHECK(same(p.pyr_src[i], last));
        if (!cvt && !eq) CHECK(same(p.pyr_src[i], frames[i]));   // a MONO8 sequence without equalisation: the caller's frame itself, not a copy
    }
    CHECK((int)cvt_slots.size() == n_cvt && (int)eq_slots.size() == n_eq);
    // the equalised positions are numbered in list order
    int next = 0;
    for (int i = 0; i < N; i++) if (p.equalize[i]) CHECK(p.eq_index[i] == next++);
}

void plans() {
    const long before = failures;
    long calls = 0;
    // 30 sequences: every format with both switches, and six that keep the handle's own values
    for (int own_case = 0; own_case < 3; own_case++) {
        const gf_tracker_seq_format own = own_case == 0 ? gf_tracker_seq_format{0, 0, 0} : own_case == 1 ? gf_tracker_seq_format{GF_PIX_RGBA8, 1, 0} : gf_tracker_seq_format{GF_PIX_BAYER_GBRG8, 0, 0};
        std::vector<gf_tracker_seq_format> fmt(30, own);
        for (int i = 0; i < 24; i++) fmt[i] = gf_tracker_seq_format{kFormats[i % 12], i / 12, (i % 5 == 0) ? 4096 : 0};
        for (int round = 0; round < 60; round++) {
            std::vector<int> seq(30);
            for (int i = 0; i < 30; i++) seq[i] = i;
            for (int i = 29; i > 0; i--) std::swap(seq[i], seq[rnd() % (i + 1)]);
            seq.resize(round == 0 ? 30 : round == 1 ? 0 : 1 + rnd() % 30);   // everyone, no one, and lists that leave sequences out
            check_call(fmt, own, seq, round % 2 ? 160 : 36, round % 3 ? 120 : 34, round % 4 == 3);
            calls++;
        }
        // the verdict: only sequences that run with the handle's own values
        gfseqfmt::Plan p;
        const int keep[4] = {27, 24, 29, 25};
        gfseqfmt::plan_list(p, fmt.data(), own, 4, keep, 160, 120);
        CHECK(p.homogeneous);
        const int one_other[4] = {27, 24, own_case == 1 ? 0 : 15, 25};   // (MONO8, 0) under an (RGBA8, 1) handle; (RGBA8, 1) under the others
        gfseqfmt::plan_list(p, fmt.data(), own, 4, one_other, 160, 120);
        CHECK(!p.homogeneous);
        // a sequence set to the handle's own values with only a host stride of its own is still homogeneous
        fmt[26] = gf_tracker_seq_format{own.pixel_format, own.equalize, 8192};
        const int strided[2] = {26, 28};
        gfseqfmt::plan_list(p, fmt.data(), own, 2, strided, 160, 120);
        CHECK(p.homogeneous);
    }
    printf("plans: %ld calls: %s\n", calls, failures == before ? "ok" : "FAILED");
}

void large() {
    const long before = failures;
    // 40 frames of 8192 x 8192 in RGBA8 and MONO16: 256 MiB and 128 MiB each, the block is past 2^32 after the sixteenth; nothing is allocated
    const int w = 8192, h = 8192, B = 40;
    std::vector<gf_tracker_seq_format> fmt(B);
    std::vector<int> seq(B);
    for (int i = 0; i < B; i++) { fmt[i] = gf_tracker_seq_format{i % 2 ? GF_PIX_MONO16 : GF_PIX_RGBA8, i % 3 == 0, 0}; seq[i] = B - 1 - i; }
    gfseqfmt::Plan p;
    gfseqfmt::plan_list(p, fmt.data(), gf_tracker_seq_format{0, 0, 0}, B, seq.data(), w, h);
    unsigned long long off = 0;
    for (int i = 0; i < B; i++) {
        CHECK((unsigned long long)p.offset[i] == off);
        off += (unsigned long long)w * h * (seq[i] % 2 ? 2 : 4);
    }
    CHECK((unsigned long long)p.total_bytes == off && off == 20ull * (1ull << 28) + 20ull * (1ull << 27) && off > (1ull << 32));
    std::vector<gf_frame_ref> frames(B);
    const uintptr_t base = 0x10000ull;
    gfseqfmt::tight_frames(p, reinterpret_cast<const void*>(base), w, frames.data());
    CHECK(reinterpret_cast<uintptr_t>(frames[B - 1].data) == base + p.offset[B - 1] && reinterpret_cast<uintptr_t>(frames[B - 1].data) - base > (1ull << 32));
    gfseqfmt::plan_sources(p, frames.data(), reinterpret_cast<const void*>(0x100000000000ull), reinterpret_cast<const void*>(0x200000000000ull), w, h);
    CHECK(reinterpret_cast<uintptr_t>(p.pyr_src[B - 2].data) == (fmt[seq[B - 2]].equalize ? 0x200000000000ull + (unsigned long long)p.eq_index[B - 2] * w * h : 0x100000000000ull + (unsigned long long)(B - 2) * w * h));
    CHECK((unsigned long long)(B - 2) * w * h > (1ull << 31));
    printf("large: %s\n", failures == before ? "ok" : "FAILED");
}

}  // namespace

int main() {
    limits();
    plans();
    large();
    printf(failures ? "all: FAILED\n" : "all: ok\n");
    return failures ? 1 : 0;
}
