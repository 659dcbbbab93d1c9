// The rules of csrc/gf_frame_ref.hpp that host and device share, on the CPU: for every line "data pitch row_bytes u16 may_be_null" on stdin (numbers; data is
// an address that is never dereferenced) one line "verdict form unaligned16 unaligned4" on stdout.  Plain C++: the header needs no HIP for this part.
#include <cstdio>

#include "../../ground-fusion_amd/csrc/gf_frame_ref.hpp"

int main() {
    unsigned long long data, pitch, row;
    int u16, may_null;
    while (std::scanf("%llu %llu %llu %d %d", &data, &pitch, &row, &u16, &may_null) == 5) {
        gf_frame_ref r;
        r.data = reinterpret_cast<const void*>(static_cast<uintptr_t>(data));
        r.pitch = static_cast<size_t>(pitch);
        std::printf("%d %d %d %d\n", (int)gfref::check(r, static_cast<size_t>(row), u16 != 0, may_null != 0), gfref::form(static_cast<uintptr_t>(data), r.pitch),
                    (int)gfref::unaligned(static_cast<uintptr_t>(data), r.pitch, 16), (int)gfref::unaligned(static_cast<uintptr_t>(data), r.pitch, 4));
    }
    return 0;
}
