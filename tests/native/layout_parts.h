// layout_parts.h — what rebuild_check.cpp, blas_check.cpp and shapes_check.cpp ask of a device workspace carved by
// ptsharp_amd/csrc/pt_update_layout.h.  They lay it out from a null base, so a part's pointer is its offset, and
// state per part, from the tables' counts, the bytes its kernel indexes.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

struct LayoutPart {
    const void* at;   // where the part starts
    size_t need;      // the bytes its kernel indexes
};
// The rules broken: every part 256-B aligned, the parts in the order given with none reaching into the next, the
// last one inside `bytes`, and never an empty allocation.
inline int layout_violations(const std::vector<LayoutPart>& parts, size_t bytes) {
    int bad = 0;
    size_t end = 0;
    for (const LayoutPart& p : parts) {
        const size_t off = (size_t)(uintptr_t)p.at;
        bad += off % 256 != 0;
        bad += off < end;
        end = off + p.need;
    }
    return bad + (end > bytes) + (bytes == 0);
}
