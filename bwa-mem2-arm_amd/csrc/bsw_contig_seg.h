// bsw_contig_seg.h -- the contig table's lookup (include/bsw_contigs.h, "SEGMENTS"), stated once
// for the host and for every stage kernel.  A ContigView goes into a kernel's parameters by value:
// pointers into HBM (DeviceCtx::d_ctg_*), never arrays.  off == nullptr: no table is set and the
// stage runs the code it ran before the table existed.
#pragma once
#include <stdint.h>
#include "bsw_formulas.h"

namespace bsw {

struct ContigView {
    const int64_t *off;                 // [n + 1] prefix sums of the lengths; nullptr: no table
    const uint8_t *names;               // the names' bytes, flat
    const int32_t *name_off;            // [n + 1]: contig k's name is names[name_off[k], name_off[k + 1])
    int32_t n;
    int64_t l_pac;                      // the call's: > 0 two strands (off[n] == l_pac), 0 one strand
};

// the contig of forward coordinate y: the largest k with off[k] <= y, clamped to [0, n) -- so any y,
// in range or not, reads inside the table
BSW_HD int contig_of(const ContigView &c, int64_t y)
{
    int lo = 0, hi = c.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (c.off[mid] <= y) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// seg(x) on the (two-strand) text: the reverse strand's segments are the forward ones mirrored
BSW_HD int contig_seg(const ContigView &c, int64_t x)
{
    if (c.l_pac > 0 && x >= c.l_pac) return 2 * c.n - 1 - contig_of(c, 2 * c.l_pac - 1 - x);
    return contig_of(c, x);
}

BSW_HD int contig_rid(const ContigView &c, int64_t x)
{
    const int s = contig_seg(c, x);
    return s < c.n ? s : 2 * c.n - 1 - s;
}

// bns_fetch_seq(.., mid, ..): [lo, hi) clipped to the segment that holds mid; returns that segment's rid
BSW_HD int contig_clip(const ContigView &c, int64_t mid, int64_t &lo, int64_t &hi)
{
    const int s = contig_seg(c, mid);
    const bool fwd = s < c.n;
    const int k = fwd ? s : 2 * c.n - 1 - s;
    const int64_t b0 = fwd ? c.off[k] : 2 * c.l_pac - c.off[k + 1], b1 = fwd ? c.off[k + 1] : 2 * c.l_pac - c.off[k];
    if (lo < b0) lo = b0;
    if (hi > b1) hi = b1;
    return k;
}

// [b, e), b < e, bridges a join (the strand boundary included)
BSW_HD bool contig_crosses(const ContigView &c, int64_t b, int64_t e) { return contig_seg(c, b) != contig_seg(c, e - 1); }

}  // namespace bsw
