// sg_range_index.h -- the coarse range index of a filed table, in its two layouts, and the one function that files both: k_table_index
// (snowgpu_tables.hip) runs it on the device, tests/host_harness/range_index_vs_search.cpp the same code on the host.
//
//   bin_q   bin-major, q[b][k]: records of bin b nearer than SG_QSTEP_M * k metres.  64 bytes per bin: a reader that wants two
//           neighbouring steps of ONE bin finds them in one line (snowgpu_rows.hip).
//   bin_qs  step-major, qs[k][b], one word per (step, bin): low 16 bits q[b][k], high 16 bits q[b][k + 1] -- for the last step the
//           bin's record count, so that every step has an upper count.  A row holds n_bins + 1 words, the last one bin 0 again: the bin
//           after n_bins - 1 needs no wrap-around test.  The lanes of a wave of the pass over all rows are beams of neighbouring azimuth
//           and similar range: their 8-byte loads of (bin b, bin b + 1) at one step fall on a handful of cache lines, where the four
//           dword loads per beam of the bin-major layout took a line each (sg_beam.h: sg_wave_scan).
//           Only for tables whose longest bin fits 16 bits (SG_QS_MAX_BIN); others have none and the scan uses bin_q.
#pragma once
#include "sg_common.h"

#define SG_QS_MAX_BIN 65535u
#define SG_QS_ROW(n_bins) ((size_t)(n_bins) + 1)                    /* words per step */
#define SG_QS_WORDS(n_bins) ((size_t)SG_QSTEPS * SG_QS_ROW(n_bins))  /* words of the whole array */

#define SG_QS_FITS(max_bin) ((max_bin) <= SG_QS_MAX_BIN)              /* a table gets the step-major index if its longest bin fits the 16-bit counts */

// records of the (range-sorted) bin [e0, e1) nearer than `lim`
__device__ __forceinline__ uint32_t sg_bin_count_below(const SgEntry *entries, uint32_t e0, uint32_t e1, double lim)
{
    uint32_t lo = e0, hi = e1;
    while (lo < hi) {
        const uint32_t m = (lo + hi) >> 1;
        if (entries[m].rho < lim) lo = m + 1; else hi = m;
    }
    return lo - e0;
}

// Entry (bin b, step k) of both layouts.  qs may be null (a bin longer than SG_QS_MAX_BIN records: no step-major index).
__device__ __forceinline__ void sg_range_index_fill(const SgEntry *entries, const uint32_t *start, int n_bins, int b, int k, uint32_t *q, uint32_t *qs)
{
    const uint32_t e0 = start[b], e1 = start[b + 1];
    const uint32_t c = sg_bin_count_below(entries, e0, e1, SG_QSTEP_M * (double)k);
    q[(size_t)b * SG_QSTEPS + k] = c;
    if (!qs) return;
    const uint32_t u = k + 1 < SG_QSTEPS ? sg_bin_count_below(entries, e0, e1, SG_QSTEP_M * (double)(k + 1)) : e1 - e0;
    const uint32_t w = c | (u << 16);
    qs[(size_t)k * SG_QS_ROW(n_bins) + b] = w;
    if (b == 0) qs[(size_t)k * SG_QS_ROW(n_bins) + n_bins] = w;
}
