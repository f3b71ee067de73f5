// sg_range_index.h -- the range index of a filed table, in its two layouts, and the one function that files both: k_table_index
// (snowgpu_tables.hip) runs it on the device, the harnesses under tests/host_harness the same code on the host.
//
//   bin_q   bin-major, q[b][k]: records of bin b nearer than SG_QSTEP_M * k metres, SG_QSTEPS steps.  64 bytes per bin: a reader that
//           wants two neighbouring steps of ONE bin finds them in one line (snowgpu_rows.hip).
//   bin_qs  step-major, qs[k][b], one word per (step, bin): low 16 bits the records of bin b nearer than step_m * k metres, high 16 bits
//           those nearer than step_m * (k + 1) -- for the last step the bin's record count, so that every step has an upper count.  A row
//           holds n_bins + 1 words, the last one bin 0 again: the bin after n_bins - 1 needs no wrap-around test.  The lanes of a wave of
//           the pass over all rows are beams of neighbouring azimuth and similar range: their 8-byte loads of (bin b, bin b + 1) at one
//           step fall on a handful of cache lines (sg_beam.h: sg_wave_scan).  That scan takes every record below the UPPER count of the
//           target's step as a candidate and searches nothing, so the step length decides how many candidates lie beyond the target.
//           Its shape -- steps, step length -- travels in the table descriptor (SgTable: qs_steps, qs_per_m); the library files
//           SG_QS_FILE_STEPS steps of SG_QS_FILE_STEP_M metres, and a descriptor that names no shape has SG_QSTEPS steps of SG_QSTEP_M.
//           Only for tables whose longest bin fits 16 bits (SG_QS_MAX_BIN); others have none and the scan searches from bin_q.
#pragma once
#include "sg_common.h"

#define SG_QS_MAX_BIN 65535u
#define SG_QS_ROW(n_bins) ((size_t)(n_bins) + 1)                    /* words per step */
#define SG_QS_WORDS_OF(steps, n_bins) ((size_t)(steps) * SG_QS_ROW(n_bins))   /* words of a whole array of `steps` steps */
#define SG_QS_WORDS(n_bins) SG_QS_WORDS_OF(SG_QSTEPS, n_bins)        /* ... of the legacy shape */

#define SG_QS_FITS(max_bin) ((max_bin) <= SG_QS_MAX_BIN)              /* a table gets the step-major index if its longest bin fits the 16-bit counts */

// The step-major index the library files with a table (snowgpu_api.cpp: register_table): 64 steps of 2 m -- ranges from 126 m on share
// the last step.  At most 64 steps (k_table_index is one wave per bin, one lane per step); the step length a power of two (SgTable).
#ifndef SG_QS_FILE_STEPS
#define SG_QS_FILE_STEPS 64
#define SG_QS_FILE_STEP_M 2.0
#endif

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

// Entry (bin b, step k) of an index of `steps` steps of `step_m` metres, in either layout or both: q (bin-major, `steps` words per bin)
// and qs (step-major) may each be null.
__device__ __forceinline__ void sg_range_index_fill_steps(const SgEntry *entries, const uint32_t *start, int n_bins, int b, int k, int steps, double step_m,
                                                          uint32_t *q, uint32_t *qs)
{
    const uint32_t e0 = start[b], e1 = start[b + 1];
    const uint32_t c = sg_bin_count_below(entries, e0, e1, step_m * (double)k);
    if (q) q[(size_t)b * steps + k] = c;
    if (!qs) return;
    const uint32_t u = k + 1 < steps ? sg_bin_count_below(entries, e0, e1, step_m * (double)(k + 1)) : e1 - e0;
    const uint32_t w = c | (u << 16);
    qs[(size_t)k * SG_QS_ROW(n_bins) + b] = w;
    if (b == 0) qs[(size_t)k * SG_QS_ROW(n_bins) + n_bins] = w;
}

// The same for the legacy shape, SG_QSTEPS steps of SG_QSTEP_M metres, both layouts.  qs may be null (a bin longer than SG_QS_MAX_BIN
// records: no step-major index).
__device__ __forceinline__ void sg_range_index_fill(const SgEntry *entries, const uint32_t *start, int n_bins, int b, int k, uint32_t *q, uint32_t *qs)
{
    sg_range_index_fill_steps(entries, start, n_bins, b, k, SG_QSTEPS, SG_QSTEP_M, q, qs);
}
