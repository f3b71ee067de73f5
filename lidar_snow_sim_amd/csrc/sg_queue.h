// sg_queue.h -- the dict queue of the pass over all rows (SgBeamArgs::dq): its layout, the store of a slot and the load / resolution of one.
//
// A beam that met flakes hands k_power / k_power_few its range, its azimuth and ONE WORD per listed flake (sg_beam.h: sg_hit_word -- the
// record's index in its table | bit 30: the right interval angle is the beam's right limit | bit 31: the left one its left limit), the
// word the scan's own LDS list holds.  The interval angles and the range of a flake are the record's tangent angles and range unless a bit
// says otherwise, so the READER resolves the word: the records are cache-resident lines the scan just read, the reader's memory path is
// idle where the scan's is its limit, and the beam's limits are computed on the reader's side anyway (phase 2).
//
// Layout: "blocked SoA" in 32-bit words.  64 consecutive slots form a group; a group holds its planes back to back: the ranges (H words
// per slot), the azimuths (H words per slot), then `lmax` planes of one word per slot -- 64 (2 H + lmax) words per group.  A wave reads /
// writes a contiguous run per plane, and everything a beam needs sits within one group.  H: 32-bit words per header field --
//   SG_DQ_ROW_HEADER 1   range and azimuth in the ROW dtype (float32 rows: one word each, widened by the reader: the double that was stored
//                        before was the widening of exactly these values)
//   SG_DQ_ROW_HEADER 0   float64 whatever the rows are
// lmax is the first pass's list capacity (4, 8, 16, 63): the format is the same for every one of them.
// Plane numbers: 0 = range, 1 = azimuth, 2 + j = word of flake j (near -> far).
// The tier hand-over buffers (tq) and the overflow slots (ov) keep float64 planes of (a1, a2, rho): other code writes them.
#pragma once
#include "sg_beam.h"

#ifndef SG_DQ_ROW_HEADER
#define SG_DQ_ROW_HEADER 1
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define SG_DQ_RECORD(entries, w) (sg_gptr(entries) + ((w) & 0x3fffffffu))
#else
#define SG_DQ_RECORD(entries, w) ((entries) + ((w) & 0x3fffffffu))
#endif

// 32-bit words per header field for rows of `elem_size` bytes per element
__host__ __device__ __forceinline__ constexpr int sg_dq_hdr(int elem_size) { return SG_DQ_ROW_HEADER ? elem_size / 4 : 2; }
// 32-bit words per slot (host: the queue of n slots takes (n + 64) of these -- whole groups)
__host__ __device__ __forceinline__ constexpr int sg_dq_slot_words(int lmax, int hdr) { return 2 * hdr + lmax; }
// first 32-bit word of cell (slot, plane); a header cell is `hdr` words long and aligned to as many
__host__ __device__ __forceinline__ int64_t sg_dq_cell(int64_t slot, int plane, int lmax, int hdr)
{
    const int64_t group = (slot >> 6) * (int64_t)(64 * sg_dq_slot_words(lmax, hdr));
    const int c = (int)(slot & 63);
    return plane < 2 ? group + (int64_t)((plane * 64 + c) * hdr) : group + (int64_t)(128 * hdr + (plane - 2) * 64 + c);
}

// ---- writer (k_beams) ----
template <typename T>
__host__ __device__ __forceinline__ void sg_dq_store_header(uint32_t *q, int64_t slot, int lmax, T d_t, T theta_t)
{
    constexpr int H = sg_dq_hdr((int)sizeof(T));
    using S = std::conditional_t<H == 2, double, float>;      // (H == 1: float32 rows, stored as they are)
    *reinterpret_cast<S *>(q + sg_dq_cell(slot, 0, lmax, H)) = (S)d_t;
    *reinterpret_cast<S *>(q + sg_dq_cell(slot, 1, lmax, H)) = (S)theta_t;
}
template <typename T>
__host__ __device__ __forceinline__ void sg_dq_store_word(uint32_t *q, int64_t slot, int lmax, int j, uint32_t w)
{
    q[sg_dq_cell(slot, 2 + j, lmax, sg_dq_hdr((int)sizeof(T)))] = w;
}

// ---- readers (k_power_few, k_power) ----
// range and azimuth, widened (exact)
template <typename T>
__host__ __device__ __forceinline__ void sg_dq_load_header(const uint32_t *q, int64_t slot, int lmax, double &d, double &theta_c)
{
    constexpr int H = sg_dq_hdr((int)sizeof(T));
    using S = std::conditional_t<H == 2, double, float>;
    d = (double)*reinterpret_cast<const S *>(q + sg_dq_cell(slot, 0, lmax, H));
    theta_c = (double)*reinterpret_cast<const S *>(q + sg_dq_cell(slot, 1, lmax, H));
}
template <typename T>
__host__ __device__ __forceinline__ uint32_t sg_dq_load_word(const uint32_t *q, int64_t slot, int lmax, int j)
{
    return q[sg_dq_cell(slot, 2 + j, lmax, sg_dq_hdr((int)sizeof(T)))];
}

// One word resolved: interval angles (geometry.py:26-27) and range of the flake, given the beam's limits (sg_beam_limits of its azimuth).
__host__ __device__ __forceinline__ void sg_dq_resolve(uint32_t w, const SgEntry *__restrict__ entries, double theta_r, double theta_l, double &a1, double &a2,
                                                       double &rho)
{
    const auto *f = SG_DQ_RECORD(entries, w);
    a1 = (w & 0x40000000u) ? theta_r : f->t0;
    a2 = (w & 0x80000000u) ? theta_l : f->t1;
    rho = f->rho;
}
// the range alone (k_power's three-column form fetches it again after the dict)
__host__ __device__ __forceinline__ double sg_dq_rho(uint32_t w, const SgEntry *__restrict__ entries) { return SG_DQ_RECORD(entries, w)->rho; }

// N words with ONE round of loads: the tail of every record -- tangent angles (16 bytes) and range (8 bytes) -- is requested before the
// first is used, whether the word is one of the list (j < L) and whether its bits will want the angles or not: under those conditions
// the compiler waits for each record before it asks for the next.  w[j], j >= L: any value (record 0 is read; a1 / a2 / rho[j] unspecified).
template <int N>
__host__ __device__ __forceinline__ void sg_dq_resolve_all(const uint32_t (&w)[N], int L, const SgEntry *__restrict__ entries, double theta_r, double theta_l,
                                                           double (&a1)[N], double (&a2)[N], double (&rho)[N])
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned int Raw2 __attribute__((ext_vector_type(2)));
    SgTailRaw ang[N];
    Raw2 rng[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const SG_GLOBAL SgEntry *f = SG_DQ_RECORD(entries, j < L ? w[j] : 0u);
        ang[j] = *reinterpret_cast<const SG_GLOBAL SgTailRaw *>(&f->t0);
        rng[j] = *reinterpret_cast<const SG_GLOBAL Raw2 *>(&f->rho);
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
        a1[j] = (w[j] & 0x40000000u) ? theta_r : __hiloint2double((int)ang[j].y, (int)ang[j].x);
        a2[j] = (w[j] & 0x80000000u) ? theta_l : __hiloint2double((int)ang[j].w, (int)ang[j].z);
        rho[j] = __hiloint2double((int)rng[j].y, (int)rng[j].x);
    }
#else
    for (int j = 0; j < N; ++j) sg_dq_resolve(j < L ? w[j] : 0u, entries, theta_r, theta_l, a1[j], a2[j], rho[j]);
#endif
}
