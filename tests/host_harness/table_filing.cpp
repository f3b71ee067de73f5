// Host harness: the product's host filing of a snowflake table (sg_table_host.h: sg_file_table_host) and the range index as the library
// files it (sg_range_index.h: sg_range_index_fill_steps -- the function k_table_index runs on the device -- for bin_q, SG_QSTEPS steps of
// SG_QSTEP_M metres, and for bin_qs, SG_QS_FILE_STEPS steps of SG_QS_FILE_STEP_M metres, the latter only if the longest bin fits 16 bits),
// written out whole for tests/test_table_filing.py to compare with its NumPy restatement.
//   in:  int64 K, then K x 3 float64 (x, y, disk radius)
//   out: int32 rc (sg_file_table_host: 0, 1 bad row, 2 too many records), int64 bad row (-1), uint32 max_bin, uint32 n_entries, int32 has_qs;
//        and for rc == 0: bin_start (SG_NBINS + 1 uint32); per record src, flags (uint32 each) and rho (float64); whether the spare record
//        behind the last bin is all zero bytes (int32); bin_q (SG_NBINS x SG_QSTEPS uint32); bin_qs (SG_QS_FILE_STEPS x (SG_NBINS + 1) uint32)
//        if has_qs.  Index words nobody wrote keep the filler 0xdeadbeef.
// usage: table_filing <in> <out>; exit status 0 unless a file could not be read or written.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>
#undef __device__
#define __device__
#include "sg_range_index.h"
#include "sg_table_host.h"

template <typename T> static bool put(FILE *f, const T *p, size_t n) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: table_filing <in> <out>\n"); return 2; }
    FILE *fi = fopen(argv[1], "rb");
    if (!fi) { perror(argv[1]); return 2; }
    int64_t k = -1;
    if (fread(&k, sizeof k, 1, fi) != 1 || k < 0 || k > (1 << 24)) { fprintf(stderr, "bad row count\n"); return 2; }
    std::vector<double> xyr((size_t)k * 3);
    if (k && fread(xyr.data(), sizeof(double), xyr.size(), fi) != xyr.size()) { fprintf(stderr, "short table\n"); return 2; }
    fclose(fi);

    std::vector<SgEntry> entries;
    std::vector<uint32_t> start;
    uint32_t max_bin = 0;
    int64_t bad = -1;
    const int32_t rc = sg_file_table_host(xyr.data(), k, entries, start, max_bin, &bad);
    const uint32_t n_entries = rc == 0 ? start[SG_NBINS] : 0;
    const int32_t has_qs = rc == 0 && SG_QS_FITS(max_bin);

    FILE *fo = fopen(argv[2], "wb");
    if (!fo) { perror(argv[2]); return 2; }
    bool ok = put(fo, &rc, 1) && put(fo, &bad, 1) && put(fo, &max_bin, 1) && put(fo, &n_entries, 1) && put(fo, &has_qs, 1);
    if (rc == 0) {
        std::vector<uint32_t> src(n_entries), flags(n_entries);
        std::vector<double> rho(n_entries);
        for (uint32_t e = 0; e < n_entries; ++e) { src[e] = entries[e].src; flags[e] = entries[e].flags; rho[e] = entries[e].rho; }
        static const unsigned char zero[sizeof(SgEntry)] = {0};
        const int32_t spare_zero = entries.size() == (size_t)n_entries + 1 && memcmp(&entries[n_entries], zero, sizeof(SgEntry)) == 0;
        std::vector<uint32_t> q((size_t)SG_NBINS * SG_QSTEPS, 0xdeadbeefu), qs;
        if (has_qs) qs.assign(SG_QS_WORDS_OF(SG_QS_FILE_STEPS, SG_NBINS), 0xdeadbeefu);
        for (int b = 0; b < SG_NBINS; ++b) {                            // k_table_index: one wave per bin, one lane per step of either
            for (int s = 0; s < SG_QSTEPS; ++s)
                sg_range_index_fill_steps(entries.data(), start.data(), SG_NBINS, b, s, SG_QSTEPS, SG_QSTEP_M, q.data(), nullptr);
            if (has_qs)
                for (int s = 0; s < SG_QS_FILE_STEPS; ++s)
                    sg_range_index_fill_steps(entries.data(), start.data(), SG_NBINS, b, s, SG_QS_FILE_STEPS, SG_QS_FILE_STEP_M, nullptr, qs.data());
        }
        ok = ok && put(fo, start.data(), start.size()) && put(fo, src.data(), src.size()) && put(fo, flags.data(), flags.size()) &&
             put(fo, rho.data(), rho.size()) && put(fo, &spare_zero, 1) && put(fo, q.data(), q.size()) && put(fo, qs.data(), qs.size());
    }
    if (fclose(fo) != 0 || !ok) { fprintf(stderr, "write failed\n"); return 2; }
    return 0;
}
