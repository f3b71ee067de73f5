// Host harness: the packed result transfer's host side (lidar_snow_sim_amd/csrc/sg_assemble.h) on fabricated device words -- every frame
// of a batch through sg_assemble_frame as a job of an AsmPool with 3 threads, as host_batch_pipelined hands them out.  No GPU, no HIP.
// usage: assemble_frames <dir>.  Reads <dir>/{head,offsets,kept,mvcnt,rows,chn,meta,inten,mv,out_rows,out_src}.bin, writes
// <dir>/out_rows.out and <dir>/out_src.out.  head.bin: int64 kind (0 float32, 1 float32 compact, 2 float64), n_frames, out_src wanted.
// Every buffer is a heap block of the file's exact size: a read or write past it is an AddressSanitizer report.
// Built (plain, address + undefined, thread) and run by tests/test_host_logic.py.
#include <cstdio>
#include <string>

#include "../../lidar_snow_sim_amd/csrc/sg_assemble.h"

static std::vector<char> slurp(const std::string &path)
{
    FILE *fh = std::fopen(path.c_str(), "rb");
    if (!fh) { std::fprintf(stderr, "cannot read %s\n", path.c_str()); std::exit(2); }
    std::fseek(fh, 0, SEEK_END);
    std::vector<char> buf((size_t)std::ftell(fh));
    std::fseek(fh, 0, SEEK_SET);
    if (!buf.empty() && std::fread(buf.data(), 1, buf.size(), fh) != buf.size()) { std::fprintf(stderr, "short read of %s\n", path.c_str()); std::exit(2); }
    std::fclose(fh);
    return buf;
}

static void dump(const std::string &path, const std::vector<char> &buf)
{
    FILE *fh = std::fopen(path.c_str(), "wb");
    if (!fh || (!buf.empty() && std::fwrite(buf.data(), 1, buf.size(), fh) != buf.size())) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); std::exit(2); }
    std::fclose(fh);
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: assemble_frames <dir>\n"); return 2; }
    const std::string d = std::string(argv[1]) + "/";
    const std::vector<char> head = slurp(d + "head.bin"), offsets = slurp(d + "offsets.bin"), kept = slurp(d + "kept.bin"), mvcnt = slurp(d + "mvcnt.bin"),
                            rows = slurp(d + "rows.bin"), chn = slurp(d + "chn.bin"), meta = slurp(d + "meta.bin"), inten = slurp(d + "inten.bin"),
                            mv = slurp(d + "mv.bin");
    std::vector<char> out_rows = slurp(d + "out_rows.bin"), out_src = slurp(d + "out_src.bin");
    const int64_t *h = (const int64_t *)head.data(), *off = (const int64_t *)offsets.data();
    const int64_t kind = h[0], n_frames = h[1];
    const bool want_src = h[2] != 0;
    const size_t esz = kind == 2 ? 8 : 4, in_w = kind == 1 ? 4 : 5;
    void (*const assemble)(const SgAsmFrame &) = kind == 2 ? sg_assemble_frame<double, false> : (kind == 1 ? sg_assemble_frame<float, true> : sg_assemble_frame<float, false>);
    {
        AsmPool pool;
        pool.start(3);
        int64_t mv_at = 0;
        for (int64_t f = 0; f < n_frames; ++f) {
            const size_t fo = (size_t)off[f];
            const int64_t n_rows = off[f + 1] - off[f];
            const SgAsmFrame a{rows.data() + fo * in_w * esz, kind == 1 ? (const uint8_t *)chn.data() + fo : nullptr, (const uint32_t *)meta.data() + fo,
                               inten.data() + fo * esz, mv.data() + (size_t)mv_at * 3 * esz, out_rows.data() + fo * 5 * esz,
                               want_src ? (int32_t *)out_src.data() + fo : nullptr, (uint32_t)n_rows, ((const int64_t *)kept.data())[f]};
            pool.push([=]() { assemble(a); });
            mv_at += sg_moved_rows(((const int64_t *)mvcnt.data())[f], n_rows);
        }
        pool.wait_idle();
    }
    dump(d + "out_rows.out", out_rows);
    dump(d + "out_src.out", out_src);
    return 0;
}
