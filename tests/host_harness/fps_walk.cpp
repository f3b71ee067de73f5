// The usable test, the distance, the candidate key and its fold of the keypoint stage (csrc/sg_fps.h) compiled for the host, walking ONE
// frame as the kernel does: the usable rows compacted in input order, then K - 1 rounds in which every point is dealt to one of 1024
// "lanes", every lane folds its points' keys, and the lanes' keys are folded into the round's winner.
//   fps_walk <dtype 0 | 1> <K> <x0> <y0> <z0> <x1> <y1> <z1> <in: n x 3 float64> <keep: n bytes> <out> <seed>
//       seed 0: the kernel's own assignment (position k 1024 + lane in a resident tier, four consecutive positions per lane beyond), a
//       lane's best by a strict comparison in rising position, lanes folded wave by wave;
//       seed > 0: a random lane per point, every lane's points in a random order, the 1024 keys folded as a random tree.
//       out: int32 m, int32 index[K] (-1 for m = 0), dist[K] in the dtype (-1 for m = 0).
// Prints "tiers" and the usable rows of tiers 0, 1 and 2 for float32, then for float64.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "sg_fps.h"

template <typename T>
static int run(int K, const SgFpsRange &r, const std::vector<double> &p, const std::vector<uint8_t> &keep, uint64_t seed, FILE *fo)
{
    const size_t n = keep.size();
    std::vector<T> x, y, z, t;
    std::vector<int32_t> src;
    for (size_t i = 0; i < n; ++i) {
        const T px = (T)p[3 * i], py = (T)p[3 * i + 1], pz = (T)p[3 * i + 2];
        if (keep[i] != 0 && sg_fps_usable<T>(r, px, py, pz)) { x.push_back(px); y.push_back(py); z.push_back(pz); src.push_back((int32_t)i); }
    }
    const int32_t m = (int32_t)x.size();
    std::vector<int32_t> index((size_t)K, -1);
    std::vector<T> dist((size_t)K, (T)-1);
    if (m > 0) {
        t.assign((size_t)m, (T)INFINITY);
        const bool resident = m <= SgFpsTier<T>::P1 * SG_FPS_BLOCK;
        std::mt19937_64 rng(seed);
        std::vector<std::vector<int32_t>> lanes(SG_FPS_BLOCK);
        for (int32_t q = 0; q < m; ++q) lanes[seed ? rng() % SG_FPS_BLOCK : (resident ? q % SG_FPS_BLOCK : (q / 4) % SG_FPS_BLOCK)].push_back(q);
        index[0] = src[0];
        dist[0] = (T)INFINITY;
        int32_t s = 0;
        std::vector<SgFpsKey<T>> keys(SG_FPS_BLOCK);
        for (int j = 1; j < K; ++j) {
            for (int l = 0; l < SG_FPS_BLOCK; ++l) {
                std::vector<int32_t> &mine = lanes[l];
                if (seed) std::shuffle(mine.begin(), mine.end(), rng);
                SgFpsKey<T> k = sg_fps_no_key<T>();
                T bt = (T)0;
                int32_t bp = -1;
                for (int32_t q : mine) {
                    t[q] = sg_fps_min(t[q], sg_fps_dist(x[q], y[q], z[q], x[s], y[s], z[s]));
                    if (seed) k = sg_fps_fold(k, sg_fps_key(t[q], (uint32_t)q));
                    else if (bp < 0 || t[q] > bt) { bt = t[q]; bp = q; }
                }
                keys[l] = seed || bp < 0 ? k : sg_fps_key(bt, (uint32_t)bp);
            }
            SgFpsKey<T> best = sg_fps_no_key<T>();
            if (seed) {
                std::vector<SgFpsKey<T>> pool = keys;
                while (pool.size() > 1) {
                    const size_t a = rng() % pool.size();
                    std::swap(pool[a], pool.back());
                    const SgFpsKey<T> ka = pool.back();
                    pool.pop_back();
                    const size_t b = rng() % pool.size();
                    pool[b] = rng() & 1 ? sg_fps_fold(ka, pool[b]) : sg_fps_fold(pool[b], ka);
                }
                best = pool[0];
            } else {
                for (int w = 0; w < SG_FPS_WAVES; ++w) {
                    SgFpsKey<T> wk = sg_fps_no_key<T>();
                    for (int l = 0; l < 64; ++l) wk = sg_fps_fold(wk, keys[w * 64 + l]);
                    best = w ? sg_fps_fold(best, wk) : wk;
                }
            }
            s = (int32_t)sg_fps_key_pos(best);
            if (s < 0 || s >= m) return 6;
            index[j] = src[s];
            dist[j] = sg_fps_key_t(best);
            if (!(dist[j] == t[s])) return 7;
        }
    }
    fwrite(&m, sizeof(int32_t), 1, fo);
    fwrite(index.data(), sizeof(int32_t), (size_t)K, fo);
    fwrite(dist.data(), sizeof(T), (size_t)K, fo);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 13) return 2;
    const int dtype = atoi(argv[1]), K = atoi(argv[2]);
    if (K < 1 || (dtype != 0 && dtype != 1)) return 2;
    SgFpsRange r;
    for (int j = 0; j < 3; ++j) { r.lo[j] = atof(argv[3 + j]); r.hi[j] = atof(argv[6 + j]); }
    std::vector<double> p;
    std::vector<uint8_t> keep;
    FILE *fi = fopen(argv[9], "rb");
    if (!fi) return 4;
    double c[3];
    while (fread(c, sizeof(double), 3, fi) == 3) p.insert(p.end(), c, c + 3);
    fclose(fi);
    fi = fopen(argv[10], "rb");
    if (!fi) return 4;
    keep.resize(p.size() / 3);
    const size_t got = fread(keep.data(), 1, keep.size(), fi);
    fclose(fi);
    if (got != keep.size()) return 4;
    FILE *fo = fopen(argv[11], "wb");
    if (!fo) return 5;
    const uint64_t seed = (uint64_t)atoll(argv[12]);
    const int rc = dtype == 0 ? run<float>(K, r, p, keep, seed, fo) : run<double>(K, r, p, keep, seed, fo);
    fclose(fo);
    printf("tiers %d %d %d %d %d %d\n", SG_FPS_TIER0_ROWS_F32, SG_FPS_TIER1_ROWS_F32, SG_FPS_TIER2_ROWS_F32, SG_FPS_TIER0_ROWS_F64, SG_FPS_TIER1_ROWS_F64,
           SG_FPS_TIER2_ROWS_F64);
    return rc;
}
