// host_topk_test.cpp -- Som::findBestMatchingUnits and Som::topographicError of the C++ mirror (vsom_bmu_topk_batch).
// Trains a map, takes the K best matching units of every row and the topographic error, and writes the state, the rows,
// the lists, their distances and the error to <outdir>/topk.bin (tests/test_gpu_host_topk.py repeats them through the
// Python binding); checks the argument refusals and exits non-zero on a failure.
//   usage: host_topk_test <outdir>
#include "SOM.hpp"
#include "vsom_hip.h"
#include "DataSet.hpp"
#include "Transformation.hpp"

#include <cstdint>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

static std::vector<float> make_rows(size_t n, size_t d, unsigned seed)
{
    std::vector<float> r(n * d);
    unsigned s = seed;
    for (auto &v : r) {
        s = s * 1664525u + 1013904223u;
        v = (float)((s >> 8) & 0xFFFF) / 65536.0f * 2.0f - 1.0f;
    }
    return r;
}

static int fail(const std::string &what)
{
    std::cerr << "FAIL: " << what << "\n";
    return 1;
}

int main(int argc, char **argv)
{
    if (argc < 2)
        return fail("usage: host_topk_test <outdir>");
    const std::string out = argv[1];
    const size_t W = 13, H = 9, J = 11, NROWS = 400, N = W * H, K = 5;
    auto rows = make_rows(NROWS, J, 777u);
    ArrayDataLoader loader(rows.data(), NROWS, J);
    DataSet ds(loader);
    Som som{W, H, ds, Transformation::Standard(loader.getNames())};
    som.randomInitialize(3, 1);
    som.train(ds, 2, 0.0, 0.0, 3.0, 0.2, Som::WeigthDecayFunction::BatchMap);
    std::cout << "group_members=" << (som.group() ? vsom_group_size(som.group()) : 1) << "\n";
    ds.loadNextDataFromStream();

    std::vector<float> dist;
    const std::vector<uint64_t> idx = som.findBestMatchingUnits(&ds, K, &dist);
    const double te = som.topographicError(&ds);
    if (idx.size() != ds.size() * K || dist.size() != idx.size())
        return fail("list sizes");
    for (size_t r = 0; r < ds.size(); ++r)
        for (size_t j = 0; j < K; ++j)
            if (idx[r * K + j] >= N || (j > 0 && !(dist[r * K + j - 1] <= dist[r * K + j])))
                return fail("row " + std::to_string(r) + ": not a list of nodes in distance order");
    if (!(te >= 0.0 && te <= 1.0))
        return fail("topographic error out of [0, 1]");
    {
        const size_t D = som.getDepth();
        std::vector<float> m(N * D), s(N * D), S(N * D), w(N);
        std::vector<uint64_t> h(N);
        som.getState(m.data(), s.data(), S.data(), w.data(), h.data());
        std::ofstream f(out + "/topk.bin", std::ios::binary);
        const uint64_t hdr[4] = {W, H, J, ds.size()};
        f.write((const char *)hdr, sizeof(hdr));
        const uint64_t k = K;
        f.write((const char *)&k, 8);
        f.write((const char *)m.data(), m.size() * 4);
        f.write((const char *)ds.contiguous(), ds.size() * J * 4);
        f.write((const char *)idx.data(), idx.size() * 8);
        f.write((const char *)dist.data(), dist.size() * 4);
        f.write((const char *)&te, 8);
    }
    std::cout << "topographic_error=" << te << "\n";

    // refusals: k = 0, k > 64, k > N
    for (size_t bad : {(size_t)0, (size_t)65}) {
        bool threw = false;
        try {
            som.findBestMatchingUnits(&ds, bad);
        } catch (const std::invalid_argument &) {
            threw = true;
        }
        if (!threw)
            return fail("k = " + std::to_string(bad) + " was accepted");
    }
    {
        ArrayDataLoader small(rows.data(), 10, J);
        DataSet sds(small);
        Som tiny{2, 2, sds, Transformation::Standard(small.getNames())};
        tiny.randomInitialize(1, 1);
        sds.loadNextDataFromStream();
        bool threw = false;
        try {
            tiny.findBestMatchingUnits(&sds, 5);
        } catch (const std::invalid_argument &) {
            threw = true;
        }
        if (!threw)
            return fail("k > N was accepted");
        if (tiny.findBestMatchingUnits(&sds, 4).size() != 40)
            return fail("k = N");
    }
    std::cout << "refusals ok\n";
    std::cout << "host_topk_test ok\n";
    return 0;
}
