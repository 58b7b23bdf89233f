// host_similarity_test.cpp -- Som::similarityRows and Som::measureSimilarity of the C++ mirror (vsom_similarity_batch).
// Trains a non-square map, takes the per-row report and measureSimilarity's result for several (numberOfSigmas, minBmuHits,
// rule) settings and writes the state, the rows, the validity flags and the reports to <outdir>/similarity.bin
// (tests/test_gpu_host_similarity.py repeats them through the Python binding and a restated reference loop).  Asserts that
// measureSimilarity on a device state the host mirror has not seen downloads no state; exits non-zero on a failure.
//   usage: host_similarity_test <outdir>
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

template <typename T> static void put(std::ofstream &f, const std::vector<T> &v)
{
    f.write((const char *)v.data(), (std::streamsize)(v.size() * sizeof(T)));
}

int main(int argc, char **argv)
{
    if (argc < 2)
        return fail("usage: host_similarity_test <outdir>");
    const std::string out = argv[1];
    const size_t W = 13, H = 9, J = 11, NROWS = 400, N = W * H;
    auto rows = make_rows(NROWS, J, 4242u);
    ArrayDataLoader loader(rows.data(), NROWS, J);
    DataSet ds(loader);
    Som som{W, H, ds, Transformation::Standard(loader.getNames())};
    som.randomInitialize(5, 1);
    som.train(ds, 3, 0.0, 0.0, 3.0, 0.2, Som::WeigthDecayFunction::BatchMap);
    std::cout << "group_members=" << (som.group() ? vsom_group_size(som.group()) : 1) << "\n";
    ds.loadNextDataFromStream();
    const size_t n = ds.size();

    // a device state the host mirror has not seen: the mirror is refreshed, one more epoch dirties it again
    (void)som.getNeuron((size_t)0);
    (void)som.trainBatchSomEpoch(ds, 1.5, false);
    const size_t before = som.stateDownloads();

    struct Setting { int sigmas; size_t hits; bool floor; };
    const std::vector<Setting> settings = {{3, 1, false}, {3, 1, true}, {1, 0, false}, {1, 0, true},
                                           {1000000, 1, false}, {1000000, 1, true}, {3, 1000000, true}};
    std::vector<Som::SimilarityRows> reports;
    std::vector<int32_t> verdicts;
    for (const Setting &s : settings) {
        reports.push_back(som.similarityRows(&ds, s.sigmas, s.hits, s.floor, true, true));
        verdicts.push_back(s.floor ? -1 : som.measureSimilarity(&ds, s.sigmas, s.hits));
        const Som::SimilarityRows &r = reports.back();
        if (r.columns != J || r.bmu.size() != n || r.outside.size() != n || r.delta.size() != n * J)
            return fail("report sizes");
        for (size_t i = 0; i < n; ++i)
            if (r.bmu[i] >= N || (r.amaxCol[i] != UINT32_MAX && r.amaxCol[i] >= J) || r.outside[i] > J)
                return fail("row " + std::to_string(i) + ": report out of range");
        if (!s.floor && verdicts.back() != (int)(r.outside[Som::measureSimilarityRow(r.first, r.dmax)] == 0))
            return fail("measureSimilarity differs from the finish of its own report");
    }
    if (som.stateDownloads() != before)
        return fail("measureSimilarity / similarityRows downloaded the model state");
    std::cout << "no state download ok\n";
    (void)som.getNeuron((size_t)0);
    if (som.stateDownloads() != before + 1)
        return fail("the device state was not dirty: the download check above checked nothing");

    {
        const size_t D = som.getDepth();
        std::vector<float> m(N * D), sg(N * D), S(N * D), w(N);
        std::vector<uint64_t> h(N);
        som.getState(m.data(), sg.data(), S.data(), w.data(), h.data());
        std::vector<uint8_t> valid(n * J, 0);
        for (size_t i = 0; i < n; ++i) {
            const Eigen::VectorXi v = ds.getValidity(i);
            for (size_t d = 0; d < J && d < (size_t)v.size(); ++d)
                valid[i * J + d] = v[(Eigen::Index)d] != 0;
        }
        std::ofstream f(out + "/similarity.bin", std::ios::binary);
        const uint64_t hdr[5] = {W, H, J, n, settings.size()};
        f.write((const char *)hdr, sizeof(hdr));
        put(f, m);
        put(f, sg);
        put(f, h);
        f.write((const char *)ds.contiguous(), (std::streamsize)(n * J * 4));
        put(f, valid);
        for (size_t k = 0; k < settings.size(); ++k) {
            const int64_t par[4] = {settings[k].sigmas, (int64_t)settings[k].hits, settings[k].floor, verdicts[k]};
            f.write((const char *)par, sizeof(par));
            const Som::SimilarityRows &r = reports[k];
            put(f, r.bmu);
            put(f, r.dist);
            put(f, r.dmax);
            put(f, r.dmaxCol);
            put(f, r.first);
            put(f, r.amax);
            put(f, r.amaxCol);
            put(f, r.outside);
            put(f, r.delta);
        }
    }

    std::cout << "host_similarity_test ok\n";
    return 0;
}
