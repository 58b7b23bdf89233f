// host_masked_test.cpp -- Som::findMaskedBmus and Som::impute of the C++ mirror (vsom_bmu_masked_batch).
// Trains a non-square map and checks, on a data set whose columns are all valid, that findMaskedBmus reproduces
// Som::findRestrictedBmu row by row (for several minBmuHits), that impute returns the rows themselves, and that neither
// call downloads the model state into the host mirror; exits non-zero on a failure.
//   usage: host_masked_test
#include "SOM.hpp"
#include "vsom_hip.h"
#include "DataSet.hpp"
#include "Transformation.hpp"

#include <cstdint>
#include <cstring>
#include <iostream>
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

int main()
{
    const size_t W = 13, H = 9, J = 11, NROWS = 200, N = W * H;
    auto rows = make_rows(NROWS, J, 2718u);
    ArrayDataLoader loader(rows.data(), NROWS, J);
    DataSet ds(loader);
    Som som{W, H, ds, Transformation::Standard(loader.getNames())};
    som.randomInitialize(7, 1);
    som.train(ds, 2, 0.0, 0.0, 3.0, 0.2, Som::WeigthDecayFunction::BatchMap);
    ds.loadNextDataFromStream();
    const size_t n = ds.size();
    if (n != NROWS)
        return fail("the data set did not load its rows");
    for (size_t i = 0; i < n; ++i) {
        const Eigen::VectorXi v = ds.getValidity(i);
        for (Eigen::Index d = 0; d < v.size(); ++d)
            if (!v[d])
                return fail("the data set is not all valid");
    }

    const size_t before = som.stateDownloads();
    const Eigen::VectorXf ones = Eigen::VectorXf::Ones((Eigen::Index)J);
    size_t away = 0;      // rows a restriction moved: the restricted searches below are not all the plain one
    std::vector<uint64_t> plain;
    for (size_t hits : {(size_t)0, (size_t)2, (size_t)5, (size_t)1000000}) {
        std::vector<float> dist;
        const std::vector<uint64_t> bmu = som.findMaskedBmus(&ds, hits, &dist);
        if (bmu.size() != n || dist.size() != n)
            return fail("result sizes");
        if (hits == 0)
            plain = bmu;
        for (size_t i = 0; i < n; ++i) {
            if (bmu[i] >= N)
                return fail("row " + std::to_string(i) + ": unit out of range");
            const size_t want = som.getIndex(som.findRestrictedBmu(ds.getData(i), ones, hits, ones));
            if (bmu[i] != want)
                return fail("row " + std::to_string(i) + ", minBmuHits " + std::to_string(hits) + ": findMaskedBmus " +
                            std::to_string(bmu[i]) + ", findRestrictedBmu " + std::to_string(want));
            away += bmu[i] != plain[i];
        }
    }
    if (away == 0)
        return fail("no restriction moved a row: the restricted searches checked nothing beyond the plain one");
    const std::vector<float> fill = som.impute(&ds, 2);
    if (fill.size() != n * J || std::memcmp(fill.data(), ds.contiguous(), n * J * sizeof(float)) != 0)
        return fail("impute of an all-valid data set is not the data set");
    if (som.stateDownloads() != before)
        return fail("findMaskedBmus / impute / findRestrictedBmu downloaded the model state");
    std::cout << "state_downloads=" << som.stateDownloads() << "\n";
    std::cout << "host_masked_test ok\n";
    return 0;
}
