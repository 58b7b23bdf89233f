// host_topk_masked_test.cpp -- Som::findBestMatchingUnitsMasked / topographicErrorMasked / imputeBlend of the C++ mirror
// (vsom_bmu_topk_masked_batch).
// Trains a non-square map and checks
//   1. on a data set whose columns are all valid: with minBmuHits 0 the lists and distances are findBestMatchingUnits' bit
//      for bit, every count is k, topographicErrorMasked is topographicError over every row, and imputeBlend is the rows
//      themselves, widened to double;
//   2. on a data set with validity zeros and NaN / +inf / 1e30 stored there: entry 0 and its distance are findMaskedBmus'
//      for several minBmuHits, the lists are padded from count on, a valid column of imputeBlend is the row's own value bit
//      for bit, an invalid one is finite and lies between the smallest and largest value of the row's units in that column,
//      imputeBlend with k = 1 is impute widened to double, and the flags matter (some list differs from the all-valid one);
//   3. a restriction nobody meets leaves node 0 alone (count 1, no row counted by topographicErrorMasked), a bad k is refused,
//      and none of it downloads the model state into the host mirror.
// Exits non-zero on a failure.
//   usage: host_topk_masked_test
#include "SOM.hpp"
#include "vsom_hip.h"
#include "DataSet.hpp"
#include "Transformation.hpp"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <iostream>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

static std::vector<float> make_rows(size_t n, size_t d, unsigned seed)
{
    std::vector<float> r(n * d);
    unsigned s = seed;
    for (auto &v : r) {
        s = s * 1664525u + 1013904223u;
        v = (float)((s >> 8) & 0xFFFF) / 65536.0f;
    }
    return r;
}

static int fail(const std::string &what)
{
    std::cerr << "FAIL: " << what << "\n";
    return 1;
}

// an ArrayDataLoader whose rows carry validity zeros -- about one value in five, decided by (row, column) -- with
// NaN / +inf / 1e30 stored at those positions
class FlaggedLoader : public ArrayDataLoader {
public:
    FlaggedLoader(const float *rows, size_t nrows, size_t depth) : ArrayDataLoader(rows, nrows, depth) {}
    bool peekFlat(size_t &) override { return false; }       // (the flat path hands over all-valid rows)
    static bool ok(size_t i, size_t d) { return ((i * 7 + d * 3) % 5) != 0; }
    size_t load() override
    {
        const size_t n = ArrayDataLoader::load();
        const float junk[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), 1e30f};
        for (size_t i = 0; i < data.size(); ++i)
            for (size_t d = 0; d < data[i].valid.size(); ++d) {
                data[i].valid[d] = ok(i, d);
                if (!ok(i, d))
                    data[i].values[(Eigen::Index)d] = junk[(i + d) % 3];
            }
        return n;
    }
};

template <typename T> static bool same_bits(const std::vector<T> &a, const std::vector<T> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

int main()
{
    const size_t W = 13, H = 9, J = 11, NROWS = 200, K = 5, N = W * H;
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
    std::vector<float> map(N * J);      // the model vectors, read once, before the counter is taken
    for (size_t i = 0; i < N; ++i) {
        const Eigen::VectorXf m = som.getNeuron(i);
        for (size_t d = 0; d < J; ++d)
            map[i * J + d] = m[(Eigen::Index)d];
    }
    const size_t before = som.stateDownloads();

    // 1. all valid
    {
        std::vector<float> dm, du;
        std::vector<uint32_t> count;
        const std::vector<uint64_t> m = som.findBestMatchingUnitsMasked(&ds, K, 0, &dm, &count);
        const std::vector<uint64_t> u = som.findBestMatchingUnits(&ds, K, &du);
        if (!same_bits(m, u) || !same_bits(dm, du))
            return fail("all valid: findBestMatchingUnitsMasked differs from findBestMatchingUnits");
        for (size_t i = 0; i < n; ++i)
            if (count[i] != K)
                return fail("all valid: a count is not k");
        size_t counted = 0;
        const double tem = som.topographicErrorMasked(&ds, 0, &counted), te = som.topographicError(&ds);
        if (tem != te || counted != n)
            return fail("all valid: topographicErrorMasked differs from topographicError");
        const std::vector<double> blend = som.imputeBlend(&ds, K, 0);
        if (blend.size() != n * J)
            return fail("all valid: imputeBlend has the wrong size");
        for (size_t i = 0; i < n * J; ++i)
            if (blend[i] != (double)rows[i])
                return fail("all valid: imputeBlend is not the rows");
    }

    // 2. validity zeros with garbage behind them
    FlaggedLoader floader(rows.data(), NROWS, J);
    DataSet fds(floader);
    fds.loadNextDataFromStream();
    if (fds.size() != NROWS)
        return fail("the flagged data set did not load its rows");
    size_t moved = 0, padded = 0;
    const std::vector<uint64_t> allValid = som.findBestMatchingUnitsMasked(&ds, K, 0);
    for (size_t hits : {(size_t)0, (size_t)2, (size_t)5}) {
        const std::string at = " (minBmuHits " + std::to_string(hits) + ")";
        std::vector<float> dist, d1;
        std::vector<uint32_t> count;
        const std::vector<uint64_t> idx = som.findBestMatchingUnitsMasked(&fds, K, hits, &dist, &count);
        const std::vector<uint64_t> bmu = som.findMaskedBmus(&fds, hits, &d1);
        for (size_t i = 0; i < n; ++i) {
            if (idx[i * K] != bmu[i] || std::memcmp(&dist[i * K], &d1[i], 4) != 0)
                return fail("masked: entry 0 is not findMaskedBmus'" + at);
            if (count[i] < 1 || count[i] > K)
                return fail("masked: a count is out of range" + at);
            for (size_t j = 0; j < K; ++j) {
                const bool real = j < count[i];
                if (real ? (idx[i * K + j] >= N || !std::isfinite(dist[i * K + j]))
                         : (idx[i * K + j] != UINT64_MAX || !std::isnan(dist[i * K + j])))
                    return fail("masked: garbage reached a list, or the padding is wrong" + at);
                if (real && j > 0 && dist[i * K + j] < dist[i * K + j - 1])
                    return fail("masked: a list is not ascending" + at);
            }
            padded += count[i] < K;
            if (hits == 0)
                for (size_t j = 0; j < K; ++j)
                    moved += idx[i * K + j] != allValid[i * K + j];
        }
        const std::vector<double> blend = som.imputeBlend(&fds, K, hits);
        for (size_t i = 0; i < n; ++i)
            for (size_t d = 0; d < J; ++d) {
                const double b = blend[i * J + d];
                if (FlaggedLoader::ok(i, d)) {
                    if (b != (double)rows[i * J + d])
                        return fail("masked: a valid column of imputeBlend is not the row's own value" + at);
                    continue;
                }
                double lo = INFINITY, hi = -INFINITY;
                for (size_t j = 0; j < count[i]; ++j) {
                    const double m = (double)map[idx[i * K + j] * J + d];
                    lo = m < lo ? m : lo;
                    hi = m > hi ? m : hi;
                }
                const double slack = 1e-12 * (std::fabs(lo) + std::fabs(hi));
                if (!(b >= lo - slack && b <= hi + slack))
                    return fail("masked: an imputed value is not a weighted mean of its units' values" + at);
            }
        // one unit: impute itself
        const std::vector<double> b1 = som.imputeBlend(&fds, 1, hits);
        const std::vector<float> fill = som.impute(&fds, hits);
        for (size_t i = 0; i < n * J; ++i)
            if (b1[i] != (double)fill[i])
                return fail("masked: imputeBlend with one unit is not impute" + at);
    }
    if (moved == 0)
        return fail("masked: the validity flags moved no list entry");

    // 3. a restriction nobody meets: node 0 alone
    {
        std::vector<uint32_t> count;
        const std::vector<uint64_t> idx = som.findBestMatchingUnitsMasked(&fds, 2, 1000000, nullptr, &count);
        for (size_t i = 0; i < n; ++i)
            if (count[i] != 1 || idx[2 * i] != 0 || idx[2 * i + 1] != UINT64_MAX)
                return fail("node 0 alone: the list is not (0, padding)");
        size_t counted = 7;
        if (som.topographicErrorMasked(&fds, 1000000, &counted) != 0.0 || counted != 0)
            return fail("node 0 alone: topographicErrorMasked counted a row");
    }
    for (size_t bad : {(size_t)0, (size_t)65, N + 1}) {
        bool refused = false;
        try {
            som.findBestMatchingUnitsMasked(&fds, bad, 0);
        } catch (const std::invalid_argument &) {
            refused = true;
        }
        if (!refused)
            return fail("k = " + std::to_string(bad) + " was not refused");
    }
    const size_t downloads = som.stateDownloads() - before;
    std::cout << "moved=" << moved << " padded=" << padded << " state_downloads=" << downloads << "\n";
    if (downloads != 0)
        return fail("the masked top-k calls downloaded the model state");
    std::cout << "host_topk_masked_test ok\n";
    return 0;
}
