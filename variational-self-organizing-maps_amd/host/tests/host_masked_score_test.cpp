// host_masked_score_test.cpp -- Som::similarityRowsMasked / measureSimilarityMasked / evaluateRowsMasked / evaluateMasked of
// the C++ mirror (vsom_similarity_masked_batch, vsom_evaluate_masked_batch).
// Trains a non-square map and checks
//   1. on a data set whose columns are all valid: the masked report is similarityRows' bit for bit (both sigma rules, several
//      minBmuHits, the dense delta included) with nvalid = J, measureSimilarityMasked is measureSimilarity, evaluateRowsMasked
//      is evaluateRows and evaluateMasked is evaluate;
//   2. on a data set with validity zeros and NaN / +inf / 1e30 stored there: units and distances are findMaskedBmus', nvalid
//      counts the flags, delta is 0 at every invalid position and dmax_col / amax_col name valid columns, every reported value
//      is free of the garbage, and the flags matter (some unit differs from the all-valid search of the same rows);
//   3. none of it downloads the model state into the host mirror.
// Exits non-zero on a failure.
//   usage: host_masked_score_test
#include "SOM.hpp"
#include "vsom_hip.h"
#include "DataSet.hpp"
#include "Transformation.hpp"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <iostream>
#include <limits>
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

static const char *differs(const Som::SimilarityRows &a, const Som::SimilarityRows &b)
{
    if (!same_bits(a.bmu, b.bmu)) return "bmu";
    if (!same_bits(a.dist, b.dist)) return "dist";
    if (!same_bits(a.dmax, b.dmax)) return "dmax";
    if (!same_bits(a.dmaxCol, b.dmaxCol)) return "dmaxCol";
    if (!same_bits(a.first, b.first)) return "first";
    if (!same_bits(a.amax, b.amax)) return "amax";
    if (!same_bits(a.amaxCol, b.amaxCol)) return "amaxCol";
    if (!same_bits(a.outside, b.outside)) return "outside";
    if (!same_bits(a.delta, b.delta)) return "delta";
    return nullptr;
}

int main()
{
    const size_t W = 13, H = 9, J = 11, NROWS = 200;
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
    const size_t before = som.stateDownloads();

    // 1. all valid
    for (size_t hits : {(size_t)0, (size_t)2, (size_t)5})
        for (bool floor : {false, true}) {
            const std::string at = " (minBmuHits " + std::to_string(hits) + ", floor " + std::to_string(floor) + ")";
            const Som::SimilarityRowsMasked m = som.similarityRowsMasked(&ds, 3, hits, floor, true);
            const Som::SimilarityRows u = som.similarityRows(&ds, 3, hits, floor, false, true);
            if (const char *what = differs(m, u))
                return fail(std::string("all valid: similarityRowsMasked differs from similarityRows in ") + what + at);
            for (size_t i = 0; i < n; ++i)
                if (m.nvalid[i] != J)
                    return fail("all valid: nvalid is not the number of columns" + at);
            if (!floor && som.measureSimilarityMasked(&ds, 3, hits) != som.measureSimilarity(&ds, 3, hits))
                return fail("all valid: measureSimilarityMasked differs from measureSimilarity" + at);
        }
    {
        const Som::EvaluateRowsMasked m = som.evaluateRowsMasked(ds);
        const Som::EvaluateRows u = som.evaluateRows(ds);
        if (!same_bits(m.bmu, u.bmu) || !same_bits(m.dist, u.dist) || !same_bits(m.bsum, u.bsum) || !same_bits(m.nrepl, u.nrepl) ||
            std::memcmp(&m.error, &u.error, sizeof(double)) != 0)
            return fail("all valid: evaluateRowsMasked differs from evaluateRows");
        const double em = som.evaluateMasked(ds), eu = som.evaluate(ds);
        if (std::memcmp(&em, &eu, sizeof(double)) != 0 || std::memcmp(&em, &m.error, sizeof(double)) != 0)
            return fail("all valid: evaluateMasked differs from evaluate");
        std::cout << std::hexfloat << "evaluate_all_valid " << em << std::defaultfloat << "\n";
    }

    // 2. validity zeros with garbage behind them
    FlaggedLoader floader(rows.data(), NROWS, J);
    DataSet fds(floader);
    fds.loadNextDataFromStream();
    if (fds.size() != NROWS)
        return fail("the flagged data set did not load its rows");
    size_t moved = 0;
    for (size_t hits : {(size_t)0, (size_t)2}) {
        const std::string at = " (minBmuHits " + std::to_string(hits) + ")";
        std::vector<float> dist;
        const std::vector<uint64_t> bmu = som.findMaskedBmus(&fds, hits, &dist);
        const Som::SimilarityRowsMasked m = som.similarityRowsMasked(&fds, 3, hits, true, true);
        const Som::EvaluateRowsMasked e = som.evaluateRowsMasked(fds, hits);
        const Som::SimilarityRowsMasked plain = som.similarityRowsMasked(&ds, 3, hits, true, false);
        if (!same_bits(m.bmu, bmu) || !same_bits(m.dist, dist))
            return fail("masked: similarityRowsMasked' units / distances are not findMaskedBmus'" + at);
        if (!same_bits(e.bmu, bmu) || !same_bits(e.dist, dist))
            return fail("masked: evaluateRowsMasked' units / distances are not findMaskedBmus'" + at);
        double error = 0;
        for (size_t i = 0; i < n; ++i) {
            uint32_t cnt = 0;
            for (size_t d = 0; d < J; ++d) {
                cnt += FlaggedLoader::ok(i, d);
                const float v = m.delta[i * J + d];
                if (!FlaggedLoader::ok(i, d) && (v != 0.f || std::signbit(v)))
                    return fail("masked: delta is not +0 at an invalid position" + at);
                if (!std::isfinite(v) || std::fabs(v) > 1e6f)
                    return fail("masked: garbage reached delta" + at);
            }
            if (m.nvalid[i] != cnt || e.nvalid[i] != cnt)
                return fail("masked: nvalid does not count the flags" + at);
            if (m.dmaxCol[i] >= J || !FlaggedLoader::ok(i, m.dmaxCol[i]) || m.amaxCol[i] >= J || !FlaggedLoader::ok(i, m.amaxCol[i]))
                return fail("masked: dmax_col / amax_col does not name a valid column" + at);
            if (m.dmax[i] != m.delta[i * J + m.dmaxCol[i]] || m.amax[i] != std::fabs(m.delta[i * J + m.amaxCol[i]]))
                return fail("masked: dmax / amax is not the delta of its column" + at);
            if (!std::isfinite(m.dist[i]) || !std::isfinite(m.first[i]) || !std::isfinite(e.bsum[i]))
                return fail("masked: garbage reached dist / first / bsum" + at);
            error += 1.0 / ((double)i + 1.0) * ((double)e.dist[i] + std::sqrt((double)e.bsum[i]) - error);
            moved += m.bmu[i] != plain.bmu[i];
        }
        if (std::memcmp(&error, &e.error, sizeof(double)) != 0)
            return fail("masked: error is not the running mean of the returned rows" + at);
        const double em = som.evaluateMasked(fds, hits);
        if (std::memcmp(&em, &e.error, sizeof(double)) != 0)
            return fail("masked: evaluateMasked is not evaluateRowsMasked' error" + at);
        const Som::SimilarityRowsMasked w = som.similarityRowsMasked(&fds, 3, hits, false, false);
        if (som.measureSimilarityMasked(&fds, 3, hits) != (int)(w.outside[Som::measureSimilarityRow(w.first, w.dmax)] == 0))
            return fail("masked: measureSimilarityMasked differs from the finish of its own report" + at);
    }
    if (moved == 0)
        return fail("no flag moved a row's unit: the masked search checked nothing beyond the all-valid one");

    // 3. all of it on the device state
    if (som.stateDownloads() != before)
        return fail("the masked scorers downloaded the model state");
    std::cout << "rows_moved_by_flags=" << moved << "\n";
    std::cout << "state_downloads=" << som.stateDownloads() - before << "\n";
    std::cout << "host_masked_score_test ok\n";
    return 0;
}
