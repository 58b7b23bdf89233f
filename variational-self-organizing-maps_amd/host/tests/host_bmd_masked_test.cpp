// host_bmd_masked_test.cpp -- Som::findRestrictedBmdMasked / drawModelVectorsMasked / generateRowsMasked of the C++ mirror
// (vsom_bmd_masked_batch, vsom_generate_masked_batch).
// Trains a non-square map and checks
//   1. on a data set whose columns are all valid: drawModelVectorsMasked is drawModelVectors bit for bit (units and masses,
//      several minBmuHits), findRestrictedBmdMasked with an all-ones validity sums to 1 and peaks where findRestrictedBmd
//      does, and generateRowsMasked(draws 1, keepObserved false) is generateRows(perRow) bit for bit;
//   2. on a data set with validity zeros and NaN / +inf / 1e30 stored there: every mass is finite and positive, every unit a
//      node, generateRowsMasked' units are drawModelVectorsMasked' for every draw, a kept column is the row's own value bit for
//      bit (with NaN as its L), every sampled column is finite, `draws` calls of one draw repeat one call of `draws`, and the
//      flags matter (some unit differs from the draw over the all-valid rows with the same uniform);
//   3. bad sizes are refused, and none of it downloads the model state into the host mirror.
// Exits non-zero on a failure.
//   usage: host_bmd_masked_test
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

// values in [lo, hi) from the same generator
static std::vector<double> make_uniforms(size_t n, unsigned seed, double lo, double hi)
{
    std::vector<double> r(n);
    unsigned s = seed;
    for (auto &v : r) {
        s = s * 1664525u + 1013904223u;
        v = lo + (hi - lo) * ((double)((s >> 8) & 0xFFFF) / 65536.0);
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
    const size_t W = 13, H = 9, J = 11, NROWS = 200, K = 3, N = W * H;
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
    const std::vector<double> u1 = make_uniforms(n, 11u, 0.0, 1.0), uK = make_uniforms(n * K, 13u, 0.0, 1.0);
    const std::vector<double> l1 = make_uniforms(n * J, 17u, 0.001, 0.999), lK = make_uniforms(n * K * J, 19u, 0.001, 0.999);

    // 1. all valid
    for (size_t hits : {(size_t)0, (size_t)2, (size_t)5}) {
        const std::string at = " (minBmuHits " + std::to_string(hits) + ")";
        std::vector<double> nm, nu;
        const std::vector<uint64_t> m = som.drawModelVectorsMasked(&ds, hits, u1, &nm);
        const std::vector<uint64_t> u = som.drawModelVectors(&ds, hits, u1, &nu);
        if (!same_bits(m, u) || !same_bits(nm, nu))
            return fail("all valid: drawModelVectorsMasked differs from drawModelVectors" + at);
        const Som::GeneratedRows gm = som.generateRowsMasked(ds, hits, u1, l1, 1, false);
        const Som::GeneratedRows gu = som.generateRows(ds, hits, u1, l1, true);
        if (!same_bits(gm.unit, gu.unit) || !same_bits(gm.record, gu.record) || gm.columns != gu.columns)
            return fail("all valid: generateRowsMasked(1 draw, nothing kept) differs from generateRows(perRow)" + at);
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
        std::vector<double> norm;
        const std::vector<uint64_t> plain = som.drawModelVectorsMasked(&ds, hits, u1);
        const std::vector<uint64_t> drawn = som.drawModelVectorsMasked(&fds, hits, u1, &norm);
        for (size_t i = 0; i < n; ++i) {
            if (!(norm[i] > 0.0) || !std::isfinite(norm[i]) || drawn[i] >= N)
                return fail("masked: garbage reached a mass or a unit" + at);
            moved += drawn[i] != plain[i];
        }
        // NaN as the L of every kept column
        std::vector<double> l = lK;
        for (size_t i = 0; i < n; ++i)
            for (size_t k = 0; k < K; ++k)
                for (size_t d = 0; d < J; ++d)
                    if (FlaggedLoader::ok(i, d))
                        l[(i * K + k) * J + d] = std::numeric_limits<double>::quiet_NaN();
        const Som::GeneratedRows g = som.generateRowsMasked(fds, hits, uK, l, K, true);
        if (g.unit.size() != n * K || g.record.size() != n * K * J || g.columns != J)
            return fail("masked: generateRowsMasked' sizes" + at);
        for (size_t k = 0; k < K; ++k) {
            std::vector<double> uk(n), lk(n * J);
            for (size_t i = 0; i < n; ++i) {
                uk[i] = uK[i * K + k];
                std::memcpy(&lk[i * J], &l[(i * K + k) * J], J * sizeof(double));
            }
            const std::vector<uint64_t> dk = som.drawModelVectorsMasked(&fds, hits, uk);
            const Som::GeneratedRows gk = som.generateRowsMasked(fds, hits, uk, lk, 1, true);
            for (size_t i = 0; i < n; ++i) {
                if (g.unit[i * K + k] != dk[i] || gk.unit[i] != dk[i])
                    return fail("masked: generateRowsMasked' units are not drawModelVectorsMasked'" + at);
                if (std::memcmp(&g.record[(i * K + k) * J], &gk.record[i * J], J * sizeof(double)) != 0)
                    return fail("masked: a call with `draws` draws differs from the calls with one" + at);
            }
        }
        for (size_t i = 0; i < n; ++i) {
            const Eigen::VectorXf x = fds.getData(i);
            for (size_t k = 0; k < K; ++k)
                for (size_t d = 0; d < J; ++d) {
                    const double rec = g.record[(i * K + k) * J + d], own = (double)x[(Eigen::Index)d];
                    if (FlaggedLoader::ok(i, d) ? std::memcmp(&rec, &own, sizeof(double)) != 0 : !std::isfinite(rec))
                        return fail("masked: a kept column is not the row's value, or garbage reached a sampled one" + at);
                }
        }
    }
    if (moved == 0)
        return fail("no flag moved a row's draw: the masked distribution checked nothing beyond the all-valid one");

    // 3. refusals, and all of it on the device state
    int refused = 0;
    try {
        (void)som.generateRowsMasked(fds, 0, u1, lK, K, true);
    } catch (const std::invalid_argument &) {
        ++refused;
    }
    try {
        (void)som.generateRowsMasked(fds, 0, uK, l1, K, true);
    } catch (const std::invalid_argument &) {
        ++refused;
    }
    try {
        (void)som.generateRowsMasked(fds, 0, u1, l1, 0, true);
    } catch (const std::invalid_argument &) {
        ++refused;
    }
    try {
        (void)som.drawModelVectorsMasked(&fds, 0, uK);
    } catch (const std::invalid_argument &) {
        ++refused;
    }
    if (refused != 4)
        return fail("a bad size was not refused");
    if (som.stateDownloads() != before)
        return fail("the masked distribution calls downloaded the model state");
    std::cout << "draws_moved_by_flags=" << moved << "\n";
    std::cout << "state_downloads=" << som.stateDownloads() - before << "\n";
    // (last: the unmasked findRestrictedBmd of the mirror works on the downloaded state)
    {
        const Eigen::VectorXf v = ds.getData(3), ones = Eigen::VectorXf::Ones((Eigen::Index)J);
        const std::vector<double> p = som.findRestrictedBmdMasked(v, ones, 0);
        const std::vector<double> q = som.findRestrictedBmd(v, ones, 0, ones);
        if (p.size() != N || q.size() != N)
            return fail("findRestrictedBmdMasked does not return one probability per node");
        double sum = 0;
        size_t ap = 0, aq = 0;
        for (size_t i = 0; i < N; ++i) {
            sum += p[i];
            ap = p[i] > p[ap] ? i : ap;
            aq = q[i] > q[aq] ? i : aq;
        }
        if (std::fabs(sum - 1.0) > 1e-12 || ap != aq)
            return fail("all valid: findRestrictedBmdMasked is not the row's distribution");
        std::cout << std::hexfloat << "bmd_all_valid_peak " << p[ap] << std::defaultfloat << "\n";
    }
    std::cout << "host_bmd_masked_test ok\n";
    return 0;
}
