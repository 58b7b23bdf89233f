// host_resident_masked_test.cpp -- Som::trainBatchSomResidentMasked of the C++ mirror (vsom_batch_schedule_masked).
// 1. On a one-chunk DataSet whose loader clears about one flag in five (and every flag of one column) the resident masked
//    schedule leaves the state, the metrics and the rows' BMUs of trainBatchSomMasked bit for bit: the reference
//    fixture's shape (10x10x9, 20 rows, sigma0 5, decay 0.05: 33 of 40 epochs run, the one-launch kernel) and a map above
//    the one-launch bound (24x20x11, 300 rows: the library runs the loop of masked epochs).  NaN / +inf / 1e30 at the
//    invalid positions change nothing, and the column without a valid row is +0 with a NaN sigma.
// 2. A DataSet that loads as two chunks throws std::invalid_argument and trains nothing.
// Neither call downloads the model state into the host mirror.  Exits non-zero on a failure.
//   usage: host_resident_masked_test
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
        v = (float)((s >> 8) & 0xFFFF) / 65536.0f * 2.0f - 1.0f;
    }
    return r;
}

static int fail(const std::string &what)
{
    std::cerr << "FAIL: " << what << "\n";
    return 1;
}

// an ArrayDataLoader whose rows carry validity zeros -- about one value in five, decided by (row of the chunk, column), and
// all of column DEAD -- and, with `garbage`, NaN / +inf / 1e30 at those positions
class FlaggedLoader : public ArrayDataLoader {
    bool m_garbage;

public:
    static constexpr size_t DEAD = 4;
    FlaggedLoader(const float *rows, size_t nrows, size_t depth, size_t maxLoad, bool garbage)
        : ArrayDataLoader(rows, nrows, depth, maxLoad), m_garbage(garbage)
    {
    }
    bool peekFlat(size_t &) override { return false; }       // (the flat path hands over all-valid rows)
    size_t load() override
    {
        const size_t n = ArrayDataLoader::load();
        const float junk[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), 1e30f};
        for (size_t i = 0; i < data.size(); ++i)
            for (size_t d = 0; d < data[i].valid.size(); ++d) {
                const bool ok = d != DEAD && ((i * 7 + d * 3) % 5) != 0;
                data[i].valid[d] = ok;
                if (!ok && m_garbage)
                    data[i].values[(Eigen::Index)d] = junk[(i + d) % 3];
            }
        return n;
    }
};

struct State {
    std::vector<float> map, sigma, S, weight;
    std::vector<uint64_t> hits;
    std::vector<float> mse;
    std::vector<size_t> lastBMU;
};

static State state_of(const Som &som, const DataSet &ds, size_t N, size_t J)
{
    State st;
    st.map.resize(N * J);
    st.sigma.resize(N * J);
    st.S.resize(N * J);
    st.weight.resize(N);
    st.hits.resize(N);
    som.getState(st.map.data(), st.sigma.data(), st.S.data(), st.weight.data(), st.hits.data());
    st.mse = som.getMetrics().MeanSquaredError;
    st.lastBMU = ds.getLastBMU();
    return st;
}

static bool same_bits(const std::vector<float> &a, const std::vector<float> &b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

static const char *differs(const State &a, const State &b)
{
    if (!same_bits(a.map, b.map))
        return "map";
    if (!same_bits(a.sigma, b.sigma))
        return "sigmaMap";
    if (!same_bits(a.S, b.S))
        return "SMap";
    if (!same_bits(a.weight, b.weight))
        return "weightMap";
    if (a.hits != b.hits)
        return "bmuHits";
    if (!same_bits(a.mse, b.mse))
        return "MeanSquaredError";
    if (a.lastBMU != b.lastBMU || a.lastBMU.empty())
        return "lastBMU";
    return nullptr;
}

// trainBatchSomMasked (m = 0) against trainBatchSomResidentMasked on zeros (m = 1) and on garbage (m = 2) at the invalid
// positions of the same one-chunk rows; `ran`: the epochs before sigma < 1
static int compare(const char *name, size_t W, size_t H, size_t J, size_t NROWS, size_t epochs, double sigma0, double decay,
                   size_t ran)
{
    const auto rows = make_rows(NROWS, J, 2718u);
    State st[3];
    for (int m = 0; m < 3; ++m) {
        FlaggedLoader loader(rows.data(), NROWS, J, NROWS, m == 2);
        DataSet ds(loader);
        Som som{W, H, ds, Transformation::Standard(loader.getNames())};
        som.randomInitialize(7, 1);
        const size_t before = som.stateDownloads();
        if (m == 0)
            som.trainBatchSomMasked(ds, epochs, sigma0, decay);
        else
            som.trainBatchSomResidentMasked(ds, epochs, sigma0, decay);
        if (som.stateDownloads() != before)
            return fail(std::string(name) + ": training downloaded the model state");
        if (m && (!loader.isAtStartOfDataStream() || ds.hasReadWholeDataStream()))
            return fail(std::string(name) + ": the stream position was not reset");
        st[m] = state_of(som, ds, W * H, J);
    }
    if (const char *what = differs(st[0], st[1]))
        return fail(std::string(name) + ": " + what + " differs from trainBatchSomMasked");
    if (const char *what = differs(st[1], st[2]))
        return fail(std::string(name) + ": garbage at invalid positions changed " + what);
    if (st[1].mse.size() != epochs || !(st[1].mse[ran - 1] > 0.f))
        return fail(std::string(name) + ": the schedule did not run its epochs");
    for (size_t i = ran; i < epochs; ++i)
        if (st[1].mse[i] != 0.f)
            return fail(std::string(name) + ": a metric beyond the stop at sigma < 1 was written");
    for (size_t n = 0; n < W * H; ++n) {
        uint32_t bits;
        std::memcpy(&bits, &st[1].map[n * J + FlaggedLoader::DEAD], 4);
        if (bits != 0 || !std::isnan(st[1].sigma[n * J + FlaggedLoader::DEAD]))
            return fail(std::string(name) + ": the column without a valid row is not +0 / NaN at node " + std::to_string(n));
    }
    return 0;
}

int main()
{
    // 1. the one-launch path and the library's own loop
    if (int rc = compare("10x10x9", 10, 10, 9, 20, 40, 5.0, 0.05, 33))
        return rc;
    if (int rc = compare("24x20x11", 24, 20, 11, 300, 4, 3.0, 0.15, 4))
        return rc;

    // 2. two chunks: refused before anything trains
    {
        const size_t W = 6, H = 5, J = 6, NROWS = 30;
        const auto rows = make_rows(NROWS, J, 99u);
        FlaggedLoader loader(rows.data(), NROWS, J, 20, false);
        DataSet ds(loader);
        Som som{W, H, ds, Transformation::Standard(loader.getNames())};
        som.randomInitialize(7, 1);
        std::vector<float> m0(W * H * J), m1(W * H * J), sg(W * H * J), S(W * H * J), wt(W * H);
        std::vector<uint64_t> hits(W * H);
        som.getState(m0.data(), sg.data(), S.data(), wt.data(), hits.data());
        bool thrown = false;
        try {
            som.trainBatchSomResidentMasked(ds, 3, 2.0, 0.1);
        } catch (const std::invalid_argument &) {
            thrown = true;
        }
        if (!thrown)
            return fail("a two-chunk data set was not refused");
        som.getState(m1.data(), sg.data(), S.data(), wt.data(), hits.data());
        if (!same_bits(m0, m1))
            return fail("the refused call changed the map");
        for (uint64_t h : hits)
            if (h)
                return fail("the refused call counted BMU hits");
    }
    std::cout << "host_resident_masked_test ok\n";
    return 0;
}
