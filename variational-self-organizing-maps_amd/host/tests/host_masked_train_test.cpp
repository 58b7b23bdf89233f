// host_masked_train_test.cpp -- Som::trainBatchSomMasked / trainBatchSomEpochMasked of the C++ mirror
// (vsom_batch_epoch_masked).
// 1. On an all-valid DataSet a three-epoch masked schedule leaves the state, the metrics and the rows' BMUs of
//    trainBatchSom bit for bit (two chunks per epoch).
// 2. On a DataSet whose loader clears about one flag in five (and every flag of one column), the state after the masked
//    schedule does not depend on what the invalid positions hold: NaN, +inf and 1e30 there change nothing; the column
//    without a valid row is +0 with a NaN sigma; and the flags matter (the state differs from the all-valid one).
// Neither call downloads the model state into the host mirror.  Exits non-zero on a failure.
//   usage: host_masked_train_test
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
};

static State state_of(const Som &som, size_t N, size_t J)
{
    State st;
    st.map.resize(N * J);
    st.sigma.resize(N * J);
    st.S.resize(N * J);
    st.weight.resize(N);
    st.hits.resize(N);
    som.getState(st.map.data(), st.sigma.data(), st.S.data(), st.weight.data(), st.hits.data());
    st.mse = som.getMetrics().MeanSquaredError;
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
    return nullptr;
}

int main()
{
    const size_t W = 13, H = 9, J = 11, NROWS = 200, CHUNK = 120, N = W * H, EPOCHS = 3;
    const double sigma0 = 3.0, decay = 0.15;
    auto rows = make_rows(NROWS, J, 2718u);

    // 1. all valid: the masked schedule is trainBatchSom
    State plain, masked;
    std::vector<size_t> lbPlain, lbMasked;
    for (int m = 0; m < 2; ++m) {
        ArrayDataLoader loader(rows.data(), NROWS, J, CHUNK);
        DataSet ds(loader);
        Som som{W, H, ds, Transformation::Standard(loader.getNames())};
        som.randomInitialize(7, 1);
        const size_t before = som.stateDownloads();
        if (m == 0)
            som.trainBatchSom(ds, EPOCHS, sigma0, decay);
        else
            som.trainBatchSomMasked(ds, EPOCHS, sigma0, decay);
        if (som.stateDownloads() != before)
            return fail("training downloaded the model state");
        std::vector<size_t> &lb = m == 0 ? lbPlain : lbMasked;
        for (size_t s = 0; s < ds.size(); ++s)
            lb.push_back(ds.getLastBMU(s));
        (m == 0 ? plain : masked) = state_of(som, N, J);
    }
    if (const char *what = differs(plain, masked))
        return fail(std::string("all-valid masked schedule: ") + what + " differs from trainBatchSom");
    if (lbPlain != lbMasked || lbPlain.empty())
        return fail("all-valid masked schedule: the BMUs of the last chunk differ from trainBatchSom");
    if (plain.mse.size() != EPOCHS || !(plain.mse[EPOCHS - 1] > 0.f))
        return fail("the schedule did not run its epochs");

    // 2. flags cleared: what the invalid positions hold changes nothing
    State zeros, junk;
    for (int m = 0; m < 2; ++m) {
        FlaggedLoader loader(rows.data(), NROWS, J, CHUNK, m == 1);
        DataSet ds(loader);
        Som som{W, H, ds, Transformation::Standard(loader.getNames())};
        som.randomInitialize(7, 1);
        som.trainBatchSomMasked(ds, EPOCHS, sigma0, decay);
        (m == 0 ? zeros : junk) = state_of(som, N, J);
    }
    if (!differs(masked, zeros))
        return fail("cleared flags changed nothing: the masked schedule ignored them");
    for (size_t n = 0; n < N; ++n) {
        uint32_t bits;
        std::memcpy(&bits, &zeros.map[n * J + FlaggedLoader::DEAD], 4);
        if (bits != 0 || !std::isnan(zeros.sigma[n * J + FlaggedLoader::DEAD]))
            return fail("the column without a valid row is not +0 / NaN at node " + std::to_string(n));
    }
    // (NaN sigmas compare as bits here: both runs compute sqrt(0/0) the same way)
    if (const char *what = differs(zeros, junk))
        return fail(std::string("garbage at invalid positions changed ") + what);
    std::cout << "host_masked_train_test ok\n";
    return 0;
}
