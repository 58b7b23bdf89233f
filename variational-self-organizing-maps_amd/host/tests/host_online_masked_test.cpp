// host_online_masked_test.cpp -- Som::trainBasicSomMasked of the C++ mirror (vsom_train_online_chunk_masked).
// A 9 x 7 x 11 map is trained for four epochs (sigma 3 down through the clamp at 1.0, two chunks per epoch) on a DataSet
// whose loader clears about one flag in five and every flag of one column, with NaN / +inf / 1e30 at those positions.
// 1. On an all-valid DataSet the masked schedule leaves the state, the metrics and the rows' BMUs of trainBasicSom bit for bit.
// 2. The flags matter (the state differs from the all-valid one), garbage at the invalid positions changes nothing, and the
//    column without a valid row keeps its map, SMap and sigmaMap bits.
// Training downloads no model state.  Prints as hexfloat what tests/test_gpu_host_online_masked.py replays through the
// Python binding: the starting state, the rows, the flags, the schedule, the final state, the metrics and the last chunk's
// BMUs.  Exits non-zero on a failure.
//   usage: host_online_masked_test
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

static bool flag_of(size_t i, size_t d, size_t dead) { return d != dead && ((i * 7 + d * 3) % 5) != 0; }

// an ArrayDataLoader whose rows carry validity zeros -- decided by (row of the chunk, column), and all of column DEAD --
// and, with `garbage`, NaN / +inf / 1e30 at those positions
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
                const bool ok = flag_of(i, d, DEAD);
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

static void print(const char *name, const std::vector<float> &v)
{
    std::cout << name << std::hexfloat;
    for (float x : v)
        std::cout << ' ' << x;
    std::cout << std::defaultfloat << "\n";
}

template <class T>
static void print_int(const char *name, const std::vector<T> &v)
{
    std::cout << name;
    for (T x : v)
        std::cout << ' ' << x;
    std::cout << "\n";
}

int main()
{
    const size_t W = 9, H = 7, J = 11, NROWS = 50, CHUNK = 30, N = W * H, EPOCHS = 4;
    const double eta0 = 0.5, etaDecay = 0.1, sigma0 = 3.0, sigmaDecay = 0.45;   // sigma 3, 1.91, 1.22, then the clamp at 1.0
    const auto fn = Som::WeigthDecayFunction::InverseProportional;
    auto rows = make_rows(NROWS, J, 1618u);

    // 1. all valid: the masked schedule is trainBasicSom
    State plain, masked, start;
    std::vector<size_t> lbPlain, lbMasked;
    for (int m = 0; m < 2; ++m) {
        ArrayDataLoader loader(rows.data(), NROWS, J, CHUNK);
        DataSet ds(loader);
        Som som{W, H, ds, Transformation::Standard(loader.getNames())};
        som.randomInitialize(7, 1);
        const size_t before = som.stateDownloads();
        if (m == 0)
            som.trainBasicSom(ds, EPOCHS, eta0, etaDecay, sigma0, sigmaDecay, fn);
        else
            som.trainBasicSomMasked(ds, EPOCHS, eta0, etaDecay, sigma0, sigmaDecay, fn);
        if (som.stateDownloads() != before)
            return fail("training downloaded the model state");
        std::vector<size_t> &lb = m == 0 ? lbPlain : lbMasked;
        for (size_t s = 0; s < ds.size(); ++s)
            lb.push_back(ds.getLastBMU(s));
        (m == 0 ? plain : masked) = state_of(som, N, J);
    }
    if (const char *what = differs(plain, masked))
        return fail(std::string("all-valid masked schedule: ") + what + " differs from trainBasicSom");
    if (lbPlain != lbMasked || lbPlain.empty())
        return fail("all-valid masked schedule: the BMUs of the last chunk differ from trainBasicSom");
    if (plain.mse.size() != EPOCHS || !(plain.mse[EPOCHS - 1] > 0.f))
        return fail("the schedule did not run its epochs");

    // 2. flags cleared
    State zeros, junk;
    std::vector<uint64_t> lbJunk;
    for (int m = 0; m < 2; ++m) {
        FlaggedLoader loader(rows.data(), NROWS, J, CHUNK, m == 1);
        DataSet ds(loader);
        Som som{W, H, ds, Transformation::Standard(loader.getNames())};
        som.randomInitialize(7, 1);
        if (m == 1)
            start = state_of(som, N, J);
        som.trainBasicSomMasked(ds, EPOCHS, eta0, etaDecay, sigma0, sigmaDecay, fn);
        (m == 0 ? zeros : junk) = state_of(som, N, J);
        if (m == 1)
            for (size_t s = 0; s < ds.size(); ++s)
                lbJunk.push_back((uint64_t)ds.getLastBMU(s));
    }
    if (!differs(masked, zeros))
        return fail("cleared flags changed nothing: the masked schedule ignored them");
    if (const char *what = differs(zeros, junk))
        return fail(std::string("garbage at invalid positions changed ") + what);
    for (size_t n = 0; n < N; ++n) {
        const size_t at = n * J + FlaggedLoader::DEAD;
        if (std::memcmp(&junk.map[at], &start.map[at], 4) || std::memcmp(&junk.S[at], &start.S[at], 4) ||
            std::memcmp(&junk.sigma[at], &start.sigma[at], 4))
            return fail("the column without a valid row was written at node " + std::to_string(n));
    }

    // what the Python binding replays
    std::vector<int> valid(NROWS * J);
    for (size_t r = 0; r < NROWS; ++r)
        for (size_t d = 0; d < J; ++d)
            valid[r * J + d] = flag_of(r % CHUNK, d, FlaggedLoader::DEAD);
    std::cout << "shape " << W << ' ' << H << ' ' << J << ' ' << NROWS << ' ' << CHUNK << ' ' << EPOCHS << "\n";
    std::cout << "schedule " << std::hexfloat << eta0 << ' ' << etaDecay << ' ' << sigma0 << ' ' << sigmaDecay
              << std::defaultfloat << "\n";
    print("rows", rows);
    print_int("valid", valid);
    print("map0", start.map);
    print("sigma0", start.sigma);
    print("S0", start.S);
    print("weight0", start.weight);
    print("map", junk.map);
    print("sigma", junk.sigma);
    print("S", junk.S);
    print("weight", junk.weight);
    print_int("hits", junk.hits);
    print("mse", junk.mse);
    print_int("lastbmu", lbJunk);
    std::cout << "host_online_masked_test ok\n";
    return 0;
}
