// host_accum_test.cpp -- Som::trainBatchSomWhole of the C++ mirror (vsom_batch_accum_begin / _chunk / _end).
// 1. On a one-chunk DataSet it leaves the state, the metrics and the rows' BMUs of trainBatchSom bit for bit.
// 2. The split does not matter: the same rows loaded as 20 + 10, as 7 + 7 + 7 + 7 + 2 and as one chunk give the same
//    state and metrics (with resetBmu and without), and the BMUs the data set holds at the end are those of the one-chunk
//    run's last rows.  With resetBmu the one-chunk run is trainBatchSom, so every split equals it.
// 3. A Som over several devices throws.
// No call downloads the model state into the host mirror.  Exits non-zero on a failure.
//   usage: host_accum_test
#include "SOM.hpp"
#include "vsom_hip.h"
#include "DataSet.hpp"
#include "Transformation.hpp"

#include <cstdint>
#include <cstring>
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

struct State {
    std::vector<float> map, sigma, S, weight;
    std::vector<uint64_t> hits;
    std::vector<float> mse;
    std::vector<size_t> lastBMU;
};

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

enum Driver { BATCH, WHOLE_RESET, WHOLE_KEEP };

// the rows as chunks of `chunk`, trained by `driver`; *rc != 0 on a failure
static State run(Driver driver, Transformation (*kind)(const std::vector<std::string> &), size_t W, size_t H, size_t J,
                 const std::vector<float> &rows, size_t NROWS, size_t chunk, size_t epochs, double sigma0, double decay, int *rc)
{
    ArrayDataLoader loader(rows.data(), NROWS, J, chunk);
    DataSet ds(loader);
    Som som{W, H, ds, kind(loader.getNames())};
    som.randomInitialize(7, 1);
    const size_t before = som.stateDownloads();
    if (driver == BATCH)
        som.trainBatchSom(ds, epochs, sigma0, decay);
    else
        som.trainBatchSomWhole(ds, epochs, sigma0, decay, false, driver == WHOLE_RESET);
    if (som.stateDownloads() != before)
        *rc = fail("training downloaded the model state");
    if (!loader.isAtStartOfDataStream() || ds.hasReadWholeDataStream())
        *rc = fail("the stream position was not reset");
    State st;
    const size_t N = W * H;
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

static Transformation standard(const std::vector<std::string> &n) { return Transformation::Standard(n); }
static Transformation median(const std::vector<std::string> &n) { return Transformation::StandardMedianEstimator(n); }

static int compare(const char *name, Transformation (*kind)(const std::vector<std::string> &))
{
    const size_t W = 9, H = 7, J = 11, NROWS = 30, epochs = 5;
    const double sigma0 = 3.0, decay = 0.3;      // sigma 3, 2.22, 1.65, 1.22, then 0.90 < 1: four epochs run
    const auto rows = make_rows(NROWS, J, 2718u);
    int rc = 0;
    const State batch = run(BATCH, kind, W, H, J, rows, NROWS, NROWS, epochs, sigma0, decay, &rc);
    if (rc)
        return rc;
    if (!(batch.mse[3] > 0.f) || batch.mse[4] != 0.f)
        return fail(std::string(name) + ": the schedule did not run four epochs");
    for (Driver driver : {WHOLE_RESET, WHOLE_KEEP}) {
        const State one = run(driver, kind, W, H, J, rows, NROWS, NROWS, epochs, sigma0, decay, &rc);
        if (rc)
            return rc;
        if (one.lastBMU.size() != NROWS)
            return fail(std::string(name) + ": the one-chunk run holds no BMUs");
        if (driver == WHOLE_RESET) {
            if (const char *what = differs(one, batch))
                return fail(std::string(name) + ": one chunk: " + what + " differs from trainBatchSom");
            if (one.lastBMU != batch.lastBMU)
                return fail(std::string(name) + ": one chunk: lastBMU differs from trainBatchSom");
        }
        for (size_t chunk : {size_t{20}, size_t{7}}) {
            const State split = run(driver, kind, W, H, J, rows, NROWS, chunk, epochs, sigma0, decay, &rc);
            if (rc)
                return rc;
            const std::string tag = std::string(name) + (driver == WHOLE_RESET ? " reset" : " keep") + ", chunks of " +
                                    std::to_string(chunk);
            if (const char *what = differs(split, one))
                return fail(tag + ": " + what + " differs from the one-chunk epoch");
            const size_t tail = NROWS % chunk ? NROWS % chunk : chunk;
            if (split.lastBMU.size() != tail)
                return fail(tag + ": the data set does not hold its last chunk's BMUs");
            for (size_t s = 0; s < tail; ++s)
                if (split.lastBMU[s] != one.lastBMU[NROWS - tail + s])
                    return fail(tag + ": lastBMU of the last chunk differs");
        }
    }
    return 0;
}

int main()
{
    if (int rc = compare("standard", standard))
        return rc;
    if (int rc = compare("median", median))
        return rc;

    // several devices (the same one twice: the group's flow on one GPU)
    {
        const size_t W = 6, H = 5, J = 4, NROWS = 30;
        const auto rows = make_rows(NROWS, J, 99u);
        Som::setDevices({0, 0});
        ArrayDataLoader loader(rows.data(), NROWS, J, 20);
        DataSet ds(loader);
        Som som{W, H, ds, Transformation::Standard(loader.getNames())};
        Som::setDevices({});
        som.randomInitialize(7, 1);
        bool thrown = false;
        try {
            som.trainBatchSomWhole(ds, 3, 2.0, 0.1);
        } catch (const std::runtime_error &) {
            thrown = true;
        }
        if (!thrown)
            return fail("a multi-device Som was not refused");
    }
    std::cout << "host_accum_test ok\n";
    return 0;
}
