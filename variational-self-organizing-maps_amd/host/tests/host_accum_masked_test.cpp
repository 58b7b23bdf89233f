// host_accum_masked_test.cpp -- Som::trainBatchSomWholeMasked of the C++ mirror (vsom_batch_accum_chunk_masked).
// The golden SQLite database has no NULL (every column is NOT NULL), so the rows come from an ArrayDataLoader whose flags
// are cleared by (row of the STREAM, column): the mask of a row does not depend on how the stream is cut into chunks.
// 1. On an all-valid DataSet the masked driver leaves the state, the metrics and the BMUs of trainBatchSomWhole bit for bit.
// 2. With flags cleared, on one chunk and resetBmu, it is trainBatchSomMasked bit for bit.
// 3. The split does not matter: chunks of 20 and of 7 give the one-chunk state and metrics (with resetBmu and without), and
//    the BMUs the data set holds at the end are those of the one-chunk run's last rows.
// 4. What the invalid positions hold (NaN, +inf, 1e30) changes nothing; the column without a valid row is +0 / NaN; the
//    flags matter.
// 5. A Som over several devices throws.
// No call downloads the model state into the host mirror.  Exits non-zero on a failure.
//   usage: host_accum_masked_test [state.bin]
// state.bin receives map, sigmaMap, weightMap (float), bmuHits (uint64) and the metrics (float) of the flagged Standard run
// in chunks of 7 that keeps the BMUs, for a comparison with the Python mirror.
#include "SOM.hpp"
#include "vsom_hip.h"
#include "DataSet.hpp"
#include "Transformation.hpp"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
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

// row r of the stream, column d: all of column DEAD invalid, column LATE invalid from row 24 on (dirty in the last chunk
// only, for both splits), column EARLY invalid in rows 0-2 only, and about one value in five elsewhere
class FlaggedLoader : public ArrayDataLoader {
    bool m_garbage;

public:
    static constexpr size_t DEAD = 4, LATE = 6, EARLY = 9;
    static bool valid(size_t r, size_t d)
    {
        if (d == DEAD)
            return false;
        if (d == LATE)
            return r < 24;
        if (d == EARLY)
            return r > 2;
        return d == 0 || ((r * 7 + d * 3) % 5) != 0;     // (column 0 stays clean)
    }
    FlaggedLoader(const float *rows, size_t nrows, size_t depth, size_t maxLoad, bool garbage)
        : ArrayDataLoader(rows, nrows, depth, maxLoad), m_garbage(garbage)
    {
    }
    bool peekFlat(size_t &) override { return false; }       // (the flat path hands over all-valid rows)
    size_t load() override
    {
        const size_t first = m_currentIndex;                 // the stream row of the chunk's first row
        const size_t n = ArrayDataLoader::load();
        const float junk[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), 1e30f};
        for (size_t i = 0; i < data.size(); ++i)
            for (size_t d = 0; d < data[i].valid.size(); ++d) {
                const bool ok = valid(first + i, d);
                data[i].valid[d] = ok;
                if (!ok && m_garbage)
                    data[i].values[(Eigen::Index)d] = junk[(first + i + d) % 3];
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

enum Driver { WHOLE, MASKED_CHUNKS, WHOLE_MASKED };
enum Flags { ALL_VALID, FLAGGED, FLAGGED_JUNK };

static const size_t W = 9, H = 7, J = 11, NROWS = 30, EPOCHS = 5;
static const double SIGMA0 = 3.0, DECAY = 0.3;      // sigma 3, 2.22, 1.65, 1.22, then 0.90 < 1: four epochs run

typedef Transformation (*Kind)(const std::vector<std::string> &);
static Transformation standard(const std::vector<std::string> &n) { return Transformation::Standard(n); }
static Transformation median(const std::vector<std::string> &n) { return Transformation::StandardMedianEstimator(n); }

static State run(Driver driver, Flags flags, Kind kind, const std::vector<float> &rows, size_t chunk, bool resetBmu, int *rc)
{
    ArrayDataLoader plain(rows.data(), NROWS, J, chunk);
    FlaggedLoader flagged(rows.data(), NROWS, J, chunk, flags == FLAGGED_JUNK);
    IDataLoader &loader = flags == ALL_VALID ? static_cast<IDataLoader &>(plain) : flagged;
    DataSet ds(loader);
    Som som{W, H, ds, kind(loader.getNames())};
    som.randomInitialize(7, 1);
    const size_t before = som.stateDownloads();
    if (driver == WHOLE)
        som.trainBatchSomWhole(ds, EPOCHS, SIGMA0, DECAY, false, resetBmu);
    else if (driver == MASKED_CHUNKS)
        som.trainBatchSomMasked(ds, EPOCHS, SIGMA0, DECAY);
    else
        som.trainBatchSomWholeMasked(ds, EPOCHS, SIGMA0, DECAY, false, resetBmu);
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

static int compare(const std::string &name, Kind kind, const std::vector<float> &rows)
{
    int rc = 0;
    // 1. all valid
    for (size_t chunk : {NROWS, size_t{20}, size_t{7}})
        for (bool reset : {true, false}) {
            const State a = run(WHOLE, ALL_VALID, kind, rows, chunk, reset, &rc);
            const State b = run(WHOLE_MASKED, ALL_VALID, kind, rows, chunk, reset, &rc);
            if (rc)
                return rc;
            const std::string tag = name + ": all valid, chunks of " + std::to_string(chunk) + (reset ? " reset" : " keep");
            if (const char *what = differs(a, b))
                return fail(tag + ": " + what + " differs from trainBatchSomWhole");
            if (a.lastBMU != b.lastBMU || a.lastBMU.empty())
                return fail(tag + ": lastBMU differs from trainBatchSomWhole");
            if (!(a.mse[3] > 0.f) || a.mse[4] != 0.f)
                return fail(tag + ": the schedule did not run four epochs");
        }
    // 2. flags cleared, one chunk: the masked epoch itself
    const State chunks = run(MASKED_CHUNKS, FLAGGED, kind, rows, NROWS, true, &rc);
    const State valid = run(WHOLE_MASKED, ALL_VALID, kind, rows, NROWS, true, &rc);
    for (bool reset : {true, false}) {
        const State one = run(WHOLE_MASKED, FLAGGED, kind, rows, NROWS, reset, &rc);
        if (rc)
            return rc;
        if (reset) {
            if (const char *what = differs(one, chunks))
                return fail(name + ": one chunk: " + what + " differs from trainBatchSomMasked");
            if (one.lastBMU != chunks.lastBMU || one.lastBMU.size() != NROWS)
                return fail(name + ": one chunk: lastBMU differs from trainBatchSomMasked");
            if (!differs(one, valid))
                return fail(name + ": cleared flags changed nothing");
        }
        // 3. the split does not matter; 4. nor does what the invalid positions hold
        for (size_t chunk : {size_t{20}, size_t{7}})
            for (Flags flags : {FLAGGED, FLAGGED_JUNK}) {
                const State split = run(WHOLE_MASKED, flags, kind, rows, chunk, reset, &rc);
                if (rc)
                    return rc;
                const std::string tag = name + (reset ? " reset" : " keep") + ", chunks of " + std::to_string(chunk) +
                                        (flags == FLAGGED_JUNK ? ", junk at invalid positions" : "");
                if (const char *what = differs(split, one))
                    return fail(tag + ": " + what + " differs from the one-chunk epoch");
                const size_t tail = NROWS % chunk ? NROWS % chunk : chunk;
                if (split.lastBMU.size() != tail)
                    return fail(tag + ": the data set does not hold its last chunk's BMUs");
                for (size_t s = 0; s < tail; ++s)
                    if (split.lastBMU[s] != one.lastBMU[NROWS - tail + s])
                        return fail(tag + ": lastBMU of the last chunk differs");
                for (size_t n = 0; n < W * H; ++n) {
                    uint32_t bits;
                    std::memcpy(&bits, &split.map[n * J + FlaggedLoader::DEAD], 4);
                    if (bits != 0 || !std::isnan(split.sigma[n * J + FlaggedLoader::DEAD]))
                        return fail(tag + ": the column without a valid row is not +0 / NaN at node " + std::to_string(n));
                }
            }
    }
    return 0;
}

int main(int argc, char **argv)
{
    const auto rows = make_rows(NROWS, J, 2718u);
    if (int rc = compare("standard", standard, rows))
        return rc;
    if (int rc = compare("median", median, rows))
        return rc;

    if (argc > 1) {
        int rc = 0;
        const State st = run(WHOLE_MASKED, FLAGGED, standard, rows, 7, false, &rc);
        if (rc)
            return rc;
        std::ofstream f(argv[1], std::ios::binary);
        f.write((const char *)st.map.data(), (std::streamsize)(st.map.size() * 4));
        f.write((const char *)st.sigma.data(), (std::streamsize)(st.sigma.size() * 4));
        f.write((const char *)st.weight.data(), (std::streamsize)(st.weight.size() * 4));
        f.write((const char *)st.hits.data(), (std::streamsize)(st.hits.size() * 8));
        f.write((const char *)st.mse.data(), (std::streamsize)(st.mse.size() * 4));
        if (!f)
            return fail(std::string("cannot write ") + argv[1]);
    }

    // several devices (the same one twice: the group's flow on one GPU)
    {
        Som::setDevices({0, 0});
        ArrayDataLoader loader(rows.data(), NROWS, J, 20);
        DataSet ds(loader);
        Som som{W, H, ds, Transformation::Standard(loader.getNames())};
        Som::setDevices({});
        som.randomInitialize(7, 1);
        bool thrown = false;
        try {
            som.trainBatchSomWholeMasked(ds, 3, 2.0, 0.1);
        } catch (const std::runtime_error &) {
            thrown = true;
        }
        if (!thrown)
            return fail("a multi-device Som was not refused");
    }
    std::cout << "host_accum_masked_test ok\n";
    return 0;
}
