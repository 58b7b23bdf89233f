// host_evaluate_test.cpp -- Som::evaluate and Som::evaluateRows of the C++ mirror (vsom_evaluate_batch).
// Trains a 10x10x9 map on 50 rows in [0,1] whose loader flags 3 columns binary and some values invalid, and prints, in
// hexfloat where a value is a float: the model state, the rows, the flags, evaluateRows' per-row report, Som::evaluate of that
// data set and of an all-continuous, all-valid one, and stateDownloads() (tests/test_gpu_host_evaluate.py repeats the calls
// through the Python binding on the same state).  Asserts that evaluate on a device state the host mirror has not seen
// downloads no state.  A Som whose hooks are device source (Transformation::Device) keeps the host loop: its evaluate must
// equal the running mean of its own per-row findBmu / euclidianWeightedDist, and its evaluateRows must refuse by name.
// Exits non-zero on a failure.
//   usage: host_evaluate_test
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

static const size_t W = 10, H = 10, J = 9, NROWS = 50, N = W * H;

static unsigned next(unsigned &s) { return s = s * 1664525u + 1013904223u; }

// rows in [0,1]; columns 1, 4 and 8 (the binary ones) hold 0 or 1
static std::vector<float> make_rows(unsigned seed)
{
    std::vector<float> r(NROWS * J);
    unsigned s = seed;
    for (size_t i = 0; i < r.size(); ++i) {
        const unsigned v = (next(s) >> 8) & 0xFFFF;
        const size_t d = i % J;
        r[i] = (d == 1 || d == 4 || d == 8) ? (float)(v & 1) : (float)v / 65536.0f;
    }
    return r;
}

// an ArrayDataLoader whose rows carry validity zeros (about one value in five, decided by (row, column)) and whose binary
// columns stay marked continuous: with ArrayDataLoader's complementary flags val = validity * continuous (Som.cpp:505) is 0
// at every binary column and the binary error vanishes
class FlaggedLoader : public ArrayDataLoader {
    std::vector<int> m_ones;

public:
    FlaggedLoader(const float *rows, size_t nrows, size_t depth) : ArrayDataLoader(rows, nrows, depth), m_ones(depth, 1) {}
    const std::vector<int> &getContinuous() const noexcept override { return m_ones; }
    bool peekFlat(size_t &) override { return false; }       // (the flat path hands over all-valid rows)
    size_t load() override
    {
        const size_t n = ArrayDataLoader::load();
        for (size_t i = 0; i < data.size(); ++i)
            for (size_t d = 0; d < data[i].valid.size(); ++d)
                data[i].valid[d] = ((i * 7 + d * 3) % 5) != 0;
        return n;
    }
};

static int fail(const std::string &what)
{
    std::cerr << "FAIL: " << what << "\n";
    return 1;
}

// the caller's hooks of the Transformation::Device Som: the plain residual x - m, as device source and as lambdas
static const char *kSource = R"(
__device__ float vsom_compare(uint32_t r, const float *x, const float *model, const float *dispersion,
                              const float *value_weight, uint32_t J, uint32_t D)
{
    return x[r] - model[r];
}
__device__ float vsom_step(uint32_t d, const float *x, const float *model, const float *value_weight,
                           uint32_t J, uint32_t D)
{
    return x[d] - model[d];
}
)";

// Som::evaluate of a Transformation::Device Som: a device context the scoring call refuses, so the host loop serves it
static int device_source_som(const std::vector<float> &rows, const std::vector<float> &map)
{
    using V = Eigen::VectorXf;
    const auto residual = [](const V &x, const V &m) { return V(x - m); };
    const Transformation onDevice = Transformation::Device(
        "residual", kSource, [](size_t j) { return j; }, [](size_t j) { return j; },
        [residual](const V &x, const V &m, const V &, const V &) { return residual(x, m); },
        [residual](const V &x, const V &m, const V &) { return residual(x, m); });
    ArrayDataLoader loader(rows.data(), NROWS, J);
    DataSet ds(loader);
    Som som(W, H, ds, onDevice);
    if (som.context() == nullptr)
        return fail("the device transformation did not create a device context");
    som.setState(map.data(), nullptr, nullptr, nullptr, nullptr);
    ds.loadNextDataFromStream();
    if (ds.size() != NROWS)
        return fail("the device-source data set did not load its rows");
    const double e = som.evaluate(ds);
    const V ones = V::Ones(J);
    double want = 0;
    for (size_t i = 0; i < NROWS; ++i) {
        const V x = ds.getData(i);
        const SomIndex b = som.findBmu(x, ones, ones);
        want += 1.0 / ((double)i + 1.0) * ((double)(float)som.euclidianWeightedDist(b, x, ones, ones) - want);
    }
    if (std::memcmp(&e, &want, sizeof e) != 0 || !(e > 0))
        return fail("evaluate of a Transformation::Device Som is not the running mean of its rows' BMU distances");
    bool refused = false;
    try {
        (void)som.evaluateRows(ds);
    } catch (const std::runtime_error &err) {
        refused = std::string(err.what()).find("Transformation::Device") != std::string::npos;
    }
    if (!refused)
        return fail("evaluateRows of a Transformation::Device Som did not refuse by name");
    std::cout << std::hexfloat << "evaluate_device_source " << e << "\n" << std::defaultfloat;
    return 0;
}

template <typename T> static void line(const char *key, const T *v, size_t n)
{
    std::cout << key;
    for (size_t i = 0; i < n; ++i)
        std::cout << " " << v[i];
    std::cout << "\n";
}

int main()
{
    auto rows = make_rows(777u);
    FlaggedLoader loader(rows.data(), NROWS, J);
    std::vector<ColumnSpec> spec;
    for (size_t d = 0; d < J; ++d)
        spec.emplace_back("c" + std::to_string(d), 1.0f, (d == 1 || d == 4 || d == 8) ? 1 : 0);
    loader.setColumnSpec(spec);
    ArrayDataLoader plainLoader(rows.data(), NROWS, J);
    DataSet ds(loader), plain(plainLoader);
    Som som{W, H, ds, Transformation::Standard(loader.getNames())};
    som.randomInitialize(9, 1);
    som.train(ds, 3, 0.0, 0.0, 4.0, 0.2, Som::WeigthDecayFunction::BatchMap);
    std::cout << "group_members=" << (som.group() ? vsom_group_size(som.group()) : 1) << "\n";
    ds.loadNextDataFromStream();
    plain.loadNextDataFromStream();
    if (ds.size() != NROWS || plain.size() != NROWS)
        return fail("the data sets did not load their rows");

    // a device state the host mirror has not seen: the mirror is refreshed, one more epoch dirties it again
    (void)som.getNeuron((size_t)0);
    (void)som.trainBatchSomEpoch(ds, 1.5, false);
    const size_t before = som.stateDownloads();

    const double e = som.evaluate(ds);
    const Som::EvaluateRows r = som.evaluateRows(ds);
    const double ep = som.evaluate(plain);
    if (r.bmu.size() != NROWS || r.dist.size() != NROWS || r.bsum.size() != NROWS || r.nrepl.size() != NROWS)
        return fail("report sizes");
    for (size_t i = 0; i < NROWS; ++i)
        if (r.bmu[i] >= N || r.nrepl[i] > J)
            return fail("row " + std::to_string(i) + ": report out of range");
    if (som.stateDownloads() != before)
        return fail("evaluate / evaluateRows downloaded the model state");
    std::cout << "state_downloads_by_evaluate=" << som.stateDownloads() - before << "\n";
    (void)som.getNeuron((size_t)0);
    if (som.stateDownloads() != before + 1)
        return fail("the device state was not dirty: the download check above checked nothing");

    std::vector<float> m(N * J), sg(N * J), S(N * J), w(N);
    std::vector<uint64_t> h(N);
    som.getState(m.data(), sg.data(), S.data(), w.data(), h.data());
    std::vector<int> valid(NROWS * J, 0);
    for (size_t i = 0; i < NROWS; ++i) {
        const Eigen::VectorXi v = ds.getValidity(i);
        for (size_t d = 0; d < J && d < (size_t)v.size(); ++d)
            valid[i * J + d] = v[(Eigen::Index)d];
    }
    const Eigen::ArrayXi bin = ds.getBinary(), con = ds.getContinuous();
    std::cout << std::hexfloat;
    line("map", m.data(), m.size());
    line("rows", ds.contiguous(), NROWS * J);
    line("valid", valid.data(), valid.size());
    line("binary", bin.data(), (size_t)bin.size());
    line("continuous", con.data(), (size_t)con.size());
    line("bmu", r.bmu.data(), NROWS);
    line("dist", r.dist.data(), NROWS);
    line("bsum", r.bsum.data(), NROWS);
    line("nrepl", r.nrepl.data(), NROWS);
    std::cout << "rows_error " << r.error << "\n";
    std::cout << "evaluate " << e << "\n";
    std::cout << "evaluate_plain " << ep << "\n";
    if (device_source_som(rows, m))
        return 1;
    std::cout << "host_evaluate_test ok\n";
    return 0;
}
