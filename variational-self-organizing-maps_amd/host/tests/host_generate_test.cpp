// host_generate_test.cpp -- Som::generateRows, Som::decodeUnits and Som::autoEncoder of the C++ mirror (vsom_generate_batch,
// vsom_decode_nodes).  Sets a 10x10x9 state (map in [0,1], sigma in [0.05, 0.3], every seventh node without hits), draws and
// decodes 20 rows under both rules with given random numbers and prints, in hexfloat where a value is a float, the state, the
// rows, the random numbers and the results (tests/test_gpu_host_generate.py checks them against the Python binding and the
// float64 restatement).  Asserts that decodeUnits repeats generateRows' records bit for bit, that bad sizes are refused, and
// that autoEncoder downloads no model state; autoEncoder's own text is printed between marker lines, once with mass and once
// with min hits above every hit (every row takes node 0).  Exits non-zero on a failure.
//   usage: host_generate_test
#include "SOM.hpp"
#include "vsom_hip.h"
#include "DataSet.hpp"
#include "Transformation.hpp"

#include <cstdint>
#include <cstring>
#include <iostream>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

static const size_t W = 10, H = 10, J = 9, NROWS = 20, N = W * H;
static const uint64_t MIN_HITS = 2;

static unsigned next(unsigned &s) { return s = s * 1664525u + 1013904223u; }
static float unit_float(unsigned &s) { return (float)((next(s) >> 8) & 0xFFFF) / 65536.0f; }

static int fail(const std::string &what)
{
    std::cerr << "FAIL: " << what << "\n";
    return 1;
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
    unsigned s = 2024u;
    std::vector<float> rows(NROWS * J), m(N * J), sg(N * J), S(N * J, 0.f), w(N, 1.f);
    std::vector<uint64_t> h(N);
    for (auto &v : rows)
        v = unit_float(s);
    for (auto &v : m)
        v = unit_float(s);
    for (auto &v : sg)
        v = 0.05f + 0.25f * unit_float(s);
    for (size_t i = 0; i < N; ++i)
        h[i] = i % 7 == 3 ? 0 : 3 + i % 5;
    ArrayDataLoader loader(rows.data(), NROWS, J);
    DataSet ds(loader);
    Som som{W, H, ds, Transformation::Standard(loader.getNames())};
    som.setState(m.data(), sg.data(), S.data(), w.data(), h.data());
    std::cout << "group_members=" << (som.group() ? vsom_group_size(som.group()) : 1) << "\n";
    ds.loadNextDataFromStream();
    if (ds.size() != NROWS)
        return fail("the data set did not load its rows");

    // ---- generateRows / decodeUnits with given random numbers
    std::vector<double> u(NROWS), l(NROWS * J);
    std::mt19937_64 g(31);
    for (auto &x : u)
        x = std::generate_canonical<double, 53>(g);
    for (auto &x : l)
        x = (double)(g() % 999 + 1) / 1000;       // the reference's grid without its 0
    l[0] = 0.5;
    l[J + 1] = 0.0;
    l[2 * J + 2] = 1.0;
    const Som::GeneratedRows pr = som.generateRows(ds, MIN_HITS, u, l, true);
    const Som::GeneratedRows aw = som.generateRows(ds, MIN_HITS, u, l, false);
    if (pr.columns != J || pr.unit.size() != NROWS || pr.record.size() != NROWS * J || aw.unit.size() != NROWS ||
        aw.record.size() != NROWS * J)
        return fail("report sizes");
    for (size_t i = 0; i < NROWS; ++i)
        if (pr.unit[i] >= N || aw.unit[i] >= N || h[pr.unit[i]] < MIN_HITS || h[aw.unit[i]] < MIN_HITS)
            return fail("row " + std::to_string(i) + ": a unit out of range or without the hits");
    const std::vector<double> again = som.decodeUnits(pr.unit, l);
    if (again.size() != pr.record.size() || std::memcmp(again.data(), pr.record.data(), again.size() * 8) != 0)
        return fail("decodeUnits does not repeat generateRows' records");
    const std::vector<uint64_t> nodes = {0, 37, 99};
    const std::vector<double> ln(l.begin(), l.begin() + 3 * J);
    const std::vector<double> dec = som.decodeUnits(nodes, ln);
    if (!som.decodeUnits({}, {}).empty())
        return fail("decodeUnits of nothing");
    int refused = 0;
    try {
        (void)som.generateRows(ds, MIN_HITS, std::vector<double>(NROWS - 1, 0.5), l, true);
    } catch (const std::invalid_argument &) {
        ++refused;
    }
    try {
        (void)som.generateRows(ds, MIN_HITS, u, std::vector<double>(NROWS * J - 1, 0.5), true);
    } catch (const std::invalid_argument &) {
        ++refused;
    }
    try {
        (void)som.decodeUnits(nodes, l);
    } catch (const std::invalid_argument &) {
        ++refused;
    }
    try {
        (void)som.decodeUnits({N}, std::vector<double>(J, 0.5));
    } catch (const std::runtime_error &) {
        ++refused;
    }
    if (refused != 4)
        return fail("a bad size or node was not refused");
    // no mass: UINT64_MAX and NaN
    const Som::GeneratedRows none = som.generateRows(ds, (size_t)1 << 30, u, l, true);
    for (size_t i = 0; i < NROWS; ++i)
        if (none.unit[i] != UINT64_MAX)
            return fail("no mass: a unit was drawn");
    for (double v : none.record) {
        uint64_t bits;
        std::memcpy(&bits, &v, 8);
        if (bits != 0x7FF8000000000000ull)
            return fail("no mass: a record value is not the quiet NaN");
    }

    std::cout << std::hexfloat;
    line("map", m.data(), m.size());
    line("sigma", sg.data(), sg.size());
    line("hits", h.data(), h.size());
    line("rows", ds.contiguous(), NROWS * J);
    line("u", u.data(), u.size());
    line("l", l.data(), l.size());
    line("unit_per_row", pr.unit.data(), NROWS);
    line("record_per_row", pr.record.data(), pr.record.size());
    line("unit_as_written", aw.unit.data(), NROWS);
    line("record_as_written", aw.record.data(), aw.record.size());
    line("decode_units", nodes.data(), nodes.size());
    line("decode_record", dec.data(), dec.size());
    std::cout << std::defaultfloat;

    // ---- autoEncoder: its text, on a device state the host mirror has not seen
    (void)som.getNeuron((size_t)0);
    som.setState(m.data(), sg.data(), S.data(), w.data(), h.data());
    const size_t before = som.stateDownloads();
    std::cout << "autoencoder_begin\n";
    const int ok1 = som.autoEncoder(&ds, MIN_HITS);
    std::cout << "autoencoder_end\n";
    std::cout << "autoencoder_nomass_begin\n";
    const int ok2 = som.autoEncoder(&ds, (size_t)1 << 30);
    std::cout << "autoencoder_nomass_end\n";
    if (!ok1 || !ok2)
        return fail("autoEncoder did not return true");
    if (som.stateDownloads() != before)
        return fail("autoEncoder downloaded the model state");
    std::cout << "state_downloads_by_autoencoder=" << som.stateDownloads() - before << "\n";
    (void)som.getNeuron((size_t)0);
    if (som.stateDownloads() != before + 1)
        return fail("the device state was not dirty: the download check above checked nothing");
    std::cout << "host_generate_test ok\n";
    return 0;
}
