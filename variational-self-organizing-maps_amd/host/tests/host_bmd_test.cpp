// host_bmd_test.cpp -- Som::drawModelVectors and Som::variationalAutoEncoder of the C++ mirror (vsom_bmd_batch).
// Trains a map, draws a node for every row with given uniforms and writes the state, the rows, the uniforms, the draws
// and the norms to <outdir>/bmd_draws.bin (tests/test_gpu_host_bmd.py repeats the draws through the Python binding);
// then checks variationalAutoEncoder over 100 calls on engineered states and exits non-zero on a failure.
//   usage: host_bmd_test <outdir>
#include "SOM.hpp"
#include "vsom_hip.h"
#include "DataSet.hpp"
#include "Transformation.hpp"

#include <cstdint>
#include <fstream>
#include <iostream>
#include <random>
#include <set>
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

// the distinct results of 100 calls
static std::set<size_t> vae_results(const Som &som, const DataSet &ds, size_t minHits)
{
    std::set<size_t> seen;
    for (int i = 0; i < 100; ++i)
        seen.insert(som.variationalAutoEncoder(&ds, minHits));
    return seen;
}

int main(int argc, char **argv)
{
    if (argc < 2)
        return fail("usage: host_bmd_test <outdir>");
    const std::string out = argv[1];
    const size_t W = 12, H = 9, J = 10, NROWS = 300, N = W * H;
    const uint64_t MIN_HITS = 2;
    auto rows = make_rows(NROWS, J, 4242u);
    ArrayDataLoader loader(rows.data(), NROWS, J);
    DataSet ds(loader);
    Som som{W, H, ds, Transformation::Standard(loader.getNames())};
    som.randomInitialize(5, 1);
    som.train(ds, 2, 0.0, 0.0, 3.0, 0.2, Som::WeigthDecayFunction::BatchMap);   // hits, some nodes without any
    std::cout << "group_members=" << (som.group() ? vsom_group_size(som.group()) : 1) << "\n";
    ds.loadNextDataFromStream();

    // ---- drawModelVectors with given uniforms
    std::vector<double> u(ds.size()), norm;
    std::mt19937_64 g(99);
    for (auto &x : u)
        x = std::generate_canonical<double, 53>(g);
    u[0] = 0.0;
    u[1] = std::nextafter(1.0, 0.0);
    const std::vector<uint64_t> drawn = som.drawModelVectors(&ds, MIN_HITS, u, &norm);
    {
        const size_t D = som.getDepth();
        std::vector<float> m(N * D), s(N * D), S(N * D), w(N);
        std::vector<uint64_t> h(N);
        som.getState(m.data(), s.data(), S.data(), w.data(), h.data());
        std::ofstream f(out + "/bmd_draws.bin", std::ios::binary);
        const uint64_t hdr[5] = {W, H, J, ds.size(), MIN_HITS};
        f.write((const char *)hdr, sizeof(hdr));
        f.write((const char *)m.data(), m.size() * 4);
        f.write((const char *)h.data(), h.size() * 8);
        f.write((const char *)ds.contiguous(), ds.size() * J * 4);
        f.write((const char *)u.data(), u.size() * 8);
        f.write((const char *)drawn.data(), drawn.size() * 8);
        f.write((const char *)norm.data(), norm.size() * 8);
    }

    // ---- variationalAutoEncoder: the last row's draw
    const size_t D = som.getDepth();
    std::vector<float> m(N * D), s(N * D), S(N * D), w(N);
    std::vector<uint64_t> h(N);
    som.getState(m.data(), s.data(), S.data(), w.data(), h.data());
    // one eligible node (not node 0)
    std::vector<uint64_t> h1(N, 0);
    h1[37] = 5;
    som.setState(m.data(), s.data(), S.data(), w.data(), h1.data());
    auto seen = vae_results(som, ds, 1);
    if (seen != std::set<size_t>{37})
        return fail("one eligible node: drew something else");
    std::cout << "vae_one ok\n";
    // two eligible nodes with identical model rows: both are drawn, nothing else
    std::vector<uint64_t> h2(N, 0);
    h2[20] = 3;
    h2[85] = 4;
    std::vector<float> m2 = m;
    for (size_t d = 0; d < D; ++d)
        m2[85 * D + d] = m2[20 * D + d];
    som.setState(m2.data(), s.data(), S.data(), w.data(), h2.data());
    seen = vae_results(som, ds, 1);
    if (seen != std::set<size_t>{20, 85})
        return fail("two identical eligible nodes: not exactly {20, 85}");
    std::cout << "vae_two ok\n";
    // no mass: 0
    som.setState(m.data(), s.data(), S.data(), w.data(), h.data());
    seen = vae_results(som, ds, 1u << 30);
    if (seen != std::set<size_t>{0})
        return fail("no mass: not 0");
    std::cout << "vae_none ok\n";
    std::cout << "host_bmd_test ok\n";
    return 0;
}
