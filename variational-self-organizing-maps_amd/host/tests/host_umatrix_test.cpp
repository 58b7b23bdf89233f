// host_umatrix_test.cpp -- Som::updateUMatrix of the C++ mirror on the maps host_api_test does not reach: non-square maps
// (W != H in both directions) and a StandardMedianEstimator map, plus a non-square CLR map.  Each map is
// trained, updateUMatrix runs (through vsom_umatrix), and the state and the matrix are written to <outdir>/umatrix_<k>.bin
// (tests/test_gpu_host_umatrix.py holds them against the oracle and the Python binding).  One case trains with
// updateUMatrixAfterEpoch = true and checks that an explicit call afterwards changes nothing.
//   usage: host_umatrix_test <outdir>
#include "SOM.hpp"
#include "vsom_hip.h"
#include "DataSet.hpp"
#include "Transformation.hpp"

#include <cstdint>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

static std::vector<float> make_rows(size_t n, size_t d, unsigned seed)
{
    std::vector<float> r(n * d);
    unsigned s = seed;
    for (auto &v : r) {
        s = s * 1664525u + 1013904223u;
        v = (float)((s >> 8) & 0xFFFF) / 65536.0f + 0.05f;     // positive: CLR takes logarithms of ratios
    }
    return r;
}

static int fail(const std::string &what)
{
    std::cerr << "FAIL: " << what << "\n";
    return 1;
}

struct Case { size_t W, H, J; int kind; bool afterEpoch; };

int main(int argc, char **argv)
{
    if (argc < 2)
        return fail("usage: host_umatrix_test <outdir>");
    const std::string out = argv[1];
    const Case cases[] = {{13, 5, 11, 0, false}, {5, 13, 11, 0, true}, {7, 11, 9, 1, false}, {9, 4, 5, 2, false}};
    const size_t NROWS = 240;
    int k = 0;
    for (const Case &c : cases) {
        auto rows = make_rows(NROWS, c.J, 100u + (unsigned)k);
        ArrayDataLoader loader(rows.data(), NROWS, c.J);
        DataSet ds(loader);
        const Transformation t = c.kind == 0   ? Transformation::Standard(loader.getNames())
                                 : c.kind == 1 ? Transformation::StandardMedianEstimator(loader.getNames())
                                               : Transformation::CombinatorialLinearRegression(loader.getNames());
        Som som{c.W, c.H, ds, t};
        som.randomInitialize(5 + k, 1);
        som.train(ds, 2, 0.0, 0.0, 3.0, 0.2, Som::WeigthDecayFunction::BatchMap, c.afterEpoch);
        if (k == 0)
            std::cout << "group_members=" << (som.group() ? vsom_group_size(som.group()) : 1) << "\n";
        const std::vector<double> trained = som.getUMatrix().getData();
        som.updateUMatrix(Eigen::VectorXf::Ones((Eigen::Index)c.J));
        const std::vector<double> um = som.getUMatrix().getData();
        const size_t N = c.W * c.H, D = som.getDepth();
        if (um.size() != N)
            return fail("matrix size");
        if (c.afterEpoch && std::memcmp(trained.data(), um.data(), N * 8) != 0)
            return fail("the matrix left by train(..., updateUMatrixAfterEpoch) is not that of the final state");
        if (!c.afterEpoch)
            for (double v : trained)
                if (v != 0.0)
                    return fail("a matrix without any updateUMatrix call");
        std::vector<float> m(N * D), s(N * D), S(N * D), w(N);
        std::vector<uint64_t> h(N);
        som.getState(m.data(), s.data(), S.data(), w.data(), h.data());
        std::ofstream f(out + "/umatrix_" + std::to_string(k) + ".bin", std::ios::binary);
        const uint64_t hdr[5] = {c.W, c.H, c.J, (uint64_t)c.kind, D};
        f.write((const char *)hdr, sizeof(hdr));
        f.write((const char *)m.data(), m.size() * 4);
        f.write((const char *)s.data(), s.size() * 4);
        f.write((const char *)um.data(), um.size() * 8);
        ++k;
    }
    std::cout << "cases=" << k << "\n";
    std::cout << "host_umatrix_test ok\n";
    return 0;
}
