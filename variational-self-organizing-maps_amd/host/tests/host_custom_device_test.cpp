// host_custom_device_test -- a caller's Transformation that is not a built-in, trained twice from the same state:
// once with its hooks as C++ lambdas (the host path, src/vsom_custom.cpp) and once with the same hooks as device
// source (Transformation::Device -> vsom_create_custom).  Every result must be bit-identical.  Needs a GPU.
//   host_custom_device_test           exit 0 and "custom device parity ok" when everything matches
#include "SOM.hpp"
#include "DataSet.hpp"
#include "Transformation.hpp"

#include <cmath>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

using V = Eigen::VectorXf;

// sigma-normalised residual (x - m) / dispersion, Stepper = x - m
static const char *kSource = R"(
__device__ float vsom_compare(uint32_t r, const float *x, const float *model, const float *dispersion,
                              const float *value_weight, uint32_t J, uint32_t D)
{
    return (x[r] - model[r]) / dispersion[r];
}
__device__ float vsom_step(uint32_t d, const float *x, const float *model, const float *value_weight,
                           uint32_t J, uint32_t D)
{
    return x[d] - model[d];
}
)";

static V comparer(const V &x, const V &m, const V &disp, const V &)
{
    V r(m.size());
    for (Eigen::Index i = 0; i < m.size(); ++i)
        r[i] = (x[i] - m[i]) / disp[i];
    return r;
}

static V stepper(const V &x, const V &m, const V &)
{
    V r(m.size());
    for (Eigen::Index i = 0; i < m.size(); ++i)
        r[i] = x[i] - m[i];
    return r;
}

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

static int g_fail = 0;

static bool same(const float *a, const float *b, size_t n)
{
    for (size_t i = 0; i < n; ++i) {
        uint32_t x, y;
        std::memcpy(&x, a + i, 4);
        std::memcpy(&y, b + i, 4);
        if (x != y && !(std::isnan(a[i]) && std::isnan(b[i])))
            return false;
    }
    return true;
}

static void compare(const char *what, Som &host, Som &dev)
{
    const size_t N = host.getWidth() * host.getHeight(), D = host.getDepth();
    std::vector<float> m[2], s[2], S[2], w[2];
    std::vector<uint64_t> h[2];
    Som *soms[2] = {&host, &dev};
    for (int k = 0; k < 2; ++k) {
        m[k].resize(N * D); s[k].resize(N * D); S[k].resize(N * D); w[k].resize(N); h[k].resize(N);
        soms[k]->getState(m[k].data(), s[k].data(), S[k].data(), w[k].data(), h[k].data());
    }
    const auto mh = host.getMetrics().MeanSquaredError, md = dev.getMetrics().MeanSquaredError;
    const bool ok = same(m[0].data(), m[1].data(), N * D) && same(s[0].data(), s[1].data(), N * D) &&
                    same(S[0].data(), S[1].data(), N * D) && same(w[0].data(), w[1].data(), N) && h[0] == h[1] &&
                    mh.size() == md.size() && same(mh.data(), md.data(), mh.size());
    std::cout << what << (ok ? ": identical" : ": DIFFERENT") << "\n";
    if (!ok)
        ++g_fail;
}

int main()
{
    struct Case { size_t W, H, J, rows, chunk; };
    const Case cases[] = {{7, 5, 13, 150, 64}, {4, 6, 3, 40, 40}};
    unsigned seed = 11;
    for (const Case &cs : cases) {
        const auto rows = make_rows(cs.rows, cs.J, seed++);
        const size_t N = cs.W * cs.H;
        const auto init = make_rows(N, cs.J, seed++);
        std::vector<float> sig(N * cs.J);
        for (size_t i = 0; i < sig.size(); ++i)
            sig[i] = 0.25f + 0.5f * std::fabs(init[i]);
        const Transformation onHost{.Comparer = comparer, .Stepper = stepper};
        const Transformation onDevice = Transformation::Device("sigma-normalised", kSource, [](size_t J) { return J; },
                                                               [](size_t J) { return J; }, comparer, stepper);
        for (int mode = 0; mode < 3; ++mode) {
            ArrayDataLoader la(rows.data(), cs.rows, cs.J, cs.chunk), lb(rows.data(), cs.rows, cs.J, cs.chunk);
            DataSet da(la), db(lb);
            Som host(cs.W, cs.H, da, onHost), dev(cs.W, cs.H, db, onDevice);
            if (dev.context() == nullptr) {
                std::cout << "the device transformation did not create a device context\n";
                return 1;
            }
            host.setState(init.data(), sig.data(), nullptr, nullptr, nullptr);
            dev.setState(init.data(), sig.data(), nullptr, nullptr, nullptr);
            std::string what = std::to_string(cs.W) + "x" + std::to_string(cs.H) + "x" + std::to_string(cs.J);
            if (mode == 0) {
                host.trainBatchSom(da, 3, 2.5, 0.2);
                dev.trainBatchSom(db, 3, 2.5, 0.2);
                what += " batch";
            } else {
                const auto fn = mode == 1 ? Som::WeigthDecayFunction::Exponential : Som::WeigthDecayFunction::InverseProportional;
                host.trainBasicSom(da, 3, 0.5, 0.3, 1.6, 0.4, fn);   // sigma 1.6, 1.07, then 1 (the local search)
                dev.trainBasicSom(db, 3, 0.5, 0.3, 1.6, 0.4, fn);
                what += mode == 1 ? " online exponential" : " online inverse-proportional";
            }
            compare(what.c_str(), host, dev);
            V v(cs.J);
            for (size_t j = 0; j < cs.J; ++j)
                v[j] = rows[j];
            const V ones = V::Ones(cs.J);
            if (host.findBmu(v, ones, ones) == dev.findBmu(v, ones, ones) &&
                host.findLocalBmu(v, ones, 0, ones) == dev.findLocalBmu(v, ones, 0, ones) &&
                (float)host.euclidianWeightedDist((size_t)1, v, ones, ones) == (float)dev.euclidianWeightedDist((size_t)1, v, ones, ones))
                std::cout << what << " searches: identical\n";
            else {
                std::cout << what << " searches: DIFFERENT\n";
                ++g_fail;
            }
        }
    }
    if (g_fail) {
        std::cout << g_fail << " mismatches\n";
        return 1;
    }
    std::cout << "custom device parity ok\n";
    return 0;
}
