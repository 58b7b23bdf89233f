// host_custom_validity_test -- hooks that USE their valueWeight argument, over a loader with NULLs and column weights.
//   host_custom_validity_test host      the hooks as C++ lambdas through a Som (the host path, src/vsom_custom.cpp; the
//                                       state stays on the host: no GPU).  Prints the inputs and every result as hexfloat
//                                       lines "<case>.<name> v v ..." for tests/test_custom_validity_ref.py.
//   host_custom_validity_test device    the same runs twice, as lambdas and as device source (Transformation::Device ->
//                                       vsom_create_custom): batch and online through Som::train, the single-vector
//                                       members, a Som assigned to after weighted use, evaluate.  Everything must be
//                                       bit-identical; exit 0 and
//                                       "custom validity device parity ok".  Needs a GPU.
#include "SOM.hpp"
#include "DataSet.hpp"
#include "Transformation.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

using V = Eigen::VectorXf;

// Comparer = vw .* (model - x) [/ dispersion] over the valid entries, Stepper = x - model over the valid entries
static const char *kSelect = R"(
__device__ float vsom_compare(uint32_t r, const float *x, const float *model, const float *dispersion,
                              const float *value_weight, uint32_t J, uint32_t D)
{
    return value_weight[r] != 0.f ? value_weight[r] * (model[r] - x[r]) : 0.f;
}
__device__ float vsom_step(uint32_t d, const float *x, const float *model, const float *value_weight,
                           uint32_t J, uint32_t D)
{
    return value_weight[d] != 0.f ? x[d] - model[d] : 0.f;
}
)";
static const char *kScaled = R"(
__device__ float vsom_compare(uint32_t r, const float *x, const float *model, const float *dispersion,
                              const float *value_weight, uint32_t J, uint32_t D)
{
    return value_weight[r] != 0.f ? (value_weight[r] * (model[r] - x[r])) / dispersion[r] : 0.f;
}
__device__ float vsom_step(uint32_t d, const float *x, const float *model, const float *value_weight,
                           uint32_t J, uint32_t D)
{
    return value_weight[d] != 0.f ? x[d] - model[d] : 0.f;
}
)";

static V vec(const float *p, size_t n)
{
    V v((Eigen::Index)n);
    std::memcpy(v.data(), p, n * sizeof(float));
    return v;
}

template <bool Scaled>
static V comparer(const V &x, const V &m, const V &disp, const V &vw)
{
    V r(m.size());
    for (Eigen::Index i = 0; i < m.size(); ++i) {
        float t = vw[i] * (m[i] - x[i]);
        if (Scaled)
            t = t / disp[i];
        r[i] = vw[i] != 0.f ? t : 0.f;
    }
    return r;
}

static V stepper(const V &x, const V &m, const V &vw)
{
    V r(m.size());
    for (Eigen::Index i = 0; i < m.size(); ++i)
        r[i] = vw[i] != 0.f ? x[i] - m[i] : 0.f;
    return r;
}

// rows with NULLs (valid = 0, the value is whatever the loader left there) and column weights, in chunks; the stream
// wraps to its start after the last chunk
class NullLoader : public IDataLoader {
public:
    NullLoader(std::vector<float> rows, std::vector<int> valid, std::vector<float> weights, size_t chunk)
        : IDataLoader(chunk), m_rows(std::move(rows)), m_valid(std::move(valid)), m_weights(std::move(weights)),
          m_J(m_weights.size()), m_n(m_rows.size() / m_weights.size()), m_binary(m_J, 0), m_continuous(m_J, 1)
    {
        m_continuous[0] = 0;      // (evaluate searches with validity * continuous)
    }
    size_t load() override
    {
        data.clear();
        const size_t end = std::min(m_n, m_currentIndex + *m_maxLoadCount);
        for (size_t i = m_currentIndex; i < end; ++i) {
            RowData r;
            r.values = vec(m_rows.data() + i * m_J, m_J);
            r.valid.assign(m_valid.begin() + i * m_J, m_valid.begin() + (i + 1) * m_J);
            data.push_back(r);
        }
        const size_t got = end - m_currentIndex;
        m_currentIndex = end == m_n ? 0 : end;
        return got;
    }
    std::vector<RowData> getPreview(size_t) override { return {}; }
    bool open(const char *) override { return true; }
    std::vector<std::string> findAllColumns() override { return getNames(); }
    void setColumnSpec(const std::vector<ColumnSpec>) noexcept override {}
    const std::vector<ColumnSpec> getColumnSpec() noexcept override { return {}; }
    float getWeight(size_t i) override { return m_weights[i]; }
    const std::vector<float> getWeights() const noexcept override { return m_weights; }
    const std::vector<int> &getBinary() const noexcept override { return m_binary; }
    const std::vector<int> &getContinuous() const noexcept override { return m_continuous; }
    std::string getName(size_t i) const noexcept override { return "c" + std::to_string(i); }
    const std::vector<std::string> getNames() const noexcept override
    {
        std::vector<std::string> n;
        for (size_t i = 0; i < m_J; ++i)
            n.push_back(getName(i));
        return n;
    }
    size_t getDepth() const noexcept override { return m_J; }
    bool isAtStartOfDataStream() const noexcept override { return m_currentIndex == 0; }

private:
    std::vector<float> m_rows;
    std::vector<int> m_valid;
    std::vector<float> m_weights;
    size_t m_J, m_n;
    std::vector<int> m_binary, m_continuous;
};

static unsigned g_seed = 1;
static float uniform()
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)((g_seed >> 8) & 0xFFFF) / 65536.0f;
}

struct Inputs {
    size_t W, H, J, rows, chunk;
    std::vector<float> x, weights, init, sig;
    std::vector<int> valid;
};

static Inputs make_inputs(size_t W, size_t H, size_t J, size_t rows, size_t chunk, unsigned seed)
{
    Inputs in{W, H, J, rows, chunk, {}, {}, {}, {}, {}};
    g_seed = seed;
    in.x.resize(rows * J);
    in.valid.resize(rows * J);
    for (size_t i = 0; i < rows * J; ++i) {
        in.x[i] = uniform() * 2.f - 1.f;
        in.valid[i] = uniform() >= 0.2f;                // about 20 % NULLs
        if (i / J == 3 || i % J == J - 2)               // one row with no valid field, one column that is always NULL
            in.valid[i] = 0;
        if (!in.valid[i])
            in.x[i] = 7.f;                              // (what a loader leaves at a NULL must not matter)
    }
    in.weights.assign(J, 1.f);
    in.weights[1] = 0.f;
    in.weights[2] = 2.5f;
    in.weights[J - 1] = 0.5f;
    in.init.resize(W * H * J);
    in.sig.resize(W * H * J);
    for (size_t i = 0; i < W * H * J; ++i) {
        in.init[i] = uniform() * 2.f - 1.f;
        in.sig[i] = i % 3 == 0 ? 0.f : 0.25f + 0.5f * uniform();   // zeros: the 1e-5 floor of the distance
    }
    return in;
}

static void dump(const std::string &name, const float *p, size_t n)
{
    std::printf("%s", name.c_str());
    for (size_t i = 0; i < n; ++i)
        std::printf(" %a", (double)p[i]);
    std::printf("\n");
}

static void dump(const std::string &name, const std::vector<uint64_t> &v)
{
    std::printf("%s", name.c_str());
    for (uint64_t x : v)
        std::printf(" %llu", (unsigned long long)x);
    std::printf("\n");
}

// everything a run leaves behind
struct Result {
    std::vector<float> map, sigma, S, weight, mse, singles;
    std::vector<uint64_t> hits, last;
};

static bool same(const std::vector<float> &a, const std::vector<float> &b)
{
    if (a.size() != b.size())
        return false;
    for (size_t i = 0; i < a.size(); ++i) {
        uint32_t x, y;
        std::memcpy(&x, &a[i], 4);
        std::memcpy(&y, &b[i], 4);
        if (x != y && !(std::isnan(a[i]) && std::isnan(b[i])))
            return false;
    }
    return true;
}

static bool same(const Result &a, const Result &b)
{
    return same(a.map, b.map) && same(a.sigma, b.sigma) && same(a.S, b.S) && same(a.weight, b.weight) && same(a.mse, b.mse) &&
           same(a.singles, b.singles) && a.hits == b.hits && a.last == b.last;
}

// Reassign: a Som that has used the weights is assigned another Som's map (its context is replaced) and trains on with
// the same weights; then evaluate(), whose search hands the hooks validity * continuous and the data set's weights
enum Mode { Batch, OnlineExp, OnlineInv, Singles, Reassign, ModeCount };
static const char *kModeName[] = {"batch", "exp", "inv", "singles", "reassign"};

static Result run(const Inputs &in, const Transformation &t, Mode mode, bool wantDevice)
{
    NullLoader loader(in.x, in.valid, in.weights, in.chunk);
    DataSet data(loader);
    Som som(in.W, in.H, data, t);
    if (wantDevice != (som.context() != nullptr))
        throw std::runtime_error(wantDevice ? "the device transformation did not create a device context"
                                            : "the host transformation created a device context");
    som.setState(in.init.data(), in.sig.data(), nullptr, nullptr, nullptr);
    Result r;
    const size_t N = in.W * in.H, J = in.J;
    std::unique_ptr<Som> second;
    Som *out = &som;              // the Som whose state is the run's result
    if (mode == Reassign) {
        const V w = vec(in.weights.data(), J), v = vec(in.x.data(), J), ones = V::Ones((Eigen::Index)J);
        som.train(data, 1, 0.0, 0.0, 2.0, 0.3, Som::WeigthDecayFunction::BatchMap);
        second = std::make_unique<Som>(in.W, in.H, data, t);
        Som &other = *second;
        const SomIndex before = other.findBmu(v, ones, w);         // `other` has the weights ...
        r.singles.push_back((float)(before.getY() * in.W + before.getX()));
        other = som;                                               // ... gets a new context with som's map ...
        const SomIndex after = other.findBmu(v, ones, w);          // ... and must use the same weights again
        r.singles.push_back((float)(after.getY() * in.W + after.getX()));
        r.singles.push_back((float)other.euclidianWeightedDist((size_t)1, v, ones, w));
        other.train(data, 1, 0.5, 0.3, 1.6, 0.6, Som::WeigthDecayFunction::Exponential);
        r.singles.push_back((float)other.evaluate(data));
        const V unit = V::Ones((Eigen::Index)J);
        (void)other.findBmu(v, ones, unit);                         // evaluate after other weights were in use
        r.singles.push_back((float)other.evaluate(data));
        out = second.get();
    } else if (mode == Batch)
        som.train(data, 2, 0.0, 0.0, 2.0, 0.3, Som::WeigthDecayFunction::BatchMap);               // sigma 2, 1.48
    else if (mode == OnlineExp || mode == OnlineInv)
        som.train(data, 2, 0.5, 0.3, 1.6, 0.6,                                                    // sigma 1.6, then 1 (local)
                  mode == OnlineExp ? Som::WeigthDecayFunction::Exponential : Som::WeigthDecayFunction::InverseProportional);
    else {
        const V w = vec(in.weights.data(), J);
        size_t last = 0;
        for (size_t s = 0; s < 6; ++s) {
            V v = vec(in.x.data() + s * J, J), valid((Eigen::Index)J);
            for (size_t d = 0; d < J; ++d)
                valid[(Eigen::Index)d] = (float)in.valid[s * J + d];
            const SomIndex f = som.findBmu(v, valid, w), l = som.findLocalBmu(v, valid, 2, w);
            r.singles.push_back((float)(f.getY() * in.W + f.getX()));
            r.singles.push_back((float)(l.getY() * in.W + l.getX()));
            r.singles.push_back((float)som.euclidianWeightedDist((size_t)(s + 1), v, valid, w));
            const auto tr = som.trainSingle(v, valid, w, 0.4, s % 2 ? 0.9 : 1.7, last,
                                            s < 3 ? Som::WeigthDecayFunction::Exponential : Som::WeigthDecayFunction::InverseProportional);
            r.singles.push_back((float)(tr.bmu.getY() * in.W + tr.bmu.getX()));
            r.singles.push_back(tr.distanceError);
            for (Eigen::Index d = 0; d < tr.residual.size(); ++d)
                r.singles.push_back(tr.residual[d]);
        }
        r.last.push_back(last);
    }
    r.map.resize(N * J); r.sigma.resize(N * J); r.S.resize(N * J); r.weight.resize(N); r.hits.resize(N);
    out->getState(r.map.data(), r.sigma.data(), r.S.data(), r.weight.data(), r.hits.data());
    if (mode != Singles) {
        r.mse = out->getMetrics().MeanSquaredError;
        for (size_t s = 0; s < data.size(); ++s)
            r.last.push_back(data.getLastBMU(s));
    }
    return r;
}

int main(int argc, char **argv)
{
    const std::string what = argc > 1 ? argv[1] : "";
    if (what != "host" && what != "device") {
        std::cerr << "usage: host_custom_validity_test host|device\n";
        return 2;
    }
    struct Hook { const char *name, *source; V (*cmp)(const V &, const V &, const V &, const V &); };
    const Hook hooks[] = {{"select", kSelect, comparer<false>}, {"scaled", kScaled, comparer<true>}};
    const Inputs inputs[] = {make_inputs(5, 4, 6, 23, 12, 7), make_inputs(4, 6, 9, 20, 20, 19)};
    int fail = 0;
    for (size_t k = 0; k < 2; ++k) {
        const Inputs &in = inputs[k];
        if (what == "host") {
            const std::string c = "in" + std::to_string(k);
            const float shape[] = {(float)in.W, (float)in.H, (float)in.J, (float)in.rows, (float)in.chunk};
            dump(c + ".shape", shape, 5);
            dump(c + ".x", in.x.data(), in.x.size());
            std::vector<float> vf(in.valid.begin(), in.valid.end());
            dump(c + ".valid", vf.data(), vf.size());
            dump(c + ".weights", in.weights.data(), in.weights.size());
            dump(c + ".init", in.init.data(), in.init.size());
            dump(c + ".sig", in.sig.data(), in.sig.size());
        }
        for (const Hook &h : hooks)
            for (int m = 0; m < ModeCount; ++m) {
                const std::string c = "in" + std::to_string(k) + "." + h.name + "." + kModeName[m];
                std::cout.setstate(std::ios::failbit);      // (the training members narrate their epochs)
                const Transformation onHost{.Comparer = h.cmp, .Stepper = stepper};
                const Result a = run(in, onHost, (Mode)m, false);
                if (what == "host") {
                    std::cout.clear();
                    dump(c + ".map", a.map.data(), a.map.size());
                    dump(c + ".sigma", a.sigma.data(), a.sigma.size());
                    dump(c + ".S", a.S.data(), a.S.size());
                    dump(c + ".weight", a.weight.data(), a.weight.size());
                    dump(c + ".mse", a.mse.data(), a.mse.size());
                    dump(c + ".singles", a.singles.data(), a.singles.size());
                    dump(c + ".hits", a.hits);
                    dump(c + ".last", a.last);
                    continue;
                }
                const Transformation onDevice = Transformation::Device(h.name, h.source, [](size_t J) { return J; },
                                                                       [](size_t J) { return J; }, h.cmp, stepper);
                const Result b = run(in, onDevice, (Mode)m, true);
                std::cout.clear();
                const bool ok = same(a, b);
                std::cout << c << (ok ? ": identical" : ": DIFFERENT") << "\n";
                fail += !ok;
            }
    }
    if (what == "device") {
        if (fail) {
            std::cout << fail << " mismatches\n";
            return 1;
        }
        std::cout << "custom validity device parity ok\n";
    }
    return 0;
}
