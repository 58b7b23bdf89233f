// vsom_api.hpp -- host-side C++ interface of the MI355X VSOM build.
//
// One header declares the types a caller of the reference's libsom uses on the training hot path
// (ColumnSpec, RowData, IDataLoader, DataSet, SomIndex, UMatrix, Transformation, Som), with the
// reference's names, member signatures and error behaviour, so that code written against
// include/SOM.hpp & co. recompiles against this build.  The small headers SOM.hpp,
// Transformation.hpp, DataSet.hpp, IDataLoader.hpp, SomIndex.hpp, UMatrix.hpp, ColumnSpec.hpp next
// to this file only forward to it.  Every hot-path member of Som is a thin call into the C ABI of
// libvsom_hip.so (include/vsom_hip.h); nothing here computes training arithmetic on the CPU.
#pragma once
#include "vsom_dense.hpp"
#include <cstdint>

// ===== ColumnSpec ============================================================================
// Mirror of the reference's include/ColumnSpec.hpp:5-16 (loader-side value type).
#include <string>

struct ColumnSpec {
    ColumnSpec(const std::string name, const float weight, const int isBinary)
        : name{name}, weight{weight}, isBinary{isBinary} {}
    const std::string name;
    const float weight;
    const int isBinary;
};

// ===== IDataLoader ===========================================================================
// Mirror of the reference's include/IDataLoader.hpp:11-48 (abstract chunked loader).  The SQLite
// and MNIST loaders of the reference are out of scope; ArrayDataLoader is the in-memory loader the
// tests and examples use.

#include <optional>
#include <string>
#include <vector>

struct RowData {
    Eigen::VectorXf values;
    std::vector<int> valid;
};

class IDataLoader {
public:
    virtual ~IDataLoader() = default;
    IDataLoader(std::optional<size_t> maxLoadCount = std::nullopt)
        : m_maxLoadCount{maxLoadCount}, m_currentIndex{0} {}
    virtual size_t load() = 0;
    virtual std::vector<RowData> getPreview(size_t count) = 0;
    virtual bool open(const char *path) = 0;
    virtual std::vector<std::string> findAllColumns() = 0;
    std::vector<RowData> data;

    virtual void setColumnSpec(const std::vector<ColumnSpec> columnSpec) noexcept = 0;
    virtual const std::vector<ColumnSpec> getColumnSpec() noexcept = 0;
    virtual float getWeight(size_t index) = 0;
    virtual const std::vector<float> getWeights() const noexcept = 0;
    virtual const std::vector<int> &getBinary() const noexcept = 0;
    virtual const std::vector<int> &getContinuous() const noexcept = 0;
    virtual std::string getName(size_t index) const noexcept = 0;
    virtual const std::vector<std::string> getNames() const noexcept = 0;
    virtual size_t getDepth() const noexcept = 0;
    virtual bool isAtStartOfDataStream() const noexcept = 0;

    // [MI355X build] optional fast path of DataSet::loadNextDataFromStream (the step right before the hot path:
    // the reference reloads every chunk every epoch, Som.cpp:737,1157).  peekFlat: this loader can write a chunk
    // straight into a caller's buffer, and `rows` is what the NEXT load() would return.  loadFlat: write those rows
    // (row-major, getDepth() floats each; every value valid) into dst, advance the stream exactly as load() does and
    // leave `data` empty.  A loader that overrides neither keeps the reference's contract: load() fills `data`.
    virtual bool peekFlat(size_t &rows) { (void)rows; return false; }
    virtual size_t loadFlat(float *dst, size_t rows) { (void)dst; (void)rows; return 0; }

protected:
    std::optional<size_t> m_maxLoadCount;
    size_t m_currentIndex;
};

// In-memory loader: rows x depth floats, load() yields the next <= maxLoadCount rows and wraps
// to the start after the last chunk (the streaming contract of SqliteDataLoader.cpp:465-479).
class ArrayDataLoader : public IDataLoader {
public:
    ArrayDataLoader(const float *rows, size_t nrows, size_t depth,
                    std::optional<size_t> maxLoadCount = std::nullopt);
    size_t load() override;
    bool peekFlat(size_t &rows) override;
    size_t loadFlat(float *dst, size_t rows) override;
    std::vector<RowData> getPreview(size_t count) override;
    bool open(const char *) override { return true; }
    std::vector<std::string> findAllColumns() override { return getNames(); }
    void setColumnSpec(const std::vector<ColumnSpec> columnSpec) noexcept override;
    const std::vector<ColumnSpec> getColumnSpec() noexcept override;
    float getWeight(size_t index) override { return m_weights[index]; }
    const std::vector<float> getWeights() const noexcept override { return m_weights; }
    const std::vector<int> &getBinary() const noexcept override { return m_binary; }
    const std::vector<int> &getContinuous() const noexcept override { return m_continuous; }
    std::string getName(size_t index) const noexcept override { return m_names[index]; }
    const std::vector<std::string> getNames() const noexcept override { return m_names; }
    size_t getDepth() const noexcept override { return m_depth; }
    bool isAtStartOfDataStream() const noexcept override { return m_currentIndex == 0; }

private:
    std::vector<float> m_rows;
    size_t m_nrows, m_depth;
    std::vector<float> m_weights;
    std::vector<int> m_binary, m_continuous;
    std::vector<std::string> m_names;
};

// ----- MnistDataLoader -------------------------------------------------------------------------
// Mirror of the reference's include/MnistDataLoader.hpp:9-51 / src/MnistDataLoader.cpp:9-134.
// open(folder) remembers the folder; load() reads the next <= maxLoadCount images of
// `folder/train-images-idx3-ubyte` + `train-labels-idx1-ubyte` (IDX, big-endian headers, magic
// 0x803 / 0x801): 784 raw pixel values 0..255 as float followed by the one-hot label (10 values),
// depth 794, valid = 1 (MnistDataLoader.cpp:61-81).  The stream position advances by the rows read
// and returns to 0 after an empty read or a read of >= 60000 rows (:53-55).  Own IDX parser (the
// reference delegates to extern/mnistReader).
class MnistDataLoader : public IDataLoader {
public:
    MnistDataLoader(std::optional<size_t> maxLoadCount = std::nullopt, bool verbose = false);
    size_t load() override;
    bool peekFlat(size_t &rows) override;
    size_t loadFlat(float *dst, size_t rows) override;
    std::vector<RowData> getPreview(size_t count) override;
    bool open(const char *path) override;
    std::vector<std::string> findAllColumns() override { return _names; }
    void setColumnSpec(const std::vector<ColumnSpec>) noexcept override {}
    const std::vector<ColumnSpec> getColumnSpec() noexcept override;
    float getWeight(size_t index) override { return _weights.at(index); }
    const std::vector<float> getWeights() const noexcept override { return _weights; }
    const std::vector<int> &getBinary() const noexcept override { return _isBinary; }
    const std::vector<int> &getContinuous() const noexcept override { return _isContinuous; }
    std::string getName(size_t index) const noexcept override { return _names.at(index); }
    const std::vector<std::string> getNames() const noexcept override { return _names; }
    size_t getDepth() const noexcept override { return _names.size(); }
    bool isAtStartOfDataStream() const noexcept override { return m_currentIndex == 0; }

protected:
    std::vector<float> _weights;
    std::vector<int> _isBinary, _isContinuous;
    std::vector<std::string> _names;
    std::string _filePath;
    bool _verbose;
    mutable std::vector<unsigned char> _img, _lab;   // file bytes, kept between loads
    std::vector<RowData> readRows(size_t skip, size_t limit) const;
    size_t rowsAvailable(size_t skip, size_t limit) const;     // rows readRows(skip, limit) would return
    void convertRows(size_t skip, size_t nrows, float *flat, std::vector<RowData> *rows) const;
};

// ----- SqliteDataLoader ------------------------------------------------------------------------
// Mirror of the reference's include/SqliteDataLoader.hpp:11-103 / src/SqliteDataLoader.cpp for the
// calls the training drivers and tests/performance/perf_tests.cpp:77-84 make: open, setTable,
// setColumnSpec / column-spec file, findAllTables, findAllColumns, load (Id-range chunk query
// `SELECT <cols>,Id FROM <table> WHERE Id>=? AND Id<=?`, SqliteDataLoader.cpp:481-548), getPreview.
// The SQLite C library is bound at run time (dlopen of libsqlite3.so.0): the build image has the
// shared object but no header, and the reference's vendored extern/sqlite/sqlite3.c is absent.
struct sqlite3;
class SqliteDataLoader : public IDataLoader {
public:
    SqliteDataLoader(const std::string &specFilePath, std::optional<size_t> maxLoadCount = std::nullopt,
                     bool verbose = false);
    SqliteDataLoader(bool db, const std::string &dbPath, std::optional<size_t> maxLoadCount = std::nullopt);
    ~SqliteDataLoader() override;
    SqliteDataLoader(const SqliteDataLoader &) = delete;
    SqliteDataLoader &operator=(const SqliteDataLoader &) = delete;
    void setTable(const std::string &name) noexcept { _tableName = name; }
    void setColumnSpec(const std::vector<ColumnSpec> columnSpec) noexcept override;
    const std::vector<ColumnSpec> getColumnSpec() noexcept override { return _columnSpec; }
    size_t load() override;
    std::vector<RowData> getPreview(size_t count) override;
    bool open(const char *dbPath) override;
    bool open() { return open(_dbPath.c_str()); }
    std::vector<std::string> findAllColumns() override;
    std::vector<std::string> findAllTables();
    const std::vector<float> getWeights() const noexcept override;
    float getWeight(size_t index) override { return _columnSpec.at(index).weight; }
    const std::vector<int> &getBinary() const noexcept override { return _isBinary; }
    const std::vector<int> &getContinuous() const noexcept override { return _isContinuous; }
    std::string getName(size_t index) const noexcept override { return _columnSpec.at(index).name; }
    const std::vector<std::string> getNames() const noexcept override;
    size_t getDepth() const noexcept override { return vectorLength; }
    bool isAtStartOfDataStream() const noexcept override { return !currentLoadId.has_value(); }

protected:
    std::vector<ColumnSpec> _columnSpec;
    std::vector<std::string> _tableNames, _columnNames;
    std::vector<int> _isBinary, _isContinuous;
    std::string _tableName, _dbPath;
    sqlite3 *db = nullptr;
    bool _verbose = false, hasOpenDatabase = false;
    size_t vectorLength = 0;
    std::optional<long long> currentLoadId;
    void loadColumnSpecData(const std::string &path);
    std::vector<std::string> queryStrings(const std::string &sql);
    long long queryInteger(const std::string &sql);
    // rows with Id in [startId or MIN(Id), ...], at most maxCount ids wide; returns {rows, next id, MAX(Id)}
    struct Fetch { std::vector<RowData> rows; std::optional<long long> nextId; long long maxId; };
    Fetch fetch(std::optional<long long> startId, std::optional<size_t> maxCount);
};

// ===== DataSet ===============================================================================
// Mirror of the reference's include/DataSet.hpp:10-62 (chunk container consumed by the hot path).

#include <string>
#include <vector>

class DataSet {
protected:
    struct DataRow {
        Eigen::VectorXf *data;
        std::vector<int> *valid;
        size_t *lastBMU;
    };
    // [MI355X build] built lazily by ensureRows() (hence mutable): see vsom_host.cpp
    mutable std::vector<DataRow> allData;
    mutable std::vector<Eigen::VectorXf> data;
    mutable std::vector<std::vector<int>> valid;
    std::vector<size_t> index;
    mutable std::vector<size_t> lastBMU;
    IDataLoader &_loader;
    size_t depth, n, loadedNumberOfChunks;
    bool _verbose;

public:
    DataSet(IDataLoader &dataLoader, bool verbose = false)
        : _loader{dataLoader}, depth{}, n{}, loadedNumberOfChunks{0}, _verbose{verbose} {}
    ~DataSet() = default;   // (copyable like the reference's: see the copy constructor below)
    const std::vector<DataRow> getAll() const;
    std::vector<DataRow> getAll();
    std::vector<Eigen::VectorXf> getPreviewData(size_t count) const;
    Eigen::VectorXf getData(size_t index) const;
    const Eigen::VectorXi getValidity(size_t index) const;
    const Eigen::ArrayXi getBinary() const;
    const Eigen::ArrayXi getContinuous() const;
    const Eigen::VectorXf getWeights() const;
    float getWeight(size_t index);
    const std::vector<std::string> getNames() const noexcept;
    std::string getName(size_t) const;
    const std::vector<size_t> &getLastBMU() const noexcept;
    size_t &getLastBMU(size_t);
    size_t size() const;
    void addVector(Eigen::VectorXf);
    void display() const;
    void loadNextDataFromStream();
    size_t vectorLength() const;
    bool hasReadWholeDataStream() const noexcept;
    void resetStreamLoadPosition() noexcept;
    void shuffle();

    // [MI355X build] contiguous B x depth row-major copy of the current chunk in PINNED host memory
    // (two buffers used alternately, so the asynchronous host->device copy of one chunk can still be
    // running while the next chunk is being loaded into the other)
    const float *contiguous() const noexcept { return m_flat[m_cur].p; }
    DataSet(const DataSet &other);
    DataSet &operator=(const DataSet &) = delete;

private:
    struct Pinned {
        float *p = nullptr;
        size_t cap = 0;
        bool pinned = false;
        Pinned() = default;
        Pinned(const Pinned &) = delete;
        Pinned &operator=(const Pinned &) = delete;
        ~Pinned();
        void reserve(size_t n);
    };
    Pinned m_flat[2];
    int m_cur = 0;
    mutable bool m_rowsBuilt = true;
    bool m_fromFlat = false;      // the current chunk came through IDataLoader::loadFlat (the loader's `data` is empty)
    void ensureRows() const;
};

// ===== SomIndex ==============================================================================
// Mirror of the reference's include/SomIndex.hpp:7-27.
#include <stddef.h>

class Som;

class SomIndex {
protected:
    size_t x, y;

public:
    SomIndex(size_t x = 0, size_t y = 0) noexcept;
    SomIndex(const Som &map, size_t index) noexcept;   // y = (index - index % W) / H  (SomIndex.cpp:13-18)
    ~SomIndex() = default;
    size_t getSomIndex(const Som &som);
    size_t getX() const noexcept;
    size_t getY() const noexcept;
    void setX(size_t index) noexcept;
    void setY(size_t index) noexcept;
    bool operator==(const SomIndex &other) const { return x == other.x && y == other.y; }
};

// ===== UMatrix ===============================================================================
// Mirror of the reference's include/UMatrix.hpp:6-23 (value type; the U-matrix computation itself
// is outside the hot path).
#include <vector>

class UMatrix {
private:
    std::vector<double> data;
    size_t width, height;

public:
    UMatrix(std::vector<double> Data, size_t Width, size_t Height) : data{Data}, width{Width}, height{Height} {}
    double getValueAtIndex(size_t Width, size_t Height) const { return data[Height * width + Width]; }
    double getValueAtIndex(SomIndex Index) const { return data[Index.getY() * width + Index.getX()]; }
    const std::vector<double> &getData() const noexcept { return data; }
    size_t getWidth() const noexcept { return width; }
    size_t getHeight() const noexcept { return height; }
};

// ===== Transformation ========================================================================
// Mirror of the reference's include/Transformation.hpp:10-41: same public members, same three
// factories, aggregate-initialisable with designated initialisers (tests/test1.cpp:56-84).
//
// [MI355X build] the std::function hooks cannot run on the device.  The three built-in
// transformations are recognised by the *type* of the callable stored in Comparer/Stepper
// (vsom::*Comparer / vsom::*Stepper below) and run as HIP kernels -- they have no host training path.
// Any other callable (a caller's own lambdas, tests/test1.cpp:56-84) makes the Som keep its state on the
// host and run distance / search / batch epoch / online step there with the caller's hooks
// (src/vsom_custom.cpp).  A custom Transformation that also carries its hooks as device source (DeviceSource,
// Transformation::Device) trains on the GPU instead (vsom_create_custom, csrc/vsom_custom.hip).  The
// built-in functors also work on the host, so code that calls transform.Comparer(...) directly keeps working.

#include <functional>
#include <sstream>
#include <string>
#include <vector>

namespace vsom {
using T = Eigen::VectorXf;
struct StandardComparer { T operator()(const T &value, const T &model, const T &dispersion, const T &valueWeight) const; };
struct StandardStepper { T operator()(const T &value, const T &model, const T &valueWeight) const; };
struct MedianStepper { T operator()(const T &value, const T &model, const T &valueWeight) const; };
struct ClrComparer { T operator()(const T &value, const T &model, const T &dispersion, const T &valueWeight) const; };
struct ClrStepper { T operator()(const T &value, const T &model, const T &valueWeight) const; };
struct IdentityLength { size_t operator()(size_t vectorLength) const { return vectorLength; } };
struct ClrLength { size_t operator()(size_t vectorLength) const { return vectorLength * (vectorLength - 1u); } };
enum Kind { Standard = 0, Median = 1, Clr = 2, Custom = -1 };
}   // namespace vsom

struct Transformation {
    using T = Eigen::VectorXf;
    std::function<T(const T &value, const T &model, const T &dispersion, const T &valueWeight)> Comparer{vsom::StandardComparer{}};
    std::function<T(const T &value, const T &model, const T &valueWeight)> Stepper{vsom::StandardStepper{}};
    std::vector<std::string> names{};
    std::function<std::vector<std::string>(const T &model)> Displayer{[&names = names](const T &) { return names; }};
    std::function<size_t(size_t vectorLength)> Length{vsom::IdentityLength{}};
    std::string Name{"Standard transformation"};
    // [MI355X build] the caller's hooks as HIP device source (include/vsom_hip.h, vsom_create_custom: vsom_compare /
    // vsom_step per output element).  Non-empty on a Custom transformation: the Som compiles it with hipRTC and trains
    // on the device; empty: the host path of src/vsom_custom.cpp.  Comparer / Stepper stay the host hooks for direct calls.
    // The device hooks get the valueWeight the host hooks get: the Som sets the loaded chunk's validity
    // (DataSet::getValidity) and the loader's column weights (DataSet::getWeights) on the context after every chunk it
    // uploads, and findBmu / findLocalBmu / euclidianWeightedDist / trainSingle pass their valid and weights along.
    std::string DeviceSource{};
    // residual length of DeviceSource's Comparer for a sample length J (empty: Length(J))
    std::function<size_t(size_t vectorLength)> ResidualLength{};

    static Transformation Standard(const std::vector<std::string> &columnNames);
    static Transformation StandardMedianEstimator(const std::vector<std::string> &columnNames);
    static Transformation CombinatorialLinearRegression(const std::vector<std::string> &columnNames);
    // [MI355X build] a custom transformation that trains on the device from `source` (see DeviceSource)
    static Transformation Device(const std::string &name, const std::string &source, std::function<size_t(size_t)> length,
                                 std::function<size_t(size_t)> residualLength,
                                 std::function<T(const T &, const T &, const T &, const T &)> comparer,
                                 std::function<T(const T &, const T &, const T &)> stepper);

    // [MI355X build] which device kernels implement this transformation (vsom::Custom = none)
    int kind() const noexcept;
};

// ===== Som ===================================================================================
// Mirror of `class Som` (reference include/SOM.hpp:39-189).  State lives in HBM inside a vsom_ctx;
// the getters copy it back on demand (they return by value in the reference too).
#include <atomic>
#include <mutex>

#define VERSION 1.00

// argv positions of the reference's CLI (include/SOM.hpp:17-35; apps/main.cpp indexes argv with them)
#define ARG_SETTING 2

#define ARG_DB_FILE 3
#define ARG_SOM_FILE 4

// Training parameters
#define ARG_SOM_HEIGHT 5
#define ARG_SOM_WIDTH 6
#define ARG_SOM_ETA0 7
#define ARG_SOM_ETA_DEC 8
#define ARG_SOM_SIGMA0 9
#define ARG_SOM_SIGMA_DEC 10
#define ARG_SOM_EPOCHS 11
#define ARG_SOM_INIT_SIGMA 12
#define ARG_SOM_WEIGHT_DECAY_FUNCTION 13

// Measuring parameters
#define ARG_ALLOWED_STD_DEV 6
#define ARG_MIN_BMU_HITS 5

#define SIGMA_SWITCH_TO_LOCAL 1

struct vsom_ctx;
struct vsom_group;

class Som {
protected:
    struct TrainingReturnValue {
        SomIndex bmu;
        Eigen::VectorXf residual;
        float distanceError;
    };
    struct Metrics {
        std::vector<float> MeanSquaredError;
        std::vector<float> DistanceError;
        Metrics() : MeanSquaredError{}, DistanceError{} {}
        Metrics(size_t size) : MeanSquaredError(size), DistanceError(size) {}
    };
    Transformation transform;
    Metrics metrics;
    std::vector<double> uMatrix;
    std::atomic<bool> _isTraining;
    size_t height, width, depth;

    void Construct(size_t inWidth, size_t inHeight, size_t inDepth, std::vector<std::string> names);

public:
    enum class WeigthDecayFunction { Exponential, InverseProportional, BatchMap };
    std::mutex metricsMutex;

    Som(size_t width, size_t height, DataSet dataset, Transformation transformation = Transformation{});
    Som(size_t width, size_t height, size_t depth, Transformation transformation = Transformation{});
    Som(const char *filename);
    Som(const Som &som);
    Som &operator=(const Som &other);
    ~Som();

    // ---- training hot path (src/Som.cpp:716-947, 1113-1192) -> libvsom_hip.so ----------------
    void train(DataSet &data, size_t numberOfEpochs, double eta0, double etaDecay, double sigma0,
               double sigmaDecay, WeigthDecayFunction weightDecayFunction, bool updateUMatrixAfterEpoch = false);
    void trainBasicSom(DataSet &data, size_t numberOfEpochs, double eta0, double etaDecay, double sigma0,
                       double sigmaDecay, WeigthDecayFunction weightDecayFunction, bool updateUMatrixAfterEpoch = false);
    void trainBatchSom(DataSet &data, size_t numberOfEpochs, double sigma0, double sigmaDecay,
                       bool updateUMatrixAfterEpoch = false);
    float trainBatchSomEpoch(DataSet &data, double currentSigma, bool isFirst);
    // [MI355X build] extension: trainBatchSomEpoch / trainBatchSom over the VALID entries of the rows only (the data set's
    // validity flags; one vsom_batch_epoch_masked call per chunk, include/vsom_hip.h): a missing field neither attracts the
    // search nor enters the means and sigmas of its column.  The driver is trainBatchSom's: the sigma schedule, the stop at
    // sigma < 1, the chunk loop and the metrics.  With every column valid the result is trainBatchSom's bit for bit.
    // Standard / Median on one device only.
    float trainBatchSomEpochMasked(DataSet &data, double currentSigma, bool isFirst);
    void trainBatchSomMasked(DataSet &data, size_t numberOfEpochs, double sigma0, double sigmaDecay,
                             bool updateUMatrixAfterEpoch = false);
    // [MI355X build] extension: trainBatchSom for a data set that is ONE chunk -- the chunk is uploaded once and the whole
    // sigma schedule (the epochs before the first sigma < 1) runs as one vsom_batch_schedule call (include/vsom_hip.h).  The
    // state, the metrics and the rows' lastBMU are trainBatchSom's bit for bit.  Throws std::invalid_argument before it
    // trains when the first load does not read the whole stream.  One device only.
    void trainBatchSomResident(DataSet &data, size_t numberOfEpochs, double sigma0, double sigmaDecay);
    // [MI355X build] extension: trainBatchSomResident over the VALID entries of the rows only -- one
    // vsom_batch_schedule_masked call with the chunk's validity flags.  The state, the metrics and the rows' lastBMU are
    // trainBatchSomMasked's on the same one-chunk data set bit for bit; the same one-chunk rule.  Standard / Median.
    void trainBatchSomResidentMasked(DataSet &data, size_t numberOfEpochs, double sigma0, double sigmaDecay);
    // [MI355X build] extension: trainBatchSom's driver with ONE batch epoch per pass over the stream -- the chunks of a
    // pass accumulate into one epoch over all rows (vsom_batch_accum_begin / _chunk / _end, include/vsom_hip.h), where
    // trainBatchSom runs an epoch per chunk and ends a pass with the batch map of its last chunk alone.  The same sigma
    // schedule and stop at sigma < 1; MeanSquaredError[i] is the MSE of epoch i over all rows; updateUMatrix runs after
    // the epoch's end.  A DataSet cannot tell how many rows its stream holds, so the stream is read once before the first
    // epoch to count them.  resetBmu = true is the reference's behaviour (a load zeroes lastBMU: the epochs after the
    // first walk from unit 0); with false every row's BMU of the previous epoch starts that row's walk.  Chunk k+1 is
    // loaded and copied while chunk k accumulates.  Standard / Median on one device only.
    void trainBatchSomWhole(DataSet &data, size_t numberOfEpochs, double sigma0, double sigmaDecay,
                            bool updateUMatrixAfterEpoch = false, bool resetBmu = true);
    // [MI355X build] extension: trainBatchSomWhole over the VALID entries of the rows only -- every chunk goes into the epoch
    // with its validity flags (vsom_batch_accum_chunk_masked, include/vsom_hip.h), so that a missing field neither attracts
    // the search nor enters the means and sigmas of its column, and the epoch still covers all rows of the stream (the
    // SqliteDataLoader's case: NULLs and maxLoadCount rows per load).  Driver, metrics and resetBmu are trainBatchSomWhole's.
    void trainBatchSomWholeMasked(DataSet &data, size_t numberOfEpochs, double sigma0, double sigmaDecay,
                                  bool updateUMatrixAfterEpoch = false, bool resetBmu = true);
    // [MI355X build] extension: trainBasicSom over the VALID entries of the rows only (the data set's validity flags; one
    // vsom_train_online_chunk_masked call per chunk, include/vsom_hip.h): a missing field neither attracts the search nor
    // steps its column of the window's nodes.  Schedule, sigma clamp at 1.0, running MSE and metrics are trainBasicSom's;
    // the chunk loop is the plain one (upload, then the blocking call).  With every column valid the result is
    // trainBasicSom's bit for bit.  Standard / Median on one device only.
    void trainBasicSomMasked(DataSet &data, size_t numberOfEpochs, double eta0, double etaDecay, double sigma0,
                             double sigmaDecay, WeigthDecayFunction weightDecayFunction, bool updateUMatrixAfterEpoch = false);
    TrainingReturnValue trainSingle(const Eigen::VectorXf &v, const Eigen::VectorXf &valid,
                                    const Eigen::VectorXf &weights, const double eta, const double sigma,
                                    size_t &lastBMU, const WeigthDecayFunction weightDecayFunction);
    SomIndex findBmu(const Eigen::VectorXf &v) const;
    SomIndex findBmu(const Eigen::VectorXf &v, const Eigen::VectorXf &valid, const Eigen::VectorXf &weights) const;
    SomIndex findLocalBmu(const Eigen::VectorXf &v, const Eigen::VectorXf &valid, const size_t &lastBMUref,
                          const Eigen::VectorXf &weights) const;
    double euclidianWeightedDist(const SomIndex &pos, const Eigen::VectorXf &v, const Eigen::VectorXf &valid,
                                 const Eigen::VectorXf &weights) const;
    double euclidianWeightedDist(const size_t &pos, const Eigen::VectorXf &v, const Eigen::VectorXf &valid,
                                 const Eigen::VectorXf &weights) const;
    double static calculateNeighbourhoodWeight(const size_t &currentX, const size_t &currentY, const size_t &bmuX,
                                               const size_t &bmuY, const double &currentSigma);

    // ---- consumers of the search outside the training loop: distances and
    //      (restricted) BMU searches on the device, scalar post-processing on the host ------------
    double evaluate(const DataSet &dataset) const;
    int measureSimilarity(const DataSet *dataset, int numberOfSigmas, size_t minBmuHits) const;
    int autoEncoder(const DataSet *dataset, size_t minBmuHits) const;
    size_t variationalAutoEncoder(const DataSet *dataset, size_t minBmuHits) const;
    SomIndex findRestrictedBmu(const Eigen::VectorXf &v, const Eigen::VectorXf &valid, const size_t minBmuHits,
                               const Eigen::VectorXf &weights) const;
    std::vector<double> findRestrictedBmd(const Eigen::VectorXf &v, const Eigen::VectorXf &valid, size_t minBmuHits,
                                          const Eigen::VectorXf &weights) const;
    // [MI355X build] extension: one model vector per row of `data`, drawn from the row's findRestrictedBmd distribution
    // with the caller's uniform u[r] in [0,1) (one vsom_bmd_batch call; UINT64_MAX where the row has no mass);
    // *norm (if given) receives every row's normalising mass C.  Built-in transformations on the device only.
    std::vector<uint64_t> drawModelVectors(const DataSet *data, size_t minBmuHits, const std::vector<double> &u,
                                           std::vector<double> *norm = nullptr) const;
    // [MI355X build] extension: the k best matching units of every row of `data`, row-major (rows x k; one
    // vsom_bmu_topk_batch call): entry 0 is findBmu's BMU, the others follow in (distance, index) order; *dist (if given)
    // receives their distances.  1 <= k <= min(64, N).  Built-in transformations on the device only.
    std::vector<uint64_t> findBestMatchingUnits(const DataSet *data, size_t k, std::vector<float> *dist = nullptr) const;
    // [MI355X build] extension: the fraction of rows of `data` whose best and second-best units are not grid neighbours
    // (node n at row n / width, column n % width; an error when max(|d row|, |d column|) != 1, no wrap); the count is
    // summed in row order in double and divided by the row count (0 for no rows).  N >= 2.
    double topographicError(const DataSet *data) const;
    // [MI355X build] extension: findBestMatchingUnits for records with missing fields (the data set's validity flags; one
    // vsom_bmu_topk_masked_batch call, include/vsom_hip.h): the k best matching units of every row over its VALID columns
    // only, among node 0 and the nodes with at least minBmuHits hits; entry 0 is findMaskedBmus' unit.  A row with fewer
    // than k candidates is padded with UINT64_MAX (distance NaN); *count (if given) receives every row's real entries,
    // *dist their distances.  1 <= k <= min(64, N).  Standard / Median on the device only.
    std::vector<uint64_t> findBestMatchingUnitsMasked(const DataSet *data, size_t k, size_t minBmuHits,
                                                      std::vector<float> *dist = nullptr,
                                                      std::vector<uint32_t> *count = nullptr) const;
    // [MI355X build] extension: topographicError over the rows of `data` that have a valid column and a second unit
    // (findBestMatchingUnitsMasked with k = 2); 0 when there are none.  *rowsCounted (if given) receives their number.
    double topographicErrorMasked(const DataSet *data, size_t minBmuHits, size_t *rowsCounted = nullptr) const;
    // [MI355X build] extension: rows x sample length, row-major, in double: every row of `data` with its invalid columns
    // filled from its k findBestMatchingUnitsMasked units, each weighted as the BMD weights it (the same call; NaN at the
    // invalid columns of a row without mass) -- between impute (one unit) and generateRowsMasked (random).
    std::vector<double> imputeBlend(const DataSet *data, size_t k, size_t minBmuHits) const;
    // [MI355X build] extension: the per-row report measureSimilarity computes and throws away, for every row of `data`
    // (one vsom_similarity_batch call, include/vsom_hip.h): the row's restricted BMU and its distance, dmax / first (what
    // the reference's running maximum needs), the anomaly score amax = the largest |x - m| / sM / numberOfSigmas over
    // the valid columns with the column that causes it, the number of valid columns outside m +- sM * numberOfSigmas,
    // and with wantDelta the dense rows x columns matrix.  floor: sM = max(sigma, 1e-5) (what a user wants); otherwise
    // the reference's select as written (a cap at 1e-5).  useValidity: the data set's validity flags decide which columns
    // count (otherwise all do).  Built-in transformations on the device only.
    struct SimilarityRows {
        size_t columns = 0;                       // min(sample length, depth)
        std::vector<uint64_t> bmu;
        std::vector<float> dist, dmax, first, amax;
        std::vector<uint32_t> dmaxCol, amaxCol, outside;
        std::vector<float> delta;                 // rows x columns, empty unless asked for
    };
    SimilarityRows similarityRows(const DataSet *data, int numberOfSigmas, size_t minBmuHits, bool floor = true,
                                  bool useValidity = true, bool wantDelta = false) const;
    // [MI355X build] extension: the best matching unit of every row of `data` over its VALID columns only (the data set's
    // validity flags; one vsom_bmu_masked_batch call, include/vsom_hip.h): Som::findRestrictedBmu on the distance whose
    // residual is +0 at invalid columns, so a missing field no longer counts as a measured zero.  *dist (if given)
    // receives the masked distances.  With every column valid the result is findRestrictedBmu's.  Standard / Median on the
    // device only.
    std::vector<uint64_t> findMaskedBmus(const DataSet *data, size_t minBmuHits, std::vector<float> *dist = nullptr) const;
    // [MI355X build] extension: rows x sample length, row-major: every row of `data` with its invalid columns filled from
    // the model vector of its findMaskedBmus unit (the same call).
    std::vector<float> impute(const DataSet *data, size_t minBmuHits) const;
    // [MI355X build] extension: what evaluate sums, for every row of `data` (one vsom_evaluate_batch call, include/vsom_hip.h):
    // the row's BMU and its distance, bsum = binaryError.dot(binaryError) (Som.cpp:509-514, before the sqrt of :519), the
    // number of terms replaced by -99999 that count, and the running mean `error` evaluate returns.  The data set's
    // getBinary / getContinuous are the column factors, its validity flags the mask.  Built-in transformations on the
    // device only; throws when the data set holds a validity flag outside {0, 1} (the byte mask cannot carry it).
    struct EvaluateRows {
        std::vector<uint64_t> bmu;
        std::vector<float> dist, bsum;
        std::vector<uint32_t> nrepl;
        double error = 0;
    };
    EvaluateRows evaluateRows(const DataSet &data) const;
    // [MI355X build] extensions: similarityRows / measureSimilarity / evaluateRows / evaluate for records with missing fields
    // (one vsom_similarity_masked_batch / vsom_evaluate_masked_batch call, include/vsom_hip.h): every row of `data` is
    // searched over its VALID columns only, as findMaskedBmus, and scored against that unit in those columns -- dmax / first
    // range over the valid columns, delta is 0 at invalid ones, an invalid column's binary error term is +0 -- and nvalid
    // counts the row's valid columns.  The data set's validity flags are the mask (any non-zero flag is valid), its
    // getBinary / getContinuous the column factors.  measureSimilarityMasked takes the reference's sigma select as written
    // and measureSimilarity's finish; evaluateMasked returns the running mean.  Standard / Median on the device only; no
    // state is downloaded.
    struct SimilarityRowsMasked : SimilarityRows {
        std::vector<uint32_t> nvalid;
    };
    struct EvaluateRowsMasked : EvaluateRows {
        std::vector<uint32_t> nvalid;
    };
    SimilarityRowsMasked similarityRowsMasked(const DataSet *data, int numberOfSigmas, size_t minBmuHits, bool floor = true,
                                              bool wantDelta = false) const;
    int measureSimilarityMasked(const DataSet *data, int numberOfSigmas, size_t minBmuHits) const;
    EvaluateRowsMasked evaluateRowsMasked(const DataSet &data, size_t minBmuHits = 0) const;
    double evaluateMasked(const DataSet &data, size_t minBmuHits = 0) const;
    // [MI355X build] extension: autoEncoder's records with the caller's random numbers, for every row of `data` (one
    // vsom_generate_batch call, include/vsom_hip.h): a unit per row drawn with the uniform u[r] in [0,1) from the row's own
    // restricted distribution (perRow) or from that of the LAST row (the reference as written), and every column sampled as
    // log(l / (1 - l)) / 1.6 * sigma + mean around that unit; l is rows x columns, row-major, columns = min(sample length,
    // depth).  A row without mass has unit UINT64_MAX and a record of NaN.  Built-in transformations on the device only.
    struct GeneratedRows {
        std::vector<uint64_t> unit;
        std::vector<double> record;               // rows x columns
        size_t columns = 0;
    };
    GeneratedRows generateRows(const DataSet &data, size_t minBmuHits, const std::vector<double> &u,
                               const std::vector<double> &l, bool perRow = true) const;
    // [MI355X build] extensions: findRestrictedBmd / drawModelVectors / generateRows for records with missing fields (one
    // vsom_bmd_masked_batch / vsom_generate_masked_batch call, include/vsom_hip.h): the distribution over the units is taken
    // over the VALID columns only -- `valid` for the one vector (any non-zero entry is valid), the data set's validity flags
    // for its rows -- so a missing field no longer counts as a measured zero.  generateRowsMasked draws `draws` units per row
    // with the uniforms u[r * draws + k] and samples a record around each, l being rows x draws x sample length; with
    // keepObserved a valid column of the record is the row's own value: sampled (multiple) imputation next to impute.  unit
    // is rows x draws, record rows x draws x columns; a draw without mass has unit UINT64_MAX and a record of NaN.
    // Standard / Median on the device only; no state is downloaded.
    std::vector<double> findRestrictedBmdMasked(const Eigen::VectorXf &v, const Eigen::VectorXf &valid,
                                                size_t minBmuHits = 0) const;
    std::vector<uint64_t> drawModelVectorsMasked(const DataSet *data, size_t minBmuHits, const std::vector<double> &u,
                                                 std::vector<double> *norm = nullptr) const;
    GeneratedRows generateRowsMasked(const DataSet &data, size_t minBmuHits, const std::vector<double> &u,
                                     const std::vector<double> &l, size_t draws = 1, bool keepObserved = true) const;
    // [MI355X build] extension: the same sampling around given units (one vsom_decode_nodes call): units.size() x columns
    std::vector<double> decodeUnits(const std::vector<uint64_t> &units, const std::vector<double> &l) const;
    // the finish of measureSimilarity from such a report: the row the reference reports (Som.cpp:684-690: one running
    // maximum over every delta of every row, compared signed, stored as fabs); 0 when no delta exceeds the start value
    static size_t measureSimilarityRow(const std::vector<float> &first, const std::vector<float> &dmax);
    // how often this Som has downloaded the model state into its host mirror (refreshHost): for tests that a call runs
    // on the device state
    size_t stateDownloads() const noexcept { return nDownloads; }
    double euclidianWeightedDistRaw(const size_t &pos, const Eigen::VectorXf &v, const Eigen::VectorXf &valid,
                                    const Eigen::VectorXf &weights) const;
    void updateUMatrix(const Eigen::VectorXf &weights);

    // ---- accessors / bookkeeping (src/Som.cpp:85-110, 159-281, 977-997, 1189-1206) -------------
    void display() const;
    void displayUMatrix() const;
    UMatrix getUMatrix() const noexcept;
    Eigen::VectorXf getWeigthMap() const noexcept;
    std::vector<size_t> getBmuHits() const noexcept;
    size_t getHeight() const noexcept;
    size_t getWidth() const noexcept;
    size_t getDepth() const noexcept;
    size_t getIndex(SomIndex index) const noexcept;
    Eigen::VectorXf getNeuron(SomIndex index) const noexcept;
    Eigen::VectorXf getNeuron(size_t index) const noexcept;
    Eigen::VectorXf getSigmaNeuron(SomIndex index) const noexcept;
    Eigen::VectorXf getSigmaNeuron(size_t index) const noexcept;
    std::vector<std::string> getNeuronStrings(SomIndex index) const noexcept;
    std::vector<std::string> getSigmaNeuronStrings(SomIndex index) const noexcept;
    float getMaxValueOfFeature(size_t modelVectorIndex) const;
    float getMinValueOfFeature(size_t modelVectorIndex) const;
    float getMaxSigmaOfFeature(size_t modelVectorIndex) const;
    float getMinSigmaOfFeature(size_t modelVectorIndex) const;
    Metrics getMetrics() const noexcept;
    bool isTraining() const noexcept;
    bool isCompatibleWithData(DataSet &data) const noexcept;
    void randomInitialize(int seed, float sigma);
    void addBmu(SomIndex position);
    void save(const char *filename) const;   // Octave text format of the reference (Som.cpp:1209-1294)
    void load(const char *filename);         // that format (Som.cpp:1343-1597), or saveBinary's
    // Som.cpp:1296-1341: sets width / height from the file's "# columns:" / "# rows:" lines and returns a
    // vector of the file's model-vector length (length 1 when the file names none).  [MI355X build] when
    // the dimensions change, the device state is rebuilt zeroed at the new size (the reference leaves its
    // `map` vectors at the old size, which the next access overruns).
    Eigen::VectorXf getSizeFromFile(const char *filename);
    void saveBinary(const char *filename) const;   // [MI355X build] lossless, incl. SMap

    // ---- [MI355X build] bulk state access (row-major N x depth) and device selection -----------
    void setState(const float *map, const float *sigma, const float *S, const float *weight, const uint64_t *hits);
    void getState(float *map, float *sigma, float *S, float *weight, uint64_t *hits) const;
    static void setDefaultDevice(int device);
    // devices the batch-map training runs on (opt-in; default: the default device alone): {} = the list in
    // VSOM_DEVICES or the default device, one entry = single GPU, several = sample/node-sharded epochs through
    // vsom_group_* (vsom_host.cpp, training_devices)
    static void setDevices(const std::vector<int> &devices);
    // arithmetic of the Standard update chains of Soms created afterwards: false = strict, bit-identical to
    // the reference (default); true = contracted (fused multiply-adds, results within 1e-5: vsom_hip.h)
    static void setContractedArithmetic(bool on);
    // any vsom_update_mode of include/vsom_hip.h (0 strict, 1 contracted, 2 only the sigma^2 accumulation
    // contracted: map and BMUs stay bit-identical over whole schedules)
    static void setUpdateArithmetic(int mode);
    vsom_ctx *context() const noexcept { return ctx; }
    vsom_group *group() const noexcept { return grp; }

private:
    vsom_ctx *ctx = nullptr;          // the context searches, getters and the online path use (member 0 of grp)
    vsom_group *grp = nullptr;        // set when the Som trains on more than one GPU; owns ctx then
    bool replicasStale = false;       // member 0 was trained alone (online path): the others lag behind
    void destroyContext();
    void copyStateFrom(const Som &other);
    void joinGroup() const;
    void syncReplicas();
    size_t inLen = 0;                 // J: sample length (depth = transform.Length(J))
    mutable bool hostStale = true;    // host mirrors below are out of date
    mutable size_t nDownloads = 0;    // vsom_get_state calls of refreshHost
    mutable std::vector<float> hMap, hSigma, hWeight;
    mutable std::vector<uint64_t> hHits;
    // host execution for user-supplied hooks (kind() == vsom::Custom; src/vsom_custom.cpp): the state then
    // lives in hMap / hSigma / hS / hWeight / hHits and ctx stays null
    mutable std::vector<float> hS;
    void hostEnsure() const;
    double hostDist(size_t pos, const Eigen::VectorXf &v, const Eigen::VectorXf &valid, const Eigen::VectorXf &weights) const;
    size_t hostFindBmu(const Eigen::VectorXf &v, const Eigen::VectorXf &valid, const Eigen::VectorXf &weights) const;
    size_t hostFindLocalBmu(const Eigen::VectorXf &v, const Eigen::VectorXf &valid, size_t start, const Eigen::VectorXf &weights) const;
    size_t hostFindRestrictedBmu(const Eigen::VectorXf &v, const Eigen::VectorXf &valid, size_t minBmuHits, const Eigen::VectorXf &weights) const;
    double hostDistRaw(size_t pos, const Eigen::VectorXf &v, const Eigen::VectorXf &valid, const Eigen::VectorXf &weights) const;
    float hostBatchEpoch(DataSet &dataset, double currentSigma, bool isFirst);
    void hostTrainBatchSom(DataSet &data, size_t numberOfEpochs, double sigma0, double sigmaDecay, bool updateUMatrixAfterEpoch);
    TrainingReturnValue hostTrainSingle(const Eigen::VectorXf &v, const Eigen::VectorXf &valid, const Eigen::VectorXf &weights,
                                        double eta, double sigma, size_t &lastBMU, WeigthDecayFunction fn);
    void hostTrainBasicSom(DataSet &data, size_t numberOfEpochs, double eta0, double etaDecay, double sigma0, double sigmaDecay,
                           WeigthDecayFunction fn, bool updateUMatrixAfterEpoch);
    void createContext();
    // device hooks (Transformation::Device): the hooks' valueWeight comes from the context's column weights and the loaded
    // chunk's validity (include/vsom_hip.h, "value_weight"); devWeights is what the context holds (empty: all 1)
    bool deviceHooks() const noexcept;
    mutable std::vector<float> devWeights;
    void applyDeviceWeights(const Eigen::VectorXf &weights) const;
    void applyChunkValidity(const DataSet &data) const;
    void requireDevicePath(const char *what) const;
    void trainWhole(const char *what, bool masked, DataSet &data, size_t numberOfEpochs, double sigma0, double sigmaDecay,
                    bool updateUMatrixAfterEpoch, bool resetBmu);
    void trainResident(bool masked, const char *name, DataSet &data, size_t numberOfEpochs, double sigma0, double sigmaDecay);
    bool evaluateOnDevice(const DataSet &data, EvaluateRows &r) const;   // false: a validity flag outside {0, 1}
    void maskedRows(const DataSet *data, size_t minBmuHits, uint64_t *bmu, float *dist, float *fill) const;
    void topkMaskedRows(const char *what, const DataSet *data, size_t k, size_t minBmuHits, uint64_t *idx, float *dist,
                        uint32_t *count, uint32_t *nvalid, double *blend) const;
    void refreshHost() const;
    void stageOne(const Eigen::VectorXf &v) const;
};
