"""Python host-side mirror of the reference's `Som` / `DataSet` / `Transformation` interface for
the training hot path, over the C ABI (capi.py -> libvsom_hip.so).  Same member names, argument
meaning and error behaviour as include/SOM.hpp:107-171, so the parity tests read like the
reference's perf harness (tests/performance/perf_tests.cpp:74-140).  The C++ mirror with the
exact signatures lives in host/ (SOM.hpp); this one exists for tests/bench plumbing.

Nothing here computes on the CPU: every search/update call goes to the HIP library.
"""
import ctypes
import enum
import math
import sys

import numpy as np

from . import capi


def topographic_error(idx2, width):
    """Topographic error of best / second-best unit pairs idx2 (n x >= 2; columns 0 and 1 are used) on a map `width`
    nodes wide: node n sits at grid row n // width, column n % width (the storage layout updateUMatrix walks), and a row
    counts as an error when max(|d row|, |d column|) != 1 between its two units -- no wrap.  The count over n, summed in
    row order in double; 0.0 for n = 0."""
    idx2 = np.asarray(idx2)
    width = int(width)
    n = idx2.shape[0] if idx2.ndim else 0
    if n == 0:
        return 0.0
    if idx2.ndim != 2 or idx2.shape[1] < 2:
        raise ValueError("idx2 must be n x k with k >= 2")
    a = idx2[:, 0].astype(np.int64)
    b = idx2[:, 1].astype(np.int64)
    cheb = np.maximum(np.abs(a // width - b // width), np.abs(a % width - b % width))
    te = 0.0
    for e in (cheb != 1):
        te += 1.0 if e else 0.0
    return te / n


def measure_similarity_from_rows(first, dmax, outside):
    """The finish of Som::measureSimilarity (Som.cpp:631-714) from the per-row report of vsom_similarity_batch: (the row
    the reference reports, its return value).  The reference walks every delta of every row with one running maximum that
    starts at -99999999.f, compares the SIGNED delta with it and stores the delta's fabs (:684-690); `first[r]` is the
    delta of row r's lowest column above that start value (NaN: none) and `dmax[r]` the row's largest signed delta (NaN
    deltas excluded).  The walk equals: start at the first row whose `first` is not NaN with maxValue = |first|; for that
    row and every later one, dmax > maxValue makes maxValue = dmax and that row the reported one.  Row 0 is reported when
    no delta ever exceeds the start value (or there are no rows: then the result is True, as the mirrors return).  The
    return value is outside[row] == 0: no valid column of the reported row lies outside its approved interval."""
    first = np.asarray(first, dtype=np.float32)
    dmax = np.asarray(dmax, dtype=np.float32)
    outside = np.asarray(outside)
    n = first.shape[0]
    if dmax.shape[0] != n or outside.shape[0] != n:
        raise ValueError("first, dmax and outside must have one entry per row")
    if n == 0:
        return 0, True
    row = 0
    started = np.flatnonzero(~np.isnan(first))
    if started.size:
        r = int(started[0])
        row = r
        maxValue = np.float32(abs(first[r]))
        for i in range(r, n):
            if dmax[i] > maxValue:
                maxValue = dmax[i]
                row = i
    return row, bool(outside[row] == 0)


class WeigthDecayFunction(enum.IntEnum):      # SOM.hpp:70-75 (spelling as in the reference)
    Exponential = 0
    InverseProportional = 1
    BatchMap = 2


class Transformation:
    """Transformation.hpp:10-41: the three built-in factories, or Custom -- the caller's hooks as device source."""

    def __init__(self, kind=capi.STANDARD, names=None, name="Standard transformation", source=None, length=None,
                 residual_len=None):
        self.kind, self.names, self.Name = kind, list(names or []), name
        self.DeviceSource, self._length, self._residual_len = source, length, residual_len

    @staticmethod
    def Custom(source, length=None, residual_len=None, columnNames=(), name="Custom transformation"):
        """hooks vsom_compare / vsom_step as HIP device source (include/vsom_hip.h, vsom_create_custom); length and
        residual_len are the model depth and the residual length, each an int or a function of the sample length
        (default: the sample length)"""
        return Transformation(capi.CUSTOM, columnNames, name, source, length, residual_len)

    def ResidualLength(self, vectorLength):
        if self.kind == capi.CUSTOM:
            r = self._residual_len
            return vectorLength if r is None else int(r(vectorLength) if callable(r) else r)
        return vectorLength * (vectorLength - 1) // 2 if self.kind == capi.CLR else vectorLength

    @staticmethod
    def Standard(columnNames=()):
        return Transformation(capi.STANDARD, columnNames, "Standard transformation")

    @staticmethod
    def StandardMedianEstimator(columnNames=()):
        return Transformation(capi.MEDIAN, columnNames, "Standard median estimator transformation")

    @staticmethod
    def CombinatorialLinearRegression(columnNames=()):
        return Transformation(capi.CLR, columnNames, "Linear regression")

    def Length(self, vectorLength):            # Transformation.cpp:31-35,69-73,162-165
        if self.kind == capi.CUSTOM:
            n = self._length
            return vectorLength if n is None else int(n(vectorLength) if callable(n) else n)
        return vectorLength * (vectorLength - 1) if self.kind == capi.CLR else vectorLength


class SomIndex:
    """SomIndex.hpp:7-27."""

    def __init__(self, x=0, y=0):
        self.x, self.y = int(x), int(y)

    @staticmethod
    def fromLinear(som, index):                # SomIndex.cpp:13-18 (divides by HEIGHT, Q10)
        x = index % som.getWidth()
        return SomIndex(x, (index - x) // som.getHeight())

    def getSomIndex(self, som):
        return som.getWidth() * self.y + self.x

    def getX(self):
        return self.x

    def getY(self):
        return self.y

    def __eq__(self, o):
        return self.x == o.x and self.y == o.y

    def __repr__(self):
        return f"SomIndex({self.x},{self.y})"


class ArrayDataSet:
    """DataSet over an in-memory array with IDataLoader's chunked streaming
    (IDataLoader.hpp:22-23,46; DataSet.cpp:113-160): load() yields the next <= maxLoadCount rows,
    lastBMU is zeroed on every load, the stream wraps after the last chunk."""

    def __init__(self, X, maxLoadCount=None, names=None, weights=None):
        self.X = np.ascontiguousarray(X, dtype=np.float32)
        self.depth = self.X.shape[1]
        self.maxLoadCount = maxLoadCount or self.X.shape[0]
        self._pos = 0
        self._chunks = 0
        self.data = self.X[0:0]
        self.lastBMU = np.zeros(0, np.uint64)
        self._names = list(names or [f"c{i}" for i in range(self.depth)])
        self._weights = np.ones(self.depth, np.float32) if weights is None else np.asarray(weights, np.float32)

    def vectorLength(self):
        return self.depth

    def getNames(self):
        return self._names

    def getWeights(self):
        return self._weights

    def size(self):
        return self.data.shape[0]

    def totalRows(self):
        """extension: the rows of the whole stream (trainBatchSomWhole asks for it)"""
        return self.X.shape[0]

    def isAtStartOfDataStream(self):
        return self._pos == 0

    def hasReadWholeDataStream(self):           # DataSet.cpp:113-116
        return self._chunks > 0 and self.isAtStartOfDataStream()

    def resetStreamLoadPosition(self):          # DataSet.cpp:108-111
        self._chunks = 0

    def loadNextDataFromStream(self):           # DataSet.cpp:118-160
        if self.isAtStartOfDataStream():
            self._chunks = 0
        end = min(self._pos + self.maxLoadCount, self.X.shape[0])
        self.data = self.X[self._pos:end]
        self._pos = 0 if end >= self.X.shape[0] else end
        self.lastBMU = np.zeros(self.data.shape[0], np.uint64)   # :136-137
        self._chunks += 1

    def getData(self, i):
        return self.data[i].copy()

    def getLastBMU(self):
        return self.lastBMU


def batch_sigma_schedule(numberOfEpochs, sigma0, sigmaDecay):
    """The sigma of every epoch that trainBatchSom runs (Som.cpp:727-730): sigma0 * exp(-sigmaDecay * i) for
    i = 0, 1, ..., ending before the first value below 1 (sigma = 1.0 exactly still trains)."""
    out = []
    for i in range(numberOfEpochs):
        sigma = sigma0 * math.exp(-sigmaDecay * float(i))         # :727
        if sigma < 1.0:                                           # :729-730
            break
        out.append(sigma)
    return out


class Metrics:
    def __init__(self, n=0):
        self.MeanSquaredError = [0.0] * n
        self.DistanceError = [0.0] * n


class Som:
    """`class Som` (SOM.hpp:39-189), hot-path members only."""

    WeigthDecayFunction = WeigthDecayFunction

    def __init__(self, width, height, depth_or_dataset, transformation=None, device=0):
        self.transform = transformation or Transformation()
        if hasattr(depth_or_dataset, "vectorLength"):          # Som(w,h,DataSet,T)  SOM.hpp:78-82
            in_len = depth_or_dataset.vectorLength()
            self.transform.names = depth_or_dataset.getNames()
        else:                                                    # Som(w,h,depth,T)    SOM.hpp:83-87
            depth = int(depth_or_dataset)
            in_len = self._in_len_from_depth(depth)
        self.width, self.height = int(width), int(height)
        t = self.transform
        if t.kind == capi.CUSTOM:
            self.ctx = capi.Context(width, height, in_len, capi.CUSTOM, device=device, source=t.DeviceSource,
                                    depth=t.Length(in_len), residual_len=t.ResidualLength(in_len))
        else:
            self.ctx = capi.Context(width, height, in_len, t.kind, device=device)
        self.depth = self.ctx.depth
        self.in_len = in_len
        self.metrics = Metrics()
        self._isTraining = False
        self._verbose = False

    def _in_len_from_depth(self, depth):
        if self.transform.kind != capi.CLR:
            return depth
        J = int(round((1 + math.sqrt(1 + 4 * depth)) / 2))     # depth = J(J-1), perf_tests.cpp:338-339
        if J * (J - 1) != depth:
            raise ValueError("depth is not J*(J-1) for any J (CombinatorialLinearRegression)")
        return J

    def close(self):
        self.ctx.close()

    # ---- accessors (Som.cpp:164-212, 268-281) -------------------------------------------
    def getWidth(self):
        return self.width

    def getHeight(self):
        return self.height

    def getDepth(self):
        return self.depth

    def getIndex(self, i):
        return i.getY() * self.width + i.getX()

    def _node(self, i):
        return self.getIndex(i) if isinstance(i, SomIndex) else int(i)

    def getNeuron(self, i):
        return self.ctx.get_state(sigma=False, S=False, weight=False, hits=False)["map"][self._node(i)].copy()

    def getSigmaNeuron(self, i):
        return self.ctx.get_state(map=False, S=False, weight=False, hits=False)["sigma"][self._node(i)].copy()

    def getWeigthMap(self):
        return self.ctx.get_state(map=False, sigma=False, S=False, hits=False)["weight"]

    def getBmuHits(self):
        return self.ctx.get_state(map=False, sigma=False, S=False, weight=False)["hits"]

    def getMetrics(self):
        return self.metrics

    def isTraining(self):
        return self._isTraining

    def isCompatibleWithData(self, data):
        return self.transform.Length(data.vectorLength()) == self.depth

    def state(self):
        return self.ctx.get_state()

    def setState(self, **kw):
        self.ctx.set_state(**kw)

    def randomInitialize(self, seed, sigma):
        """Som.cpp:977-997: glibc srand/rand sequence, node-major, dim-minor."""
        libc = ctypes.CDLL(None)
        libc.srand(ctypes.c_uint(int(seed) & 0xFFFFFFFF))
        n, d = self.width * self.height, self.depth
        mod = int(np.float32(2000) * np.float32(sigma))
        r = np.fromiter((libc.rand() % mod for _ in range(n * d)), dtype=np.int64, count=n * d)
        m = ((r.astype(np.float32) - np.float32(1000.0) * np.float32(sigma)) / np.float32(1000.0)).astype(np.float32)
        self.metrics = Metrics(d)
        self.ctx.set_state(map=m.reshape(n, d), sigma=np.zeros((n, d), np.float32),
                           S=np.zeros((n, d), np.float32), weight=np.zeros(n, np.float32),
                           hits=np.zeros(n, np.uint64))

    def addBmu(self, pos):                       # Som.cpp:1189-1192
        st = self.ctx.get_state(map=False, sigma=False, S=False, weight=False)
        st["hits"][self.getIndex(pos)] += 1
        self.ctx.set_state(hits=st["hits"])

    @staticmethod
    def calculateNeighbourhoodWeight(currentX, currentY, bmuX, bmuY, currentSigma):
        return capi.neighbourhood_weight(currentX, currentY, bmuX, bmuY, currentSigma)

    # ---- search (Som.cpp:115-141, 283-309, 335-454) --------------------------------------
    def _stage_one(self, v):
        v = np.ascontiguousarray(v, dtype=np.float32).reshape(1, -1)
        self.ctx.upload_chunk(v)

    # Transformation.Custom: the hooks' valueWeight is real on the device (capi.Context.set_column_weights /
    # set_chunk_validity and the valid= keyword); the built-in transformations ignore valid and weights, as the reference's do
    def _custom(self):
        return self.ctx.transform == capi.CUSTOM

    def _setWeights(self, weights):
        """the context's column weights := weights (None: all 1), when they are not what it holds already"""
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
        if w is not None and (w == 1).all():
            w = None
        held = getattr(self, "_devWeights", None)
        if (w is None) != (held is None) or (w is not None and w.tobytes() != held.tobytes()):
            self.ctx.set_column_weights(w)
            self._devWeights = None if w is None else w.copy()

    def _chunkToDevice(self, data):
        """upload the data set's loaded rows; with custom hooks also its column weights and -- when it has an attribute
        `validity` (loaded rows x J, nonzero = valid) with an invalid entry -- the chunk's validity"""
        self.ctx.upload_chunk(data.data)
        if not self._custom():
            return
        self._setWeights(data.getWeights() if hasattr(data, "getWeights") else None)
        valid = getattr(data, "validity", None)
        if valid is not None and not np.asarray(valid).all():
            self.ctx.set_chunk_validity(np.asarray(valid))

    def _vectorValid(self, valid, weights):
        """valid= of the single-vector calls of a custom context (None elsewhere), after setting the weights"""
        if not self._custom():
            return None
        self._setWeights(weights)
        return None if valid is None else np.asarray(valid)

    def findBmu(self, v, valid=None, weights=None):
        idx, _ = self.ctx.find_bmu(v, valid=self._vectorValid(valid, weights))
        return SomIndex(idx % self.width, idx // self.width)

    def findLocalBmu(self, v, valid, lastBMUref, weights=None):
        if self._custom():
            idx, _ = self.ctx.find_local_bmu(v, lastBMUref, valid=self._vectorValid(valid, weights))
            return SomIndex(idx % self.width, idx // self.width)
        self._stage_one(v)
        self.ctx.set_last_bmu(np.array([lastBMUref], np.uint64))
        idx, _ = self.ctx.bmu_local_batch()
        return SomIndex(int(idx[0]) % self.width, int(idx[0]) // self.width)

    def euclidianWeightedDist(self, pos, v, valid=None, weights=None):
        if self._custom():
            return float(self.ctx.dist_single(v, self._node(pos), valid=self._vectorValid(valid, weights)))
        self._stage_one(v)
        return float(self.ctx.distances([self._node(pos)], [0])[0])

    # ---- restricted best matching distribution (Som.cpp:457-487, 525-566) -------------------
    @staticmethod
    def _rows(data):
        """the loaded rows of a DataSet (DataSet::getData(i), i < size()), or a 2-D array as it is"""
        return data.data if hasattr(data, "data") else np.ascontiguousarray(data, dtype=np.float32)

    def findRestrictedBmd(self, v, valid=None, minBmuHits=0, weights=None):
        """Som::findRestrictedBmd: float64[N], p_i / C with p_i = exp(-d_i^2 / 2) on the nodes with at least
        minBmuHits hits (0 elsewhere)"""
        self._stage_one(v)
        return self.ctx.restricted_bmd(minBmuHits, 0, 1, probs=True)["prob"][0]

    def drawModelVectors(self, data, minBmuHits, u):
        """extension: one node per loaded row of `data`, drawn from its restricted distribution with the caller's
        uniform u[r] in [0, 1) (uint64; UINT64_MAX where the row has no mass)"""
        X = self._rows(data)
        self.ctx.upload_chunk(X)
        return self.ctx.restricted_bmd(minBmuHits, u=u)["draw"]

    def variationalAutoEncoder(self, data, minBmuHits, seed=None):
        """Som::variationalAutoEncoder: the node drawn for the LAST loaded row (the reference's other draws have no
        effect); 0 when that row has no mass, as the reference's discrete_distribution returns then"""
        X = self._rows(data)
        if X.shape[0] == 0:
            return 0
        u = np.random.default_rng(seed).random(1)
        d = int(self.drawModelVectors(X[-1:], minBmuHits, u)[0])
        return 0 if d == 0xFFFFFFFFFFFFFFFF else d

    # ---- generated records (Som.cpp:568-623) ----------------------------------------------------
    def generateRows(self, data, minBmuHits, u, l, perRow=True):
        """extension: Som::autoEncoder's records for every loaded row of `data` with the caller's random numbers
        (capi.Context.generate): a unit per row drawn with the uniform u[r] in [0, 1) from the row's own restricted
        distribution (perRow=True) or from that of the last row (perRow=False, the reference as written), and every column
        sampled as log(l / (1 - l)) / 1.6 * sigma + mean around it, l: float64[rows, min(J, D)].  {"unit", "record"};
        a row without mass has the unit capi.NO_UNIT and a record of NaN."""
        X = self._rows(data)
        self.ctx.upload_chunk(X)
        if X.shape[0] == 0:
            return {"unit": np.zeros(0, np.uint64), "record": np.zeros((0, min(self.ctx.in_len, self.ctx.depth)), np.float64)}
        return self.ctx.generate(minBmuHits, u, l, capi.GENERATE_PER_ROW if perRow else capi.GENERATE_AS_WRITTEN)

    def decodeUnits(self, units, l):
        """extension: the records of given units (capi.Context.decode_nodes): float64[len(units), min(J, D)], row i sampled
        around unit units[i] with l[i]"""
        return self.ctx.decode_nodes(units, l)

    def autoEncoder(self, data, minBmuHits, seed=None):
        """Som::autoEncoder as written: every loaded row gets a unit drawn from the LAST row's restricted distribution and a
        record sampled around it; the uniforms and the reference's L = (rand() % 1000) / 1000 come from
        numpy.random.default_rng(seed).  Returns (unit uint64[rows], record float64[rows, min(J, D)]); a row without mass
        takes node 0, what the reference's discrete_distribution returns then.  (The reference prints; the text output is
        the C++ mirror's.)"""
        X = self._rows(data)
        n, cols = X.shape[0], min(self.ctx.in_len, self.ctx.depth)
        rng = np.random.default_rng(seed)
        u = rng.random(n)
        l = rng.integers(0, 1000, (n, cols)).astype(np.float64) / 1000.0
        rep = self.generateRows(X, minBmuHits, u, l, perRow=False)
        unit, record = rep["unit"], rep["record"]
        none = unit == np.uint64(capi.NO_UNIT)
        if none.any():
            unit[none] = 0
            record[none] = self.ctx.decode_nodes(np.zeros(int(none.sum()), np.uint64), l[none])
        return unit, record

    # ---- similarity of records to their best matching units (Som.cpp:631-714) -----------------
    def similarityRows(self, data, numOfSigmas, minBmuHits, floor=True, valid=None, delta=False):
        """extension: the per-row report measureSimilarity computes and throws away, for every loaded row of `data`
        (capi.Context.similarity): the row's BMU among the nodes with at least minBmuHits hits, its anomaly score amax
        (the largest |x - m| / sM / numOfSigmas over the valid columns) with the column that causes it, the number of
        valid columns outside m +- sM * numOfSigmas, and with delta=True the dense matrix.  floor=True takes
        sM = max(sigma, 1e-5) (what a user wants), floor=False the reference's select as written (a cap at 1e-5)."""
        X = self._rows(data)
        self.ctx.upload_chunk(X)
        rule = capi.SIGMA_FLOOR if floor else capi.SIGMA_AS_WRITTEN
        return self.ctx.similarity(minBmuHits, numOfSigmas, sigma_rule=rule, valid=valid, delta=delta)

    def measureSimilarity(self, data, numOfSigmas, minBmuHits):
        """Som::measureSimilarity: whether the record with the largest relative distance to its BMU in any column lies
        inside the approved interval in all its valid columns (reference semantics, its sigma select as written).  The
        validity comes from the data set when it has one (an attribute `validity`, rows x J)."""
        X = self._rows(data)
        if X.shape[0] == 0:
            return True
        rep = self.similarityRows(X, numOfSigmas, minBmuHits, floor=False, valid=getattr(data, "validity", None))
        return measure_similarity_from_rows(rep["first"], rep["dmax"], rep["outside"])[1]

    # ---- validation loss (Som.cpp:490-523) -------------------------------------------------------
    def evaluateRows(self, data, binary=None, continuous=None, valid=None):
        """extension: what Som::evaluate sums, for every loaded row of `data` (capi.Context.evaluate): the row's BMU and
        its distance, bsum (binaryError.dot(binaryError)), nrepl (terms replaced by -99999 that count), and the running
        mean `error`.  binary defaults to all 0, continuous to all 1 (DataSet::getBinary / getContinuous of a data set
        that flags nothing binary); valid: rows x J, nonzero = valid -- when None it comes from the data set if that has
        one (an attribute `validity`), as in measureSimilarity, and otherwise every column is valid."""
        if valid is None:
            valid = getattr(data, "validity", None)
        X = self._rows(data)
        J = self.ctx.in_len
        binary = np.zeros(J, np.float32) if binary is None else binary
        continuous = np.ones(J, np.float32) if continuous is None else continuous
        self.ctx.upload_chunk(X)
        if X.shape[0] == 0:
            return {"bmu": np.zeros(0, np.uint64), "dist": np.zeros(0, np.float32), "bsum": np.zeros(0, np.float32),
                    "nrepl": np.zeros(0, np.uint32), "error": 0.0}
        return self.ctx.evaluate(binary, continuous, valid=valid)

    def evaluate(self, data, binary=None, continuous=None, valid=None):
        """Som::evaluate: the mean over the loaded rows of `data` of the distance to the BMU plus the norm of the binary
        error (arguments as evaluateRows)."""
        return self.evaluateRows(data, binary, continuous, valid)["error"]

    # ---- search over the valid columns, imputation, classification (extensions) ----------------
    def _masked(self, data, valid, minBmuHits, fill):
        X = self._rows(data)
        self.ctx.upload_chunk(X)
        if X.shape[0] == 0:
            return {"bmu": np.zeros(0, np.uint64), "dist": np.zeros(0, np.float32), "nvalid": np.zeros(0, np.uint32),
                    "fill": np.zeros((0, self.ctx.in_len), np.float32) if fill else None}
        if valid is None:
            valid = np.ones(self.ctx.in_len, np.uint8)
        return self.ctx.bmu_masked(valid, min_hits=minBmuHits, fill=fill)

    def findBmuMasked(self, data, minBmuHits=0):
        """extension: the best matching unit of every loaded row of `data` over its valid columns only, among node 0 and
        the nodes with at least minBmuHits hits (capi.Context.bmu_masked): {"bmu", "dist", "nvalid"}.  The validity comes
        from the data set when it has one (an attribute `validity`, rows x J, nonzero = valid), as in measureSimilarity;
        without one every column is valid."""
        rep = self._masked(data, getattr(data, "validity", None), minBmuHits, False)
        return {k: rep[k] for k in ("bmu", "dist", "nvalid")}

    def impute(self, data, minBmuHits=0):
        """extension: float32[rows, J], every loaded row of `data` with its invalid columns filled from its best matching
        unit over the valid ones (validity as in findBmuMasked)"""
        return self._masked(data, getattr(data, "validity", None), minBmuHits, True)["fill"]

    # ---- the two scorers over the valid columns only (extensions) --------------------------------
    def _validity(self, data):
        valid = getattr(data, "validity", None)
        return np.ones(self.ctx.in_len, np.uint8) if valid is None else valid

    def similarityRowsMasked(self, data, numOfSigmas, minBmuHits, floor=True, delta=False):
        """extension: similarityRows for records with missing fields (capi.Context.similarity_masked): every loaded row of
        `data` searched over its valid columns only, as findBmuMasked, and scored against that unit in those columns;
        similarityRows' report (dmax / first over the valid columns, delta 0 at invalid ones) and nvalid.  The validity
        comes from the data set when it has one (an attribute `validity`, rows x J, nonzero = valid); without one every
        column is valid."""
        X = self._rows(data)
        self.ctx.upload_chunk(X)
        n, J = X.shape[0], self.ctx.in_len
        if n == 0:
            rep = {k: np.zeros(0, np.float32) for k in ("dist", "dmax", "first", "amax")}
            rep.update({k: np.zeros(0, np.uint32) for k in ("dmax_col", "amax_col", "outside", "nvalid")})
            rep.update(bmu=np.zeros(0, np.uint64), delta=np.zeros((0, J), np.float32) if delta else None)
            return rep
        rule = capi.SIGMA_FLOOR if floor else capi.SIGMA_AS_WRITTEN
        return self.ctx.similarity_masked(self._validity(data), minBmuHits, numOfSigmas, sigma_rule=rule, delta=delta)

    def measureSimilarityMasked(self, data, numOfSigmas, minBmuHits):
        """extension: measureSimilarity for records with missing fields: the same finish (the reference's sigma select as
        written) over the report of similarityRowsMasked -- the record with the largest relative distance to its masked
        BMU in any VALID column, and whether it lies inside the approved interval in all its valid columns."""
        X = self._rows(data)
        if X.shape[0] == 0:
            return True
        rep = self.similarityRowsMasked(data, numOfSigmas, minBmuHits, floor=False)
        return measure_similarity_from_rows(rep["first"], rep["dmax"], rep["outside"])[1]

    def evaluateRowsMasked(self, data, binary=None, continuous=None, minBmuHits=0):
        """extension: evaluateRows for records with missing fields (capi.Context.evaluate_masked): every loaded row of
        `data` searched over its valid columns only and its binary error summed over those columns; evaluateRows' report
        and nvalid.  binary / continuous default as in evaluateRows, the validity as in similarityRowsMasked."""
        X = self._rows(data)
        J = self.ctx.in_len
        binary = np.zeros(J, np.float32) if binary is None else binary
        continuous = np.ones(J, np.float32) if continuous is None else continuous
        self.ctx.upload_chunk(X)
        if X.shape[0] == 0:
            return {"bmu": np.zeros(0, np.uint64), "dist": np.zeros(0, np.float32), "bsum": np.zeros(0, np.float32),
                    "nrepl": np.zeros(0, np.uint32), "error": 0.0, "nvalid": np.zeros(0, np.uint32)}
        return self.ctx.evaluate_masked(self._validity(data), binary, continuous, min_hits=minBmuHits)

    def evaluateMasked(self, data, binary=None, continuous=None, minBmuHits=0):
        """extension: evaluate for records with missing fields: the mean over the loaded rows of `data` of the masked
        distance to the masked BMU plus the norm of the binary error over the valid columns (arguments as
        evaluateRowsMasked)."""
        return self.evaluateRowsMasked(data, binary, continuous, minBmuHits)["error"]

    # ---- the distribution over the units and sampled records, over the valid columns only (extensions) ----
    def findRestrictedBmdMasked(self, v, valid, minBmuHits=0):
        """extension: findRestrictedBmd over the valid columns of v only (capi.Context.restricted_bmd_masked): float64[N];
        valid: J entries, nonzero = valid"""
        self._stage_one(v)
        return self.ctx.restricted_bmd_masked(np.asarray(valid).reshape(-1), minBmuHits, 0, 1, probs=True)["prob"][0]

    def drawModelVectorsMasked(self, data, minBmuHits, u):
        """extension: drawModelVectors for records with missing fields: one node per loaded row of `data`, drawn with the
        uniform u[r] from the row's restricted distribution over its valid columns (validity as in findBmuMasked)"""
        X = self._rows(data)
        self.ctx.upload_chunk(X)
        if X.shape[0] == 0:
            return np.zeros(0, np.uint64)
        return self.ctx.restricted_bmd_masked(self._validity(data), minBmuHits, u=u)["draw"]

    def generateRowsMasked(self, data, minBmuHits, u, l, draws=1, keepObserved=True):
        """extension: sampled imputation with the caller's random numbers (capi.Context.generate_masked): for every loaded
        row of `data`, `draws` units drawn with the uniforms u[r, k] from the row's restricted distribution over its valid
        columns, and around each a record that keeps the row's valid columns (keepObserved) and samples the others as
        generateRows does, l: float64[rows, draws, J].  {"unit": uint64[rows, draws], "record": float64[rows, draws, J]};
        a draw without mass has the unit capi.NO_UNIT and a record of NaN.  Validity as in findBmuMasked."""
        X = self._rows(data)
        self.ctx.upload_chunk(X)
        if X.shape[0] == 0:
            return {"unit": np.zeros((0, int(draws)), np.uint64),
                    "record": np.zeros((0, int(draws), self.ctx.in_len), np.float64)}
        return self.ctx.generate_masked(self._validity(data), minBmuHits, u, l, draws=draws, keep_observed=keepObserved)

    def imputeSampled(self, data, minBmuHits=0, draws=1, seed=None):
        """extension: multiple imputation next to impute: float64[rows, draws, J], `draws` completions of every loaded row
        of `data` -- its valid columns as they are, the others sampled around units drawn from the row's distribution over
        the valid ones (generateRowsMasked).  The uniforms and L = integers(1, 1000) / 1000 (never 0 or 1: no +-inf) come
        from numpy.random.default_rng(seed)."""
        X = self._rows(data)
        n, K, J = X.shape[0], int(draws), self.ctx.in_len
        rng = np.random.default_rng(seed)
        u = rng.random((n, K))
        l = rng.integers(1, 1000, (n, K, J)).astype(np.float64) / 1000.0
        return self.generateRowsMasked(data, minBmuHits, u, l, draws=K, keepObserved=True)["record"]

    def classify(self, data, label_columns, minBmuHits=0):
        """extension: a trained map with label columns used as a classifier.  Every loaded row of `data` is matched on the
        columns outside `label_columns` (a column mask; what the rows hold in the label columns is ignored), and its
        label is the argmax over its unit's values in the label columns, the lowest column on ties (numpy's argmax: a NaN
        counts as the largest).  Returns (label int64[rows], an index into label_columns; bmu uint64[rows])."""
        cols = np.asarray(label_columns, dtype=np.int64).ravel()
        J = self.ctx.in_len
        if cols.size == 0 or cols.min() < 0 or cols.max() >= J:
            raise ValueError(f"label_columns must name at least one column in [0, {J})")
        valid = np.ones(J, np.uint8)
        valid[cols] = 0
        rep = self._masked(data, valid, minBmuHits, True)
        return np.argmax(rep["fill"][:, cols], axis=1).astype(np.int64), rep["bmu"]

    # ---- k best matching units, topographic error (extensions) ---------------------------------
    def findBestMatchingUnits(self, data, k, dist=False):
        """extension: the k best matching units of every loaded row of `data` (uint64[rows, k]; entry 0 is findBmu's
        BMU, the others follow in (distance, index) order); with dist=True also their distances (float32[rows, k])"""
        X = self._rows(data)
        self.ctx.upload_chunk(X)
        if X.shape[0] == 0:
            return (np.zeros((0, int(k)), np.uint64), np.zeros((0, int(k)), np.float32)) if dist else \
                np.zeros((0, int(k)), np.uint64)
        idx, d = self.ctx.bmu_topk(k, dist=dist)
        return (idx, d) if dist else idx

    def topographicError(self, data):
        """extension: the fraction of loaded rows of `data` whose best and second-best units are not grid neighbours"""
        if self.width * self.height < 2:
            raise ValueError("the topographic error needs a map of at least 2 nodes")
        return topographic_error(self.findBestMatchingUnits(data, 2), self.width)

    # ---- the same over the valid columns only (extensions) ---------------------------------------
    def _topk_masked(self, data, k, minBmuHits, dist, blend):
        X = self._rows(data)
        self.ctx.upload_chunk(X)
        n, k, J = X.shape[0], int(k), self.ctx.in_len
        if n == 0:
            return {"idx": np.zeros((0, k), np.uint64), "dist": np.zeros((0, k), np.float32) if dist else None,
                    "count": np.zeros(0, np.uint32), "nvalid": np.zeros(0, np.uint32),
                    "blend": np.zeros((0, J), np.float64) if blend else None}
        return self.ctx.bmu_topk_masked(k, self._validity(data), min_hits=minBmuHits, dist=dist, blend=blend)

    def findBestMatchingUnitsMasked(self, data, k, minBmuHits=0, dist=False):
        """extension: findBestMatchingUnits for records with missing fields (capi.Context.bmu_topk_masked): the k best
        matching units of every loaded row of `data` over its valid columns only, among node 0 and the nodes with at least
        minBmuHits hits.  {"idx": uint64[rows, k] (entry 0 is findBmuMasked's unit; a row with fewer than k candidates is
        padded with capi.NO_UNIT), "count": uint32[rows] (the real entries), "nvalid": uint32[rows]} and, with dist=True,
        "dist": float32[rows, k].  Validity as in findBmuMasked."""
        rep = self._topk_masked(data, k, minBmuHits, dist, False)
        return {key: rep[key] for key in ("idx", "count", "nvalid") + (("dist",) if dist else ())}

    def topographicErrorMasked(self, data, minBmuHits=0):
        """extension: topographicError for records with missing fields: (error, rows_counted) -- topographic_error over the
        rows that have a valid column and a second unit (nvalid >= 1 and count >= 2), 0.0 when there are none"""
        if self.width * self.height < 2:
            raise ValueError("the topographic error needs a map of at least 2 nodes")
        rep = self._topk_masked(data, 2, minBmuHits, False, False)
        keep = (rep["nvalid"] >= 1) & (rep["count"] >= 2)
        return topographic_error(rep["idx"][keep], self.width), int(keep.sum())

    def imputeBlend(self, data, k, minBmuHits=0):
        """extension: float64[rows, J], every loaded row of `data` with its invalid columns filled from its k best matching
        units over the valid ones, each weighted as the BMD weights it (exp(-d^2 / 2), relative to the best) -- between
        impute (one unit) and imputeSampled (random).  A row without mass holds NaN at its invalid columns."""
        return self._topk_masked(data, k, minBmuHits, False, True)["blend"]

    # ---- batch training (Som.cpp:716-879) --------------------------------------------------
    def trainBatchSomEpoch(self, dataset, currentSigma, isFirst):
        self._chunkToDevice(dataset)
        if not isFirst:
            self.ctx.set_last_bmu(dataset.lastBMU)
        mse = self.ctx.batch_epoch(currentSigma, isFirst)
        dataset.lastBMU[...] = self.ctx.get_last_bmu()
        return mse

    def trainBatchSomEpochMasked(self, dataset, currentSigma, isFirst):
        """extension: trainBatchSomEpoch over the valid entries of the loaded rows only (capi.Context.batch_epoch_masked): a
        missing field neither attracts the search nor enters the means and sigmas.  The validity comes from the data set
        when it has one (an attribute `validity`, loaded rows x J, nonzero = valid), as in findBmuMasked; without one every
        column is valid."""
        self.ctx.upload_chunk(dataset.data)
        if not isFirst:
            self.ctx.set_last_bmu(dataset.lastBMU)
        valid = getattr(dataset, "validity", None)
        if valid is None:
            valid = np.ones(self.ctx.in_len, np.uint8)
        mse = self.ctx.batch_epoch_masked(currentSigma, isFirst, valid)
        dataset.lastBMU[...] = self.ctx.get_last_bmu()
        return mse

    # ---- U-matrix (Som.cpp:143-157, 999-1111) -------------------------------------------------
    def updateUMatrix(self, weights=None):
        """Mean sigma-normalised raw distance of every node to its 3/5/8 neighbours, diagonals weighted 0.3;
        one stencil launch on the device (vsom_umatrix).  Custom contexts and maps with width < 2 or height < 2 keep
        the earlier route: the distances on the device (vsom_distances_raw), their combination in double on the host
        in the reference's order of additions."""
        W, H = self.width, self.height
        if W >= 2 and H >= 2 and self.ctx.transform != capi.CUSTOM:
            self.uMatrix = self.ctx.umatrix()
            return self.uMatrix
        DI = (0, 0, 1, -1, -1, 1, -1, 1)       # W, E, S(i+1), N(i-1), NW, SW, NE, SE  (:1017-1024)
        DJ = (-1, 1, 0, 0, -1, -1, 1, 1)
        nodes, nbrs, slot = [], [], {}
        for i in range(H):
            for j in range(W):
                for k in range(8):
                    ni, nj = i + DI[k], j + DJ[k]
                    if 0 <= ni < H and 0 <= nj < W:
                        slot[(i * W + j, k)] = len(nodes)
                        nodes.append(i * W + j)
                        nbrs.append(ni * W + nj)
        d = self.ctx.distances_raw(nodes, nbrs, True).astype(np.float64) if nodes else np.zeros(0)
        f = 0.3
        Wk, Ek, Sk, Nk, NWk, SWk, NEk, SEk = range(8)
        U = np.zeros(W * H, np.float64)
        for i in range(H):
            for j in range(W):
                n = i * W + j
                R = lambda k: float(d[slot[(n, k)]])   # noqa: E731
                if 0 < j < W - 1 and 0 < i < H - 1:
                    u = (R(Wk) + R(Ek) + R(Sk) + R(Nk) + R(NWk) * f + R(SWk) * f + R(NEk) * f + R(SEk) * f) / 8
                elif i == 0 and 0 < j < W - 1:
                    u = (R(Wk) + R(Ek) + R(Sk) + R(SWk) * f + R(SEk) * f) / 5
                elif i == H - 1 and 0 < j < W - 1:
                    u = (R(Wk) + R(Ek) + R(Nk) + R(NWk) * f + R(NEk) * f) / 5
                elif j == 0 and 0 < i < H - 1:
                    u = (R(Ek) + R(Sk) + R(Nk) + R(NEk) * f + R(SEk) * f) / 5
                elif j == W - 1 and 0 < i < H - 1:
                    u = (R(Wk) + R(Sk) + R(Nk) + R(NWk) * f + R(SWk) * f) / 5
                elif j == 0 and i == 0 and W > 1 and H > 1:
                    u = (R(Ek) + R(Sk) + R(SEk) * f) / 3
                elif j == W - 1 and i == 0 and W > 1 and H > 1:
                    u = (R(Wk) + R(Sk) + R(SWk) * f) / 3
                elif j == 0 and i == H - 1 and W > 1 and H > 1:
                    u = (R(Ek) + R(Nk) + R(NEk) * f) / 3
                elif j == W - 1 and i == H - 1 and W > 1 and H > 1:
                    u = (R(Wk) + R(Nk) + R(NWk) * f) / 3
                else:
                    u = 0.0
                U[n] = u
        self.uMatrix = U
        return U

    def getUMatrix(self):
        return getattr(self, "uMatrix", np.zeros(self.width * self.height, np.float64))

    def trainBatchSom(self, data, numberOfEpochs, sigma0, sigmaDecay, updateUMatrixAfterEpoch=False):
        self._trainBatchSom(self.trainBatchSomEpoch, data, numberOfEpochs, sigma0, sigmaDecay, updateUMatrixAfterEpoch)

    def trainBatchSomMasked(self, data, numberOfEpochs, sigma0, sigmaDecay, updateUMatrixAfterEpoch=False):
        """extension: trainBatchSom with trainBatchSomEpochMasked as its epoch -- the same sigma schedule, stop at
        sigma < 1, chunk loop and metrics"""
        self._trainBatchSom(self.trainBatchSomEpochMasked, data, numberOfEpochs, sigma0, sigmaDecay, updateUMatrixAfterEpoch)

    def _trainBatchSom(self, epoch, data, numberOfEpochs, sigma0, sigmaDecay, updateUMatrixAfterEpoch):
        self.metrics = Metrics(numberOfEpochs)                    # :719
        for i in range(numberOfEpochs):
            if self._verbose:
                print(f"Training VSOM epoch {i}/{numberOfEpochs}")
            sigma = sigma0 * math.exp(-sigmaDecay * float(i))     # :727
            if sigma < 1.0:                                       # :729-730
                return
            mse = np.float32(0.0)
            count = 0
            while not data.hasReadWholeDataStream():              # :735
                data.loadNextDataFromStream()
                mse = np.float32(mse + epoch(data, sigma, i == 0))
                count += 1
            mse = np.float32(mse / np.float32(count))             # :743
            self.metrics.MeanSquaredError[i] = mse
            data.resetStreamLoadPosition()
            if updateUMatrixAfterEpoch:
                self.updateUMatrix(data.getWeights())             # :751-752 / :1183-1184

    @staticmethod
    def _streamRows(data):
        """the rows of the whole stream: the data set's totalRows() or len(), else one counting pass over the stream"""
        if hasattr(data, "totalRows"):
            return int(data.totalRows())
        if hasattr(data, "__len__"):
            return len(data)
        total = 0
        while not data.hasReadWholeDataStream():
            data.loadNextDataFromStream()
            total += data.size()
        data.resetStreamLoadPosition()
        return total

    def trainBatchSomWhole(self, data, numberOfEpochs, sigma0, sigmaDecay, updateUMatrixAfterEpoch=False, reset_bmu=True):
        """extension: trainBatchSom's driver with ONE batch epoch per pass over the stream -- the chunks of a pass
        accumulate into one epoch over all rows (capi.Context.batch_accum_begin / _chunk / _end), where trainBatchSom runs
        an epoch per chunk and ends a pass with the batch map of its last chunk alone.  The same sigma schedule and stop
        at sigma < 1; metrics.MeanSquaredError[i] is the MSE of epoch i over all rows; updateUMatrix runs after the
        epoch's end.  The row count of the stream comes from data.totalRows() or len(data); a data set with neither is
        streamed once before the first epoch to count its rows.
        reset_bmu=True is the reference's behaviour: a load zeroes lastBMU, so the epochs after the first walk from unit
        0.  With reset_bmu=False every row's BMU of the previous epoch is kept (a host array of one entry per row) and
        starts that row's walk.  Chunk k+1 is copied to the device (prefetch / commit) while chunk k accumulates.
        Standard and Median on one device, strict update mode."""
        self._trainBatchSomWhole(False, data, numberOfEpochs, sigma0, sigmaDecay, updateUMatrixAfterEpoch, reset_bmu)

    def trainBatchSomWholeMasked(self, data, numberOfEpochs, sigma0, sigmaDecay, updateUMatrixAfterEpoch=False,
                                 reset_bmu=True):
        """extension: trainBatchSomWhole over the valid entries of the rows only -- every chunk goes into the epoch with
        capi.Context.batch_accum_chunk_masked, so that a missing field neither attracts the search nor enters the means
        and sigmas of its column, and the epoch still covers all rows of the stream.  The validity of a chunk comes from
        the data set when it has one (an attribute `validity`, loaded rows x J, nonzero = valid), as in
        trainBatchSomEpochMasked; without one every column is valid.  Driver, schedule, metrics and reset_bmu are
        trainBatchSomWhole's, the prefetch / commit pipeline included."""
        self._trainBatchSomWhole(True, data, numberOfEpochs, sigma0, sigmaDecay, updateUMatrixAfterEpoch, reset_bmu)

    def _chunkValidity(self, data):
        """the loaded chunk's validity as the masked calls take it (a copy: the next load replaces the data set's)"""
        valid = getattr(data, "validity", None)
        if valid is None:
            return np.ones(self.ctx.in_len, np.uint8)
        return np.array(valid)

    def _trainBatchSomWhole(self, masked, data, numberOfEpochs, sigma0, sigmaDecay, updateUMatrixAfterEpoch, reset_bmu):
        self.metrics = Metrics(numberOfEpochs)                    # :719
        sigmas = batch_sigma_schedule(numberOfEpochs, sigma0, sigmaDecay)
        if not sigmas:
            return
        total = self._streamRows(data)
        prev = None if reset_bmu else np.zeros(total, np.uint64)
        ctx = self.ctx
        for i, sigma in enumerate(sigmas):
            if self._verbose:
                print(f"Training VSOM epoch {i}/{numberOfEpochs}")
            ctx.batch_accum_begin(sigma, i == 0, total)
            try:
                off = 0
                rows = None                                       # the rows on their way to the device: kept alive
                have = not data.hasReadWholeDataStream()          # :735
                if have:
                    data.loadNextDataFromStream()
                    rows = np.ascontiguousarray(data.data, dtype=np.float32)
                    valid = self._chunkValidity(data) if masked else None
                    ctx.prefetch_chunk(rows)
                while have:
                    ctx.commit_chunk()                            # lastBMU := 0 (DataSet.cpp:136-137)
                    B, lb_ref = rows.shape[0], data.lastBMU
                    if prev is not None and i > 0:
                        ctx.set_last_bmu(prev[off:off + B])
                    if masked:
                        ctx.batch_accum_chunk_masked(valid)
                    else:
                        ctx.batch_accum_chunk()
                    have = not data.hasReadWholeDataStream()
                    if have:                                      # the next chunk's load and copy beside this one's chains
                        data.loadNextDataFromStream()
                        rows = np.ascontiguousarray(data.data, dtype=np.float32)
                        valid = self._chunkValidity(data) if masked else None
                        ctx.prefetch_chunk(rows)
                    if prev is not None or not have:
                        lb = ctx.get_last_bmu()
                        if prev is not None:
                            prev[off:off + B] = lb
                        if not have:
                            lb_ref[...] = lb                      # the chunk the data set still holds keeps its BMUs
                    off += B
                mse = ctx.batch_accum_end()
            except BaseException:
                try:
                    ctx.batch_accum_abort()
                except capi.VsomError:
                    pass
                raise
            self.metrics.MeanSquaredError[i] = mse
            data.resetStreamLoadPosition()                        # :749
            if updateUMatrixAfterEpoch:
                self.updateUMatrix(data.getWeights())             # :751-752

    def trainBatchSomResident(self, data, numberOfEpochs, sigma0, sigmaDecay):
        """extension: trainBatchSom for a data set that is ONE chunk, with the chunk uploaded once and the whole sigma
        schedule run by one call (capi.Context.batch_schedule) -- the same map, metrics and lastBMU as trainBatchSom,
        which reloads the chunk (lastBMU := 0) and calls the device once per epoch.  Raises ValueError before it trains
        when the first load does not read the whole stream."""
        self._trainBatchSomResident(False, "trainBatchSomResident", data, numberOfEpochs, sigma0, sigmaDecay)

    def trainBatchSomResidentMasked(self, data, numberOfEpochs, sigma0, sigmaDecay):
        """extension: trainBatchSomResident over the valid entries of the rows only (capi.Context.batch_schedule_masked)
        -- the same map, metrics and lastBMU as trainBatchSomMasked on the one-chunk data set.  The validity comes from
        the data set when it has one (an attribute `validity`, loaded rows x J, nonzero = valid), as in
        trainBatchSomEpochMasked; without one every column is valid.  The same one-chunk rule: ValueError before it
        trains when the first load does not read the whole stream."""
        self._trainBatchSomResident(True, "trainBatchSomResidentMasked", data, numberOfEpochs, sigma0, sigmaDecay)

    def _trainBatchSomResident(self, masked, name, data, numberOfEpochs, sigma0, sigmaDecay):
        self.metrics = Metrics(numberOfEpochs)                    # :719
        sigmas = batch_sigma_schedule(numberOfEpochs, sigma0, sigmaDecay)
        if not sigmas:
            return
        data.loadNextDataFromStream()
        if not data.hasReadWholeDataStream():
            data.resetStreamLoadPosition()      # (a caller that falls back to trainBatchSom starts from a clean stream)
            raise ValueError(f"{name} needs a data set that loads as one chunk; use "
                             f"{'trainBatchSomMasked' if masked else 'trainBatchSom'}")
        self.ctx.upload_chunk(data.data)
        if masked:
            mses = self.ctx.batch_schedule_masked(sigmas, self._chunkValidity(data), reset_bmu=True)
        else:
            mses = self.ctx.batch_schedule(sigmas, reset_bmu=True)
        for i, mse in enumerate(mses):
            self.metrics.MeanSquaredError[i] = np.float32(np.float32(np.float32(0.0) + mse) / np.float32(1))   # :743
        data.lastBMU[...] = self.ctx.get_last_bmu()
        data.resetStreamLoadPosition()

    # ---- online training (Som.cpp:885-947, 1135-1187) ---------------------------------------
    def trainSingle(self, v, valid, weights, eta, sigma, lastBMU, weightDecayFunction):
        bmu, residual, dist, last = self.ctx.train_single(v, eta, sigma, lastBMU, int(weightDecayFunction),
                                                          valid=self._vectorValid(valid, weights))
        return SomIndex(bmu % self.width, bmu // self.width), residual, dist, last

    def trainBasicSom(self, data, numberOfEpochs, eta0, etaDecay, sigma0, sigmaDecay,
                      weightDecayFunction, updateUMatrixAfterEpoch=False):
        self._trainBasicSom(False, data, numberOfEpochs, eta0, etaDecay, sigma0, sigmaDecay, weightDecayFunction,
                            updateUMatrixAfterEpoch)

    def trainBasicSomMasked(self, data, numberOfEpochs, eta0, etaDecay, sigma0, sigmaDecay,
                            weightDecayFunction, updateUMatrixAfterEpoch=False):
        """extension: trainBasicSom over the valid entries of the rows only -- every chunk goes through
        capi.Context.train_online_chunk_masked, so that a missing field neither attracts the search nor steps its column
        of the window's nodes.  The validity of a chunk comes from the data set when it has one (an attribute `validity`,
        loaded rows x J, nonzero = valid), as in trainBatchSomEpochMasked; without one every column is valid.  Driver,
        schedule, sigma clamp at 1.0, running MSE and metrics are trainBasicSom's.  Standard and Median."""
        self._trainBasicSom(True, data, numberOfEpochs, eta0, etaDecay, sigma0, sigmaDecay, weightDecayFunction,
                            updateUMatrixAfterEpoch)

    def _trainBasicSom(self, masked, data, numberOfEpochs, eta0, etaDecay, sigma0, sigmaDecay, weightDecayFunction,
                       updateUMatrixAfterEpoch):
        self.metrics = Metrics(numberOfEpochs)
        for i in range(numberOfEpochs):
            eta = eta0 * math.exp(-etaDecay * float(i))           # :1145
            sigma = sigma0 * math.exp(-sigmaDecay * float(i))     # :1146
            if sigma < 1.0:
                sigma = 1.0                                       # :1148-1149
            mse = np.float32(0.0)
            count = 0
            while not data.hasReadWholeDataStream():
                data.loadNextDataFromStream()
                if masked:
                    self.ctx.upload_chunk(data.data)              # lastBMU zeroed by the load
                else:
                    self._chunkToDevice(data)                     # (custom hooks: with the chunk's validity and the weights)
                # ONE running accumulator over the epoch's chunks (Som.cpp:1153,1167)
                if masked:
                    mse, lb = self.ctx.train_online_chunk_masked(eta, sigma, int(weightDecayFunction),
                                                                 self._chunkValidity(data), first_chunk=(count == 0))
                    data.lastBMU[...] = lb
                else:
                    mse = self.ctx.train_online_chunk(eta, sigma, int(weightDecayFunction), first_chunk=(count == 0))
                    data.lastBMU[...] = self.ctx.get_last_bmu()
                count += 1
            mse = np.float32(mse / np.float32(count))             # :1175
            self.metrics.MeanSquaredError[i] = mse
            data.resetStreamLoadPosition()
            if updateUMatrixAfterEpoch:
                self.updateUMatrix(data.getWeights())             # :751-752 / :1183-1184

    def train(self, data, numberOfEpochs, eta0, etaDecay, sigma0, sigmaDecay, weightDecayFunction,
              updateUMatrixAfterEpoch=False):
        """Som.cpp:1113-1132: dispatch; exceptions are printed to stderr, not raised."""
        self._isTraining = True
        try:
            if int(weightDecayFunction) == WeigthDecayFunction.BatchMap:
                self.trainBatchSom(data, numberOfEpochs, sigma0, sigmaDecay, updateUMatrixAfterEpoch)
            else:
                self.trainBasicSom(data, numberOfEpochs, eta0, etaDecay, sigma0, sigmaDecay,
                                   weightDecayFunction, updateUMatrixAfterEpoch)
        except Exception as e:      # noqa: BLE001  (mirrors the reference's catch-and-print)
            print(e, file=sys.stderr)
        self._isTraining = False
