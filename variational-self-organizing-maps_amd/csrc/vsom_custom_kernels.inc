// vsom_custom_kernels.inc -- device side of the caller-defined Transformation (vsom_create_custom).
//
// This text is compiled by hipRTC together with the caller's hook source, which defines
//   __device__ float vsom_compare(uint32_t r, const float *x, const float *model, const float *dispersion,
//                                 const float *value_weight, uint32_t J, uint32_t D);
//   __device__ float vsom_step(uint32_t d, const float *x, const float *model, const float *value_weight,
//                              uint32_t J, uint32_t D);
// Every kernel reproduces one loop of host/src/vsom_custom.cpp with the same fp32 operations (the module is built
// with -ffp-contract=off and correctly rounded division / square root), so a hook that computes what a host hook
// computes gives the same bits.  Neighbourhood weights come from host-built tables (glibc's exp, like the host).
//
// value_weight: every kernel that hands the hooks a value_weight row takes `vw` with a row stride `vws` (in floats); the
// row of sample s is vw + s * vws, and stride 0 is one shared [J] vector.  vsom_custom.hip passes what Som.cpp builds at
// that call: valid .* weights for the searches and the online step, valid alone for the batch residual and phase 2.
// The kernels with one thread per sample branch on the stride once: with stride 0 the pointer stays uniform over the
// wavefront, so the hooks' reads of value_weight stay scalar loads, as they were before the stride existed.
R"VSOMRTC(
typedef unsigned long long vc_u64;

// r.dot(r) in Eigen 3.4's SSE packet order (vsom_custom.cpp, packet_order_square_sum); sq(i) yields element i squared
template <class F>
__device__ float vc_packet_sum(uint32_t n, F sq)
{
    if (n == 0)
        return 0.f;
    const uint32_t whole = n & ~3u, pairs = n & ~7u;
    if (whole == 0) {
        float s = sq(0);
        for (uint32_t i = 1; i < n; ++i)
            s = s + sq(i);
        return s;
    }
    float l0[4], l1[4];
    for (uint32_t k = 0; k < 4; ++k)
        l0[k] = sq(k);
    if (whole > 4) {
        for (uint32_t k = 0; k < 4; ++k)
            l1[k] = sq(4 + k);
        for (uint32_t base = 8; base < pairs; base += 8) {
            for (uint32_t k = 0; k < 4; ++k)
                l0[k] = l0[k] + sq(base + k);
            for (uint32_t k = 0; k < 4; ++k)
                l1[k] = l1[k] + sq(base + 4 + k);
        }
        for (uint32_t k = 0; k < 4; ++k)
            l0[k] = l0[k] + l1[k];
        if (whole > pairs)
            for (uint32_t k = 0; k < 4; ++k)
                l0[k] = l0[k] + sq(pairs + k);
    }
    float s = (l0[0] + l0[2]) + (l0[1] + l0[3]);
    for (uint32_t i = whole; i < n; ++i)
        s = s + sq(i);
    return s;
}

// ||Comparer(x, model, disp, vw)||^2
__device__ float vc_sqnorm(const float *x, const float *model, const float *disp, const float *vw, uint32_t J, uint32_t D,
                           uint32_t R)
{
    return vc_packet_sum(R, [&](uint32_t r) {
        const float c = vsom_compare(r, x, model, disp, vw, J, D);
        return c * c;
    });
}

// Som::euclidianWeightedDist (hostDist): sigf holds the floored sigmaMap, select(sigma < 1e-5, 1e-5, sigma)
struct VcDist {
    const float *map, *sigf, *vw;      // vw: the value_weight row of the sample the distances are taken for
    uint32_t J, D, R;
    __device__ float operator()(vc_u64 node, const float *x) const
    {
        return vc_sqnorm(x, map + node * D, sigf + node * D, vw, J, D, R);
    }
};

// validity bytes and column weights -> the two value_weight arrays: valid as 0.0f / 1.0f, and valid * weights (one fp32
// product per element).  bytes == null: all valid; weights == null: all 1.  n = rows * J elements; the column of element
// i is i % J (a column mask or weights alone are one row).
extern "C" __global__ void vc_expand_validity(const unsigned char *__restrict__ bytes, const float *__restrict__ weights,
    float *__restrict__ valid, float *__restrict__ vw, vc_u64 n, uint32_t J)
{
    const vc_u64 i = (vc_u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const float v = (bytes == nullptr || bytes[i] != 0) ? 1.f : 0.f;
    const float w = weights ? weights[i % J] : 1.f;
    valid[i] = v;
    vw[i] = v * w;
}

extern "C" __global__ void vc_floor_sigma(const float *__restrict__ sigma, float *__restrict__ sigf, vc_u64 n)
{
    const vc_u64 i = (vc_u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const float s = sigma[i];
        sigf[i] = s < 0.00001f ? 0.00001f : s;
    }
}

// hostFindBmu for sample row blockIdx.x: node 0 first, strict '<', lowest index wins ties, NaN never wins (and a NaN
// distance of node 0 keeps node 0).  One workgroup of 256 per sample; dist_out = the BMU's distance.
extern "C" __global__ __launch_bounds__(256) void vc_search_full(const float *X, vc_u64 xstride, const float *map,
    const float *sigf, const float *vw, vc_u64 vws, uint32_t N, uint32_t J, uint32_t D, uint32_t R, vc_u64 *bmu_out,
    float *dist_out)
{
    __shared__ float sd[256];
    __shared__ uint32_t si[256];
    __shared__ float d0s;
    const VcDist dist{map, sigf, vw + (vc_u64)blockIdx.x * vws, J, D, R};
    const float *x = X + (vc_u64)blockIdx.x * xstride;
    const uint32_t t = threadIdx.x;
    float best = __builtin_inff();
    uint32_t bi = 0xFFFFFFFFu;
    for (uint32_t n = t; n < N; n += 256) {
        const float d = dist(n, x);
        if (n == 0)
            d0s = d;
        if (d < best) {
            best = d;
            bi = n;
        }
    }
    sd[t] = best;
    si[t] = bi;
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
        if (t < s) {
            const float od = sd[t + s];
            const uint32_t oi = si[t + s];
            if (od < sd[t] || (od == sd[t] && oi < si[t])) {
                sd[t] = od;
                si[t] = oi;
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        const float d0 = d0s;
        const bool keep0 = (d0 != d0) || si[0] == 0xFFFFFFFFu;
        bmu_out[blockIdx.x] = keep0 ? 0 : si[0];
        dist_out[blockIdx.x] = keep0 ? d0 : sd[0];
    }
}

// hostFindLocalBmu: size_t coordinates, wrap-then-clamp neighbours, the same walk
__device__ vc_u64 vc_local_walk(const VcDist &dist, const float *x, vc_u64 width, vc_u64 height, vc_u64 start, float &bestOut)
{
    const vc_u64 M = ~0ull;
    const vc_u64 stepX[8] = {M, 0, 1, 1, 1, 0, M, M};
    const vc_u64 stepY[8] = {1, 1, 1, 0, M, M, M, 0};
    vc_u64 anchor = start, probe = start, best = start;
    float bestDist = dist(start, x);
    auto clampTo = [](vc_u64 v, vc_u64 last) { return v < last ? v : last; };
    auto consider = [&](vc_u64 cx, vc_u64 cy) {
        const vc_u64 node = cy * width + cx;
        const float d = dist(node, x);
        if (d < bestDist) {
            bestDist = d;
            best = node;
        }
    };
    for (;;) {
        const vc_u64 px = probe % width, py = probe / width, ax = anchor % width;
        if (probe == anchor) {
            for (int i = 0; i < 8; ++i)
                consider(clampTo(px + stepX[i], width - 1), clampTo(py + stepY[i], height - 1));
            if (best == anchor)
                break;
            probe = best;
        } else {
            if (px - ax) {
                const vc_u64 cx = clampTo(px + px - ax, width - 1);
                for (int i = -1; i < 2; ++i)
                    consider(cx, clampTo(py + (vc_u64)(long long)i, height - 1));
            }
            if (best == probe)
                break;
            anchor = probe;
            probe = best;
        }
    }
    bestOut = bestDist;
    return best;
}

// one thread per sample: start[s] -> bmu_out[s] (may be the same array), dist_out[s] = the BMU's distance
extern "C" __global__ void vc_search_local(const float *X, vc_u64 xstride, const float *map, const float *sigf,
    const float *vw, vc_u64 vws, uint32_t W, uint32_t H, uint32_t J, uint32_t D, uint32_t R, const vc_u64 *start,
    vc_u64 *bmu_out, float *dist_out, uint32_t B)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= B)
        return;
    const float *x = X + (vc_u64)s * xstride;
    float d = 0.f;
    const vc_u64 b = vws == 0 ? vc_local_walk(VcDist{map, sigf, vw, J, D, R}, x, W, H, start[s], d)
                              : vc_local_walk(VcDist{map, sigf, vw + (vc_u64)s * vws, J, D, R}, x, W, H, start[s], d);
    bmu_out[s] = b;
    dist_out[s] = d;
}

// euclidianWeightedDist for `count` (node, row) pairs
extern "C" __global__ void vc_pair_dist(const float *X, vc_u64 xstride, const float *map, const float *sigf,
    const float *vw, vc_u64 vws, uint32_t J, uint32_t D, uint32_t R, const vc_u64 *nodes, const vc_u64 *rows,
    vc_u64 count, float *out)
{
    const vc_u64 i = (vc_u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count)
        return;
    const float *x = X + rows[i] * xstride;
    out[i] = vws == 0 ? VcDist{map, sigf, vw, J, D, R}(nodes[i], x) : VcDist{map, sigf, vw + rows[i] * vws, J, D, R}(nodes[i], x);
}

// hostBatchEpoch phase 1 tail: ||Comparer(x, M[bmu], S[bmu], valid)||^2 per sample (the residual takes SMap rows)
extern "C" __global__ void vc_batch_residual(const float *X, vc_u64 xstride, const float *map, const float *S,
    const float *vw, vc_u64 vws, uint32_t J, uint32_t D, uint32_t R, const vc_u64 *bmu, float *sq, uint32_t B)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= B)
        return;
    const vc_u64 b = bmu[s];
    const float *x = X + (vc_u64)s * xstride;
    sq[s] = vws == 0 ? vc_sqnorm(x, map + b * D, S + b * D, vw, J, D, R)
                     : vc_sqnorm(x, map + b * D, S + b * D, vw + (vc_u64)s * vws, J, D, R);
}

// bmuHits += 1 and the fp32 MSE summed in sample order (one thread: the order is the result)
extern "C" __global__ void vc_batch_finish(const vc_u64 *bmu, const float *sq, uint32_t B, vc_u64 *hits, float *mse)
{
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    float m = 0.f;
    for (uint32_t s = 0; s < B; ++s) {
        hits[bmu[s]] += 1;
        m += sq[s] / (float)B;
    }
    *mse = m;
}

// hostBatchEpoch phase 2: one workgroup per node, the running model, the step and the spread in LDS (3 x D floats).
// lut[dy * lutw + dx] = (float)calculateNeighbourhoodWeight(dx, dy, 0, 0, sigma); SomIndex's y divides by HEIGHT.
extern "C" __global__ __launch_bounds__(256) void vc_batch_phase2(const float *X, vc_u64 xstride, float *map,
    float *sigma, float *sigf, float *weight, const vc_u64 *bmu, const float *lut, uint32_t lutw, uint32_t W, uint32_t H,
    uint32_t B, const float *vw, vc_u64 vws, uint32_t J, uint32_t D)
{
    extern __shared__ float lds[];
    float *model = lds, *delta = lds + D, *spread = lds + 2 * D;
    const vc_u64 node = blockIdx.x;
    const uint32_t t = threadIdx.x;
    const vc_u64 hx = node % W, hy = (node - hx) / H;
    for (uint32_t d = t; d < D; d += blockDim.x) {
        model[d] = 0.f;
        spread[d] = 0.f;
    }
    __syncthreads();
    float total = 0.f;
    for (uint32_t j = 0; j < B; ++j) {
        const vc_u64 b = bmu[j], bx = b % W, by = (b - bx) / H;
        const vc_u64 dx = hx > bx ? hx - bx : bx - hx, dy = hy > by ? hy - by : by - hy;
        const float w = lut[dy * lutw + dx];
        total += w;
        const float *x = X + (vc_u64)j * xstride;
        for (uint32_t d = t; d < D; d += blockDim.x)
            delta[d] = vsom_step(d, x, model, vw + (vc_u64)j * vws, J, D);
        __syncthreads();
        const float c = w / total;
        for (uint32_t d = t; d < D; d += blockDim.x) {
            const float step = c * delta[d];
            const float sq = (w * delta[d]) * delta[d];   // the reference's second Stepper call is the same delta
            model[d] = model[d] + step;
            spread[d] = spread[d] + sq;
        }
        __syncthreads();
    }
    for (uint32_t d = t; d < D; d += blockDim.x) {
        const float s = sqrtf(spread[d] / total);
        map[node * D + d] = model[d];
        sigma[node * D + d] = s;
        sigf[node * D + d] = s < 0.00001f ? 0.00001f : s;
    }
    if (t == 0)
        weight[node] = total;
}

// hostTrainSingle's window update: one workgroup per node of an nx x ny box that covers the +-2.5 sigma window around
// *bmu; nodes outside the window leave at once.  lutd[dy * W + dx] = calculateNeighbourhoodWeight(dx, dy, 0, 0, sigma).
extern "C" __global__ __launch_bounds__(256) void vc_online_update(const float *v, float *map, float *S, float *sigma,
    float *sigf, float *weight, const vc_u64 *bmu, const double *lutd, uint32_t W, uint32_t H, const float *vw,
    vc_u64 vws, vc_u64 row, uint32_t J, uint32_t D, double eta, double sig, int decay_fn, uint32_t nx)
{
    extern __shared__ float lds[];
    float *model = lds, *delta = lds + D;
    vw += row * vws;                      // the value_weight row of sample `row`
    const vc_u64 b = *bmu, bx = b % W, by = b / W;
    const vc_u64 x0 = (vc_u64)fmax((double)bx - 2.5 * sig, 0.), y0 = (vc_u64)fmax((double)by - 2.5 * sig, 0.);
    const vc_u64 x1 = (vc_u64)fmin((double)bx + 2.5 * sig, (double)W), y1 = (vc_u64)fmin((double)by + 2.5 * sig, (double)H);
    const vc_u64 x = x0 + blockIdx.x % nx, y = y0 + blockIdx.x / nx;
    if (x >= x1 || y >= y1)
        return;
    const vc_u64 n = y * W + x;
    const uint32_t t = threadIdx.x;
    float *M = map + n * D, *Sn = S + n * D, *Sg = sigma + n * D, *Sf = sigf + n * D;
    for (uint32_t d = t; d < D; d += blockDim.x)
        model[d] = M[d];
    const float w0 = weight[n];
    __syncthreads();
    for (uint32_t d = t; d < D; d += blockDim.x)
        delta[d] = vsom_step(d, v, model, vw, J, D);
    __syncthreads();
    const vc_u64 dx = x > bx ? x - bx : bx - x, dy = y > by ? y - by : by - y;
    const double h = lutd[dy * W + dx];
    float wn, k;
    if (decay_fn == 0) {                  // Exponential
        wn = w0 + (float)(h * eta);
        k = (float)(h * eta);
    } else {                              // InverseProportional (the second Stepper call is the same delta)
        wn = w0 + (float)h;
        const double tt = wn == 0 ? 1.0 : h / wn;
        k = (float)tt;
    }
    for (uint32_t d = t; d < D; d += blockDim.x)
        model[d] = model[d] + k * delta[d];
    __syncthreads();
    const double norm = wn == 0 ? 0.000001 : wn;
    const float hf = (float)h, nf = (float)norm;
    for (uint32_t d = t; d < D; d += blockDim.x) {
        const float after = vsom_step(d, v, model, vw, J, D);   // on the updated model
        const float s = Sn[d] + hf * (delta[d] * after);
        const float g = sqrtf(fabsf(s / nf));
        M[d] = model[d];
        Sn[d] = s;
        Sg[d] = g;
        Sf[d] = g < 0.00001f ? 0.00001f : g;
    }
    if (t == 0)
        weight[n] = wn;
}

// hostTrainSingle's tail: the residual Comparer(v, M[bmu], sigmaMap[bmu], vw) (into resid when given), the distance of
// the BMU; hits[bmu] += 1 and mse += ||residual||^2 / B when given (trainBasicSom's loop body)
extern "C" __global__ void vc_online_post(const float *v, const float *map, const float *sigma, const float *sigf,
    const float *vw, vc_u64 vws, vc_u64 row, uint32_t J, uint32_t D, uint32_t R, const vc_u64 *bmu, float *resid,
    float *dist_out, vc_u64 *hits, float *mse, uint32_t B)
{
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    vw += row * vws;                      // the value_weight row of sample `row`
    const vc_u64 b = *bmu;
    const float *M = map + b * D;
    const float sq = vc_packet_sum(R, [&](uint32_t r) {
        const float c = vsom_compare(r, v, M, sigma + b * D, vw, J, D);
        if (resid)
            resid[r] = c;
        return c * c;
    });
    *dist_out = vc_sqnorm(v, M, sigf + b * D, vw, J, D, R);
    if (hits)
        hits[b] += 1;
    if (mse)
        *mse = *mse + sq / (float)B;
}
)VSOMRTC"
