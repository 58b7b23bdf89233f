// vsom_tiny_online_body.inc -- the body of the one-workgroup online chunk (vsom_online_tiny.hip): included as text inside
// the four kernel templates online_tiny[_masked]_chunk[_many]_kernel<KIND, LOCAL, U>, each of which defines `a` (its kernarg,
// or its workgroup's descriptor) and `constexpr bool MASKED` first.  MASKED: the chunk runs over the VALID entries of the
// rows only -- a validity byte beside every staged value (onl_valid(a): the descriptor's V, ldv, one; constants for the
// plain descriptor, which has none).  Every `if (MASKED)` folds at compile time.  Every piece of the map's state is in LDS,
// registers and `a`: no blockIdx, gridDim or global atomics on shared words.
    extern __shared__ __attribute__((aligned(16))) unsigned char tiny_onl_smem[];
    const int N = a.N, D = a.D, ND = N * D, tid = threadIdx.x, Dp = D | 1;      // (odd row pitch: phase B's rows hit distinct banks)
    // LDS: per-BMU window table, the neighbourhood table (double for :933's division; its two float images for :924-925),
    // the squares, a block of staged rows, the chunk's addBmu counts and lastBMU
    OnlTinyNode *s_win = reinterpret_cast<OnlTinyNode *>(tiny_onl_smem);        // [N]
    double *s_lut = reinterpret_cast<double *>(s_win + N);                      // [W * H]
    float2 *s_lf = reinterpret_cast<float2 *>(s_lut + N);                       // [W * H]  {(float)(h eta), (float)h}
    float *s_p = reinterpret_cast<float *>(s_lf + N);                           // [N Dp] squares of the sample against every node
    float *s_p2 = s_p + N * Dp;                                                 // [2][D]  squares of the BMU's row after its update
    float *s_x = s_p2 + 2 * ((D + 3) & ~3);                                     // [TINY_XBLOCK] staged rows of this block
    unsigned char *s_v = reinterpret_cast<unsigned char *>(s_x + TINY_XBLOCK);  // [TINY_XBLOCK] MASKED only: their validity bytes as
                                                                                //      the caller gave them (one: ONE row of D)
    unsigned *s_hits = reinterpret_cast<unsigned *>(s_v + (MASKED ? TINY_XBLOCK : 0));   // [N]  addBmu counts of this chunk
    float *s_d = reinterpret_cast<float *>(s_hits + N);                         // [N]  LOCAL: the sample's distances
    unsigned short *s_last = reinterpret_cast<unsigned short *>(s_d + N);       // [B]  lastBMU of every sample (a global store
                                                                                //      per sample made its wavefront wait for it)
    __shared__ u64 s_key[2];
    if (LOCAL)                                               // findLocalBmu starts from the sample's BMU of the last epoch (:891)
        for (int i = tid; i < a.B; i += 1024)
            s_last[i] = (unsigned short)a.lastbmu[i];
    for (int i = tid; i < N; i += 1024) {
        const double h = a.lutd[(size_t)(i / a.W) * a.lutw + (i % a.W)];
        s_lut[i] = h;
        s_lf[i] = make_float2((float)(h * a.eta), (float)h);
        s_hits[i] = 0u;
        int bx, by;
        u64 startX, startY, endX, endY;
        online_window((u64)i, a.W, a.H, a.sigma, bx, by, startX, startY, endX, endY);   // (ends <= W, H <= 1024)
        OnlTinyNode t;
        t.bx = (unsigned short)bx;
        t.by = (unsigned short)by;
        t.startX = (unsigned short)startX;
        t.endX = (unsigned short)endX;
        t.startY = (unsigned short)startY;
        t.endY = (unsigned short)endY;
        t.pad0 = t.pad1 = 0;
        s_win[i] = t;
    }
    const auto va = onl_valid(a);
    if (MASKED && va.one)                                    // one validity row for the whole chunk, staged once
        for (int i = tid; i < D; i += 1024)
            s_v[i] = va.V[i];
    const int vstep = va.one ? 0 : D;                        // a sample's validity row within the block
    // this thread's values: flattened (node, dim) indices tid + 1024 u.  stepped = some step of this chunk moved the value.
    // MASKED: wl = the node's weight at the value's last VALID step (online_node_update_masked writes sigmaMap[d] with the twf
    // of the step that stepped column d; later visits with d invalid raise the weight and leave sigmaMap[d])
    float m[U], sv[U], w[U], wl[U];
    int node[U], dim[U], nx[U], ny[U];
    bool own[U], stepped[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int e = tid + 1024 * u;
        own[u] = e < ND;
        node[u] = own[u] ? e / D : 0;
        dim[u] = own[u] ? e - node[u] * D : 0;
        nx[u] = node[u] % a.W;
        ny[u] = node[u] / a.W;
        m[u] = own[u] ? a.map[(size_t)node[u] * a.pitch + dim[u]] : 0.f;
        sv[u] = own[u] ? a.Smap[(size_t)node[u] * a.pitch + dim[u]] : 0.f;
        w[u] = own[u] ? a.weight[node[u]] : 0.f;
        wl[u] = 0.f;
        stepped[u] = false;
    }
    float mse = a.keep_mse ? a.fstate[1] : 0.f, lastdist = 0.f;
    if (tid < 2)
        s_key[tid] = ~0ull;
    const int L8 = D & ~7, rem = D - L8, KB = TINY_XBLOCK / D;
    int pj = -1, pbmu = 0;                                   // the sample whose post step is owed, and its BMU
    // post step of a sample (one thread): the distance of its BMU after the update (:946) from the squares the BMU's threads
    // left in that sample's parity (MASKED: +0 at the invalid columns), the MSE running sum (:1167), addBmu (:1165), lastBMU
    // (:895); re-arms the parity's key
    auto post = [&](int sj, int sbmu) {
        const int ppar = sj & 1;
        const float res = onl_tiny_row_sum(s_p2 + ppar * ((D + 3) & ~3), L8, rem);
        lastdist = res;
        const float q = res / a.fB;                          // residual.squaredNorm() / epochSize  (:1167)
        mse = mse + q;
        atomicAdd(&s_hits[sbmu], 1u);
        s_last[sj] = (unsigned short)sbmu;
        s_key[ppar] = ~0ull;
    };
    const bool exp_decay = a.decay_fn == VSOM_EXPONENTIAL;
    for (int j0 = 0; j0 < a.B; j0 += KB) {
        const int kb = min(KB, a.B - j0);
        if (j0 == 0)
            __syncthreads();                                 // the tables (later blocks: the sample loop's last barrier -- nobody reads the old rows)
        for (int i = tid; i < kb * D; i += 1024) {
            // (row and column of the value in the spelling each flavour's kernels were compiled from: either spelling gives
            //  the other flavour the same values through another instruction schedule)
            if (MASKED) {
                const int r = i / D, d = i - r * D;
                s_x[i] = a.X[(size_t)(j0 + r) * a.ldx + d];
                if (!va.one)                                 // the block's validity bytes, B x J as given
                    s_v[i] = va.V[(size_t)(j0 + r) * va.ldv + d];
            } else {
                s_x[i] = a.X[(size_t)(j0 + i / D) * a.ldx + (i % D)];
            }
        }
        __syncthreads();
        // A (first sample of the block): squares of the sample against every node.  MASKED: a select, never a product -- x at an
        // invalid position may be NaN or +-inf
        float x[U];
        bool vd[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            vd[u] = false;
            if (own[u]) {
                x[u] = s_x[dim[u]];
                const float r = m[u] - x[u];
                const float rr = r * r;
                if (MASKED)
                    vd[u] = s_v[dim[u]] != 0;
                s_p[node[u] * Dp + dim[u]] = (!MASKED || vd[u]) ? rr : 0.f;
            }
        }
        __syncthreads();
        for (int jj = 0; jj < kb; ++jj) {
            const int j = j0 + jj, par = j & 1;
            TINY_STAMP(2);
            // post step of the PREVIOUS sample (distance after the update :946, MSE :1167, addBmu :1165, lastBMU :895) by the last
            // thread, in the shadow of phase B -- its wavefront has nothing to do there on maps of at most 960 nodes.  It reads
            // the previous parity's squares and re-arms that parity's key, which nobody touches before sample j + 1's phase B.
            if (tid == 1023 && pj >= 0)
                post(pj, pbmu);
            // B: distances in Eigen's order, argmin with the reference's rules (strict <, lowest index, NaN never wins,
            //    a NaN at node 0 pins the BMU: Som.cpp:293-304 -- key 0 is below every other key and names node 0)
            if (tid < ((N + 63) & ~63)) {                        // whole wavefronts
                unsigned mybits = 0xFFFFFFFFu;
                if (tid < N) {
                    const float res = onl_tiny_row_sum(s_p + tid * Dp, L8, rem);
                    // (distances are sums of squares: their bit patterns order like their values; NaN -> all ones, never a
                    //  minimum; a NaN at node 0 -> 0, below everything)
                    mybits = (res != res) ? (tid == 0 ? 0u : 0xFFFFFFFFu) : __float_as_uint(res);
                    if (LOCAL)
                        s_d[tid] = res;
                }
                if (!LOCAL) {
                    // the wavefront's minimum, then the LOWEST lane that holds it (strict <: the lowest index wins), one LDS
                    // atomic per wavefront (N same-address atomics serialise: 100 of them were 2 us of a sample)
                    const unsigned wmin = (unsigned)__builtin_amdgcn_readlane((int)onl_wave_min_u32(mybits), 63);
                    const u64 holders = __ballot(mybits == wmin);
                    if ((tid & 63) == 0)
                        atomicMin(&s_key[par], (u64)wmin << 32 | (u64)((tid & ~63) + (__ffsll((long long)holders) - 1)));
                }
            }
            TINY_STAMP(3);
            __syncthreads();
            TINY_STAMP(4);
            if (LOCAL) {                                         // sigma <= 1: the walk from the sample's last BMU (Som.cpp:891)
                if (tid == 1023)
                    s_key[par] = (u64)onl_tiny_walk(s_d, s_win, (unsigned)a.W, (unsigned)a.H, (unsigned)s_last[j]);
                __syncthreads();
            }
            const int bmu = (int)(s_key[par] & 0xFFFFFFFFull);
            // C: the window of Som.cpp:899-944 around the BMU (online_window's bounds, from the table)
            const OnlTinyNode bn = s_win[bmu];
            TINY_STAMP(5);
            const int bx = bn.bx, by = bn.by;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!own[u])
                    continue;
                if (nx[u] < (int)bn.startX || nx[u] >= (int)bn.endX || ny[u] < (int)bn.startY || ny[u] >= (int)bn.endY)
                    continue;
                int dx = nx[u] - bx, dy = ny[u] - by;
                dx = dx < 0 ? -dx : dx;
                dy = dy < 0 ? -dy : dy;
                const int at = dy * a.W + dx;                    // calculateNeighbourhoodWeight(i,j,bx,by,sigma) :915
                // (MASKED: the node's weight and the step's scalars are the unmasked step's whatever the column's validity
                //  -- the weight counts the sample ...)
                const float wold = w[u];
                const float2 lf = s_lf[at];
                const float hf = lf.y;
                float wnew, scM;
                if (exp_decay) {
                    scM = lf.x;                                  // (float)(h eta) :925
                    wnew = wold + scM;                           // :924
                } else {
                    wnew = wold + hf;                            // :930
                    const double tw = wnew == 0 ? 1.0 : s_lut[at] / (double)wnew;   // :933
                    scM = (float)tw;
                }
                w[u] = wnew;
                if (MASKED && !vd[u])
                    continue;                                    // ... and an invalid column is not stepped: m, sv, wl keep their bits
                float dl = x[u] - m[u];                          // Stepper :912
                if (KIND == VSOM_MEDIAN)
                    dl = onl_sign(dl);
                const float tt = scM * dl;
                const float mn = m[u] + tt;                      // :925 / :935
                float dl2 = x[u] - mn;                           // Stepper(v, map_new) :941
                if (KIND == VSOM_MEDIAN)
                    dl2 = onl_sign(dl2);
                const float pr = dl * dl2;
                const float uu = hf * pr;
                sv[u] = sv[u] + uu;                              // :941
                m[u] = mn;
                wl[u] = wnew;
                stepped[u] = true;
            }
            TINY_STAMP(6);
            // D: distance of the BMU after the update (:946), MSE (:1167), addBmu (:1165), lastBMU (:895)
            float *p2 = s_p2 + par * ((D + 3) & ~3);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (own[u] && node[u] == bmu) {
                    const float r = m[u] - x[u];
                    const float rr = r * r;
                    p2[dim[u]] = (!MASKED || vd[u]) ? rr : 0.f;
                }
            TINY_STAMP(7);
            // A of the NEXT sample before the same barrier (its squares go where phase B of this sample, long done, read)
            if (jj + 1 < kb) {
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (own[u]) {
                        x[u] = s_x[(jj + 1) * D + dim[u]];
                        if (MASKED)
                            vd[u] = s_v[(jj + 1) * vstep + dim[u]] != 0;
                        const float r = m[u] - x[u];
                        const float rr = r * r;
                        s_p[node[u] * Dp + dim[u]] = (!MASKED || vd[u]) ? rr : 0.f;
                    }
            }
            TINY_STAMP(8);
            __syncthreads();
            TINY_STAMP(9);
            pj = j;
            pbmu = bmu;
        }
    }
    __syncthreads();
    if (tid == 1023 && pj >= 0)                               // the chunk's last sample
        post(pj, pbmu);
    __syncthreads();
    // state back: M and S of every value, sigmaMap = sqrt(|S / w|) (:939-942) with the final weight where a window touched
    // the node during this chunk; the weight by the node's first value.  MASKED: M, S and sigmaMap only of the values some
    // valid step touched -- the others are not written, so their bits stay (NaN payloads included) -- and sigmaMap with the
    // weight of that last valid step, not the final one
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (!own[u])
            continue;
        const size_t at = (size_t)node[u] * a.pitch + dim[u];
        if (!MASKED || stepped[u]) {
            a.map[at] = m[u];
            a.Smap[at] = sv[u];
        }
        if (stepped[u]) {
            const float wlast = MASKED ? wl[u] : w[u];
            const double tw2 = wlast == 0 ? 0.000001 : (double)wlast;   // :939
            const float twf = (float)tw2;
            a.sigmap[at] = sqrtf(fabsf(sv[u] / twf));                 // :942
        }
        if (dim[u] == 0)
            a.weight[node[u]] = w[u];
    }
    for (int i = tid; i < N; i += 1024)
        if (s_hits[i])
            a.hits[i] += (u64)s_hits[i];
    for (int i = tid; i < a.B; i += 1024)
        a.lastbmu[i] = (u64)s_last[i];
    if (a.lastbmu_host)
        for (int i = tid; i < a.B; i += 1024)
            a.lastbmu_host[i] = (u64)s_last[i];
    if (tid == 1023) {
        a.fstate[0] = lastdist;
        a.fstate[1] = mse;
        *a.mse_out = mse;
    }
