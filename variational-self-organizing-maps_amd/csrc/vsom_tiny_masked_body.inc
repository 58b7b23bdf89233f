// vsom_tiny_masked_body.inc -- the body of the one-workgroup batch epoch over the VALID entries of the chunk
// (vsom_tiny_masked.hip): vsom_tiny_batch_body.inc with the masked distance in phase 1 and a per-column weight sum in
// phase 2.  Included inside a kernel of 256 threads whose `a` is the epoch's TinyMaskedArgs and whose KIND is
// VSOM_STANDARD or VSOM_MEDIAN.  Every piece of the map's state is in LDS and `a`: no blockIdx, gridDim or global atomics
// on shared words.  a.valid: the validity bytes as the caller gave them (B x J, or J with a.one; nonzero = valid).
    extern __shared__ __attribute__((aligned(16))) unsigned char tinym_smem[];
    u64 *keys = reinterpret_cast<u64 *>(tinym_smem);         // [B]
    int2 *bxy = reinterpret_cast<int2 *>(keys + a.B);        // [B]
    float *sq = reinterpret_cast<float *>(bxy + a.B);        // [B]
    int *nan0 = reinterpret_cast<int *>(sq + a.B);           // [B]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int B = a.B, N = a.N, J = a.Dc;
    const size_t vld = a.one ? 0 : (size_t)J;                // the validity row of sample s: a.valid + s * vld

    // ---- phase 1 (Som.cpp:762-806) on the masked distance -------------------------------------------
    if (a.is_first) {
        for (int s = tid; s < B; s += 256) {
            keys[s] = ~0ull;
            nan0[s] = 0;
        }
        __syncthreads();
        const int grp = tid >> 3, k = tid & 7;
        for (int p = grp; p < B * N; p += 32) {
            const int s = p / N, n = p - s * N;
            const float dd = masked_group_dist(a.d.xa + (size_t)s * a.d.ldx, a.valid + (size_t)s * vld,
                                               a.d.ma + (size_t)n * a.d.ldm, a.d.L, k);
            if (k == 0) {
                if (n == 0 && dd != dd)
                    nan0[s] = 1;                 // a NaN at node 0 pins the BMU to 0 (Som.cpp:293-299)
                atomicMin(&keys[s], vsom_key(dd, (uint32_t)n));
            }
        }
        __syncthreads();
        for (int s = tid; s < B; s += 256) {
            const u64 key = keys[s];
            a.lastbmu[s] = nan0[s] ? 0ull : (key & 0xFFFFFFFFull);
            sq[s] = nan0[s] ? __uint_as_float(0x7FC00000u) : __uint_as_float((uint32_t)(key >> 32));
        }
    } else {
        for (int s = wave; s < B; s += 4) {
            const float *x = a.d.xa + (size_t)s * a.d.ldx;
            const unsigned char *v = a.valid + (size_t)s * vld;
            u64 idx;
            float dist;
            vsom_local_walk_with(
                [&](u64 node, int k) { return masked_group_dist(x, v, a.d.ma + (size_t)node * a.d.ldm, a.d.L, k); },
                (u64)a.W, (u64)a.H, a.lastbmu[s], lane, idx, dist);
            if (lane == 0) {
                a.lastbmu[s] = idx;
                sq[s] = dist;
            }
        }
    }
    __syncthreads();
    for (int s = tid; s < B; s += 256) {
        const u64 idx = a.lastbmu[s];
        int bx, by;
        vsom_somindex(idx, (u64)a.W, (u64)a.H, bx, by);      // SomIndex(*this, lastBMU) :847-849
        bxy[s] = make_int2(bx, by);
        a.sqres[s] = sq[s];
        atomicAdd(&a.hits[idx], 1ull);                       // bmuHits[index] += 1 :778,801
    }
    if (tid == 0) {                                          // MSE in sample order :781,804
        const float fB = (float)B;
        float run = 0.f;
        for (int s = 0; s < B; ++s)
            run = run + sq[s] / fB;
        *a.mse = run;
    }
    __syncthreads();

    // ---- phase 2 (Som.cpp:809-876): one thread per (node, column) chain, the old map is not read ------
    // LDS behind the per-sample arrays: the staged rows (when they fit), the neighbourhood table, and the validity as
    // bits -- vb[column][row / 32], row 0 of a word is bit 0; with a.one a single word per column, all ones or zero
    float *xl = reinterpret_cast<float *>(nan0 + B);
    const float *xsrc = a.d.xa;
    int xld = a.d.ldx;
    float *lutl = xl + (a.stage_x ? B * J : 0);
    unsigned *vb = reinterpret_cast<unsigned *>(lutl + a.lutw * a.luth);
    const int nw = a.nw;                                     // words per column: ceil(B / 32), or 1 with a.one
    for (int i = tid; i < a.lutw * a.luth; i += 256)
        lutl[i] = a.lut[i];
    if (a.stage_x) {
        for (int i = tid; i < B * J; i += 256) {
            const int s = i / J, e = i - s * J;
            xl[i] = a.d.xa[(size_t)s * a.d.ldx + e];        // (an invalid position is staged and never used)
        }
        xsrc = xl;
        xld = J;
    }
    for (int i = tid; i < J * nw; i += 256) {
        const int e = i / nw, w = i - e * nw;
        unsigned word = 0;
        if (a.one) {
            word = a.valid[e] ? ~0u : 0u;
        } else {
            const int nt = B - 32 * w < 32 ? B - 32 * w : 32;
            for (int t = 0; t < nt; ++t)
                if (a.valid[(size_t)(32 * w + t) * J + e])
                    word |= 1u << t;
        }
        vb[i] = word;
    }
    __syncthreads();   // table, samples and validity bits in LDS
    for (int c = tid; c < N * J; c += 256) {
        const int node = c / J, e = c - node * J;
        int cx, cy;
        vsom_somindex((u64)node, (u64)a.W, (u64)a.H, cx, cy);
        const unsigned *vbe = vb + e * nw;
        float Wall = 0.f;                                    // sumOfWeights over ALL rows: weightMap
        float Wd = 0.f, M = 0.f, S = 0.f;                    // the column's own weight sum and chains
        for (int s = 0; s < B; ++s) {
            const int2 b = bxy[s];
            int dx = cx - b.x, dy = cy - b.y;
            dx = dx < 0 ? -dx : dx;
            dy = dy < 0 ? -dy : dy;
            const float w = lutl[dy * a.lutw + dx];           // (float)calculateNeighbourhoodWeight :851
            Wall = Wall + w;
            if (!((vbe[a.one ? 0 : s >> 5] >> (s & 31)) & 1u))
                continue;                                    // a row invalid at this column is skipped
            Wd = Wd + w;                                     // :857
            const float cc = w / Wd;                         // :864 (0/0 -> NaN, SURVEY Q7)
            float dl = xsrc[(size_t)s * xld + e] - M;        // Stepper (Transformation.cpp:12 / :50)
            if (KIND == VSOM_MEDIAN)
                dl = tiny_sign(dl);
            const float t = cc * dl;
            M = M + t;                                       // :864
            float u;
            if (KIND == VSOM_MEDIAN) {
                u = w * __builtin_fabsf(dl);                 // = (w * s) * s exactly for s in {-1, +-0, 1, NaN}
            } else {
                u = w * dl;
                u = u * dl;
            }
            S = S + u;                                       // :867
        }
        const size_t row = (size_t)node * a.pitch;
        a.map[row + e] = M;                                  // :870
        a.sigma[row + e] = sqrtf(S / Wd);                    // :873 (a column without a valid row: sqrt(0/0))
        if (e == 0)
            a.weight[node] = Wall;                           // :875
    }
