// vsom_eval_row.inc -- one row's binary error by its eight lanes (vsom_eval_row.hpp), included as text.
// In scope at the include: MASKED (constexpr bool); c, this lane's place in the eight (0..7); xr, the row's values; vr, the
// row's validity bytes (plain: may be null); a.binary, a.continuous, a.C; model(d), the unit's value at logical column d.
// Leaves: s, the row's bsum (in lane 0 of the eight), and nrepl, the row's count of replaced terms (in every lane).
    const int C = a.C, a2 = C / 8 * 8;

    auto factor = [&](int d, float &fb, float &val) -> bool {      // false: the column adds +0
        fb = a.binary[d];
        const float fc = a.continuous[d];
        if constexpr (MASKED) {
            val = fc;
            return vr[d] != 0 && !ev_zero(fb, val);
        } else {
            val = (vr && vr[d] == 0) ? 0.0f : fc;
            return !ev_zero(fb, val);
        }
    };

    float acc = 0.f;
    uint32_t nrepl = 0;
    for (int d0 = c; d0 < a2; d0 += 8 * EV_STEPS) {
        float fb[EV_STEPS], val[EV_STEPS], xv[EV_STEPS], mv[EV_STEPS];
        bool on[EV_STEPS];
#pragma unroll
        for (int u = 0; u < EV_STEPS; ++u) {
            const int d = d0 + 8 * u;
            on[u] = d < a2 && factor(d, fb[u], val[u]);
        }
#pragma unroll
        for (int u = 0; u < EV_STEPS; ++u) {
            const int d = d0 + 8 * u;
            if (on[u]) {
                xv[u] = xr[d];
                mv[u] = model(d);
            }
        }
#pragma unroll
        for (int u = 0; u < EV_STEPS; ++u)
            if (on[u])
                acc += ev_square(xv[u], mv[u], fb[u], val[u], nrepl);
    }
    // the one column behind the multiples of 8 that this lane owns: packet tail (C - a2 >= 4: lanes 0..3) or scalar tail
    float q = 0.f;
    {
        const int d = a2 + c;
        float fb, val;
        if (d < C && factor(d, fb, val))
            q = ev_square(xr[d], model(d), fb, val, nrepl);
    }
    const int rest = C - a2;                        // 0..7
    const bool ptail = rest >= 4;
    float s = acc + __shfl_xor(acc, 4);             // p0 += p1 (lanes 0..3)
    if (ptail)
        s += q;                                     // p0 += the packet tail (lanes 0..3)
    s = s + __shfl_xor(s, 2);                       // lane 0: p0[0] + p0[2], lane 1: p0[1] + p0[3]
    s = s + __shfl_xor(s, 1);                       // lane 0: (p0[0] + p0[2]) + (p0[1] + p0[3])
    const int t0 = ptail ? 4 : 0, nt = rest - t0;   // the scalar tail: lanes t0 .. t0 + nt - 1, nt <= 3
    const int base = (int)(threadIdx.x & 63) & ~(EV_LANES - 1);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float qj = __shfl(q, base + t0 + j);
        if (j < nt)
            s += qj;
    }
#pragma unroll
    for (int m = 4; m >= 1; m >>= 1) {
        nrepl += __shfl_xor(nrepl, m);
    }
