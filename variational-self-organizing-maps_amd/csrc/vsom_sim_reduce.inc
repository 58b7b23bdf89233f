// vsom_sim_reduce.inc -- the results of one row over the 64 lanes of its wavefront, the closing statements of the row body
// of vsom_sim_row.hpp; included as text inside a kernel, behind the last sim_column.  Expects in scope: `l`, the lane's
// SimLane, and the constant W, the consecutive columns a lane takes per step (the lane that owns column c is (c / W) % 64).
// Defines dc / dmax, ac / amax (UINT32_MAX: no column), first and cnt (`outside`), the same in every lane: a packed
// (ordered value, ~column) key for the two maxima, the lowest column for `first`, a sum for `outside`; the winning value
// itself comes from the lane that owns the winning column.
    const u64 kd = sim_wave_max(l.dmax_c == SIM_NONE ? 0ull : ((u64)sim_ord(l.dmax_v) << 32) | (u64)(~l.dmax_c));
    const u64 ka = sim_wave_max(l.amax_c == SIM_NONE ? 0ull : ((u64)sim_ord(l.amax_v) << 32) | (u64)(~l.amax_c));
    uint32_t fc = l.first_c, cnt = l.outside;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = __shfl_xor(fc, m);
        fc = o < fc ? o : fc;
        cnt += __shfl_xor(cnt, m);
    }
    const uint32_t dc = kd ? ~(uint32_t)kd : SIM_NONE, ac = ka ? ~(uint32_t)ka : SIM_NONE;
    const float dmax = __shfl(l.dmax_v, dc == SIM_NONE ? 0 : (int)((dc / W) & 63));     // (no column: every lane holds -inf)
    const float amax = __shfl(l.amax_v, ac == SIM_NONE ? 0 : (int)((ac / W) & 63));     // (... 0)
    const float first = __shfl(l.first_v, fc == SIM_NONE ? 0 : (int)((fc / W) & 63));   // (... NaN)
