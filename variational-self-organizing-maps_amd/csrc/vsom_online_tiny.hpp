// vsom_online_tiny.hpp -- the descriptors and device helpers of the one-workgroup online chunk, plain and over valid entries
// (vsom_online_tiny.hip, vsom_tiny_online_body.inc).
#pragma once
#include "vsom_online.hpp"

struct OnlTinyArgs {
    const float *X;          // staged rows
    int ldx, B, N, W, H, D, pitch;
    float *map, *Smap, *sigmap, *weight;
    u64 *hits, *lastbmu;
    float *fstate;           // [0] distance of the last sample's BMU, [1] MSE running sum (in/out)
    const double *lutd;
    int lutw;
    double eta, sigma;
    int decay_fn;
    float fB;
    int keep_mse;            // 0: first chunk of an epoch, the running MSE starts at 0 (online_init_kernel's argument)
    float *mse_out;          // vsom_get_mse's value
    u64 *lastbmu_host;       // pinned host copy of lastBMU (vsom_train_online_chunk_fetch), or NULL
};

// OnlTinyArgs and the validity bytes (a descriptor of its own: the stride of OnlTinyArgs stays)
struct OnlTinyMaskedArgs : OnlTinyArgs {
    const unsigned char *V;  // validity bytes on the device: B rows of ldv bytes, or one row (one != 0)
    int ldv, one;
};

// the validity fields as the chunk body reads them: the masked descriptor's own, constants for the plain one (which the
// body never reads: every use is behind its compile-time MASKED)
struct OnlNoValid {
    static constexpr const unsigned char *V = nullptr;
    static constexpr int ldv = 0, one = 1;
};
__device__ __forceinline__ OnlNoValid onl_valid(const OnlTinyArgs &) { return {}; }
__device__ __forceinline__ const OnlTinyMaskedArgs &onl_valid(const OnlTinyMaskedArgs &a) { return a; }

constexpr int TINY_XBLOCK = 2048;      // values of staged rows held in LDS at a time (TINY_XBLOCK / D samples)

// minimum of a u64 over the wavefront, in lane 63: four row shifts, two row broadcasts (DPP moves of both halves; the
// cross-lane LDS permutes of a shuffle ladder were a third of a tiny-map sample)
__device__ __forceinline__ u64 onl_wave_min_u64(u64 v)
{
#define ONL_DPP_STEP(CTRL, ROWS)                                                                                         \
    {                                                                                                                    \
        const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(-1, (int)(unsigned)v, CTRL, ROWS, 0xF, false);         \
        const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(-1, (int)(unsigned)(v >> 32), CTRL, ROWS, 0xF, false); \
        const u64 o = (u64)hi << 32 | lo;                                                                                \
        v = o < v ? o : v;                                                                                               \
    }
    ONL_DPP_STEP(0x111, 0xF)   // row_shr:1
    ONL_DPP_STEP(0x112, 0xF)   // row_shr:2
    ONL_DPP_STEP(0x114, 0xF)   // row_shr:4
    ONL_DPP_STEP(0x118, 0xF)   // row_shr:8   (lane 15 of every row: the row's minimum)
    ONL_DPP_STEP(0x142, 0xA)   // row_bcast:15 into rows 1 and 3
    ONL_DPP_STEP(0x143, 0xC)   // row_bcast:31 into rows 2 and 3
#undef ONL_DPP_STEP
    return v;
}

// minimum of a u32 over the wavefront, in lane 63 (same ladder, one v_min_u32 with a DPP operand per step)
__device__ __forceinline__ unsigned onl_wave_min_u32(unsigned v)
{
#define ONL_DPP_STEP32(CTRL, ROWS)                                                                  \
    {                                                                                               \
        const unsigned o = (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, CTRL, ROWS, 0xF, false); \
        v = o < v ? o : v;                                                                          \
    }
    ONL_DPP_STEP32(0x111, 0xF)
    ONL_DPP_STEP32(0x112, 0xF)
    ONL_DPP_STEP32(0x114, 0xF)
    ONL_DPP_STEP32(0x118, 0xF)
    ONL_DPP_STEP32(0x142, 0xA)
    ONL_DPP_STEP32(0x143, 0xC)
#undef ONL_DPP_STEP32
    return v;
}

struct OnlTinyNode {           // what a thread needs to know about the sample's BMU: its coordinates and window (Som.cpp:899-907)
    unsigned short bx, by, startX, endX, startY, endY, pad0, pad1;
};

// Som::findLocalBmu (Som.cpp:335-454) over a table of the sample's distances to every node, by one thread: vsom_local_walk's
// steps and comparisons in its order (the 8 neighbours of the first try, then 3 nodes ahead while moving in X; the size_t
// wrap-then-clamp of :362-385 in 32 bits -- a wrapped coordinate is far above width - 1 either way)
__device__ __forceinline__ int onl_tiny_walk(const float *s_d, const OnlTinyNode *s_win, unsigned W, unsigned H, unsigned start)
{
    // (the coordinates of lastMeasured / lastBMU / the running minimum travel in registers: every candidate is built from its
    //  coordinates, so a step is ONE LDS round trip -- the candidates' distances, requested together, compared in order)
    unsigned lastBMU = start, minIndex = start, lastMeasured = start;
    unsigned lmX = s_win[start].bx, lmY = s_win[start].by, lbX = lmX, minX = lmX, minY = lmY;
    float minDist = s_d[start];
    for (;;) {
        if (lastMeasured == lastBMU) {
            unsigned node[8], cxs[8], cys[8];
            float di[8];
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const unsigned fsx = (g == 0 || g >= 6) ? ~0u : ((g == 1 || g == 5) ? 0u : 1u);   // firstSearchX / Y (:341-342)
                const unsigned fsy = g <= 2 ? 1u : ((g == 3 || g == 7) ? 0u : ~0u);
                unsigned cx = lmX + fsx, cy = lmY + fsy;
                cx = cx < W - 1 ? cx : W - 1;
                cy = cy < H - 1 ? cy : H - 1;
                cxs[g] = cx;
                cys[g] = cy;
                node[g] = cy * W + cx;
                di[g] = s_d[node[g]];
            }
#pragma unroll
            for (int g = 0; g < 8; ++g)
                if (di[g] < minDist) {
                    minDist = di[g];
                    minIndex = node[g];
                    minX = cxs[g];
                    minY = cys[g];
                }
            if (minIndex == lastBMU)
                break;
            lastMeasured = minIndex;
            lmX = minX;
            lmY = minY;
        } else {
            if (lmX - lbX) {                                     // moving in X: 3 nodes ahead (:390-403)
                unsigned cx = lmX + lmX - lbX;
                cx = cx < W - 1 ? cx : W - 1;
                unsigned node[3], cys[3];
                float di[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    unsigned cy = lmY + (unsigned)(i - 1);
                    cy = cy < H - 1 ? cy : H - 1;
                    cys[i] = cy;
                    node[i] = cy * W + cx;
                    di[i] = s_d[node[i]];
                }
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    if (di[i] < minDist) {
                        minDist = di[i];
                        minIndex = node[i];
                        minX = cx;
                        minY = cys[i];
                    }
            }
            // (moving in Y evaluates nothing: :406-437, vsom_local_walk)
            if (minIndex == lastMeasured)
                break;
            lastBMU = lastMeasured;
            lbX = lmX;
            lastMeasured = minIndex;
            lmX = minX;
            lmY = minY;
        }
    }
    return (int)minIndex;
}

// a row of squares added in Eigen's order: the eight accumulator classes, the packet tree, the scalar tail (vsom_group_dist's
// arithmetic by one thread)
__device__ __forceinline__ float onl_tiny_row_sum(const float *p, int L8, int rem)
{
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int d = 0; d < L8; d += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            acc[k] = acc[k] + p[d + k];
    }
    float q0 = acc[0] + acc[4], q1 = acc[1] + acc[5], q2 = acc[2] + acc[6], q3 = acc[3] + acc[7];
    int t = 0;
    if (rem >= 4) {
        q0 = q0 + p[L8];
        q1 = q1 + p[L8 + 1];
        q2 = q2 + p[L8 + 2];
        q3 = q3 + p[L8 + 3];
        t = 4;
    }
    const float t02 = q0 + q2, t13 = q1 + q3;
    float res = t02 + t13;
    for (; t < rem; ++t)
        res = res + p[L8 + t];
    return res;
}
