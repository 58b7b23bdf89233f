#!/usr/bin/env python3
"""Phase-2 chain kernels, lane = node with FOUR dims (mean-only: EIGHT) per wavefront: x from scalar loads of a transposed chunk,
(c, w) shared by the workgroup through LDS.

Som::trainBatchSomEpoch phase 2 (Som.cpp:840-870), Standard (strict / sigma-contracted / contracted) and
StandardMedianEstimator; per element the same operation sequence as gen_update_asm.py's kernels (same bits).

Decomposition.  lane = node (64 nodes per wavefront) as in gen_update_asm.py, but a wavefront owns ONE column quad
(4 dims = two packed pairs) instead of 14-16 dims, and a workgroup is 8 wavefronts = 8 consecutive quads (32
columns) of the same 64 nodes:
  * 128x128x784 -> 50 176 wavefronts, 64x64x784 -> 12 544, a 2048-node shard 6 272: small equal pieces the
    dispatcher balances over the 1024 SIMDs, six resident per SIMD (~50 VGPRs, 32 KB of LDS per workgroup).
  * x is a wave-uniform operand: the chunk is stored transposed, Xq[quad][sample] = float4 (vsom_xq.hip), so ONE
    s_load_dwordx16 brings the wavefront's four values of FOUR consecutive samples; they feed v_pk_* as SGPR
    operands -- no vector-memory or LDS traffic for x at all.
  * (c, w) is per lane (node): per block of 32 samples the workgroup stages the 16 pair-rows x 64 nodes of
    `cw2` (two 16-byte global loads per thread) into one of two LDS slots, one block ahead in registers; every
    wavefront reads {c_j, w_j, c_j+1, w_j+1} with one ds_read_b128 per sample pair (the LDS array is ~1/6 busy
    against ~1/2 for a lane = (node, quad) decomposition that reads x from LDS as well).  One s_barrier per block.
  * all-zero quads: bit j of zq[quad][j/32] says that the four values of sample j are all +-0; such a step is
    delta = -M, i.e. t = c*M ; u = w*M ; u = u*M ; M = M - t ; S = S + u -- 5 packed operations per pair instead
    of 6, bit-identical (gen_update_asm.py, compute_zero_x).  ~70 % of the (sample, quad) blocks of an MNIST chunk.
    The wavefront branches on a scalar bit per sample.
Scalar loads return out of order, so every wait is lgkmcnt(0): at the top of each group of 4 samples the
wavefront waits for everything it issued one group earlier (x of this group, (c, w) of this group's two pairs),
issues the next group's loads and computes 40-48 packed operations.

Mean-only forms (MEAN below): the chains without the S instructions and the second store, for epochs whose sigmaMap is
produced later by the full kernel (vsom_update.hip, "pending sigma"): 6 packed operations per sample and quad, 4 for a zero quad.
They never read w, so they take the c-only operand array (vsom_update.hip, cwp_kernel<.., true>): one float4
{c_j, c_j+1, c_j+2, c_j+3} per node and sample QUAD at [(j>>2)][node].  Per block of 32 samples the workgroup stages 8 quad-rows
x 64 nodes = 8 KB (ONE 16-byte global load per thread) into one of two 8-KB LDS slots, and a wavefront gets the four c of a
group of 4 samples with ONE ds_read_b128; sample i of the group takes c from half i&1 of register pair i>>1 (op_sel).

Two quads per wavefront (layout K2, the `_nt8` kernels; MEAN modes only -- the launch a deferred epoch runs): without the S half a
one-quad wavefront spends 1.8 scalar instructions and a taken branch per sample on 4.7 packed operations and issues VALU on 0.64
of its cycles.  A wavefront of these kernels owns quads 2k and 2k+1 (M in 8 VGPRs, four independent chains); a workgroup is 4
wavefronts = 256 threads over the same 64 nodes x 8 quads, so grid, XCD mapping and LDS (16 KB) are the `_nt4` kernels', 56
VGPRs, 8 wavefronts per SIMD.  Per group of 4 samples: ONE ds_read_b128 of c serves both quads, x comes from two
s_load_dwordx16 (the two quads' rows of Xq, immediate offsets, the pointers move once per block; two sets of 32 SGPRs at
s36 / s68 -- S_REC and the second row's pointers live in registers the mean-only kernels leave free), staging is two 16-byte
loads and two ds_write_b128 per thread.  Within a sample all four pairs' delta, then all four t, then all four M: dependent
operations are four apart.  Zero form: each quad has its mask word; a sample takes one of FOUR straight-line sequences (zero /
full per quad, the shorter one laid against the END of the longer) behind two scalar bit tests.  The two-form dispatch (zero
form only when both quads are zero; bit-identical too) was built and timed beside it: no difference outside the noise at C3
(1.851 against 1.859 ms, rounds spreading 3 %), four forms 1.5 % faster at C2 in every round -- the only evidence for the choice.  A
wavefront whose quads are both past the live count only stages (as a dead quad does); with one live and one dead quad it
computes both -- the dead one from the padded x rows (Xq / zq hold a multiple of 8 quad rows) -- and stores the live one.

XCD-aware grid: grid.x = 8 * column blocks, grid.y = ceil(node groups / 8) (gen_update_asm.py).

Kernarg (UpdAsmArgs, 80 bytes): Xq, cw2, map, sbuf, Xq row pitch in bytes (16 * padded samples; zq rows are
1/128 of it), ldn_bytes, B, nloc, quads, pitch_bytes, n0, -, live record (or null; word 0 = live columns), zq.
"""
import os

CT = 32                                   # samples per staged (c, w) block
SLOT_XOR = 0x4000                         # (c, w) slots of 16 KB at 0x0000 / 0x4000
LDS_BYTES = 0x8000
SLOT_XOR_C = 0x2000                       # c-only slots of 8 KB at 0x0000 / 0x2000 (the mean-only kernels)
LDS_BYTES_C = 0x4000

S_KARG = "s[0:1]"
S_WGX, S_WGY = "s2", "s3"                 # -> node group, column block
S_XP, S_CP, S_MAP, S_SBUF = (4, 5), (6, 7), (8, 9), (10, 11)
S_LDX, S_LDN, S_B, S_NLOC, S_NQ, S_PITCH, S_N0 = "s12", "s13", "s14", "s15", "s16", "s17", "s18"
S_CNT, S_TAIL, S_TMP, S_TMP2, S_CSTEP, S_Q, S_DEAD = "s19", "s20", "s21", "s22", "s23", "s24", "s25"
S_ZP = (26, 27)
S_Z, S_ZN = "s28", "s29"
S_BIG = "s[30:31]"
S_EXEC = "s[32:33]"
V_TID = 0


class K1:
    """register layout, one column quad per wavefront (the `_nt4` kernels): 8 wavefronts per workgroup"""
    NQ, P, WG = 1, (0, 1), 512
    S_REC = (38, 39)
    XSET = (40, 56)                       # two sets of 16 SGPRs: 4 samples x 4 values
    V_M, V_S, V_D, V_T, V_U = 2, 6, 10, 14, 18
    V_RING = 22                           # 2 sets x 2 pairs x {c, w, c, w}; c-only: 2 sets x {c, c, c, c}
    V_G = 38                              # staging: two 16-byte pieces (c-only: one)
    V_CR, V_CW, V_OC, V_OC2 = 46, 47, 48, 49
    V_K = 50                              # Median: both halves -2^24
    V_A = V_D
    NVGPR = 52

    @staticmethod
    def sx(xs, p):
        return sp(xs, p)


class K2:
    """two column quads per wavefront (the mean-only `_nt8` kernels): 4 wavefronts per workgroup, pairs 0-1 are quad 2k and
    pairs 2-3 quad 2k+1; an x set is 16 SGPRs of the first quad's row, then 16 of the second's"""
    NQ, P, WG = 2, (0, 1, 2, 3), 256
    S_REC = (34, 35)                      # prologue only (the epilogue's carry pair afterwards)
    S_XP2, S_ZP2 = (10, 11), (0, 1)       # second quad's x / mask rows: the mean-only kernels have no sigma buffer, and
    S_Z2, S_ZN2 = "s100", "s101"          # the kernarg pointer is dead once the prologue's loads are back
    XSET = (36, 68)                       # two sets of 32 SGPRs
    V_M, V_D, V_T, V_U = 2, 10, 18, 26
    V_RING = 34                           # 2 sets x {c, c, c, c}, shared by the two quads
    V_G = 42                              # staging: two 16-byte pieces
    V_CR, V_CW, V_OC, V_OC2 = 50, 51, 52, 53
    V_K = 54
    V_A = V_D
    NVGPR = 56

    @staticmethod
    def sx(xs, p):
        b = xs + 16 * (p >> 1) + 2 * (p & 1)
        return f"s[{b}:{b + 1}]"


def vp(base, p):
    return f"v[{base + 2 * p}:{base + 2 * p + 1}]"


def sp(base, p):
    return f"s[{base + 2 * p}:{base + 2 * p + 1}]"


def csrc(mode, cwb, nsrc):
    """(register pair, modifiers) that broadcast c as source 0 of a packed operation of nsrc sources: the low half of
    {c, w} in v[cwb:cwb+1] -- or, for the mean-only kernels, c alone in v[cwb]: either half of the aligned pair it lies in"""
    lo = "op_sel_hi:[0,1,1]" if nsrc == 3 else "op_sel_hi:[0,1]"
    if mode not in MEAN:
        return f"v[{cwb}:{cwb + 1}]", lo
    hi = "op_sel:[1,0,0]" if nsrc == 3 else "op_sel:[1,0]"
    return f"v[{cwb & ~1}:{(cwb & ~1) + 1}]", hi if cwb & 1 else lo


def compute(o, mode, xs, cwb, k=K1, P=None):
    """one sample: x in s[xs:xs+3], {c, w} in v[cwb:cwb+1] -- mean-only: c in v[cwb] -- (Som.cpp:861-867,
    Transformation.cpp:12,50)"""
    cw = f"v[{cwb}:{cwb + 1}]"
    c3, sel3 = csrc(mode, cwb, 3)
    c2, sel2 = csrc(mode, cwb, 2)
    P = P or k.P
    if mode in MED:
        # StandardMedianEstimator, 7 operations per pair -- medmean: the 5 of them that M needs -- (vsom_update.hip,
        # VSOM_MED_STEP): the transposed chunk holds
        # x * 2^24 for a Median context (vsom_xq.hip), and t = fma(M, -2^24, x * 2^24) has exactly the sign of x - M
        # (the scaling is exact, the fused difference rounds once and never to zero; NaN stays NaN);
        # p = clamp(t * 2^127) = [t > 0], n = clamp(-t * 2^127) = [t < 0] (DX10_CLAMP off: NaN passes); the four
        # accumulations are exact-product FMAs that round where the reference's separate multiply and add round.
        for p in P:   # t = M * (-2^24) + x * 2^24
            o.append(f"\tv_pk_fma_f32 {vp(k.V_D, p)}, {vp(k.V_M, p)}, v[{k.V_K}:{k.V_K + 1}], {k.sx(xs, p)}")
        for p in P:   # p = [t > 0]
            o.append(f"\tv_pk_mul_f32 {vp(k.V_T, p)}, {vp(k.V_D, p)}, {S_BIG} clamp")
        for p in P:   # n = [t < 0]
            o.append(f"\tv_pk_mul_f32 {vp(k.V_U, p)}, {vp(k.V_D, p)}, {S_BIG} neg_lo:[1,0] neg_hi:[1,0] clamp")
        for p in P:   # M = M + c*p
            o.append(f"\tv_pk_fma_f32 {vp(k.V_M, p)}, {c3}, {vp(k.V_T, p)}, {vp(k.V_M, p)} {sel3}")
        if mode == "med":
            for p in P:   # S = S + w*p
                o.append(f"\tv_pk_fma_f32 {vp(k.V_S, p)}, {cw}, {vp(k.V_T, p)}, {vp(k.V_S, p)} op_sel:[1,0,0]")
        for p in P:   # M = M - c*n
            o.append(f"\tv_pk_fma_f32 {vp(k.V_M, p)}, {c3}, {vp(k.V_U, p)}, {vp(k.V_M, p)} {sel3} neg_lo:[1,0,0] neg_hi:[1,0,0]")
        if mode == "med":
            for p in P:   # S = S + w*n
                o.append(f"\tv_pk_fma_f32 {vp(k.V_S, p)}, {cw}, {vp(k.V_U, p)}, {vp(k.V_S, p)} op_sel:[1,0,0]")
        return
    for p in P:   # delta = x - M
        o.append(f"\tv_pk_add_f32 {vp(k.V_D, p)}, {k.sx(xs, p)}, {vp(k.V_M, p)} neg_lo:[0,1] neg_hi:[0,1]")
    if mode in ("fma", "meanfma"):
        for p in P:   # M = c*delta + M
            o.append(f"\tv_pk_fma_f32 {vp(k.V_M, p)}, {c3}, {vp(k.V_D, p)}, {vp(k.V_M, p)} {sel3}")
    else:
        for p in P:   # t = c*delta
            o.append(f"\tv_pk_mul_f32 {vp(k.V_T, p)}, {c2}, {vp(k.V_D, p)} {sel2}")
    if mode == "meanfma":
        return
    if mode == "mean":
        for p in P:   # M = M + t                               (Som.cpp:864)
            o.append(f"\tv_pk_add_f32 {vp(k.V_M, p)}, {vp(k.V_M, p)}, {vp(k.V_T, p)}")
        return
    for p in P:       # u = w*delta
        o.append(f"\tv_pk_mul_f32 {vp(k.V_U, p)}, {cw}, {vp(k.V_D, p)} op_sel:[1,0]")
    if mode != "fma":
        for p in P:   # M = M + t                               (Som.cpp:864)
            o.append(f"\tv_pk_add_f32 {vp(k.V_M, p)}, {vp(k.V_M, p)}, {vp(k.V_T, p)}")
    if mode == "std":
        for p in P:   # u = u*delta
            o.append(f"\tv_pk_mul_f32 {vp(k.V_U, p)}, {vp(k.V_U, p)}, {vp(k.V_D, p)}")
        for p in P:   # S = S + u                               (Som.cpp:867)
            o.append(f"\tv_pk_add_f32 {vp(k.V_S, p)}, {vp(k.V_S, p)}, {vp(k.V_U, p)}")
    else:
        for p in P:   # S = u*delta + S
            o.append(f"\tv_pk_fma_f32 {vp(k.V_S, p)}, {vp(k.V_U, p)}, {vp(k.V_D, p)}, {vp(k.V_S, p)}")


def compute_zero(o, mode, cwb, k=K1, P=None):
    """the step of a sample whose four values are all +-0: delta = -M, signs cancel exactly in every product
    (gen_update_asm.py, compute_zero_x)"""
    cw = f"v[{cwb}:{cwb + 1}]"
    P = P or k.P
    if mode == "mean":
        c2, sel2 = csrc(mode, cwb, 2)
        for p in P:   # t = c*M ; M = M - t
            o.append(f"\tv_pk_mul_f32 {vp(k.V_T, p)}, {c2}, {vp(k.V_M, p)} {sel2}")
        for p in P:
            o.append(f"\tv_pk_add_f32 {vp(k.V_M, p)}, {vp(k.V_M, p)}, {vp(k.V_T, p)} neg_lo:[0,1] neg_hi:[0,1]")
        return
    if mode == "meanfma":
        c3, sel3 = csrc(mode, cwb, 3)
        for p in P:   # M = (-c)*M + M
            o.append(f"\tv_pk_fma_f32 {vp(k.V_M, p)}, {c3}, {vp(k.V_M, p)}, {vp(k.V_M, p)} {sel3} neg_lo:[1,0,0] neg_hi:[1,0,0]")
        return
    for p in P:       # u = w*M (M before the step)
        o.append(f"\tv_pk_mul_f32 {vp(k.V_U, p)}, {cw}, {vp(k.V_M, p)} op_sel:[1,0]")
    if mode == "std":
        for p in P:   # t = c*M
            o.append(f"\tv_pk_mul_f32 {vp(k.V_T, p)}, {cw}, {vp(k.V_M, p)} op_sel_hi:[0,1]")
        for p in P:   # u = u*M
            o.append(f"\tv_pk_mul_f32 {vp(k.V_U, p)}, {vp(k.V_U, p)}, {vp(k.V_M, p)}")
        for p in P:   # M = M - t
            o.append(f"\tv_pk_add_f32 {vp(k.V_M, p)}, {vp(k.V_M, p)}, {vp(k.V_T, p)} neg_lo:[0,1] neg_hi:[0,1]")
        for p in P:   # S = S + u
            o.append(f"\tv_pk_add_f32 {vp(k.V_S, p)}, {vp(k.V_S, p)}, {vp(k.V_U, p)}")
        return
    for p in P:       # S = u*M + S
        o.append(f"\tv_pk_fma_f32 {vp(k.V_S, p)}, {vp(k.V_U, p)}, {vp(k.V_M, p)}, {vp(k.V_S, p)}")
    if mode == "sfma":
        for p in P:   # t = c*M ; M = M - t
            o.append(f"\tv_pk_mul_f32 {vp(k.V_T, p)}, {cw}, {vp(k.V_M, p)} op_sel_hi:[0,1]")
        for p in P:
            o.append(f"\tv_pk_add_f32 {vp(k.V_M, p)}, {vp(k.V_M, p)}, {vp(k.V_T, p)} neg_lo:[0,1] neg_hi:[0,1]")
    else:
        for p in P:   # M = (-c)*M + M
            o.append(f"\tv_pk_fma_f32 {vp(k.V_M, p)}, {cw}, {vp(k.V_M, p)}, {vp(k.V_M, p)} op_sel_hi:[0,1,1] neg_lo:[1,0,0] neg_hi:[1,0,0]")


MED = ("med", "medmean")
# the chains without their S half (a deferred sigmaMap, vsom_update.hip): M's own operation sequence -- "mean" is the M
# chain of "std" and of "sfma", "meanfma" that of "fma", "medmean" that of "med" -- the same x loads, zero-quad branch and
# barriers, the c-only operand array staged in half the bytes, and the sigma buffer never written
MEAN = ("mean", "meanfma", "medmean")
_lab = [0]


def merged(k, mode, xs, cwb, zero):
    """one sample of a two-quad wavefront: quad i takes the zero form where zero[i]; the two sequences are laid stage by
    stage (a stage = one operation on each pair of a quad), aligned at their last stage, so dependent operations stay four
    apart"""
    seqs = []
    for i in range(2):
        q = []
        P = k.P[2 * i:2 * i + 2]
        compute_zero(q, mode, cwb, k, P) if zero[i] else compute(q, mode, xs, cwb, k, P)
        seqs.append([q[j:j + 2] for j in range(0, len(q), 2)])
    n = max(len(q) for q in seqs)
    out = []
    for j in range(n):
        for q in seqs:
            if j - (n - len(q)) >= 0:
                out += q[j - (n - len(q))]
    return out


def step(o, mode, xs, cwb, bit, k=K1):
    """one sample, the zero form when bit `bit` of the block's mask word is set.  Two quads per wavefront: each quad has its
    own mask word and takes its own form -- four straight-line sequences, reached with two scalar branches"""
    if mode in MED or os.environ.get("VSOM_GEN_NT_NOZ"):
        return compute(o, mode, xs, cwb, k)
    _lab[0] += 1
    n = _lab[0]
    if k.NQ == 2:
        o.append(f"\ts_bitcmp1_b32 {S_Z}, {bit}")
        o.append(f"\ts_cbranch_scc1 .Lz{n}")
        o.append(f"\ts_bitcmp1_b32 {k.S_Z2}, {bit}")
        o.append(f"\ts_cbranch_scc1 .Lfz{n}")
        o.extend(merged(k, mode, xs, cwb, (False, False)))
        o.append(f"\ts_branch .Le{n}")
        o.append(f".Lfz{n}:")
        o.extend(merged(k, mode, xs, cwb, (False, True)))
        o.append(f"\ts_branch .Le{n}")
        o.append(f".Lz{n}:")
        o.append(f"\ts_bitcmp1_b32 {k.S_Z2}, {bit}")
        o.append(f"\ts_cbranch_scc1 .Lzz{n}")
        o.extend(merged(k, mode, xs, cwb, (True, False)))
        o.append(f"\ts_branch .Le{n}")
        o.append(f".Lzz{n}:")
        o.extend(merged(k, mode, xs, cwb, (True, True)))
        o.append(f".Le{n}:")
        return
    o.append(f"\ts_bitcmp1_b32 {S_Z}, {bit}")
    o.append(f"\ts_cbranch_scc1 .Lz{n}")
    compute(o, mode, xs, cwb, k)
    o.append(f"\ts_branch .Le{n}")
    o.append(f".Lz{n}:")
    compute_zero(o, mode, cwb, k)
    o.append(f".Le{n}:")


def kernel(name, mode, k=K1):
    o = []
    E = o.append
    conly = mode in MEAN                                        # the c-only operand array: 8 quad-rows of 16 B per block
    two = k.NQ == 2                                             # two column quads per wavefront (MEAN modes only)
    assert conly or not two
    slot_xor = SLOT_XOR_C if conly else SLOT_XOR
    S_REC, XSET = k.S_REC, k.XSET
    V_M, V_G, V_CR, V_CW, V_OC, V_OC2, V_K, V_A, V_RING = k.V_M, k.V_G, k.V_CR, k.V_CW, k.V_OC, k.V_OC2, k.V_K, k.V_A, k.V_RING
    pieces2 = two or not conly                                  # two 16-byte staging pieces per thread
    E(f"\t.text\n\t.globl {name}\n\t.p2align 8\n\t.type {name},@function\n{name}:")
    E(f"\ts_load_dwordx8 s[4:11], {S_KARG}, 0x0")              # Xq, cw2, map, sbuf
    E(f"\ts_load_dwordx4 s[12:15], {S_KARG}, 0x20")            # xq row pitch, ldn_bytes, B, nloc
    E(f"\ts_load_dwordx2 s[16:17], {S_KARG}, 0x30")            # quads, pitch_bytes
    E(f"\ts_load_dword {S_N0}, {S_KARG}, 0x38")
    E(f"\ts_load_dwordx2 s[{S_REC[0]}:{S_REC[1]}], {S_KARG}, 0x40")
    E(f"\ts_load_dwordx2 s[{S_ZP[0]}:{S_ZP[1]}], {S_KARG}, 0x48")
    E(f"\ts_and_b32 {S_TMP}, {S_WGX}, 7")                      # XCD label
    E(f"\ts_lshr_b32 {S_TMP2}, {S_WGX}, 3")                    # column block
    E(f"\ts_lshl_b32 {S_WGY}, {S_WGY}, 3")
    E(f"\ts_add_u32 {S_WGX}, {S_WGY}, {S_TMP}")                # node group = wgy*8 + xcd
    E(f"\ts_mov_b32 {S_WGY}, {S_TMP2}")
    E(f"\tv_and_b32_e32 v{V_TID}, 0x3ff, v{V_TID}")
    E(f"\tv_readfirstlane_b32 {S_Q}, v{V_TID}")
    E(f"\ts_lshr_b32 {S_Q}, {S_Q}, 6")                         # wavefront of the workgroup
    if two:
        E(f"\ts_lshl_b32 {S_Q}, {S_Q}, 1")                     # its first quad of the block's eight
    E(f"\ts_lshl_b32 {S_TMP}, {S_WGY}, 3")
    E(f"\ts_add_u32 {S_Q}, {S_Q}, {S_TMP}")                    # this wavefront's (first) column quad
    E(f"\ts_waitcnt lgkmcnt(0)")
    E(f"\ts_cmp_eq_u64 s[{S_REC[0]}:{S_REC[1]}], 0")
    E(f"\ts_cbranch_scc1 .L_nq_{name}")
    E(f"\ts_load_dword {S_NQ}, s[{S_REC[0]}:{S_REC[1]}], 0x0")   # live columns (device value)
    E(f"\ts_waitcnt lgkmcnt(0)")
    E(f"\ts_add_u32 {S_NQ}, {S_NQ}, 3")
    E(f"\ts_lshr_b32 {S_NQ}, {S_NQ}, 2")
    E(f".L_nq_{name}:")
    E(f"\ts_lshl_b32 {S_TMP}, {S_WGY}, 3")                     # the whole column block beyond the quads: leave
    E(f"\ts_cmp_ge_u32 {S_TMP}, {S_NQ}")
    E(f"\ts_cbranch_scc1 .L_end_{name}")
    E(f"\ts_lshl_b32 {S_TMP}, {S_WGX}, 6")                     # first node of the workgroup
    E(f"\ts_cmp_ge_u32 {S_TMP}, {S_NLOC}")
    E(f"\ts_cbranch_scc1 .L_end_{name}")
    E(f"\ts_cmp_ge_u32 {S_Q}, {S_NQ}")                         # a dead quad inside a live block: takes part in the
    E(f"\ts_cselect_b32 {S_DEAD}, 1, 0")                       # staging and the barriers, stores nothing
    # (two quads: dead = both dead; with only the second one dead the wavefront computes both -- the dead quad from the
    #  padded x rows -- and stores the first)
    if mode in MED:
        E(f"\ts_mov_b32 s30, 0x7f000000")                         # 2^127
        E(f"\ts_mov_b32 s31, 0x7f000000")
        E(f"\tv_mov_b32_e32 v{V_K}, 0xcb800000")                  # -2^24
        E(f"\tv_mov_b32_e32 v{V_K + 1}, 0xcb800000")
    # x / mask rows of this quad
    E(f"\ts_mul_i32 {S_TMP}, {S_Q}, {S_LDX}")
    E(f"\ts_mul_hi_u32 {S_TMP2}, {S_Q}, {S_LDX}")
    E(f"\ts_add_u32 s{S_XP[0]}, s{S_XP[0]}, {S_TMP}")
    E(f"\ts_addc_u32 s{S_XP[1]}, s{S_XP[1]}, {S_TMP2}")
    if two:                                                     # (Xq / zq hold a multiple of 8 quad rows: vsom_xq.hip)
        E(f"\ts_add_u32 s{k.S_XP2[0]}, s{S_XP[0]}, {S_LDX}")
        E(f"\ts_addc_u32 s{k.S_XP2[1]}, s{S_XP[1]}, 0")
    E(f"\ts_lshr_b32 {S_TMP}, {S_LDX}, 7")
    if two:
        E(f"\ts_mov_b32 {S_TMP2}, {S_TMP}")
    E(f"\ts_mul_i32 {S_TMP}, {S_TMP}, {S_Q}")
    E(f"\ts_add_u32 s{S_ZP[0]}, s{S_ZP[0]}, {S_TMP}")
    E(f"\ts_addc_u32 s{S_ZP[1]}, s{S_ZP[1]}, 0")
    if two:
        E(f"\ts_add_u32 s{k.S_ZP2[0]}, s{S_ZP[0]}, {S_TMP2}")
        E(f"\ts_addc_u32 s{k.S_ZP2[1]}, s{S_ZP[1]}, 0")
    # (c, w): staging piece of thread t = pair-row t>>6 (+8), node t&63; c-only: quad-row t>>6, node t&63 (two quads per
    # wavefront, 256 threads: quad-rows t>>6 and (t>>6) + 4)
    E(f"\tv_and_b32_e32 v{V_CR}, 63, v{V_TID}")
    E(f"\tv_lshlrev_b32_e32 v{V_CR}, 4, v{V_CR}")              # lane*16: read base (slot 0)
    E(f"\tv_lshlrev_b32_e32 v{V_CW}, 4, v{V_TID}")             # write: tid*16 (+8192; two quads: +4096)
    E(f"\tv_lshrrev_b32_e32 v{V_OC}, 6, v{V_TID}")
    E(f"\tv_mul_lo_u32 v{V_OC}, v{V_OC}, {S_LDN}")
    E(f"\tv_add_u32_e32 v{V_OC}, v{V_OC}, v{V_CR}")
    if pieces2:
        E(f"\ts_lshl_b32 {S_TMP}, {S_LDN}, {2 if two else 3}")
        E(f"\tv_add_u32_e32 v{V_OC2}, {S_TMP}, v{V_OC}")
    E(f"\ts_lshl_b32 {S_TMP}, {S_WGX}, 10")                    # node group * 64 nodes * 16 B
    if os.environ.get("VSOM_GEN_NT_CWL2"):                      # development, timing only (WRONG results): every workgroup
        E(f"\ts_and_b32 {S_TMP}, {S_TMP}, 0x400")                # stages node group 0 / 1's (c, w): 8 MB, L2-resident
    E(f"\ts_add_u32 s{S_CP[0]}, s{S_CP[0]}, {S_TMP}")
    E(f"\ts_addc_u32 s{S_CP[1]}, s{S_CP[1]}, 0")
    E(f"\ts_lshl_b32 {S_CSTEP}, {S_LDN}, {3 if conly else 4}")  # 16 pair-rows / 8 quad-rows
    for r in range(V_M, V_M + 8):                               # currentModel / currentModelSigma .setZero() :843-844
        E(f"\tv_mov_b32_e32 v{r}, 0")
    E(f"\ts_cmp_eq_u32 {S_B}, 0")
    E(f"\ts_cbranch_scc1 .L_store_{name}")
    E(f"\ts_add_u32 {S_CNT}, {S_B}, {CT - 1}")
    E(f"\ts_lshr_b32 {S_CNT}, {S_CNT}, 5")
    E(f"\ts_sub_u32 {S_CNT}, {S_CNT}, 1")                      # full blocks before the last one
    E(f"\ts_lshl_b32 {S_TMP}, {S_CNT}, 5")
    E(f"\ts_sub_u32 {S_TAIL}, {S_B}, {S_TMP}")                 # samples of the last block: 1..32

    def gload():
        E(f"\tglobal_load_dwordx4 v[{V_G}:{V_G + 3}], v{V_OC}, s[{S_CP[0]}:{S_CP[1]}]")
        if pieces2:
            E(f"\tglobal_load_dwordx4 v[{V_G + 4}:{V_G + 7}], v{V_OC2}, s[{S_CP[0]}:{S_CP[1]}]")
        E(f"\ts_add_u32 s{S_CP[0]}, s{S_CP[0]}, {S_CSTEP}")
        E(f"\ts_addc_u32 s{S_CP[1]}, s{S_CP[1]}, 0")

    def lwrite():
        E(f"\tds_write_b128 v{V_CW}, v[{V_G}:{V_G + 3}]")
        if pieces2:
            E(f"\tds_write_b128 v{V_CW}, v[{V_G + 4}:{V_G + 7}] offset:{4096 if two else 8192}")

    def xload(st, g):
        """x of group g of the block the x pointers stand at (g = 8: the next block's first) -> SGPR set st"""
        if two:     # immediate offsets; the pointers move once per block (xbump)
            E(f"\ts_load_dwordx16 s[{st}:{st + 15}], s[{S_XP[0]}:{S_XP[1]}], {hex(64 * g)}")
            E(f"\ts_load_dwordx16 s[{st + 16}:{st + 31}], s[{k.S_XP2[0]}:{k.S_XP2[1]}], {hex(64 * g)}")
            return
        E(f"\ts_load_dwordx16 s[{st}:{st + 15}], s[{S_XP[0]}:{S_XP[1]}], 0x0")
        E(f"\ts_add_u32 s{S_XP[0]}, s{S_XP[0]}, 64")
        E(f"\ts_addc_u32 s{S_XP[1]}, s{S_XP[1]}, 0")

    def zload(dst, dst2):
        """the next mask word of each quad"""
        ptrs = ((S_ZP, dst), (k.S_ZP2, dst2)) if two else ((S_ZP, dst),)
        for ptr, d in ptrs:
            E(f"\ts_load_dword {d}, s[{ptr[0]}:{ptr[1]}], 0x0")
            E(f"\ts_add_u32 s{ptr[0]}, s{ptr[0]}, 4")
            E(f"\ts_addc_u32 s{ptr[1]}, s{ptr[1]}, 0")

    def cread(ring, g):
        """{c, w} of the two sample pairs of group g -> ring set `ring`; c-only: the four c of group g"""
        if conly:
            r = V_RING + 4 * ring
            E(f"\tds_read_b128 v[{r}:{r + 3}], v{V_CR} offset:{1024 * g}")
            return
        r = V_RING + 8 * ring
        E(f"\tds_read_b128 v[{r}:{r + 3}], v{V_CR} offset:{1024 * (2 * g)}")
        E(f"\tds_read_b128 v[{r + 4}:{r + 7}], v{V_CR} offset:{1024 * (2 * g + 1)}")

    # ---- prologue: (c, w) block 0 -> slot 0, block 1 -> registers; x of group 0; mask word 0 ------
    gload()
    xload(XSET[0], 0)
    zload(S_Z, k.S_Z2 if two else None)
    E(f"\ts_mov_b32 {S_ZN}, 0")
    if two:
        E(f"\ts_mov_b32 {k.S_ZN2}, 0")
    E(f"\ts_waitcnt vmcnt(0)")
    lwrite()
    E(f"\tv_xor_b32_e32 v{V_CW}, {slot_xor}, v{V_CW}")
    E(f"\ts_waitcnt lgkmcnt(0)")
    E(f"\ts_cmp_eq_u32 {S_CNT}, 0")
    E(f"\ts_cbranch_scc1 .L_p1_{name}")
    gload()
    E(f".L_p1_{name}:")
    E(f"\ts_barrier")
    cread(0, 0)
    E(f"\ts_cmp_eq_u32 {S_CNT}, 0")
    E(f"\ts_cbranch_scc1 .L_last_{name}")
    # ---- main loop: one full block of 32 samples per iteration -----------------------------------
    E(f"\t.p2align 6\n.L_loop_{name}:")
    E(f"\ts_waitcnt vmcnt(0)")                                # block b+1 landed in the staging registers
    lwrite()                                                    # -> the slot block b-1 was read from
    # a dead quad (784 dims: the last workgroup of every node group has four) only stages: its chain steps were 2 % of
    # the launch's issue slots
    E(f"\ts_cmp_lg_u32 {S_DEAD}, 0")
    E(f"\ts_cbranch_scc1 .L_dead_{name}")
    for g in range(CT // 4):
        E(f"\ts_waitcnt lgkmcnt(0)")                          # x and (c, w) of this group (and my LDS writes)
        if g == 0:
            E(f"\ts_cmp_lt_u32 {S_CNT}, 2")                   # block b+2 -> registers (if there is one)
            E(f"\ts_cbranch_scc1 .L_nl_{name}")
            gload()
            E(f".L_nl_{name}:")
            zload(S_ZN, k.S_ZN2 if two else None)               # next block's mask word
        xload(XSET[(g + 1) % 2], g + 1)                         # next group's x (the next block's at g = 7)
        if g + 1 < CT // 4:
            cread((g + 1) % 2, g + 1)
        xs, r = XSET[g % 2], V_RING + (4 if conly else 8) * (g % 2)
        for i in range(4):
            step(o, mode, xs + 4 * i, r + (1 if conly else 2) * i, 4 * g + i, k)
    if two:                                                     # x pointers: one bump per block
        for ptr in (S_XP, k.S_XP2):
            E(f"\ts_add_u32 s{ptr[0]}, s{ptr[0]}, {16 * CT}")
            E(f"\ts_addc_u32 s{ptr[1]}, s{ptr[1]}, 0")
    E(f"\tv_xor_b32_e32 v{V_CW}, {slot_xor}, v{V_CW}")
    E(f"\tv_xor_b32_e32 v{V_CR}, {slot_xor}, v{V_CR}")
    E(f"\ts_waitcnt lgkmcnt(0)")
    E(f"\ts_mov_b32 {S_Z}, {S_ZN}")
    if two:
        E(f"\ts_mov_b32 {k.S_Z2}, {k.S_ZN2}")
    E(f"\ts_barrier")                                          # slot b+1 written by all, slot b read by all
    cread(0, 0)
    E(f"\ts_sub_u32 {S_CNT}, {S_CNT}, 1")
    E(f"\ts_cmp_lg_u32 {S_CNT}, 0")
    E(f"\ts_cbranch_scc1 .L_loop_{name}")
    E(f"\ts_branch .L_last_{name}")
    # ---- the same block for a dead quad: staging, the barrier, nothing else ------------------------
    E(f".L_dead_{name}:")
    E(f"\ts_cmp_lt_u32 {S_CNT}, 2")                           # block b+2 -> registers (if there is one)
    E(f"\ts_cbranch_scc1 .L_dnl_{name}")
    gload()
    E(f".L_dnl_{name}:")
    E(f"\tv_xor_b32_e32 v{V_CW}, {slot_xor}, v{V_CW}")
    E(f"\ts_waitcnt lgkmcnt(0)")
    E(f"\ts_barrier")
    E(f"\ts_sub_u32 {S_CNT}, {S_CNT}, 1")
    E(f"\ts_cmp_lg_u32 {S_CNT}, 0")
    E(f"\ts_cbranch_scc1 .L_loop_{name}")
    E(f"\ts_branch .L_end_{name}")
    # ---- last block: 1..32 samples, no staging ----------------------------------------------------
    E(f".L_last_{name}:")
    E(f"\ts_cmp_lg_u32 {S_DEAD}, 0")                           # (a dead quad of a chunk of at most 32 samples)
    E(f"\ts_cbranch_scc1 .L_end_{name}")
    for g in range(CT // 4):
        E(f"\ts_cmp_le_u32 {S_TAIL}, {4 * g}")
        E(f"\ts_cbranch_scc1 .L_store_{name}")
        E(f"\ts_waitcnt lgkmcnt(0)")
        if g + 1 < CT // 4:
            xload(XSET[(g + 1) % 2], g + 1)                     # (rows past the chunk: padded, never consumed)
            cread((g + 1) % 2, g + 1)
        xs, r = XSET[g % 2], V_RING + (4 if conly else 8) * (g % 2)
        for i in range(4):
            if i > 0:
                E(f"\ts_cmp_le_u32 {S_TAIL}, {4 * g + i}")
                E(f"\ts_cbranch_scc1 .L_store_{name}")
            step(o, mode, xs + 4 * i, r + (1 if conly else 2) * i, 4 * g + i, k)
    # ---- epilogue: map row <- M (Som.cpp:870), sigma buffer <- raw S --------------------------------
    E(f".L_store_{name}:")
    E(f"\ts_waitcnt vmcnt(0) lgkmcnt(0)")
    E(f"\ts_cmp_lg_u32 {S_DEAD}, 0")
    E(f"\ts_cbranch_scc1 .L_end_{name}")
    VN = f"v{V_A + 2}"
    VA = f"v[{V_A}:{V_A + 1}]"
    E(f"\tv_and_b32_e32 {VN}, 63, v{V_TID}")
    E(f"\ts_lshl_b32 {S_TMP}, {S_WGX}, 6")
    E(f"\tv_add_u32_e32 {VN}, {S_TMP}, {VN}")                   # local node index
    E(f"\tv_cmp_gt_u32_e32 vcc, {S_NLOC}, {VN}")
    E(f"\ts_and_saveexec_b64 {S_EXEC}, vcc")
    E(f"\ts_cbranch_execz .L_end_{name}")
    E(f"\tv_add_u32_e32 {VN}, {S_N0}, {VN}")                    # global node index
    E(f"\ts_lshl_b32 {S_TMP}, {S_Q}, 4")                       # quad * 16 B
    outs = [(S_MAP, V_M)] if mode in MEAN else [(S_MAP, V_M), (S_SBUF, k.V_S)]   # the mean-only kernels store M alone
    for base, tag in outs:
        E(f"\ts_add_u32 {S_TMP2}, s{base[0]}, {S_TMP}")
        E(f"\ts_addc_u32 s34, s{base[1]}, 0")
        E(f"\tv_mov_b32_e32 v{V_A}, {S_TMP2}")
        E(f"\tv_mov_b32_e32 v{V_A + 1}, s34")
        E(f"\tv_mad_u64_u32 {VA}, s[34:35], {VN}, {S_PITCH}, {VA}")
        E(f"\tglobal_store_dwordx4 {VA}, v[{tag}:{tag + 3}], off")
        if two:                                                 # the second quad, unless it is dead
            E(f"\ts_add_u32 {S_TMP}, {S_Q}, 1")
            E(f"\ts_cmp_ge_u32 {S_TMP}, {S_NQ}")
            E(f"\ts_cbranch_scc1 .L_end_{name}")
            E(f"\tglobal_store_dwordx4 {VA}, v[{tag + 4}:{tag + 7}], off offset:16")
    E(f".L_end_{name}:")
    E(f"\ts_endpgm")
    E(f".L_func_end_{name}:")
    E(f"\t.size {name}, .L_func_end_{name}-{name}")
    return "\n".join(o)


MODES = ("std", "fma", "sfma", "med", "mean", "meanfma", "medmean")


def emit():
    """[(name, text, vgprs, kernarg bytes, lds bytes, dx10_clamp, workgroup size)] for gen_update_asm.main()"""
    out = []
    for m in MODES:
        name = f"vsom_update_{m}_nt4_gfx950"
        out.append((name, kernel(name, m), K1.NVGPR, 80, LDS_BYTES_C if m in MEAN else LDS_BYTES, 0 if m in MED else 1, K1.WG))
    for m in MEAN:                                              # two column quads per wavefront
        name = f"vsom_update_{m}_nt8_gfx950"
        out.append((name, kernel(name, m, K2), K2.NVGPR, 80, LDS_BYTES_C, 0 if m in MED else 1, K2.WG))
    return out
