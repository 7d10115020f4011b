#!/usr/bin/env python3
"""Emits the hand-scheduled gfx950 instruction stream of the bridge SR-attention forward (attn_fwd_asm_kernel in attention_seg.hip).

Why a generator.  The compiler-scheduled kernel (attn_fwd_seg_kernel) runs its twelve waves per CU in lock step -- QK^T MFMAs,
then softmax VALU, then PV MFMAs, re-aligned by a barrier every 128 keys -- so the matrix pipe idles while the VALU works and
vice versa (0.265 of the bf16 MFMA peak in rounds 2-3, and hipcc would not keep a software-pipelined order: variants v60/v74/v80/v92 of
rounds 2-3, `git show 970a2e3:scripts/exp/attn_exp.hip`).  Measured on gfx950 this round (scripts/exp/overlap2.hip, profiles/r4_overlap2.txt): one wave issues
about one instruction per 5.4 cycles whatever its type, so a single wave per SIMD is issue-bound (the first version of this file:
3 query tiles per wave, 486 cycles per 8 MFMAs); but the VALU stream of one wave DOES run under the MFMAs of another wave of the same
SIMD (8 MFMAs 256 -> 269 cycles next to a VALU wave that loses 15 %).  Hence: twelve waves per CU, ONE 32-query tile per wave, and
every wave runs the same software-pipelined stream in which no phase is MFMA-only or VALU-only:

  iteration j:  PV(j)   4 MFMAs, carrying the softmax of sub-tile j+1 (exp2 in place, row sum, overflow check) and the K(j+2) fragment reads
                pack P(j+1)
                QK(j+2) 4 MFMAs, carrying the V(j+1) fragment reads, the ring store of sub-tile j+3 and the loop bookkeeping

Scores come out of the QK^T MFMAs as s * scale * log2(e) - m (Q is scaled when it is staged, -m is the C operand of the first
MFMA), so the softmax is exp2 + add + pack per score and one compare per sub-tile.  The stream is spelled with the macro assembler of
asm_stream.py (counted waits from a model of the return queues, the back-edge queue check, wait-state padding and its re-check on the
dynamic traces, the loop skeleton); this file holds the forward's register map, operand list, ring layout and schedule.

Reference semantics: softmax(Q K^T * scale) V of `M_EfficientSelfAtten` (networks/MSTr.py:2281-2287).  Numerics: a fixed integer
reference exponent m per query row, set from the first key sub-tile and raised whenever a score exceeds it by more than REREF
(a 16-key partial row sum reaching 2^30 for bf16 P, 2^14 for fp16 P, or inf / NaN) -- the scheme of attn_fwd_seg_kernel; the
rare path recomputes the score tile (it was exponentiated in place) against the raised reference.

    python gen_attn_asm.py            # writes attn_fwd_asm.inc next to this file
    python gen_attn_asm.py --timing --ablate novalu --out PATH       # an experiment build (scripts/exp): never the committed file
"""
from __future__ import annotations

import os

import asm_stream
from asm_stream import LDR_B, NSTAMP, Gen, Ins, areg, check_hazards, cvt_name, interleave, regs, vreg

# ---------------------------------------------------------------------------------------------------------------------------------
# ring layout: written into the .inc as TC_AS_* (layout_defines), where attn_fwd_asm_kernel takes it from; the dQ stream shares it
SLOT_B = 2 * 32 * LDR_B          # ring slot: K sub-tile | V sub-tile of 32 keys
NSLOT = 12                      # slots; sub-tile j+AHEAD is stored during iteration j, and the workgroup barrier comes every PERIOD iterations:
AHEAD = asm_stream.AHEAD        #   a store must be separated from the first read of its slot (2 iterations before its PV) and from the last
PERIOD = 4                      #   read of the slot's previous occupant by a barrier: AHEAD >= PERIOD + 2, NSLOT >= AHEAD + PERIOD - 1 (+ slack)
NEG_BIG = 0xF149F2CA            # -1.0e30f
# knobs (the `k` of the functions below: the parsed command line).  Experiments, none of them a product build:
#   --ahead N   AHEAD
#   --defer     ring store of the sub-tile requested ONE iteration ago, at the head of the iteration (stores run AHEAD - 1 ahead; with
#               --ahead 7, scripts/exp/build_fwd_variant.sh): 25.6 vs 25.7 us -- the wait for the global load is not what an iteration waits for
#   --timing    s_memtime stamps at section boundaries (SGPRs from STAMP_SGPR up; the kernel sees TC_ATTN_ASM_TIMING)
#   --ablate    timing experiments only (wrong results).  nostage assembles only together with --timing (how scripts/exp/build_attn_timing.sh
#               runs it): the stamps drain the queues around the loop, without them its body fails the back-edge check
ABLATIONS = ("nomfma", "noexp", "novalu", "nostage", "nobar", "noprio", "prioQ", "dot2", "dot2c")
KNOBS = (("--ahead", dict(type=int, default=AHEAD)), ("--defer", dict(action="store_true")), ("--timing", dict(action="store_true")))


def layout_defines(prefix, ahead):
    return {f"{prefix}_LDR_B": LDR_B, f"{prefix}_SLOT_B": SLOT_B, f"{prefix}_NSLOT": NSLOT, f"{prefix}_AHEAD": ahead, f"{prefix}_PERIOD": PERIOD}


# register map (the VGPRs / AGPRs the stream owns; the kernel's own values live above NV) -------------------------------------------
S = 0                                        # score tile s * qs - m, then P in fp32 (exp2 in place)          16
NEGM = 16                                    # -m broadcast: the C operand of the first QK^T MFMA            16
P = 32                                       # packed P: two B operands of 4                                  8
ST = 40                                      # ring staging (one 16-byte chunk per thread of waves 0-7)       4
L, M, RS, T0, T1, T2, T3, T4 = 44, 45, 46, 47, 48, 49, 50, 51
AK, AV, AW, MSK = 52, 53, 54, 55             # LDS addresses of the current ring slots (the subroutines own T0..T4); tail mask
NV = 56
# AGPRs (at three waves per SIMD hipcc splits the 168 registers of a wave 84 / 84, so the MFMA-only operands live here)
def O(blk): return 16 * blk                  # O^T accumulators                                              32
def QF(ks): return 32 + 4 * ks               # Q fragments                                                   16
def KF(ks): return 48 + 4 * ks               # K fragments of the next sub-tile                              16
def VF(f): return 64 + 4 * f                 # V^T fragments, f = 2 * k2 + blk                                16
NA = 80
# operands of the asm statement, by the kernel's names: %0 is the only output ("+v": the global offset of this thread's staging chunk, advanced per iteration)
OPERANDS = ("goff", "kbase", "vbase", "wbase", "qaddr", "oaddr", "lseaddr", "mask", "rsrc", "nsub", "step", "wexec")
OP_GOFF, OP_KBASE, OP_VBASE, OP_WBASE, OP_QADDR, OP_OADDR, OP_LSEADDR, OP_MASK, OP_RSRC, OP_NSUB, OP_STEP, OP_WEXEC = asm_stream.operands(OPERANDS)
S_CNT, S_THR, S_SV, S_SK, S_SW, S_PH, S_RA, S_LN2, S_STEP = 60, 61, 62, 63, 64, 65, 66, 68, 69
SGPRS = list(range(60, 70))
STAMP_SGPR = 72


# ---------------------------------------------------------------------------------------------------------------------------------
def mf_qk(g, ks):
    g.mfma(S, KF(ks), QF(ks), NEGM if ks == 0 else S, b_acc=True)


def mf_pv(g, f):
    k2, blk = f >> 1, f & 1
    g.mfma(O(blk), VF(f), P + 4 * k2, O(blk), acc_d=True)


def vf_load(g, f, addr):
    k2, blk = f >> 1, f & 1
    for e in range(2):
        g.emit(f"ds_read_b64_tr_b16 {areg(VF(f) + 2 * e, 2)}, {vreg(addr)} offset:{(2 * k2 + e) * LDR_B + 64 * blk}", "ds_read",
               [vreg(addr)], regs("a", VF(f) + 2 * e, 2))


def kf_load(g, ks, addr):
    a = addr if isinstance(addr, str) else vreg(addr)
    g.emit(f"ds_read_b128 {areg(KF(ks), 4)}, {a} offset:{32 * ks}", "ds_read", [a], regs("a", KF(ks), 4))


def max_tree(g, dst):
    """dst = max over the 16 scores of the lane: 7 x v_max3 + 1 x v_max, as closures."""
    it = [lambda: g.valu(f"v_max3_f32 {vreg(dst)}, {vreg(S)}, {vreg(S + 1)}, {vreg(S + 2)}", regs("v", S, 3), [vreg(dst)])]
    for r in range(3, 15, 2):
        it.append(lambda r=r: g.valu(f"v_max3_f32 {vreg(dst)}, {vreg(dst)}, {vreg(S + r)}, {vreg(S + r + 1)}", [vreg(dst)] + regs("v", S + r, 2), [vreg(dst)]))
    it.append(lambda: g.valu(f"v_max_f32_e32 {vreg(dst)}, {vreg(dst)}, {vreg(S + 15)}", [vreg(dst), vreg(S + 15)], [vreg(dst)]))
    return it


def mask_items(g, src):
    """Keys past Nk (bits of the VGPR / operand `src`, one per score register) get the score -1e30."""
    it = [lambda: g.valu(f"v_mov_b32_e32 {vreg(T3)}, 0x{NEG_BIG:08x}", [], [vreg(T3)])]
    for r in range(16):
        it.append(lambda r=r: g.valu(f"v_bfe_i32 {vreg(T4)}, {src}, {r}, 1", [], [vreg(T4)]))
        it.append(lambda r=r: g.valu(f"v_bfi_b32 {vreg(S + r)}, {vreg(T4)}, {vreg(T3)}, {vreg(S + r)}", [vreg(T4), vreg(T3), vreg(S + r)], [vreg(S + r)]))
    return it


def exp_sum_items(g):
    """exp2 in place and the 16-key row sum into RS: 16 + 15 instructions, each sum two instructions behind its exp."""
    def ex(r): return lambda: g.valu(f"v_exp_f32_e32 {vreg(S + r)}, {vreg(S + r)}", [vreg(S + r)], [vreg(S + r)], trans=True)
    def ad(r): return lambda: g.valu(f"v_add_f32_e32 {vreg(RS)}, {vreg(RS)}, {vreg(S + r)}", [vreg(RS), vreg(S + r)], [vreg(RS)])
    it = [ex(0), ex(1), ex(2), lambda: g.valu(f"v_add_f32_e32 {vreg(RS)}, {vreg(S)}, {vreg(S + 1)}", regs("v", S, 2), [vreg(RS)])]
    for r in range(3, 16):
        it += [ex(r), ad(r - 1)]
    it.append(ad(15))
    return it


def sm_items(g, mode):
    """Softmax of the score tile in S as closures (one instruction each unless noted): keys past Nk masked ('last'); the reference
    exponent set from this tile ('first': unconditional call); exp2 in place and the row sum; then ('loop', 'last') ONE compare of
    the row sum against REREF -- a sum that large (or inf / NaN) means some score outgrew the reference exponent, and the rare
    path recomputes the tile against a raised one; L += RS."""
    it = []
    if "novalu" in g.ablate and mode == "loop":
        return it
    if mode == "last":
        it += mask_items(g, OP_MASK)
    if mode == "first":
        it.append(lambda: g.emit(f"s_call_b64 s[{S_RA}:{S_RA + 1}], .Lfirst_%=", "call"))
    it += exp_sum_items(g)
    if mode != "first":
        def check():                           # one unit: nothing may be scheduled between the branch and its target
            g.valu(f"v_cmp_ngt_f32_e32 vcc, s{S_THR}, {vreg(RS)}", [vreg(RS)], ["vcc"])
            g.emit(f"s_cbranch_vccz .Lskip{g.uid}_%=", "branch", ["vcc"])
            g.emit(f"s_call_b64 s[{S_RA}:{S_RA + 1}], .Lslow_%=", "call")
            g.label(f".Lskip{g.uid}_%=")
            g.uid += 1
        it.append(check)
    it.append(lambda: g.valu(f"v_add_f32_e32 {vreg(L)}, {vreg(L)}, {vreg(RS)}", [vreg(L), vreg(RS)], [vreg(L)]))
    return it


def pack_items(g):
    it = [lambda q=q: g.valu(f"{cvt_name(g.half)} {vreg(P + q)}, {vreg(S + 2 * q)}, {vreg(S + 2 * q + 1)}", regs("v", S + 2 * q, 2), [vreg(P + q)])
          for q in range(8)]
    if g.ablate & {"dot2", "dot2c"}:           # what a row sum taken from the packed P would cost
        d2 = "v_dot2c_f32_bf16" if "dot2c" in g.ablate else "v_dot2_f32_bf16"
        tail = "" if "dot2c" in g.ablate else f", {vreg(L)}"
        it += [lambda q=q: g.valu(f"{d2} {vreg(L)}, {vreg(P + q)}, {vreg(T4)}{tail}", [vreg(P + q), vreg(T4), vreg(L)], [vreg(L)]) for q in range(8)]
    return it


def group(mfmas, free, head=()):
    """head: closures before the first MFMA; mfmas: closures; free: ordered closures spread evenly over the gaps after the MFMAs."""
    interleave(max(len(mfmas), 1), (lambda i: mfmas[i]()) if mfmas else None, None, free, head)


def iteration(g, mode, k):
    """Iteration j: PV(j) | softmax(j+1) | K(j+2) reads; pack P(j+1); QK(j+2) | V(j+1) reads | ring store of sub-tile j+3.
    mode 'first' (j = -1): no PV, the softmax sets the reference exponent; 'loop'; 'last' (j = nsub-2): keys past Nk masked,
    no sub-tile j+2; 'drain' (j = nsub-1): PV only."""
    first, last, drain = mode == "first", mode == "last", mode == "drain"
    stage = not (last or drain) and not ("nostage" in g.ablate and mode == "loop")
    # ---- PV(j) group
    head = []
    if mode == "loop":
        head.append(lambda: asm_stream.ring_barrier(g, S_PH, PERIOD))
    stash = lambda: asm_stream.ring_stash(g, ST, AW, S_SW, OP_WBASE, OP_WEXEC)
    if stage:
        if k.defer and not first:
            head.append(stash)
        head += asm_stream.ring_request(g, ST, OP_GOFF, OP_RSRC, OP_WEXEC, S_STEP)
    if last:
        head.append(lambda: g.valu(f"v_mov_b32_e32 {vreg(MSK)}, {OP_MASK}", [], [vreg(MSK)]))
    if not (last or drain):
        head.append(lambda: g.valu(f"v_add_u32_e32 {vreg(AK)}, s{S_SK}, {OP_KBASE}", [], [vreg(AK)]))
    mf = [] if first else [lambda f=f: mf_pv(g, f) for f in range(4)]
    free = [] if drain else sm_items(g, mode)
    if not (last or drain):                    # K(j+2) fragments: free since QK(j+1) issued in the previous iteration
        kl = [lambda ks=ks: kf_load(g, ks, AK) for ks in range(4)]
        free = free[:4] + kl + free[4:] if len(free) > 8 else kl + free
    if mf and "noprio" not in g.ablate:        # the group that carries this wave's VALU work runs at raised priority (measured -3 % loop time)
        head.append(lambda: g.salu("s_setprio 1"))
    group(mf, free, head)
    if mf and "noprio" not in g.ablate:
        g.salu("s_setprio 0")
    if drain:
        return
    for f in pack_items(g):
        f()
    # ---- QK(j+2) group
    head = [lambda: g.valu(f"v_add_u32_e32 {vreg(AV)}, s{S_SV}, {OP_VBASE}", [], [vreg(AV)])]
    mf = [] if last else [lambda ks=ks: mf_qk(g, ks) for ks in range(4)]
    free = [lambda f=f: vf_load(g, f, AV) for f in range(4)]      # V(j+1) fragments: free since PV(j) issued above
    if stage and not k.defer:
        free.append(stash)
    if not last:                               # ring slot offsets of the next iteration
        free.append(lambda: asm_stream.ring_advance(g, (S_SV, S_SK, S_SW), SLOT_B, NSLOT))
    if "prioQ" in g.ablate and mf:
        head.append(lambda: g.salu("s_setprio 1"))
    group(mf, free, head)
    if "prioQ" in g.ablate and mf:
        g.salu("s_setprio 0")


def rereference(g, first):
    """S holds s * qs - m_old: m_delta = ceil(row max over both lane halves) (first) / max(that, 0); rescale L and O by 2^-m_delta
    (not first), m += m_delta, NEGM -= m_delta, S -= m_delta."""
    for f in max_tree(g, T0):
        f()
    g.valu(f"v_mov_b32_e32 {vreg(T1)}, {vreg(T0)}", [vreg(T0)], [vreg(T1)])
    g.emit(f"v_permlane32_swap_b32_e32 {vreg(T0)}, {vreg(T1)}", "permlane", [vreg(T0), vreg(T1)], [vreg(T0), vreg(T1)])
    g.valu(f"v_max_f32_e32 {vreg(T0)}, {vreg(T0)}, {vreg(T1)}", [vreg(T0), vreg(T1)], [vreg(T0)])
    g.valu(f"v_ceil_f32_e32 {vreg(T2)}, {vreg(T0)}", [vreg(T0)], [vreg(T2)])               # T2 = m_delta
    if not first:
        g.valu(f"v_max_f32_e32 {vreg(T2)}, 0, {vreg(T2)}", [vreg(T2)], [vreg(T2)])
        g.valu(f"v_sub_f32_e32 {vreg(T1)}, 0, {vreg(T2)}", [vreg(T2)], [vreg(T1)])
        g.valu(f"v_exp_f32_e32 {vreg(T3)}, {vreg(T1)}", [vreg(T1)], [vreg(T3)], trans=True)  # T3 = 2^-m_delta
        g.valu(f"v_mul_f32_e32 {vreg(L)}, {vreg(L)}, {vreg(T3)}", [vreg(L), vreg(T3)], [vreg(L)])
        for a in range(32):
            g.valu(f"v_accvgpr_read_b32 {vreg(T1)}, {areg(a)}", [areg(a)], [vreg(T1)])
            g.valu(f"v_mul_f32_e32 {vreg(T1)}, {vreg(T1)}, {vreg(T3)}", [vreg(T1), vreg(T3)], [vreg(T1)])
            g.valu(f"v_accvgpr_write_b32 {areg(a)}, {vreg(T1)}", [vreg(T1)], [areg(a)])
    g.valu(f"v_add_f32_e32 {vreg(M)}, {vreg(M)}, {vreg(T2)}", [vreg(M), vreg(T2)], [vreg(M)])
    for r in range(16):
        g.valu(f"v_sub_f32_e32 {vreg(NEGM + r)}, {vreg(NEGM + r)}, {vreg(T2)}", [vreg(NEGM + r), vreg(T2)], [vreg(NEGM + r)])
    for r in range(16):
        g.valu(f"v_sub_f32_e32 {vreg(S + r)}, {vreg(S + r)}, {vreg(T2)}", [vreg(S + r), vreg(T2)], [vreg(S + r)])


def subroutine(g, first):
    """Called, never fallen into; returns through s[S_RA:S_RA+1].
    first: S = QK(0) is intact (called before the exp2 pass): set the reference exponent from it; the caller's exp2 pass follows.
    slow:  called after the exp2 pass found a row sum >= REREF (or inf / NaN): the scores are gone, so reload the K fragments of
           this sub-tile (ring slot S_SV: sub-tile j+1 is both the V the next PV reads and the K of these scores), redo the four
           QK^T MFMAs against the old reference, mask the tail keys (MSK), raise the reference, redo exp2 / row sum, and put the
           K(j+2) fragments back (the caller's outstanding-load queue is exactly those four reads)."""
    g.label(f".L{'first' if first else 'slow'}_%=")
    g0 = Gen(g.half, g.ablate)                 # own wait-state / queue bookkeeping: entered and left with nothing assumed
    g0.uid = 1000
    g0.nop(32)                                 # every MFMA issued before the call has retired (S, O quiescent)
    if not first:
        g0._push(Ins("s_waitcnt lgkmcnt(0)", "wait"))
        g0.valu(f"v_add_u32_e32 {vreg(T0)}, s{S_SV}, {OP_KBASE}", [], [vreg(T0)])
        for ks in range(4):
            kf_load(g0, ks, T0)
        for ks in range(4):
            mf_qk(g0, ks)
        for f in mask_items(g0, vreg(MSK)):
            f()
    rereference(g0, first)
    if not first:
        for f in exp_sum_items(g0):
            f()
        g0.valu(f"v_add_u32_e32 {vreg(T0)}, s{S_SK}, {OP_KBASE}", [], [vreg(T0)])
        for ks in range(4):
            kf_load(g0, ks, T0)
    g0.nop(4)
    g0.emit(f"s_setpc_b64 s[{S_RA}:{S_RA + 1}]", "ret")
    g.out += g0.out


def prologue(g, k):
    g.salu(f"s_mov_b32 s{S_CNT}, {OP_NSUB}")
    g.salu(f"s_mov_b32 s{S_STEP}, {OP_STEP}")
    g.salu(f"s_mov_b32 s{S_THR}, {'0x4e800000' if g.half == 'bf16' else '0x46800000'}")    # REREF: a 16-key row sum of 2^30 (bf16 P) / 2^14 (fp16 P)
    g.salu(f"s_mov_b32 s{S_LN2}, 0x3f317218")
    g.salu(f"s_mov_b32 s{S_SV}, 0")                                                       # V(0)
    g.salu(f"s_mov_b32 s{S_SK}, {SLOT_B}")                                                # K(1)
    g.salu(f"s_mov_b32 s{S_SW}, {(k.ahead - (2 if k.defer else 1)) * SLOT_B}")           # sub-tile AHEAD-1 is stored by iteration -1 (DEFER: by iteration 0)
    g.salu(f"s_mov_b32 s{S_PH}, {2 % PERIOD}")                                            # (j + 2) mod PERIOD of iteration 0
    g.salu(f"s_sub_u32 s{S_CNT}, s{S_CNT}, 2")                                            # steady iterations j = 0 .. nsub - 3
    for ks in range(4):
        g.emit(f"ds_read_b128 {areg(QF(ks), 4)}, {OP_QADDR} offset:{32 * ks}", "ds_read", [], regs("a", QF(ks), 4))
    for ks in range(4):
        kf_load(g, ks, OP_KBASE)                                                          # K(0): slot 0
    g.valu(f"v_mov_b32_e32 {vreg(L)}, 0", [], [vreg(L)])
    g.valu(f"v_mov_b32_e32 {vreg(M)}, 0", [], [vreg(M)])
    g.valu(f"v_mov_b32_e32 {vreg(MSK)}, 0", [], [vreg(MSK)])
    for r in range(16):
        g.valu(f"v_mov_b32_e32 {vreg(NEGM + r)}, 0", [], [vreg(NEGM + r)])
    for r in range(32):
        g.valu(f"v_accvgpr_write_b32 {areg(r)}, 0", [], [areg(r)])
    for ks in range(4):                                                                   # QK(0)
        mf_qk(g, ks)


def epilogue(g):
    g.nop(32)
    g.valu(f"v_mov_b32_e32 {vreg(T0)}, {vreg(L)}", [vreg(L)], [vreg(T0)])
    g.valu(f"v_mov_b32_e32 {vreg(T1)}, {vreg(L)}", [vreg(L)], [vreg(T1)])
    g.emit(f"v_permlane32_swap_b32_e32 {vreg(T0)}, {vreg(T1)}", "permlane", [vreg(T0), vreg(T1)], [vreg(T0), vreg(T1)])
    g.valu(f"v_add_f32_e32 {vreg(T0)}, {vreg(T0)}, {vreg(T1)}", [vreg(T0), vreg(T1)], [vreg(T0)])          # T0 = row sum over both halves
    g.valu(f"v_rcp_f32_e32 {vreg(T4)}, {vreg(T0)}", [vreg(T0)], [vreg(T4)], trans=True)
    g.valu(f"v_log_f32_e32 {vreg(T1)}, {vreg(T0)}", [vreg(T0)], [vreg(T1)], trans=True)
    g.valu(f"v_add_f32_e32 {vreg(T1)}, {vreg(T1)}, {vreg(M)}", [vreg(T1), vreg(M)], [vreg(T1)])
    g.valu(f"v_mul_f32_e32 {vreg(T1)}, s{S_LN2}, {vreg(T1)}", [vreg(T1)], [vreg(T1)])
    g.emit(f"ds_write_b32 {OP_LSEADDR}, {vreg(T1)}", "ds_write", [vreg(T1)])
    asm_stream.write_acc_tile(g, O, S, vreg(T4), OP_OADDR)                                # O = O^T accumulators / row sum
    g.wait_lgkm(0)


# ---------------------------------------------------------------------------------------------------------------------------------
def generate(half, k):
    g = Gen(half, k.ablate, STAMP_SGPR if k.timing else None)

    def pro():
        prologue(g, k)
        g.wait_lgkm(0)
        g.emit("s_barrier", "barrier")                   # the Q tiles (read by now) lie in ring slots that the stores of iteration 0.. reuse

    def it(mode):
        iteration(g, mode, k)
        if k.timing and mode == "loop":
            g.wait_lgkm(0)                               # (the stamp before the loop drained the queue)

    def epi():
        epilogue(g)
        g.stamp(5)
        if k.timing:
            g.salu("s_mov_b64 exec, 1")                  # lane 0 only: the lanes' lse slots are 4 bytes apart
            for s in range(NSTAMP):
                g.valu(f"v_mov_b32_e32 {vreg(S)}, s{STAMP_SGPR + 2 * s}", [], [vreg(S)])
                g.valu(f"v_mov_b32_e32 {vreg(S + 1)}, s{STAMP_SGPR + 2 * s + 1}", [], [vreg(S + 1)])
                g.emit(f"ds_write_b64 {OP_LSEADDR}, {vreg(S, 2)} offset:{4096 + 8 * s}", "ds_write", [vreg(S), vreg(S + 1)])
            g.wait_lgkm(0)
            g.salu("s_mov_b64 exec, -1")
        g.emit("s_branch .Lend_%=", "branch")            # over the subroutines

    stats = asm_stream.pipelined_loop(g, S_CNT, pro, it, epi)
    main_end = len(g.out)
    subroutine(g, True)
    subroutine(g, False)
    g.label(".Lend_%=")
    check_hazards(g.out[main_end:])                      # the subroutines on their own (each starts with 32 wait states)
    return g, dict(stats, sub=len(g.out) - main_end)


def main(argv=None):
    committed = os.path.join(os.path.dirname(os.path.abspath(__file__)), "attn_fwd_asm.inc")
    k = asm_stream.parse_args(argv, committed, ABLATIONS, KNOBS)
    defines = layout_defines("TC_AS", k.ahead)
    if k.timing:
        defines["TC_ATTN_ASM_TIMING"] = NSTAMP
    sgprs = SGPRS + (list(range(SGPRS[-1] + 1, STAMP_SGPR + 2 * NSTAMP)) if k.timing else [])
    asm_stream.write_inc(k, "gen_attn_asm.py", "TC_ATTN_FWD_ASM", {h: generate(h, k) for h in ("bf16", "f16")},
                         asm_stream.clobbers(NV, NA, sgprs), OPERANDS, defines)


if __name__ == "__main__":
    main()
