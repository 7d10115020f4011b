#!/usr/bin/env python3
"""Emits the hand-scheduled gfx950 instruction stream of the bridge SR-attention dQ kernel (attn_bwd_dq_asm_kernel in attention_seg.hip)
with the macro assembler of asm_stream.py; this file holds the dQ stream's register map, operand list and schedule.

The forward's decomposition and ring: one 12-wave workgroup per CU, a 32-query tile per wave (Q / dO fragments and the dQ^T accumulators
stay in AGPRs), 32-key K | V sub-tiles through the 12-slot LDS ring (waves 0-3 stage K, 4-7 V, buffer loads six sub-tiles ahead, a
barrier per four sub-tiles).  K is stored ONCE, rows in key_row order: 16-byte fragment reads for S^T = K Q^T and transpose reads for
dQ^T += K^T dS^T.  Three waves per SIMD leave 84 + 84 registers, so ONE pool of four 4-register fragments serves the three fragment
kinds in turn -- MFMA i of a group reads fragment i and the load behind it refills it for MFMA i of the next group:

  iteration j:  dQ^T(j)       4 MFMAs on the K^T fragments, carrying exp2 / subtract / multiply of sub-tile j+1; refill: K rows of j+2
                S^T(j+2)      4 MFMAs (C = -lse log2 e: P = exp2(S) directly), carrying pack dS(j+1); refill: V rows of j+2
                dP^T(j+2)     4 MFMAs; refill: K^T fragments of j+1; ring store of sub-tile j+6, bookkeeping

Arithmetic = attn_bwd_dq_seg_kernel<H, 1> (Q stored as q * scale * log2 e): dQ = scale * (P (dP - delta)) K.

    python gen_dq_asm.py            # writes attn_dq_asm.inc next to this file
    python gen_dq_asm.py --ahead 7 --out PATH        # an experiment build (scripts/exp): never the committed file
"""
from __future__ import annotations

import os

import asm_stream
from asm_stream import LDR_B, Gen, areg, cvt_name, interleave, regs, vreg
from gen_attn_asm import AHEAD, NSLOT, PERIOD, SLOT_B, layout_defines      # the forward's ring, nothing else: written into the .inc as TC_DQ_*

ABLATIONS = ("nomfma", "noexp")   # timing experiments only (wrong results)
KNOBS = (("--ahead", dict(type=int, default=AHEAD)),)     # to go with the forward's --ahead

# VGPRs
S, DP, NEGL = 0, 16, 32
PD = 48                           # packed dS: two B operands of 4
ST = 56
T0, T1 = 60, 61
AK, AV, AT, AW = 62, 63, 64, 65
NV = 66
# AGPRs
def DQ(blk): return 16 * blk
def QF(ks): return 32 + 4 * ks
def GF(ks): return 48 + 4 * ks
def F(i): return 64 + 4 * i
NA = 80
# operands, by the kernel's names: %0 "+v" global offset of this thread's staging chunk
OPERANDS = ("goff", "kbase", "vbase", "tbase", "wbase", "qoff", "gooff", "oaddr", "nl2", "dl0", "mask", "rsrc", "rq", "rg", "nsub", "step", "wexec", "scl")
(OP_GOFF, OP_KBASE, OP_VBASE, OP_TBASE, OP_WBASE, OP_QOFF, OP_GOOFF, OP_OADDR, OP_NL2, OP_DLT, OP_MASK,
 OP_RSRC, OP_RQ, OP_RG, OP_NSUB, OP_STEP, OP_WEXEC, OP_SCALE) = asm_stream.operands(OPERANDS)
S_CNT, S_SV, S_SK, S_SW, S_PH, S_STEP, S_SCL = 60, 62, 63, 64, 65, 69, 68
SGPRS = list(range(60, 70))


def krow_load(g, i, base):
    b = base if isinstance(base, str) else vreg(base)
    g.emit(f"ds_read_b128 {areg(F(i), 4)}, {b} offset:{32 * i}", "ds_read", [b], regs("a", F(i), 4))


def tr_load(g, i, base):
    """K^T fragment i = 2 k2 + blk: keys 16 h + 8 k2 .. + 7 (two 4-key transpose reads), d block blk."""
    k2, blk = i >> 1, i & 1
    for e in range(2):
        g.emit(f"ds_read_b64_tr_b16 {areg(F(i) + 2 * e, 2)}, {vreg(base)} offset:{(2 * k2 + e) * LDR_B + 64 * blk}", "ds_read",
               [vreg(base)], regs("a", F(i) + 2 * e, 2))


def mf_dq(g, i):
    k2, blk = i >> 1, i & 1
    g.mfma(DQ(blk), F(i), PD + 4 * k2, DQ(blk), acc_d=True)


def mf_s(g, ks):
    g.mfma(S, F(ks), QF(ks), NEGL if ks == 0 else S, b_acc=True)


def mf_dp(g, ks):
    if ks == 0:       # C = 0 (inline constant)
        g.emit(f"v_mfma_f32_32x32x16_{g.half} {vreg(DP, 16)}, {areg(F(0), 4)}, {areg(GF(0), 4)}, 0", "mfma",
               regs("a", F(0), 4) + regs("a", GF(0), 4), regs("v", DP, 16))
    else:
        g.mfma(DP, F(ks), GF(ks), DP, b_acc=True)


def valu_items(g, masked):
    """P = exp2(S) in place (keys past Nk: 0), dS = P (dP - delta) in place of dP."""
    it = [lambda r=r: g.valu(f"v_exp_f32_e32 {vreg(S + r)}, {vreg(S + r)}", [vreg(S + r)], [vreg(S + r)], trans=True) for r in range(16)]
    if masked:
        for r in range(16):
            it.append(lambda r=r: g.valu(f"v_bfe_i32 {vreg(T0)}, {OP_MASK}, {r}, 1", [], [vreg(T0)]))
            it.append(lambda r=r: g.valu(f"v_bfi_b32 {vreg(S + r)}, {vreg(T0)}, 0, {vreg(S + r)}", [vreg(T0), vreg(S + r)], [vreg(S + r)]))
    it += [lambda r=r: g.valu(f"v_sub_f32_e32 {vreg(DP + r)}, {vreg(DP + r)}, {OP_DLT}", [vreg(DP + r)], [vreg(DP + r)]) for r in range(16)]
    it += [lambda r=r: g.valu(f"v_mul_f32_e32 {vreg(DP + r)}, {vreg(DP + r)}, {vreg(S + r)}", [vreg(DP + r), vreg(S + r)], [vreg(DP + r)]) for r in range(16)]
    return it


def pack_items(g):
    return [lambda q=q: g.valu(f"{cvt_name(g.half)} {vreg(PD + q)}, {vreg(DP + 2 * q)}, {vreg(DP + 2 * q + 1)}", regs("v", DP + 2 * q, 2), [vreg(PD + q)])
            for q in range(8)]


def iteration(g, mode):
    first, last, drain = mode == "first", mode == "last", mode == "drain"
    stage = not (last or drain)
    # ---- dQ^T(j) | VALU(j+1) | K rows (j+2)
    head = []
    if mode == "loop":
        head.append(lambda: asm_stream.ring_barrier(g, S_PH, PERIOD))
    if stage:
        head += asm_stream.ring_request(g, ST, OP_GOFF, OP_RSRC, OP_WEXEC, S_STEP)
        head.append(lambda: g.valu(f"v_add_u32_e32 {vreg(AK)}, s{S_SK}, {OP_KBASE}", [], [vreg(AK)]))
    if not first:
        head.append(lambda: g.salu("s_setprio 1"))
    interleave(4, None if first else (lambda i: mf_dq(g, i)), (lambda i: krow_load(g, i, AK)) if stage else None,
               [] if drain else valu_items(g, last), head)
    if not first:
        g.salu("s_setprio 0")
    if drain:
        return
    # ---- S^T(j+2) | V rows (j+2) | pack dS(j+1): the packs read the dS registers the dP^T group overwrites, not the S registers this one
    #      writes, and sit between a V-row refill and the dP^T MFMA that needs it
    head = []
    if not last:
        head.append(lambda: g.valu(f"v_add_u32_e32 {vreg(AV)}, s{S_SK}, {OP_VBASE}", [], [vreg(AV)]))
    head.append(lambda: g.valu(f"v_add_u32_e32 {vreg(AT)}, s{S_SV}, {OP_TBASE}", [], [vreg(AT)]))
    interleave(4, None if last else (lambda i: mf_s(g, i)), None if last else (lambda i: krow_load(g, i, AV)), pack_items(g), head)
    # ---- dP^T(j+2) | K^T fragments (j+1) | ring store, slot bookkeeping
    free = []
    if stage:
        free.append(lambda: asm_stream.ring_stash(g, ST, AW, S_SW, OP_WBASE, OP_WEXEC))
    if not last:
        free.append(lambda: asm_stream.ring_advance(g, (S_SV, S_SK, S_SW), SLOT_B, NSLOT))
    noop = lambda: None
    free = [noop] * (4 - len(free)) + free
    interleave(4, None if last else (lambda i: mf_dp(g, i)), lambda i: tr_load(g, i, AT), free)


def prologue(g, ahead):
    g.salu(f"s_mov_b32 s{S_CNT}, {OP_NSUB}")
    g.salu(f"s_mov_b32 s{S_STEP}, {OP_STEP}")
    g.salu(f"s_mov_b32 s{S_SCL}, {OP_SCALE}")
    g.salu(f"s_mov_b32 s{S_SV}, 0")                                                       # K^T fragments of sub-tile 0
    g.salu(f"s_mov_b32 s{S_SK}, {SLOT_B}")                                                # K / V rows of sub-tile 1
    g.salu(f"s_mov_b32 s{S_SW}, {(ahead - 1) * SLOT_B}")
    g.salu(f"s_mov_b32 s{S_PH}, {2 % PERIOD}")
    g.salu(f"s_sub_u32 s{S_CNT}, s{S_CNT}, 2")
    for ks in range(4):                                                                   # Q / dO fragments of the wave's 32 queries: global -> AGPRs
        g.emit(f"buffer_load_dwordx4 {areg(QF(ks), 4)}, {OP_QOFF}, {OP_RQ}, 0 offen offset:{32 * ks}", "vmem_load", [], regs("a", QF(ks), 4))
        g.emit(f"buffer_load_dwordx4 {areg(GF(ks), 4)}, {OP_GOOFF}, {OP_RG}, 0 offen offset:{32 * ks}", "vmem_load", [], regs("a", GF(ks), 4))
    for i in range(4):
        krow_load(g, i, OP_KBASE)                                                         # K rows of sub-tile 0 (slot 0)
    for r in range(16):
        g.valu(f"v_mov_b32_e32 {vreg(NEGL + r)}, {OP_NL2}", [], [vreg(NEGL + r)])
    for r in range(32):
        g.valu(f"v_accvgpr_write_b32 {areg(r)}, 0", [], [areg(r)])
    g.wait_vm(0)
    for i in range(4):
        mf_s(g, i)
        g.emit(f"ds_read_b128 {areg(F(i), 4)}, {OP_VBASE} offset:{32 * i}", "ds_read", [], regs("a", F(i), 4))
    for i in range(4):
        mf_dp(g, i)


def epilogue(g):
    g.nop(32)
    asm_stream.write_acc_tile(g, DQ, S, f"s{S_SCL}", OP_OADDR)
    g.wait_lgkm(0)


def generate(half, k):
    g = Gen(half, k.ablate)
    return g, asm_stream.pipelined_loop(g, S_CNT, lambda: prologue(g, k.ahead), lambda mode: iteration(g, mode), lambda: epilogue(g))


def main(argv=None):
    committed = os.path.join(os.path.dirname(os.path.abspath(__file__)), "attn_dq_asm.inc")
    k = asm_stream.parse_args(argv, committed, ABLATIONS, KNOBS)
    asm_stream.write_inc(k, "gen_dq_asm.py", "TC_ATTN_DQ_ASM", {h: generate(h, k) for h in ("bf16", "f16")},
                         asm_stream.clobbers(NV, NA, SGPRS), OPERANDS, layout_defines("TC_DQ", k.ahead))


if __name__ == "__main__":
    main()
