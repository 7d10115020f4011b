"""The macro assembler of the hand-scheduled gfx950 attention streams (gen_attn_asm.py: forward, gen_dq_asm.py: dQ, gen_dkv_asm.py: dK / dV).

A generator spells its schedule as calls on a `Gen`; this module owns what is not specific to one kernel, above all the two checks a
human cannot be trusted with:
  * counted s_waitcnt lgkmcnt()/vmcnt() come from a model of the in-order return queues, and the loop back-edge is verified to
    reproduce the queue state the loop body was generated for (pipelined_loop);
  * the MFMA / transcendental / permlane wait-state rules hipcc's hazard recogniser applies (inline asm gets none of them) are ONE
    table (HAZARDS), enforced with s_nop along the static order (Gen.emit) and re-checked on the dynamic traces (check_hazards).
It also holds the scaffolding the three schedules share (interleave, the ring helpers, the accumulator tile write-out) and the one
place that renders a .inc file (write_inc) and parses a generator's command line (parse_args).  Nothing here reads the environment:
every knob is an argument, and a generator run with an experiment knob refuses to write the committed .inc.
"""
from __future__ import annotations

import argparse
import os
from collections import namedtuple

LDR_B = 144                     # bytes per LDS row of every operand tile: 64 halfs + 8 pad
# The kernels stage sub-tiles 0 .. AHEAD - 2 themselves; sub-tile AHEAD - 1 is the first one a stream requests.  The K | V ring of the
# forward and dQ streams and the Q | dO ring of the dK/dV stream are separate rings that share this depth ON PURPOSE (one figure for "how
# far the global loads run ahead"): changing it moves all three streams, while --ahead of gen_attn_asm.py / gen_dq_asm.py moves only theirs.
AHEAD = 6
NSTAMP = 6                      # timing builds: s_memtime stamps of pipelined_loop (0 .. 4) and of the epilogue's end (5)


def vreg(n, w=1):
    return f"v{n}" if w == 1 else f"v[{n}:{n + w - 1}]"


def areg(n, w=1):
    return f"a{n}" if w == 1 else f"a[{n}:{n + w - 1}]"


def regs(prefix, n, w=1):
    return [f"{prefix}{i}" for i in range(n, n + w)]


def operands(names):
    """The asm operands %0, %1, ... of the kernel's values `names` (the order of the asm statement's operand list)."""
    return [f"%{i}" for i in range(len(names))]


def cvt_name(half):
    return "v_cvt_pk_bf16_f32" if half == "bf16" else "v_cvt_pk_f16_f32"


class Ins:
    __slots__ = ("text", "kind", "rd", "wr", "ws")

    def __init__(self, text, kind, rd=(), wr=(), ws=1):
        self.text, self.kind, self.rd, self.wr, self.ws = text, kind, tuple(rd), tuple(wr), ws


# ---------------------------------------------------------------------------------------------------------------------------------
# The wait-state rules of LLVM's GCNHazardRecognizer that matter here (gfx940/gfx950, 8-pass XDL MFMAs).  A row: the class of the
# instruction that wrote a register, the kinds of instruction the rule holds back, whether it covers their reads only or reads and
# writes of that register, and the wait states between the two.  `tied`: the rule skips a register the consumer also writes -- an MFMA
# whose C is the D of the previous MFMA issues back to back (A / B operands here never come from an MFMA).
VALU_KINDS = ("valu", "trans", "permlane")
Hazard = namedtuple("Hazard", "name producer consumers writes ws tied")
HAZARDS = (
    Hazard("MFMA->{kind}", "mfma", VALU_KINDS + ("ds_read", "ds_write", "vmem_load"), True, 11, False),
    Hazard("VALU->MFMA", "valu", ("mfma",), False, 2, False),
    Hazard("MFMA->MFMA A/B/C", "mfma", ("mfma",), False, 11, True),
    Hazard("trans->VALU", "trans", ("valu", "permlane"), False, 1, False),
    Hazard("VALU->permlane", "valu", ("permlane",), False, 2, False),
)


class HazardClock:
    """Wait-state clock of one instruction order, and per producer class the time each register was last written by it."""

    def __init__(self):
        self.t = 0
        self.last = {"mfma": {}, "valu": {}, "trans": {}}

    def short(self, kind, rd, wr):
        """(rule, register, wait states it has) for every rule that an instruction issued now would break."""
        for h in HAZARDS:
            if kind in h.consumers:
                since = self.last[h.producer]
                for r in (list(rd) + list(wr) if h.writes else rd):
                    if r in since and self.t - since[r] - 1 < h.ws and not (h.tied and r in wr):
                        yield h, r, self.t - since[r] - 1

    def issue(self, kind, wr, ws):
        for r in wr:
            if kind == "mfma":
                self.last["mfma"][r] = self.t
                self.last["valu"].pop(r, None)
            else:
                self.last["mfma"].pop(r, None)
                if kind in VALU_KINDS:
                    self.last["valu"][r] = self.t
            if kind == "trans":
                self.last["trans"][r] = self.t
            else:
                self.last["trans"].pop(r, None)
        self.t += ws


def check_hazards(trace):
    """Raises on the first instruction of a dynamic trace (a list of Ins) that issues before a rule of HAZARDS allows it."""
    clock = HazardClock()
    for ins in trace:
        for h, r, have in clock.short(ins.kind, ins.rd, ins.wr):
            raise RuntimeError(f"{h.name.format(kind=ins.kind)} hazard on {r}: {ins.text} ({have} of {h.ws} wait states)")
        clock.issue(ins.kind, ins.wr, ins.ws)


class Gen:
    """Instruction list + in-order memory-return queues.  Everything is appended through emit(); waits and hazard padding are inserted on
    demand.  ablate: the set of timing-experiment modes (wrong results) of this invocation, each offered only by the generators that list
    it in their ABLATIONS -- 'nomfma' and 'noexp' act here, 'nobar' in ring_barrier below, the rest in the schedules;
    stamp_sgpr: the first SGPR of the s_memtime stamps of a timing build (None: stamp() emits nothing)."""

    def __init__(self, half, ablate=frozenset(), stamp_sgpr=None):
        self.half = half                    # 'bf16' | 'f16'
        self.ablate, self.stamp_sgpr = ablate, stamp_sgpr
        self.out = []                       # Ins, static program order
        self.lgkm = []                      # outstanding LDS ops: tuple of written regs (empty for stores)
        self.vm = []
        self.uid = 0
        self.clock = HazardClock()          # of the static order

    # -- queues ---------------------------------------------------------------------------------------------------------------
    def _need(self, q, name, touched):
        idx = -1
        for i, wr in enumerate(q):
            if any(r in touched for r in wr):
                idx = i
        if idx >= 0:
            n = min(len(q) - idx - 1, 15 if name == "lgkmcnt" else 63)     # the counters are 4 / 6 bits wide: a smaller count waits for more
            self._push(Ins(f"s_waitcnt {name}({n})", "wait"))
            del q[: len(q) - n]

    def wait_lgkm(self, n):
        n = min(n, 15)
        if len(self.lgkm) > n:
            self._push(Ins(f"s_waitcnt lgkmcnt({n})", "wait"))
            del self.lgkm[: len(self.lgkm) - n]

    def wait_vm(self, n):
        if len(self.vm) > n:
            self._push(Ins(f"s_waitcnt vmcnt({n})", "wait"))
            del self.vm[: len(self.vm) - n]

    def _push(self, ins):
        self.out.append(ins)
        self.clock.issue(ins.kind, ins.wr, ins.ws)

    def emit(self, text, kind, rd=(), wr=(), ws=1):
        touched = set(rd) | set(wr)
        self._need(self.lgkm, "lgkmcnt", touched)
        self._need(self.vm, "vmcnt", touched)
        self.nop(max((h.ws - have for h, _, have in self.clock.short(kind, rd, wr)), default=0))     # what hipcc's hazard recogniser does
        self._push(Ins(text, kind, rd, wr, ws))
        if kind == "ds_read":
            self.lgkm.append(tuple(wr))
        elif kind == "ds_write":
            self.lgkm.append(())
        elif kind == "vmem_load":
            self.vm.append(tuple(wr))

    def label(self, name):
        self.out.append(Ins(f"{name}:", "label", ws=0))

    def state(self):
        return (tuple(self.lgkm), tuple(self.vm))

    # -- instruction helpers ----------------------------------------------------------------------------------------------------
    def mfma(self, d, a, b, c, acc_d=False, b_acc=False):
        if "nomfma" in self.ablate:
            return
        dreg, breg = (areg if acc_d else vreg), (areg if b_acc else vreg)
        self.emit(f"v_mfma_f32_32x32x16_{self.half} {dreg(d, 16)}, {areg(a, 4)}, {breg(b, 4)}, {dreg(c, 16)}", "mfma",
                  regs("a", a, 4) + regs("a" if b_acc else "v", b, 4) + regs("a" if acc_d else "v", c, 16), regs("a" if acc_d else "v", d, 16))

    def valu(self, text, rd=(), wr=(), trans=False):
        if trans and "noexp" in self.ablate:
            text, trans = text.replace("v_exp_f32_e32", "v_mov_b32_e32"), False
        self.emit(text, "trans" if trans else "valu", rd, wr)

    def salu(self, text):
        self.emit(text, "salu")

    def stamp(self, k):
        if self.stamp_sgpr is not None:
            self.wait_lgkm(0)
            self._push(Ins(f"s_memtime s[{self.stamp_sgpr + 2 * k}:{self.stamp_sgpr + 2 * k + 1}]", "salu"))
            self._push(Ins("s_waitcnt lgkmcnt(0)", "wait"))

    def nop(self, n):
        while n > 0:
            k = min(n, 16)
            self._push(Ins(f"s_nop {k - 1}", "nop", ws=k))
            n -= k


# ---------------------------------------------------------------------------------------------------------------------------------
def interleave(n, mf, after, free, head=()):
    """head; then for i < n: mf(i), after(i) (either may be None), and an even share of the ordered `free` closures."""
    for f in head:
        f()
    per = [len(free) // n + (1 if k < len(free) % n else 0) for k in range(n)]
    pos = 0
    for i in range(n):
        for f in (mf, after):
            if f is not None:
                f(i)
        for f in free[pos: pos + per[i]]:
            f()
        pos += per[i]


def ring_barrier(g, s_ph, period):
    """Head of a steady iteration: the workgroup barrier every `period`-th one (phase counter in SGPR s_ph) -- the ring stores of the last
    `period` iterations become visible, their slots' previous occupants are dead."""
    g.wait_lgkm(0)
    if "nobar" not in g.ablate:
        g.salu(f"s_cmp_lg_u32 s{s_ph}, 0")
        g.emit(f"s_cbranch_scc1 .Lnobar{g.uid}_%=", "branch")
        g.emit("s_barrier", "barrier")
        g.label(f".Lnobar{g.uid}_%=")
        g.uid += 1
    g.salu(f"s_add_u32 s{s_ph}, s{s_ph}, 1")
    g.salu(f"s_and_b32 s{s_ph}, s{s_ph}, {period - 1}")


def ring_advance(g, sgprs, slot_b, nslot):
    """The ring slot offsets held in `sgprs` move on by one slot, wrapping after `nslot`."""
    for s in sgprs:
        g.salu(f"s_add_u32 s{s}, s{s}, {slot_b}")
        g.salu(f"s_cmp_eq_u32 s{s}, {slot_b * nslot}")
        g.salu(f"s_cselect_b32 s{s}, 0, s{s}")


def ring_request(g, st, goff, rsrc, wexec, s_step):
    """Closures: the staging waves (exec mask `wexec`) request their 16-byte chunk of the next K | V sub-tile into VGPRs st .. st + 3 and
    every thread advances its global offset `goff` by SGPR s_step."""
    return [lambda: g.salu(f"s_mov_b64 exec, {wexec}"),
            lambda: g.emit(f"buffer_load_dwordx4 {vreg(st, 4)}, {goff}, {rsrc}, 0 offen", "vmem_load", [], regs("v", st, 4)),
            lambda: g.salu("s_mov_b64 exec, -1"),
            lambda: g.valu(f"v_add_u32_e32 {goff}, s{s_step}, {goff}", [], [])]


def ring_stash(g, st, aw, s_sw, wbase, wexec):
    """The requested chunk has arrived: the staging waves store it into the ring slot at SGPR s_sw (address VGPR aw = s_sw + wbase)."""
    g.wait_vm(0)
    g.valu(f"v_add_u32_e32 {vreg(aw)}, s{s_sw}, {wbase}", [], [vreg(aw)])
    g.salu(f"s_mov_b64 exec, {wexec}")
    g.emit(f"ds_write_b128 {vreg(aw)}, {vreg(st, 4)}", "ds_write", [vreg(aw)] + regs("v", st, 4))
    g.salu("s_mov_b64 exec, -1")


def write_acc_tile(g, acc, v, scale, oaddr):
    """Two 32 x 32 fp32 accumulator blocks (first AGPR acc(blk)) times `scale` -- a VGPR, or an SGPR -- packed to 16 bits and written to the
    wave's LDS tile at `oaddr`, through the six VGPRs v .. v + 5."""
    sgpr = scale.startswith("s")
    for blk in range(2):
        for q in range(4):
            for e in range(4):
                a = acc(blk) + 4 * q + e
                g.valu(f"v_accvgpr_read_b32 {vreg(v + e)}, {areg(a)}", [areg(a)], [vreg(v + e)])
            for e in range(4):
                x = vreg(v + e)
                g.valu(f"v_mul_f32_e32 {x}, {scale}, {x}" if sgpr else f"v_mul_f32_e32 {x}, {x}, {scale}", [x] if sgpr else [x, scale], [x])
            g.valu(f"{cvt_name(g.half)} {vreg(v + 4)}, {vreg(v)}, {vreg(v + 1)}", regs("v", v, 2), [vreg(v + 4)])
            g.valu(f"{cvt_name(g.half)} {vreg(v + 5)}, {vreg(v + 2)}, {vreg(v + 3)}", regs("v", v + 2, 2), [vreg(v + 5)])
            g.emit(f"ds_write_b64 {oaddr}, {vreg(v + 4, 2)} offset:{64 * blk + 16 * q}", "ds_write", [vreg(v + 4), vreg(v + 5)])


# ---------------------------------------------------------------------------------------------------------------------------------
def pipelined_loop(g, s_cnt, prologue, iteration, epilogue, back_edge_check=True):
    """The skeleton of a software-pipelined stream over nsub >= 2 sub-tiles, SGPR s_cnt = nsub - 2 set by the prologue:

        prologue | iteration('first') | [iteration('loop') x (nsub - 2)] | iteration('last') | iteration('drain') | barrier | epilogue

    The loop body is generated once, so the outstanding-load queues at its end must be the ones it was generated for (the back-edge
    check; an ablated build, whose loop body may legitimately lack the loads, passes back_edge_check=False).  The hazard rules are
    re-checked on the two dynamic traces that differ from the static order: nsub = 4 (the loop body twice) and nsub = 2 (none).
    Returns the sections' lengths in instructions."""
    g.stamp(0)
    prologue()
    g.wait_lgkm(0)
    g.stamp(1)
    iteration("first")
    g.stamp(2)
    first_end = len(g.out)
    st_in = g.state()
    g.salu(f"s_cmp_lt_i32 s{s_cnt}, 1")
    g.emit("s_cbranch_scc1 .Llast_%=", "branch")
    g.label(".Lloop_%=")
    loop_begin = len(g.out)
    iteration("loop")
    g.salu(f"s_sub_u32 s{s_cnt}, s{s_cnt}, 1")
    g.salu(f"s_cmp_lg_u32 s{s_cnt}, 0")
    g.emit("s_cbranch_scc1 .Lloop_%=", "branch")
    loop_end = len(g.out)
    if back_edge_check and g.state() != st_in:
        raise RuntimeError(f"loop back-edge changes the outstanding-load queues:\n in  {st_in}\n out {g.state()}")
    g.label(".Llast_%=")
    last_begin = len(g.out)
    g.stamp(3)
    g.nop(11)                                            # entered from the loop or straight from the first iteration (nsub = 2)
    iteration("last")
    iteration("drain")
    g.wait_lgkm(0)
    g.emit("s_barrier", "barrier")                       # the tiles the epilogue writes lie in ring slots other waves may still be reading
    g.stamp(4)
    epilogue()
    check_hazards(g.out[:loop_end] + g.out[loop_begin:loop_end] + g.out[last_begin:])     # nsub = 4
    check_hazards(g.out[:first_end] + g.out[last_begin:])                                 # nsub = 2
    return dict(first=first_end, loop=loop_end - loop_begin, last=len(g.out) - last_begin)


# ---------------------------------------------------------------------------------------------------------------------------------
def clobbers(nv, na, sgprs):
    c = [f"v{i}" for i in range(nv)] + [f"a{i}" for i in range(na)] + [f"s{i}" for i in sgprs] + ["vcc", "scc", "memory"]
    return ", ".join(f'"{x}"' for x in c)


def parse_args(argv, committed, ablations, knobs=()):
    """The command line of a generator: --out PATH, --ablate a,b,... (from `ablations`), -v, and its own `knobs` ((flag, add_argument
    keywords) pairs).  With no knob set the output is the `committed` .inc; with any, --out is required and must be another file."""
    p = argparse.ArgumentParser(description=f"writes {os.path.basename(committed)}")
    p.add_argument("--out", help="file to write (required with an experiment knob)")
    p.add_argument("--ablate", default="", help="timing experiments only (WRONG results), comma list of: " + ", ".join(ablations))
    p.add_argument("-v", action="store_true", help="print the text")
    for flag, kw in knobs:
        p.add_argument(flag, **kw)
    a = p.parse_args(argv)
    a.ablate = frozenset(filter(None, a.ablate.split(",")))
    if a.ablate - set(ablations):
        p.error(f"unknown --ablate mode(s): {', '.join(sorted(a.ablate - set(ablations)))}")
    a.experiment = bool(a.ablate) or any(getattr(a, flag.lstrip("-")) != p.get_default(flag.lstrip("-")) for flag, _ in knobs)
    if a.experiment and (a.out is None or os.path.realpath(a.out) == os.path.realpath(committed)):
        p.error(f"an experiment build needs --out, and not the committed {os.path.basename(committed)}")
    a.out = a.out or committed
    return a


def write_inc(args, generator, macro, streams, clobber, operand_names, defines, notes=()):
    """Renders and writes a .inc: per half the R"ASM(...)ASM" macro `macro`_<HALF> of streams[half] = (Gen, sections), the clobber macro,
    the asm operands by name in % order (+ `notes`), and `defines` -- the layout the kernel must agree with.  The file is written only
    when its text differs."""
    parts = [f"// GENERATED by {generator} -- do not edit; edit the generator and re-run it (transception_amd.build does).\n"]
    for half, (g, stats) in streams.items():
        nm = sum(1 for i in g.out if i.kind == "mfma")
        parts.append(f"// {half}: {len(g.out)} lines, {nm} MFMAs; sections {stats}\n")
        parts.append(f"#define {macro}_{half.upper()} R\"ASM(\n" + "\n".join(i.text for i in g.out) + "\n)ASM\"\n")
    parts.append(f"#define {macro}_CLOBBERS {clobber}\n")
    parts.append("// asm operands in % order: " + " ".join(operand_names) + "\n")
    parts += [f"// {n}\n" for n in notes]
    parts += [f"#define {k} {v}\n" for k, v in defines.items()]
    text = "".join(parts)
    if not os.path.exists(args.out) or open(args.out).read() != text:
        with open(args.out, "w") as f:
            f.write(text)
    if args.v:
        print(text)
