"""The macro assembler of the hand-scheduled attention streams (transception_amd/csrc/asm_stream.py) and its three generators, on the
host: the committed .inc files are what the generators emit, whatever the environment holds; experiment knobs are arguments that
never reach a committed file; and the two checks the assembler exists for -- counted waits from the queue model, wait-state
padding and its re-check from ONE hazard table, the loop back-edge -- do what they say.  No GPU, no compiler."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "transception_amd", "csrc")
sys.path.insert(0, CSRC)
import asm_stream  # noqa: E402
import gen_attn_asm  # noqa: E402
import gen_dkv_asm  # noqa: E402
import gen_dq_asm  # noqa: E402
from asm_stream import Gen, Ins, check_hazards  # noqa: E402

sys.path.remove(CSRC)

GENERATORS = {"attn_fwd_asm.inc": gen_attn_asm, "attn_dq_asm.inc": gen_dq_asm, "attn_dkv_asm.inc": gen_dkv_asm}


def committed(inc):
    with open(os.path.join(CSRC, inc), "rb") as f:
        return f.read()


@pytest.mark.parametrize("inc", GENERATORS)
def test_committed_equals_generated(inc, tmp_path):
    out = tmp_path / inc
    GENERATORS[inc].main(["--out", str(out)])
    assert out.read_bytes() == committed(inc)


@pytest.mark.parametrize("inc", GENERATORS)
def test_ambient_environment_is_inert(inc, tmp_path):
    """The variables the generators used to read, set as an experiment shell would have them: a fresh interpreter still emits the
    committed bytes (and with no argument rewrites nothing)."""
    env = dict(os.environ, TC_ATTN_ABLATE="nomfma", TC_DKV_ABLATE="novalu", TC_ATTN_AHEAD="7", TC_ATTN_TIMING="1", TC_ATTN_DEFER="1")
    before = committed(inc)
    script = os.path.join(CSRC, GENERATORS[inc].__name__ + ".py")
    out = tmp_path / inc
    subprocess.run([sys.executable, script, "--out", str(out)], check=True, env=env)
    subprocess.run([sys.executable, script], check=True, env=env)
    assert out.read_bytes() == before
    assert committed(inc) == before


def streams(text):
    """What lies between every R"ASM( and )ASM"."""
    return [part.split(')ASM"')[0] for part in text.split('R"ASM(')[1:]]


KNOBS = ([("attn_fwd_asm.inc", ["--ablate", m] + (["--timing"] if m == "nostage" else [])) for m in gen_attn_asm.ABLATIONS] +     # nostage: see ABLATIONS
         [("attn_fwd_asm.inc", a) for a in (["--ahead", "7"], ["--defer"], ["--timing"], ["--ahead", "7", "--defer"], ["--ablate", "novalu,nobar"])] +
         [("attn_dq_asm.inc", ["--ablate", m]) for m in gen_dq_asm.ABLATIONS] + [("attn_dq_asm.inc", ["--ahead", "7"])] +
         [("attn_dkv_asm.inc", ["--ablate", m]) for m in gen_dkv_asm.ABLATIONS])


@pytest.mark.parametrize("inc,knob", KNOBS, ids=[f"{i.split('_')[1]}:{' '.join(k)}" for i, k in KNOBS])
def test_explicit_knob_works_and_is_contained(inc, knob, tmp_path):
    main, before = GENERATORS[inc].main, committed(inc)
    for refused in (knob, knob + ["--out", os.path.join(CSRC, inc)]):          # no --out; --out naming the committed file
        with pytest.raises(SystemExit):
            main(refused)
    out = tmp_path / "variant.inc"
    main(knob + ["--out", str(out)])
    assert streams(out.read_text()) != streams(before.decode())
    assert committed(inc) == before


def test_ahead_reaches_the_kernel_through_the_inc(tmp_path):
    for gen, name in ((gen_attn_asm, "TC_AS_AHEAD"), (gen_dq_asm, "TC_DQ_AHEAD")):
        out = tmp_path / name
        gen.main(["--ahead", "7", "--out", str(out)])
        assert f"#define {name} 7\n" in out.read_text()
        assert f"#define {name} {asm_stream.AHEAD}\n" in committed({"TC_AS_AHEAD": "attn_fwd_asm.inc", "TC_DQ_AHEAD": "attn_dq_asm.inc"}[name]).decode()


def test_unknown_ablation_is_refused(tmp_path):
    with pytest.raises(SystemExit):
        gen_dkv_asm.main(["--ablate", "b128stats", "--out", str(tmp_path / "x.inc")])


# ---- counted waits ------------------------------------------------------------------------------------------------------------------
def texts(g, start=0):
    return [i.text for i in g.out[start:]]


def test_counted_lgkm_waits():
    g = Gen("bf16")
    for r in range(3):
        g.emit(f"ds_read_b32 v{r}, v9", "ds_read", ["v9"], [f"v{r}"])
    n = len(g.out)
    g.valu("v_mov_b32_e32 v20, v7", ["v7"], ["v20"])                    # no load wrote v7 (nor v20): no wait
    assert texts(g, n) == ["v_mov_b32_e32 v20, v7"]
    g.valu("v_mov_b32_e32 v10, v0", ["v0"], ["v10"])                    # the oldest of three: two may stay outstanding
    assert texts(g, n + 1) == ["s_waitcnt lgkmcnt(2)", "v_mov_b32_e32 v10, v0"]
    n = len(g.out)
    g.valu("v_mov_b32_e32 v11, v2", ["v2"], ["v11"])                    # the youngest: none
    assert texts(g, n) == ["s_waitcnt lgkmcnt(0)", "v_mov_b32_e32 v11, v2"]
    assert g.state() == ((), ())


def test_lgkm_count_is_clamped_to_the_counter_width():
    g = Gen("bf16")
    for r in range(20):
        g.emit(f"ds_read_b32 v{r}, v99", "ds_read", ["v99"], [f"v{r}"])
    n = len(g.out)
    g.valu("v_mov_b32_e32 v50, v0", ["v0"], ["v50"])                    # 19 behind it: the 4-bit counter can say 15 at most
    assert texts(g, n) == ["s_waitcnt lgkmcnt(15)", "v_mov_b32_e32 v50, v0"]
    assert len(g.state()[0]) == 15
    g.wait_lgkm(17)                                                     # an explicit count is clamped the same way: 15 outstanding satisfy it
    assert len(g.out) == n + 2


def test_counted_vm_waits():
    g = Gen("bf16")
    for r in range(2):
        g.emit(f"buffer_load_dword v{r}, v9, s[0:3], 0 offen", "vmem_load", ["v9"], [f"v{r}"])
    n = len(g.out)
    g.valu("v_mov_b32_e32 v20, v7", ["v7"], ["v20"])
    g.valu("v_mov_b32_e32 v10, v0", ["v0"], ["v10"])
    g.valu("v_mov_b32_e32 v11, v1", ["v1"], ["v11"])
    assert texts(g, n) == ["v_mov_b32_e32 v20, v7", "s_waitcnt vmcnt(1)", "v_mov_b32_e32 v10, v0", "s_waitcnt vmcnt(0)", "v_mov_b32_e32 v11, v1"]


# ---- the hazard table -----------------------------------------------------------------------------------------------------------
def hazard_pairs():
    """Every (rule, consumer kind, how the consumer touches the register) the table covers."""
    for h in asm_stream.HAZARDS:
        for kind in h.consumers:
            yield pytest.param(h, kind, False, id=f"{h.name.format(kind=kind)}:read")
            if h.writes:
                yield pytest.param(h, kind, True, id=f"{h.name.format(kind=kind)}:write")


def pair(h, kind, writes):
    producer = Ins("producer", h.producer, [], ["v0"])
    consumer = Ins("consumer", kind, [] if writes else ["v0"], ["v0"] if writes else ["v1"])
    return producer, consumer


def passes(producer, consumer, gap):
    try:
        check_hazards([producer] + [Ins("s_nop 0", "nop")] * gap + [consumer])
        return True
    except RuntimeError:
        return False


@pytest.mark.parametrize("h,kind,writes", hazard_pairs())
def test_hazard_rule_checked_and_padded_from_one_table(h, kind, writes):
    producer, consumer = pair(h, kind, writes)
    assert not passes(producer, consumer, h.ws - 1)                    # one wait state short of this rule
    with pytest.raises(RuntimeError, match="hazard on v0: consumer"):
        check_hazards([producer, consumer])
    need = next(n for n in range(64) if passes(producer, consumer, n))  # (another rule on the same pair may ask for more)
    assert need >= h.ws
    g = Gen("bf16")
    g.emit(producer.text, producer.kind, producer.rd, producer.wr)
    g.emit(consumer.text, consumer.kind, consumer.rd, consumer.wr)
    assert [i.kind for i in g.out[:1] + g.out[-1:]] == [producer.kind, consumer.kind]
    assert all(i.kind == "nop" for i in g.out[1:-1]) and sum(i.ws for i in g.out[1:-1]) == need
    check_hazards(g.out)


def test_mfma_accumulating_into_the_previous_d_issues_back_to_back():
    g = Gen("bf16")
    g.mfma(0, 0, 16, 0, b_acc=True)                                      # D = C = v[0:15]
    g.mfma(0, 4, 20, 0, b_acc=True)
    assert [i.kind for i in g.out] == ["mfma", "mfma"]
    check_hazards(g.out)
    g.valu("v_mov_b32_e32 v40, 0", [], ["v40"])
    g.mfma(16, 8, 0, 16)                                                 # the same registers as a B operand: the full MFMA -> MFMA distance
    assert sum(i.ws for i in g.out[3:-1]) == 10 and g.out[-1].kind == "mfma"
    check_hazards(g.out)


# ---- the loop skeleton ------------------------------------------------------------------------------------------------------------
def test_back_edge_queue_check():
    def stream(leak, check=True):
        g = Gen("bf16")

        def iteration(mode):
            g.valu(f"v_mov_b32_e32 v1, 0  ; {mode}", [], ["v1"])
            if leak and mode == "loop":
                g.emit("ds_read_b32 v2, v9", "ds_read", ["v9"], ["v2"])     # still outstanding at the branch back
        return g, asm_stream.pipelined_loop(g, 40, lambda: None, iteration, lambda: None, back_edge_check=check)

    g, sections = stream(False)
    assert set(sections) == {"first", "loop", "last"} and sections["loop"] == 4
    with pytest.raises(RuntimeError, match="back-edge"):
        stream(True)
    stream(True, check=False)                                            # what an ablated dK/dV build asks for, and only that
