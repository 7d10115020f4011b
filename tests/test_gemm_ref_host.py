"""tests/gemm_ref.py without a GPU: the float64 reference against a nested-loop restatement of the formula in include/transception_hip.h
(read from the very buffers and strides a TcGemm would carry) and against torch.matmul, the buffer layout rules, the coverage of the case
tables, and the guard the exact GPU tests rest on -- every result of every input family is an fp32 value."""
import pytest
import torch

import gemm_ref as gr
from gemm_ref import ACT_NONE, ACT_SCALE, ACT_SIGMOID, Problem, gemm_ref

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _loops(p):
    """The header's definition on the flat buffers of a Problem: C[b] = alpha op(A[b]) op(B[b]) + bias + R[b] (alpha outside everything
    for TC_ACT_SCALE), sigmoid, C += ; z = b1 nb2 + b2 at element offsets b1 s?1 + b2 s?2; bgap blocks; rowsum[m] += sum_k op(A)[m, k]."""
    f = p.fields
    A, B, C = (p.bufs[n].double().tolist() for n in "ABC")
    R = p.bufs["R"].double().tolist() if "R" in p.bufs else None
    bias = p.bufs["bias"].double().tolist() if "bias" in p.bufs else None
    rs = p.bufs["rowsum"].double().tolist() if "rowsum" in p.bufs else None
    first = set()
    for b1 in range(f["nb1"]):
        for b2 in range(f["nb2"]):
            a0 = p.off["A"] + b1 * f["sA1"] + b2 * f["sA2"]
            b0 = p.off["B"] + b1 * f["sB1"] + b2 * f["sB2"]
            c0 = p.off["C"] + b1 * f["sC1"] + b2 * f["sC2"]
            for m in range(f["M"]):
                arow = [A[a0 + (k * f["lda"] + m if f["transA"] else m * f["lda"] + k)] for k in range(f["K"])]
                if rs is not None:
                    rs[p.off["rowsum"] + b1 * f["sRow1"] + m] += sum(arow)
                for n in range(f["N"]):
                    acc = 0.0
                    for k in range(f["K"]):
                        if f["transB"]:
                            bv = B[b0 + n * f["ldb"] + k]
                        else:
                            bv = B[b0 + k * f["ldb"] + n + ((k // f["bgap_every"]) * f["bgap"] if f["bgap_every"] else 0)]
                        acc += arow[k] * bv
                    extra = 0.0
                    if bias is not None:
                        extra += bias[p.off["bias"] + b1 * f["sBias1"] + n]
                    if R is not None:
                        extra += R[p.off["R"] + b1 * f["sR1"] + b2 * f["sR2"] + m * f["ldr"] + n]
                    v = f["alpha"] * (acc + extra) if f["act"] == ACT_SCALE else f["alpha"] * acc + extra
                    if f["act"] == ACT_SIGMOID:
                        v = float(torch.sigmoid(torch.tensor(v, dtype=torch.float64)))
                    at = c0 + m * f["ldc"] + n
                    if f["accumulate"] or at in first:                # (batches that share one C: each adds)
                        v += C[at]
                    first.add(at)
                    C[at] = v
    return torch.tensor(C, dtype=torch.float64), (torch.tensor(rs, dtype=torch.float64) if rs is not None else None)


TINY = [dict(M=3, N=5, K=4), dict(M=3, N=5, K=4, tA=1), dict(M=3, N=5, K=4, tB=1), dict(M=2, N=3, K=5, tA=1, tB=1),
        dict(M=3, N=4, K=3, nb1=2, nb2=3, bias=True, R=True, alpha=0.5),
        dict(M=3, N=4, K=3, nb1=3, bias=True, bias_per_batch=True, alpha=-2.0, tB=1),
        dict(M=3, N=4, K=3, bias=True, R=True, alpha=0.5, act=ACT_SCALE),
        dict(M=3, N=4, K=3, bias=True, R=True, alpha=0.5, act=ACT_SIGMOID),
        dict(M=3, N=4, K=3, bias=True, R=True, alpha=-2.0, accumulate=1, misalign=("A", "C"), odd=("B", "R")),
        dict(M=3, N=4, K=5, tA=1, nb1=2, nb2=2, accumulate=1, c_f32=1, rowsum=True, rowsum_per_batch=True),
        dict(M=3, N=4, K=5, tA=0, nb1=2, nb2=2, accumulate=1, c_f32=1, rowsum=True),
        dict(M=3, N=4, K=5, tA=1, nb1=2, nb2=2, accumulate=1, c_f32=1, atomic=1, shared_c=True, bias=True, R=True),
        dict(M=2, N=4, K=150, tB=0, bgap_every=64, bgap=8, bias=True),
        dict(M=2, N=4, K=192, tA=1, tB=0, bgap_every=64, bgap=72)]


@pytest.mark.parametrize("i", range(len(TINY)))
def test_reference_and_layout_against_nested_loops(i):
    p = Problem(f"tiny{i}", torch.float32, **TINY[i])
    want_c, want_rs = _loops(p)
    if TINY[i].get("act") == ACT_SIGMOID:
        got = p.bufs["C"].double().clone()
        got[p.idx["C"]] = p.ref
        assert torch.allclose(got, want_c, rtol=0, atol=1e-15)
    else:
        assert torch.equal(p.expect["C"].double(), want_c)
    if want_rs is not None:
        assert torch.equal(p.expect["rowsum"].double(), want_rs)


def test_reference_against_matmul():
    g = torch.Generator().manual_seed(5)
    A, B = torch.randn(2, 3, 7, 11, generator=g, dtype=torch.float64), torch.randn(2, 3, 11, 5, generator=g, dtype=torch.float64)
    bias, R, C0 = torch.randn(2, 5, generator=g, dtype=torch.float64), torch.randn(2, 3, 7, 5, generator=g, dtype=torch.float64), torch.randn(2, 3, 7, 5, generator=g, dtype=torch.float64)
    mm = torch.matmul(A, B)
    c, _ = gemm_ref(A, B)
    assert torch.equal(c, mm)
    c, _ = gemm_ref(A, [B[:, :, :4], B[:, :, 4:8], B[:, :, 8:]], 0.5, bias, R, ACT_NONE, C0)
    assert torch.allclose(c, 0.5 * mm + bias[:, None, None] + R + C0, rtol=1e-14, atol=1e-14)
    c, _ = gemm_ref(A, B, 0.5, bias, R, ACT_SCALE)
    assert torch.allclose(c, 0.5 * (mm + bias[:, None, None] + R), rtol=1e-14, atol=1e-14)
    c, _ = gemm_ref(A, B, 0.5, bias[:1], None, ACT_SIGMOID)
    assert torch.allclose(c, torch.sigmoid(0.5 * mm + bias[0]), rtol=1e-14, atol=1e-14)
    c, rs = gemm_ref(A, B, 1.0, None, None, ACT_NONE, C0[:1, :1], True, torch.zeros(2, 7, dtype=torch.float64))
    assert torch.allclose(c, mm.sum((0, 1), keepdim=True) + C0[:1, :1], rtol=1e-14, atol=1e-14)
    assert torch.allclose(rs, A.sum(3).sum(1), rtol=1e-14, atol=1e-14)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_every_input_family_is_exact(dtype):
    """The guard of tests/test_gemm_abi_gpu.py: for every case it compares exactly, the float64 result (C, rowsum, the BatchNorm partials)
    cast to fp32 is unchanged, operands are small integers of the storage type, logical elements do not overlap, and all that lies outside
    them in an operand buffer is NaN."""
    cases = gr.all_exact_cases(dtype)
    assert len({kw["tag"] for kw in cases}) == len(cases)
    for kw in cases:
        p = Problem(dtype=dtype, **kw)
        assert p.exact(), kw["tag"]
        assert float(p.ref.abs().max()) < 2 ** 24
        for name in ("A", "B", "R"):
            if name in p.bufs:
                idx = p.idx[name].reshape(-1)
                assert idx.unique().numel() == idx.numel(), (kw["tag"], name)
                assert int(p.bufs[name].isnan().sum()) == p.bufs[name].numel() - idx.numel() > 0
        idx = (p.idx["C"][:1, :1] if kw.get("shared_c") else p.idx["C"]).reshape(-1)
        assert idx.unique().numel() == idx.numel()
        assert not bool(p.expect["C"].isnan().any()) and p.expect["C"].numel() > idx.numel()
        if dtype != torch.float32 and not p.fields["c_f32"]:
            # the 16-bit C is the exact value rounded ONCE
            assert torch.equal(p.expect["C"][p.idx["C"]], p.ref.to(dtype))


def test_sixteen_bit_ties_occur():
    """Results that lie halfway between two bf16 values (257 = 256 + 1, spacing 2; 128.5) are in the families, so round-to-nearest-even is tested."""
    for kw in gr.epilogue_cases():
        if "ties" in kw["tag"]:
            r = Problem(dtype=torch.bfloat16, **kw).ref
            ties = ((r.abs() >= 256) & (r.abs() < 512) & (r % 2 == 1)) | ((r.abs() >= 128) & (r.abs() < 256) & (r % 1 == 0.5))
            assert int(ties.sum()) > 100, kw["tag"]


def test_case_tables_cover_the_lists():
    for tA, tB in gr.LAYOUTS:
        cs = gr.layout_cases(tA, tB)
        assert {(c["M"], c["K"]) for c in cs} == {(m, k) for m in gr.MS for k in gr.KS}
        assert {(c["N"], c["K"]) for c in cs} == {(n, k) for n in gr.NS for k in gr.KS}
        assert {(c["M"], c["N"]) for c in cs} == {(m, n) for m in gr.MS for n in gr.NS}
        assert {c["alpha"] for c in cs} == {1.0, 0.5, -2.0}
    ks = [c["K"] for c in gr.multi_cases(12)]
    assert len(set(ks)) == 12 and ks != sorted(ks, reverse=True)
    assert len({(c["M"], c["N"]) for c in gr.multi_cases(12)}) == 12
