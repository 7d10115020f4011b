"""tc_attn_fwd / tc_attn_bwd are the fp32 parity form: every other dtype is refused on the host, before any launch (no GPU needed)."""
import pytest


@pytest.fixture(scope="module")
def built():
    from transception_amd.build import build
    return build(verbose=False)


# non-null, 16-byte aligned addresses that are never dereferenced: every call below is refused
Q, K, V, O, DO, LSE, DELTA, DQ, DK, DV = (0x10000 * (i + 1) for i in range(10))
B, NQ, NK, LD = 2, 200, 98, 64


@pytest.mark.parametrize("dtype", ["TC_BF16", "TC_F16", 3, -1])
def test_per_group_entries_refuse_every_dtype_but_fp32_before_any_launch(built, dtype):
    """Arguments that are valid in every other respect (the fp32 call with them would launch, so it is not made here): 16-bit storage
    goes through tc_attn_fwd_seg / tc_attn_bwd_seg."""
    from transception_amd import _lib
    L = _lib.lib()
    assert (_lib.TC_F32, _lib.TC_BF16, _lib.TC_F16) == (0, 1, 2)
    dt = getattr(_lib, dtype) if isinstance(dtype, str) else dtype
    assert dt != _lib.TC_F32
    with pytest.raises(_lib.TcError, match="tc_attn_fwd failed with status -1"):
        L.tc_attn_fwd(Q, LD, NQ * LD, K, 2 * LD, V, 2 * LD, NK * 2 * LD, O, LD, NQ * LD, LSE, B, NQ, NK, 0.125, dt, None)
    with pytest.raises(_lib.TcError, match="tc_attn_bwd failed with status -1"):
        L.tc_attn_bwd(Q, LD, NQ * LD, K, 2 * LD, V, 2 * LD, NK * 2 * LD, O, LD, NQ * LD, DO, LD, NQ * LD, LSE, DELTA, DQ, LD, NQ * LD,
                      DK, 2 * LD, DV, 2 * LD, NK * 2 * LD, 0, B, NQ, NK, 0.125, dt, None)
